"""Boundary surfaces and thresholds of cell meshes on the GPU
(spray_rt_cell_surface, spray_rt_domains_cell_surface).

References, each bit for bit: the host restatement (spray_rt_cell_surface_host,
itself checked against numpy in test_cell_surface_host.py) for the extracted
arrays, a build_domains of the restated arrays in a second context for the slot
images, the oracle's brute force for queries.
"""
import numpy as np
import pytest

import build_helpers as bh
import cell_helpers as ch
import color_helpers as colh
import refit_helpers as rh
import surface_helpers as sh
import tet_helpers as th

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5
WHAT = bh.WHAT + ("COLORS", "FACES")
KEPT = tuple(w for w in WHAT if w != "COLORS")
F32 = np.float32
V, N, COL, IDS, F = range(5)


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def batch():
    return sh.gpu_batch()


@pytest.fixture(scope="module")
def restated(spray, batch):
    """(verts, normals, colors, point_ids, faces) of every mesh from the host restatement."""
    return [sh.host_surface(spray, m, s) for m, s in zip(*batch)]


def slot_colors(m, col):
    """The colour array a slot of mesh m carries: none without a field or a colour."""
    return col if m.get("cfield") is not None or m.get("color") is not None else None


def export_all(c, slot, what=WHAT):
    return {w: c.slot_export(slot, getattr(c, "SLOT_" + w)).tobytes() for w in what}


def synced(c, x):
    """x once the context's stream has run: the calls are enqueued there, and
    torch reads on another stream."""
    c.sync()
    return x


def as_bytes(mesh):
    return tuple(None if x is None else x.cpu().numpy().tobytes() for x in mesh)


def ref_bytes(mesh):
    return tuple(None if x is None else x.tobytes() for x in mesh)


def test_batch_shapes(batch, restated):
    """The meshes reach the paths they are there for."""
    meshes, sels = batch
    nc = [len(m["types"]) for m in meshes]
    assert nc[:4] == [1, 1, 1, 1] and [int(meshes[k]["types"][0]) for k in range(4)] == [10, 12, 13, 14]
    assert [len(restated[k][F]) for k in range(4)] == [4, 12, 8, 6]
    assert set(meshes[sh.MIXED]["types"].tolist()) == {12, 13, 14}
    # a quad against two triangles cut along the diagonal that misses its
    # smallest index: one triangle has the quad's triple, and nothing cancels
    cut = meshes[sh.CUT]
    quad = cut["conn"][:4]
    j = int(np.argmin(quad))
    tri = {int(quad[j]), int(quad[(j + 1) % 4]), int(quad[(j + 3) % 4])}
    assert tri in [set(cut["conn"][o:o + 3].tolist()) for o in (8, 12)]
    assert len(restated[sh.CUT][F]) == 18 and len(restated[sh.CUT][V]) == 9
    assert nc[sh.SMALL] == 64 and nc[sh.FULL] == 256             # exactly one block
    assert nc[sh.PARTIAL] == 640 and nc[sh.PARTIAL] % 256 != 0   # a partial last block
    big = meshes[sh.LARGE]
    assert nc[sh.LARGE] == 140608 and -(-nc[sh.LARGE] // 256) == 550 > 512   # past one scan stride
    assert -(-len(big["points"]) // 256) == 582 > 512
    assert nc[sh.NOCELLS] == 0 and nc[sh.EMPTY] > 0
    assert sh.kept_cells(meshes[sh.EMPTY], sels[sh.EMPTY]).sum() == 0
    assert 0 < sh.EMPTY < sh.NOCELLS < len(meshes) - 1
    for k in range(len(meshes)):
        assert (len(restated[k][F]) > 0) == (k not in (sh.EMPTY, sh.NOCELLS)), k
    # all three modes, and selects that drop some cells and keep some
    modes = {"all" if s is None else s["mode"] for s in sels}
    assert modes == {"all", "points", "cells"} and None in sels
    for k in (sh.SMALL, sh.PARTIAL):
        assert 0 < sh.kept_cells(meshes[k], sels[k]).sum() < nc[k], k
    ok = (big["values"] >= F32(sels[sh.LARGE]["lo"]))[big["conn"].reshape(-1, 8)].all(1)
    assert 0.35 * nc[sh.LARGE] < ok.sum() < 0.65 * nc[sh.LARGE]
    # vertices and triangles in the first stride of either scan and past it
    ids = restated[sh.LARGE][IDS]
    assert ids.min() < 256 * 512 < ids.max() and len(restated[sh.LARGE][F]) > 100000
    assert not np.array_equal(meshes[sh.SMALL]["conn"][:8], ch.hex_lattice((5, 5, 5))[3][:8])
    assert meshes[sh.SMALL]["cmap"][0].size == 1 and meshes[sh.FULL]["cmap"][0].size == 4096
    assert meshes[sh.ONE_TET].get("color") is None and meshes[sh.ONE_TET].get("cfield") is None
    assert meshes[sh.ONE_HEX]["color"] is not None
    assert {m.get("normals") is not None for m in meshes} == {True, False}
    assert len(np.unique(restated[sh.LARGE][COL])) > 8


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_restatement(spray, batch, restated, device):
    c = spray.RtContext(0)
    ms, sels = sh.on_device(*batch) if device else batch
    got = [as_bytes(m) for m in synced(c, c.cell_surface(ms, sels))]
    for k, ref in enumerate(restated):
        assert got[k] == ref_bytes(ref), k
    # the same batch in reversed order, without normals: the same bytes per mesh
    rev = [as_bytes(m) for m in synced(c, c.cell_surface(ms[::-1], sels[::-1], normals=False))][::-1]
    for k in range(len(ms)):
        assert rev[k] == (got[k][V], None) + got[k][COL:], k
    # twice: the same bytes
    again = [as_bytes(m) for m in synced(c, c.cell_surface(ms, sels))]
    assert again == got
    c.close()


def test_count_only_form_and_phase_times(spray, batch, restated):
    c = spray.RtContext(0)
    meshes, sels = batch
    want = [(len(r[V]), len(r[F])) for r in restated]
    assert c.cell_surface(*sh.on_device(meshes, sels), count_only=True) == want
    t = c.cell_surface_phase_times()
    assert t[0] > 0 and t[1] > 0 and t[2] == 0 and t[3] == 0    # two host reads, no emit, untimed
    assert c.cell_surface(meshes, sels, count_only=True) == want
    assert c.cell_surface([], count_only=True) == []
    # every cell of every mesh without selects
    pick = [meshes[k] for k in (sh.ONE_WEDGE, sh.SMALL)]
    assert c.cell_surface(pick, count_only=True) == [(6, 8), (125 - 27, 12 * 16)]
    c.cell_surface_phase_times(on=True)
    c.cell_surface(pick)
    t = c.cell_surface_phase_times(on=False)
    assert min(t) > 0
    c.close()


def test_short_capacities_write_nothing(spray, batch, restated):
    c = spray.RtContext(0)
    pick = (sh.ONE_HEX, sh.FULL)
    ms, sels = sh.on_device([batch[0][k] for k in pick], [batch[1][k] for k in pick])
    nv, nf = len(restated[sh.FULL][V]), len(restated[sh.FULL][F])
    counts = [(len(restated[k][V]), len(restated[k][F])) for k in pick]
    for cap in ((nv - 1, nf), (nv, nf - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.cell_surface(ms, sels, capacity=cap)
        assert e.value.code == ERR_LIMIT and "cell surface (mesh 1)" in str(e.value)
        assert e.value.counts == counts
        c.sync()
        for bufs in e.value.buffers:   # zeroed before the call: untouched
            assert all(int(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.cell_surface(ms, sels, capacity=(nv, nf)))
    assert as_bytes(got[1]) == ref_bytes(restated[sh.FULL])
    assert as_bytes(got[0]) == ref_bytes(restated[sh.ONE_HEX])
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, batch, restated):
    meshes, sels = batch
    n = len(meshes)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds = c.cell_surface_domains(list(range(n)), *sh.on_device(meshes, sels), bounds=True)
    cols = [slot_colors(m, r[COL]) for m, r in zip(meshes, restated)]
    ref_bounds = B.build_domains(list(range(n)), [r[V] for r in restated],
                                 [r[F] for r in restated], cols, [r[N] for r in restated],
                                 bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), k
        assert c.slot_info(k) == B.slot_info(k)
        assert c.slot_export(k, c.SLOT_FACES).tobytes() == restated[k][F].tobytes()
        got = c.slot_export(k, c.SLOT_COLORS)
        assert got.tobytes() == (b"" if cols[k] is None else cols[k].tobytes()), k
    assert bounds.tobytes() == ref_bounds.tobytes()
    # numpy arrays, other slots, no normals
    pick = (sh.MIXED, sh.ONE_WEDGE)
    c.cell_surface_domains([19, 18], [meshes[k] for k in pick], [sels[k] for k in pick],
                           normals=False)
    B.build_domains([19, 18], [restated[k][V] for k in pick], [restated[k][F] for k in pick],
                    [cols[k] for k in pick])
    for k in (19, 18):
        assert export_all(c, k) == export_all(B, k), k
    c.close()
    B.close()


def test_queries_equal_the_brute_force(spray, oracle, batch, restated):
    c = spray.RtContext(0)
    k = sh.PARTIAL
    c.cell_surface_domains([3], *sh.on_device([batch[0][k]], [batch[1][k]]))
    v, n, col, ids, f = restated[k]
    bh.check_queries(spray, oracle, c, 3, v, f, col, n, 77)
    c.close()


def test_refit_recolor_replace_release(spray, oracle, batch, restated):
    import torch
    meshes, sels = batch
    k = sh.PARTIAL
    v, n, col, ids, f = restated[k]
    vu, fu = rh.mesh("grid12", oracle)
    c, B = spray.RtContext(0), spray.RtContext(0)
    c.upload_domain(2, vu, fu)                               # an uploaded slot is replaced
    c.cell_surface_domains([2], *sh.on_device([meshes[k]], [sels[k]]))
    B.build_domains([2], [v], [f], [col], [n])
    assert export_all(c, 2) == export_all(B, 2)
    # a later refit
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    for rt in (c, B):
        rt.refit_domains([2], [v1], [n1])
    assert export_all(c, 2) == export_all(B, 2)
    # a recolour by another point field, gathered through point_ids on the device
    dm, ds = sh.on_device([meshes[k]], [sels[k]])
    got = synced(c, c.cell_surface(dm, ds))[0]
    assert got[IDS].cpu().numpy().view(np.uint32).tobytes() == ids.tobytes()
    field = th.busy_f(meshes[k]["points"]).astype(F32)
    cmap = (colh.table(32, 9), -0.5, 0.5)
    new = c.colormap_apply(torch.from_numpy(field).cuda()[got[IDS].long()].contiguous(), cmap)
    want = colh.colormap_numpy(field[ids], *cmap)
    assert len(np.unique(want)) > 4
    before = export_all(c, 2, KEPT)
    c.recolor_domains([2], [new])
    assert c.slot_export(2, c.SLOT_COLORS).tobytes() == want.tobytes()
    assert export_all(c, 2, KEPT) == before
    bh.check_queries(spray, oracle, c, 2, v1, f, want, n1, 78)
    # replaced by a smaller mesh, then by the empty surface, then released
    r = restated[sh.MIXED]
    c.cell_surface_domains([2], [meshes[sh.MIXED]], [sels[sh.MIXED]])
    B.build_domains([2], [r[V]], [r[F]], [r[COL]], [r[N]])
    assert export_all(c, 2) == export_all(B, 2)
    c.cell_surface_domains([2], [meshes[sh.EMPTY]], [sels[sh.EMPTY]])
    assert c.slot_info(2)["tris"] == 0
    c.release_domain(2)
    # and the context still extracts
    got = synced(c, c.cell_surface([meshes[sh.MIXED]]))
    assert as_bytes(got[0]) == ref_bytes(r)
    c.close()
    B.close()


def test_limits_of_the_batched_call(spray):
    """Rejected on the host before anything is enqueued or read."""
    import ctypes as C
    from spray_amd._native import CellMesh, lib
    c = spray.RtContext(0)
    fn = lib().spray_rt_cell_surface
    nothing = (None,) * 9

    def message():
        return lib().spray_rt_last_error(c.h).decode()

    many = (CellMesh * 65536)()   # without cells: nothing to read
    assert fn(c.h, 65536, many, None, None, *nothing) == ERR_LIMIT and "65535" in message()
    nv, nf = (C.c_size_t * 65535)(), (C.c_size_t * 65535)()
    assert fn(c.h, 65535, many, None, None, *nothing[:7], nv, nf) == 0
    assert max(nv) == max(nf) == 0
    dummy = np.zeros(16, np.uint32)
    two = (CellMesh * 2)()
    two[1].points = two[1].types = two[1].offsets = two[1].conn = dummy.ctypes.data
    two[1].npoints, two[1].ncells, two[1].nconn = 8, 2 ** 29, 8
    assert fn(c.h, 2, two, None, None, *nothing) == ERR_LIMIT
    assert "cell surface (mesh 1)" in message() and "2^29" in message()
    two[1].ncells, two[1].nconn = 1, 2 ** 32
    assert fn(c.h, 2, two, None, None, *nothing) == ERR_LIMIT and "2^32" in message()
    two[1].nconn, two[1].npoints = 8, 2 ** 21 + 1
    assert fn(c.h, 2, two, None, None, *nothing) == ERR_LIMIT and "2^21" in message()
    c.close()


def test_failed_calls_change_nothing(spray, oracle, batch, restated):
    meshes, sels = batch
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.cell_surface_domains([1], [meshes[sh.FULL]])
    before = (export_all(c, 0), export_all(c, 1))
    good = meshes[sh.MIXED]
    geom = ch.hex_lattice((17, 9, 6))
    src = sh.mesh(geom, th.wave_f, normals=True, cmap_seed=31, ntable=8)
    pts = sh.select("points", 0.3, sh.WIDE)
    cv = th.wave_f(sh.cell_centres(src)).astype(F32)
    by_cells = sh.select("cells", 0.3, sh.WIDE, cv)
    # a point of dropped cells only
    cells = src["conn"].reshape(-1, 8)
    kept = sh.kept_cells(src, pts)
    touched = np.zeros(len(src["points"]), bool)
    touched[cells[kept].reshape(-1)] = True
    quiet = np.nonzero(~touched)[0]
    assert len(quiet) > 10 and touched.any()
    used = int(quiet[len(quiet) // 2])
    assert (cells == used).any()

    def fails(bad, what, sel=pts, code=ERR_ARG):
        for ms, ss in (([good, bad], [None, sel]), sh.on_device([good, bad], [None, sel])):
            for slots in ((0, 1), (1, 0)):   # the bad mesh aimed at either loaded slot
                with pytest.raises(spray.SprayRtError) as e:
                    c.cell_surface_domains(list(slots), ms, ss)
                assert e.value.code == code and what in str(e.value)
                assert "cell surface (mesh 1, slot %d)" % slots[1] in str(e.value)
                assert (export_all(c, 0), export_all(c, 1)) == before
            with pytest.raises(spray.SprayRtError) as e:
                c.cell_surface(ms, ss)
            assert e.value.code == code and "cell surface (mesh 1)" in str(e.value)

    def poked(key, index, value):
        a = np.array(src[key], copy=True)
        a[index] = value
        return dict(src, **{key: a})

    fails(poked("types", 300, 11), "type")                              # an unknown type
    fails(poked("types", 300, ch.WEDGE), "offsets")                     # offsets against the type
    fails(poked("offsets", 301, src["offsets"][301] + 1), "offsets")
    fails(dict(src, conn=src["conn"][:-1]), "nconn")                    # offsets[i + 1] > nconn
    fails(poked("conn", 8 * 77 + 1, len(src["points"])), "index")       # an index >= npoints
    fails(poked("values", used, np.nan), "value")                       # NaNs at a dropped cell
    fails(poked("points", (used, 1), np.inf), "coordinate")
    fails(poked("normals", (used, 2), np.nan), "normal")
    fails(poked("cfield", used, np.nan), "colour")
    fails(dict(src, cmap=None), "table")
    fails(src, "cell value", dict(by_cells, cell_values=np.where(np.arange(len(cv)) == 5, np.nan, cv)
                                  .astype(F32)))
    fails(src, "mode", sh.select(3, 0.0, 1.0))
    fails(src, "bounds", sh.select("points", 1.0, 0.0))
    fails(src, "bounds", sh.select("cells", 0.0, np.inf, cv))
    fails({k: x for k, x in src.items() if k != "values"}, "values")
    fails(src, "cell_values", sh.select("cells", 0.0, 1.0))
    huge = sh.mesh((np.zeros((2 ** 21 + 1, 3), F32),) + ch.hex_lattice((4, 3, 3))[1:])
    fails(huge, "2^21", None, ERR_LIMIT)

    # an unreferenced NaN point passes: nothing reads it
    extra = dict(src, points=np.vstack([src["points"], [[np.nan] * 3]]).astype(F32),
                 values=np.append(src["values"], F32(np.nan)),
                 cfield=np.append(src["cfield"], F32(np.nan)),
                 normals=np.vstack([src["normals"], [[np.nan] * 3]]).astype(F32))
    for sel in (pts, by_cells):
        ref = ref_bytes(sh.host_surface(spray, src, sel))
        assert len(ref[F]) > 0
        for ms, ss in (([extra], [sel]), sh.on_device([extra], [sel])):
            assert as_bytes(synced(c, c.cell_surface(ms, ss))[0]) == ref
    # slots listed twice, and the good call goes through
    with pytest.raises(spray.SprayRtError) as e:
        c.cell_surface_domains([1, 1], [good, good])
    assert e.value.code == ERR_ARG and "slot 1" in str(e.value)
    assert (export_all(c, 0), export_all(c, 1)) == before
    c.cell_surface_domains([0], [good])
    assert c.slot_export(0, c.SLOT_FACES).tobytes() == restated[sh.MIXED][F].tobytes()
    assert export_all(c, 1) == before[1]
    c.close()

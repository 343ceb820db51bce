"""Clips of cell meshes by a level of their scalar field on the GPU
(spray_rt_cell_clip, spray_rt_domains_cell_clip, spray_rt_plane_values).

References, each bit for bit: the host restatement (spray_rt_cell_clip_host,
itself checked against numpy in test_cell_clip_host.py) for the extracted
arrays, a build_domains of the restated arrays in a second context for the slot
images, the oracle's brute force for queries.
"""
import numpy as np
import pytest

import build_helpers as bh
import cell_helpers as ch
import clip_helpers as clh
import color_helpers as colh
import refit_helpers as rh
import surface_helpers as sh
import tet_helpers as th

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5
WHAT = bh.WHAT + ("COLORS", "FACES")
KEPT = tuple(w for w in WHAT if w != "COLORS")
F32 = np.float32
V, N, COL, PAIRS, T, F, NCV, NCF = range(8)


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def batch():
    return clh.gpu_batch()


@pytest.fixture(scope="module")
def restated(spray, batch):
    """The eight results of every mesh from the host restatement."""
    return [clh.host_clip(spray, m, inv) for m, inv in zip(*batch)]


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
    return tuple(None if x is None else x.cpu().numpy().tobytes() for x in mesh[:NCV]) + \
        tuple(int(x) for x in mesh[NCV:])


def ref_bytes(mesh):
    return tuple(None if x is None else x.tobytes() for x in mesh[:NCV]) + tuple(mesh[NCV:])


def counts(r):
    return (len(r[V]), len(r[F]), r[NCV], r[NCF])


def test_batch_shapes(spray, batch, restated):
    """The meshes reach the paths they are there for."""
    meshes, inv = batch
    nc = [len(m["types"]) for m in meshes]
    assert nc[:4] == [1, 1, 1, 1] and [int(meshes[k]["types"][0]) for k in range(4)] == [10, 12, 13, 14]
    assert meshes[clh.HEX_TETS]["types"].tolist() == [12, 10, 10]
    assert set(meshes[clh.MIXED]["types"].tolist()) == {12, 13, 14}
    assert nc[clh.SMALL] == 64 and nc[clh.FULL] == 256             # exactly one block
    assert nc[clh.PARTIAL] == 640 and nc[clh.PARTIAL] % 256 != 0   # a partial last block
    big = meshes[clh.LARGE]
    assert nc[clh.LARGE] == 140608 and -(-nc[clh.LARGE] // 256) == 550 > 512   # past one scan stride
    assert -(-len(big["points"]) // 256) == 582 > 512
    assert nc[clh.NOCELLS] == 0 and 0 < clh.NOCELLS < len(meshes) - 1
    assert set(inv) == {True, False} and len(meshes) == 13
    for k, r in enumerate(restated):
        cap, skin = r[NCF], len(r[F]) - r[NCF]
        if k in (clh.OUTSIDE, clh.NOCELLS):
            assert cap == skin == 0 and len(r[V]) == 0, k
        elif k == clh.INSIDE:
            assert cap == 0 and skin == len(sh.host_surface(spray, meshes[k])[4]) > 0
        else:
            assert cap > 0 and skin > 0 and r[NCV] > 0 and len(r[V]) > r[NCV], k
    # about half the cells of the large mesh are cut, and both groups of
    # vertices and faces reach past the first stride of either scan
    ins = (big["values"] >= F32(big["iso"]))[big["conn"].reshape(-1, 8)]
    crossing = ins.any(1) & ~ins.all(1)
    assert 0.35 * nc[clh.LARGE] < crossing.sum() < 0.65 * nc[clh.LARGE]
    r = restated[clh.LARGE]
    own = r[PAIRS][r[NCV]:, 0]
    assert own.min() < 256 * 512 < own.max() and r[NCF] > 100000 and len(r[F]) - r[NCF] > 10000
    assert meshes[clh.SMALL]["cmap"][0].size == 1 and meshes[clh.FULL]["cmap"][0].size == 4096
    assert meshes[clh.ONE_TET].get("color") is None and meshes[clh.ONE_TET].get("cfield") is None
    assert meshes[clh.ONE_HEX]["color"] is not None
    assert {m.get("normals") is not None for m in meshes} == {True, False}


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_restatement(spray, batch, restated, device):
    c = spray.RtContext(0)
    meshes, inv = batch
    ms = ch.on_device(meshes) if device else meshes
    got = [as_bytes(m) for m in synced(c, c.cell_clip(ms, inv))]
    for k, ref in enumerate(restated):
        assert got[k] == ref_bytes(ref), k
    # the same batch in reversed order, without normals: the same bytes per mesh
    rev = [as_bytes(m) for m in synced(c, c.cell_clip(ms[::-1], inv[::-1], normals=False))][::-1]
    for k in range(len(ms)):
        assert rev[k] == (got[k][V], None) + got[k][COL:], k
    # twice: the same bytes
    again = [as_bytes(m) for m in synced(c, c.cell_clip(ms, inv))]
    assert again == got
    # no flags at all: nothing inverted
    k = clh.ONE_HEX
    plain = as_bytes(synced(c, c.cell_clip([ms[k]]))[0])
    assert plain == ref_bytes(clh.host_clip(spray, meshes[k], False))
    c.close()


def test_count_only_form_and_phase_times(spray, batch, restated):
    c = spray.RtContext(0)
    meshes, inv = batch
    want = [counts(r) for r in restated]
    assert c.cell_clip(ch.on_device(meshes), inv, count_only=True) == want
    t = c.cell_clip_phase_times()
    assert len(t) == 6 and min(t[:3]) > 0 and t[5] > 0 and t[3] == 0 and t[4] == 0   # no emit, untimed
    assert c.cell_clip(meshes, inv, count_only=True) == want
    assert c.cell_clip([], count_only=True) == []
    pick = [meshes[k] for k in (clh.ONE_WEDGE, clh.SMALL)]
    c.cell_clip_phase_times(on=True)
    c.cell_clip(pick, [True, False])
    t = c.cell_clip_phase_times(on=False)
    assert min(t) > 0
    c.close()


def test_short_capacities_write_nothing(spray, batch, restated):
    c = spray.RtContext(0)
    pick = (clh.ONE_HEX, clh.FULL)
    ms = ch.on_device([batch[0][k] for k in pick])
    inv = [batch[1][k] for k in pick]
    nv, nf = len(restated[clh.FULL][V]), len(restated[clh.FULL][F])
    want = [counts(restated[k]) for k in pick]
    for cap in ((nv - 1, nf), (nv, nf - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.cell_clip(ms, inv, capacity=cap)
        assert e.value.code == ERR_LIMIT and "cell clip (mesh 1)" in str(e.value)
        assert e.value.counts == want
        c.sync()
        for bufs in e.value.buffers:   # zeroed before the call: untouched
            assert all(float(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.cell_clip(ms, inv, capacity=(nv, nf)))
    assert as_bytes(got[1]) == ref_bytes(restated[clh.FULL])
    assert as_bytes(got[0]) == ref_bytes(restated[clh.ONE_HEX])
    c.close()


def test_plane_values(spray):
    import torch
    c = spray.RtContext(0)
    rng = np.random.default_rng(8)
    pts = (rng.normal(size=(70001, 3)) * 5).astype(F32)
    origin, normal = (0.3, -1.7, 2.9), (0.2, -0.9, 0.4)
    want = spray.plane_values_host(pts, origin, normal)
    for src in (pts, torch.from_numpy(pts).cuda()):
        got = synced(c, c.plane_values(src, origin, normal))
        assert got.cpu().numpy().tobytes() == want.tobytes()
    assert c.plane_values(np.zeros((0, 3), F32), origin, normal).numel() == 0
    for o, d in (((np.nan, 0, 0), (1, 0, 0)), ((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (np.inf, 0, 0))):
        with pytest.raises(spray.SprayRtError) as e:
            c.plane_values(pts, o, d)
        assert e.value.code == ERR_ARG and "plane values" in str(e.value)
    # a plane clip from device values: the lattice cut at x = 1.5
    m = clh.lattice_4()
    dm = ch.on_device([m])[0]
    dm["values"] = c.plane_values(dm["points"], (1.5, 0, 0), (1, 0, 0))
    got = as_bytes(synced(c, c.cell_clip([dm]))[0])
    assert got == ref_bytes(clh.host_clip(spray, m))
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, batch, restated):
    meshes, inv = batch
    n = len(meshes)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds = c.cell_clip_domains(list(range(n)), ch.on_device(meshes), inv, bounds=True)
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
    pick = (clh.MIXED, clh.ONE_WEDGE)
    c.cell_clip_domains([19, 18], [meshes[k] for k in pick], [inv[k] for k in pick], normals=False)
    B.build_domains([19, 18], [restated[k][V] for k in pick], [restated[k][F] for k in pick],
                    [cols[k] for k in pick])
    for k in (19, 18):
        assert export_all(c, k) == export_all(B, k), k
    c.close()
    B.close()


def test_queries_equal_the_brute_force(spray, oracle, batch, restated):
    c = spray.RtContext(0)
    k = clh.PARTIAL
    c.cell_clip_domains([3], ch.on_device([batch[0][k]]), [batch[1][k]])
    r = restated[k]
    bh.check_queries(spray, oracle, c, 3, r[V], r[F], r[COL], r[N], 79)
    c.close()


def test_refit_recolor_replace_release(spray, oracle, batch, restated):
    import torch
    meshes, inv = batch
    k = clh.PARTIAL
    v, n, col, pairs, t, f, ncv, ncf = restated[k]
    vu, fu = rh.mesh("grid12", oracle)
    c, B = spray.RtContext(0), spray.RtContext(0)
    c.upload_domain(2, vu, fu)                               # an uploaded slot is replaced
    c.cell_clip_domains([2], ch.on_device([meshes[k]]), [inv[k]])
    B.build_domains([2], [v], [f], [col], [n])
    assert export_all(c, 2) == export_all(B, 2)
    # a later refit
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    for rt in (c, B):
        rt.refit_domains([2], [v1], [n1])
    assert export_all(c, 2) == export_all(B, 2)
    # a recolour by another point field, gathered through vert_pairs and vert_t on the device
    got = synced(c, c.cell_clip(ch.on_device([meshes[k]]), [inv[k]]))[0]
    assert got[PAIRS].cpu().numpy().view(np.uint32).tobytes() == pairs.tobytes()
    assert got[T].cpu().numpy().tobytes() == t.tobytes()
    field = th.busy_f(meshes[k]["points"]).astype(F32)
    cmap = (colh.table(32, 9), -0.5, 0.5)
    h = torch.from_numpy(field).cuda()
    ha, hb = h[got[PAIRS][:, 0].long()], h[got[PAIRS][:, 1].long()]
    new = c.colormap_apply((ha + got[T] * (hb - ha)).contiguous(), cmap)
    a, b = pairs[:, 0], pairs[:, 1]
    g = (field[a] + (t * (field[b] - field[a]).astype(F32)).astype(F32)).astype(F32)
    want = colh.colormap_numpy(g, *cmap)
    assert len(np.unique(want)) > 4
    before = export_all(c, 2, KEPT)
    c.recolor_domains([2], [new])
    assert c.slot_export(2, c.SLOT_COLORS).tobytes() == want.tobytes()
    assert export_all(c, 2, KEPT) == before
    bh.check_queries(spray, oracle, c, 2, v1, f, want, n1, 80)
    # replaced by a smaller mesh, then by the empty clip, then released
    r = restated[clh.MIXED]
    c.cell_clip_domains([2], [meshes[clh.MIXED]], [inv[clh.MIXED]])
    B.build_domains([2], [r[V]], [r[F]], [r[COL]], [r[N]])
    assert export_all(c, 2) == export_all(B, 2)
    c.cell_clip_domains([2], [meshes[clh.OUTSIDE]], [inv[clh.OUTSIDE]])
    assert c.slot_info(2)["tris"] == 0
    c.release_domain(2)
    # and the context still extracts, the other pipelines' scratch included
    got = synced(c, c.cell_clip([meshes[clh.MIXED]], [inv[clh.MIXED]]))
    assert as_bytes(got[0]) == ref_bytes(r)
    iso = synced(c, c.cell_isosurface([meshes[clh.MIXED]]))[0]
    assert iso[0].cpu().numpy().tobytes() == r[V][:r[NCV]].tobytes()
    c.close()
    B.close()


def test_limits_of_the_batched_call(spray):
    """Rejected on the host before anything is enqueued or read."""
    import ctypes as C
    from spray_amd._native import CellMesh, lib
    c = spray.RtContext(0)
    fn = lib().spray_rt_cell_clip
    nothing = (None,) * 12

    def message():
        return lib().spray_rt_last_error(c.h).decode()

    many = (CellMesh * 65536)()   # without cells: nothing to read
    assert fn(c.h, 65536, many, None, None, *nothing) == ERR_LIMIT and "65535" in message()
    cnt = [(C.c_size_t * 65535)() for _ in range(4)]
    assert fn(c.h, 65535, many, None, None, *nothing[:8], *cnt) == 0
    assert max(max(x) for x in cnt) == 0
    dummy = np.zeros(16, np.uint32)
    two = (CellMesh * 2)()
    two[1].points = two[1].types = two[1].offsets = two[1].conn = two[1].values = dummy.ctypes.data
    two[1].npoints, two[1].ncells, two[1].nconn = 8, 2 ** 29, 8
    assert fn(c.h, 2, two, None, None, *nothing) == ERR_LIMIT
    assert "cell clip (mesh 1)" in message() and "2^29" in message()
    two[1].ncells, two[1].nconn = 1, 2 ** 32
    assert fn(c.h, 2, two, None, None, *nothing) == ERR_LIMIT and "2^32" in message()
    two[1].nconn, two[1].npoints = 8, 2 ** 21 + 1
    assert fn(c.h, 2, two, None, None, *nothing) == ERR_LIMIT and "2^21" in message()
    two[1].npoints, two[1].values = 8, None
    assert fn(c.h, 2, two, None, None, *nothing) == ERR_ARG and "values" in message()
    c.close()


def test_failed_calls_change_nothing(spray, oracle, batch, restated):
    meshes, inv = batch
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.cell_clip_domains([1], [meshes[clh.FULL]], [inv[clh.FULL]])
    before = (export_all(c, 0), export_all(c, 1))
    good = meshes[clh.MIXED]
    src = ch.mesh(ch.hex_lattice((17, 9, 6)), clh.x_minus(11.5), 0.0, normals=True, cmap_seed=31,
                  ntable=8)
    # a point of cells without a kept point only
    cells = src["conn"].reshape(-1, 8)
    part = (src["values"] >= 0)[cells].any(1)
    touched = np.zeros(len(src["points"]), bool)
    touched[cells[part].reshape(-1)] = True
    quiet = np.nonzero(~touched)[0]
    assert len(quiet) > 10 and touched.any()
    used = int(quiet[len(quiet) // 2])
    assert (cells == used).any()

    def fails(bad, what, code=ERR_ARG):
        for ms in ([good, bad], ch.on_device([good, bad])):
            for slots in ((0, 1), (1, 0)):   # the bad mesh aimed at either loaded slot
                with pytest.raises(spray.SprayRtError) as e:
                    c.cell_clip_domains(list(slots), ms, [True, False])
                assert e.value.code == code and what in str(e.value)
                assert "cell clip (mesh 1, slot %d)" % slots[1] in str(e.value)
                assert (export_all(c, 0), export_all(c, 1)) == before
            with pytest.raises(spray.SprayRtError) as e:
                c.cell_clip(ms)
            assert e.value.code == code and "cell clip (mesh 1)" in str(e.value)

    def poked(key, index, value):
        a = np.array(src[key], copy=True)
        a[index] = value
        return dict(src, **{key: a})

    fails(poked("types", 300, 11), "type")                              # an unknown type
    fails(poked("types", 300, ch.WEDGE), "offsets")                     # offsets against the type
    fails(poked("offsets", 301, src["offsets"][301] + 1), "offsets")
    fails(dict(src, conn=src["conn"][:-1]), "nconn")                    # offsets[i + 1] > nconn
    fails(poked("conn", 8 * 77 + 1, len(src["points"])), "index")       # an index >= npoints
    fails(poked("values", used, np.nan), "sample")                      # NaNs at a cell that takes no part
    fails(poked("points", (used, 1), np.inf), "coordinate")
    fails(poked("normals", (used, 2), np.nan), "normal")
    fails(poked("cfield", used, np.nan), "colour")
    fails(dict(src, cmap=None), "table")
    fails(dict(src, iso=np.nan), "isovalue")
    huge = ch.mesh((np.zeros((2 ** 21 + 1, 3), F32),) + ch.hex_lattice((4, 3, 3))[1:],
                   lambda p: np.zeros(len(p)), 0.0)
    fails(huge, "2^21", ERR_LIMIT)

    # an unreferenced NaN point passes: nothing reads it
    extra = dict(src, points=np.vstack([src["points"], [[np.nan] * 3]]).astype(F32),
                 values=np.append(src["values"], F32(np.nan)),
                 cfield=np.append(src["cfield"], F32(np.nan)),
                 normals=np.vstack([src["normals"], [[np.nan] * 3]]).astype(F32))
    ref = ref_bytes(clh.host_clip(spray, src))
    assert ref[NCF] > 0 and len(ref[F]) > 0
    for ms in ([extra], ch.on_device([extra])):
        assert as_bytes(synced(c, c.cell_clip(ms))[0]) == ref
    # slots listed twice, and the good call goes through
    with pytest.raises(spray.SprayRtError) as e:
        c.cell_clip_domains([1, 1], [good, good])
    assert e.value.code == ERR_ARG and "slot 1" in str(e.value)
    assert (export_all(c, 0), export_all(c, 1)) == before
    c.cell_clip_domains([0], [good], [inv[clh.MIXED]])
    assert c.slot_export(0, c.SLOT_FACES).tobytes() == restated[clh.MIXED][F].tobytes()
    assert export_all(c, 1) == before[1]
    c.close()

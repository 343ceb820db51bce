"""Isosurfaces of hexahedral, wedge, pyramid and tet cells on the GPU
(spray_rt_cell_isosurface, spray_rt_domains_cell_isosurface).

References, each bit for bit: the host restatement
(spray_rt_cell_isosurface_host, itself checked against numpy and against the tet
extraction in test_cell_isosurface_host.py) for the extracted arrays, a
build_domains of the restated arrays in a second context for the slot images,
the oracle's brute force for queries.
"""
import numpy as np
import pytest

import build_helpers as bh
import cell_helpers as ch
import refit_helpers as rh

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5
WHAT = bh.WHAT + ("COLORS", "FACES")
KEPT = tuple(w for w in WHAT if w != "COLORS")
F32 = np.float32


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def meshes():
    return ch.gpu_meshes()


@pytest.fixture(scope="module")
def restated(spray, meshes):
    """(verts, normals, colors, faces) of every mesh from the host restatement."""
    return [ch.host_mesh(spray, m) for m in meshes]


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


def crossing_tets(m):
    """Tets of the cells whose points are not all on one side."""
    ins = np.asarray(m["values"]) >= F32(m["iso"])
    off, conn = np.asarray(m["offsets"]).astype(np.int64), np.asarray(m["conn"])
    if len(off) < 2:
        return 0
    n = np.add.reduceat(ins[conn].astype(np.int64), off[:-1])
    lut = np.zeros(16, np.int64)
    for t, k in ch.NTETS.items():
        lut[t] = k
    return int(lut[m["types"]][(n > 0) & (n < np.diff(off))].sum())


def test_batch_shapes(meshes, restated):
    """The meshes reach the paths they are there for."""
    nc = [len(m["types"]) for m in meshes]
    assert nc[:4] == [1, 1, 1, 1] and [int(meshes[k]["types"][0]) for k in range(4)] == [10, 12, 13, 14]
    mixed = meshes[ch.MIXED]
    assert set(mixed["types"].tolist()) == {10, 12, 13, 14}
    ins = (mixed["values"] >= 0)[mixed["conn"]]
    nin = np.add.reduceat(ins.astype(int), mixed["offsets"][:-1].astype(int))
    crossed = (nin > 0) & (nin < np.diff(mixed["offsets"].astype(int)))
    assert set(mixed["types"][crossed].tolist()) == {10, 12, 13, 14}   # every type is crossed
    assert nc[ch.SMALL] == 64 and nc[ch.FULL] == 256             # exactly one block
    assert nc[ch.PARTIAL] == 640 and nc[ch.PARTIAL] % 256 != 0   # a partial last block
    assert nc[ch.LARGE] == 140608 and -(-nc[ch.LARGE] // 256) == 550 > 512   # past one scan stride
    assert nc[ch.NOCELLS] == 0 and nc[ch.EMPTY] > 0 and crossing_tets(meshes[ch.EMPTY]) == 0
    assert 0 < ch.EMPTY < ch.NOCELLS < len(meshes) - 1
    for k in range(len(meshes)):
        assert (len(restated[k][3]) > 0) == (k not in (ch.EMPTY, ch.NOCELLS)), k
    # the split leaves cells out and keeps some, in the first stride and past it
    big = meshes[ch.LARGE]
    assert 0.2 * 6 * nc[ch.LARGE] < crossing_tets(big) < 0.9 * 6 * nc[ch.LARGE]
    assert not np.array_equal(meshes[ch.SMALL]["conn"][:8], ch.hex_lattice((5, 5, 5))[3][:8])
    assert meshes[ch.SMALL]["cmap"][0].size == 1 and meshes[ch.FULL]["cmap"][0].size == 4096
    assert meshes[ch.ONE_TET].get("color") is None and meshes[ch.ONE_TET].get("cfield") is None
    assert meshes[ch.ONE_HEX]["color"] is not None
    assert {m.get("normals") is not None for m in meshes} == {True, False}
    assert len(np.unique(restated[ch.LARGE][2])) > 8


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_restatement(spray, meshes, restated, device):
    c = spray.RtContext(0)
    ms = ch.on_device(meshes) if device else meshes
    got = [as_bytes(m) for m in synced(c, c.cell_isosurface(ms))]
    for k, ref in enumerate(restated):
        assert got[k] == ref_bytes(ref), k
    # the same batch in reversed order, without normals: the same bytes per mesh
    rev = [as_bytes(m) for m in synced(c, c.cell_isosurface(ms[::-1], normals=False))][::-1]
    for k in range(len(meshes)):
        assert rev[k] == (got[k][0], None, got[k][2], got[k][3]), k
    # twice: the same bytes
    again = [as_bytes(m) for m in synced(c, c.cell_isosurface(ms))]
    assert again == got
    c.close()


def test_count_only_form_and_phase_times(spray, meshes, restated):
    c = spray.RtContext(0)
    want = [(len(r[0]), len(r[3])) for r in restated]
    assert c.cell_isosurface(ch.on_device(meshes), count_only=True) == want
    t = c.cell_phase_times()
    assert t[0] > 0 and t[1] > 0 and t[2] > 0 and t[3] == 0    # three host reads, no emit
    assert c.cell_isosurface(meshes, count_only=True) == want
    assert c.cell_isosurface([], count_only=True) == []
    c.close()


def test_short_capacities_write_nothing(spray, meshes, restated):
    c = spray.RtContext(0)
    pick = (ch.ONE_HEX, ch.FULL)
    ms = ch.on_device([meshes[k] for k in pick])
    nv, nf = len(restated[ch.FULL][0]), len(restated[ch.FULL][3])
    counts = [(len(restated[k][0]), len(restated[k][3])) for k in pick]
    for cap in ((nv - 1, nf), (nv, nf - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.cell_isosurface(ms, capacity=cap)
        assert e.value.code == ERR_LIMIT and "cell isosurface (mesh 1)" in str(e.value)
        assert e.value.counts == counts
        c.sync()
        for bufs in e.value.buffers:   # zeroed before the call: untouched
            assert all(int(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.cell_isosurface(ms, capacity=(nv, nf)))
    assert as_bytes(got[1]) == ref_bytes(restated[ch.FULL])
    assert as_bytes(got[0]) == ref_bytes(restated[ch.ONE_HEX])
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, meshes, restated):
    n = len(meshes)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds = c.cell_isosurface_domains(list(range(n)), ch.on_device(meshes), bounds=True)
    cols = [slot_colors(m, r[2]) for m, r in zip(meshes, restated)]
    ref_bounds = B.build_domains(list(range(n)), [r[0] for r in restated],
                                 [r[3] for r in restated], cols, [r[1] for r in restated],
                                 bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), k
        assert c.slot_info(k) == B.slot_info(k)
        assert c.slot_export(k, c.SLOT_FACES).tobytes() == restated[k][3].tobytes()
        got = c.slot_export(k, c.SLOT_COLORS)
        assert got.tobytes() == (b"" if cols[k] is None else cols[k].tobytes()), k
    assert bounds.tobytes() == ref_bounds.tobytes()
    # numpy arrays, other slots, no normals
    pick = (ch.MIXED, ch.ONE_WEDGE)
    c.cell_isosurface_domains([19, 18], [meshes[k] for k in pick], normals=False)
    B.build_domains([19, 18], [restated[k][0] for k in pick], [restated[k][3] for k in pick],
                    [cols[k] for k in pick])
    for k in (19, 18):
        assert export_all(c, k) == export_all(B, k), k
    c.close()
    B.close()


def test_queries_equal_the_brute_force(spray, oracle, meshes, restated):
    c = spray.RtContext(0)
    c.cell_isosurface_domains([3], ch.on_device([meshes[ch.PARTIAL]]))
    v, n, col, f = restated[ch.PARTIAL]
    bh.check_queries(spray, oracle, c, 3, v, f, col, n, 75)
    c.close()


def test_refit_recolor_replace_release(spray, oracle, meshes, restated):
    import torch
    v, n, col, f = restated[ch.PARTIAL]
    vu, fu = rh.mesh("grid12", oracle)
    c, B = spray.RtContext(0), spray.RtContext(0)
    c.upload_domain(2, vu, fu)                               # an uploaded slot is replaced
    c.cell_isosurface_domains([2], ch.on_device([meshes[ch.PARTIAL]]))
    B.build_domains([2], [v], [f], [col], [n])
    assert export_all(c, 2) == export_all(B, 2)
    # a later refit
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    for rt in (c, B):
        rt.refit_domains([2], [v1], [n1])
    assert export_all(c, 2) == export_all(B, 2)
    # a recolour
    new = rh.vertex_colors(len(v))
    before = export_all(c, 2, KEPT)
    c.recolor_domains([2], [torch.from_numpy(new.view(np.int32)).cuda()])
    assert c.slot_export(2, c.SLOT_COLORS).tobytes() == new.tobytes()
    assert export_all(c, 2, KEPT) == before
    bh.check_queries(spray, oracle, c, 2, v1, f, new, n1, 76)
    # replaced by a smaller mesh, then by the empty surface, then released
    r = restated[ch.MIXED]
    c.cell_isosurface_domains([2], [meshes[ch.MIXED]])
    B.build_domains([2], [r[0]], [r[3]], [r[2]], [r[1]])
    assert export_all(c, 2) == export_all(B, 2)
    c.cell_isosurface_domains([2], [meshes[ch.EMPTY]])
    assert c.slot_info(2)["tris"] == 0
    c.release_domain(2)
    # and the context still extracts
    got = synced(c, c.cell_isosurface([meshes[ch.MIXED]]))
    assert as_bytes(got[0]) == ref_bytes(r)
    c.close()
    B.close()


def test_failed_calls_change_nothing(spray, oracle, meshes, restated):
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.cell_isosurface_domains([1], [meshes[ch.FULL]])
    before = (export_all(c, 0), export_all(c, 1))
    good = meshes[ch.MIXED]
    src = meshes[ch.PARTIAL]
    # a point of a cell the surface does not cross, and of no crossing cell
    ins = src["values"] >= F32(src["iso"])
    cells = src["conn"].reshape(-1, 8)
    nin = ins[cells].sum(1)
    touched = np.zeros(len(ins), bool)
    touched[cells[(nin > 0) & (nin < 8)].reshape(-1)] = True
    quiet = np.nonzero(~touched)[0]
    assert len(quiet) > 10 and touched.any()
    used = int(quiet[len(quiet) // 2])
    assert (cells == used).any()

    def fails(bad, what, code=ERR_ARG):
        for ms in ([good, bad], ch.on_device([good, bad])):
            for slots in ((0, 1), (1, 0)):   # the bad mesh aimed at either loaded slot
                with pytest.raises(spray.SprayRtError) as e:
                    c.cell_isosurface_domains(list(slots), ms)
                assert e.value.code == code and what in str(e.value)
                assert "cell isosurface (mesh 1, slot %d)" % slots[1] in str(e.value)
                assert (export_all(c, 0), export_all(c, 1)) == before
            with pytest.raises(spray.SprayRtError) as e:
                c.cell_isosurface(ms)
            assert e.value.code == code and "cell isosurface (mesh 1)" in str(e.value)

    def poked(key, index, value):
        a = np.array(src[key], copy=True)
        a[index] = value
        return dict(src, **{key: a})

    fails(poked("types", 300, 11), "type")                              # an unknown type
    fails(poked("types", 300, ch.WEDGE), "offsets")                     # offsets against the type
    fails(poked("offsets", 301, src["offsets"][301] + 1), "offsets")
    fails(dict(src, conn=src["conn"][:-1]), "nconn")                    # offsets[i + 1] > nconn
    fails(poked("conn", 8 * 77 + 1, len(src["points"])), "index")       # an index >= npoints
    fails(poked("values", used, np.nan), "sample")                      # NaNs no crossing cell reads
    fails(poked("points", (used, 1), np.inf), "coordinate")
    fails(poked("normals", (used, 2), np.nan), "normal")
    mapped = ch.mesh((src["points"], src["types"], src["offsets"], src["conn"]), ch.th.wave_f, 0.3,
                     cmap_seed=31, ntable=8)
    cf = mapped["cfield"].copy()
    cf[used] = np.nan
    fails(dict(mapped, cfield=cf), "colour")
    fails(dict(mapped, cmap=None), "table")
    fails(dict(src, iso=np.nan), "isovalue")

    # an unreferenced NaN point passes: nothing reads it
    p6 = np.vstack([src["points"], [[np.nan] * 3]]).astype(F32)
    extra = dict(src, points=p6, values=np.append(src["values"], F32(np.nan)),
                 normals=np.vstack([src["normals"], [[np.nan] * 3]]).astype(F32))
    ref = ref_bytes(restated[ch.PARTIAL])
    for ms in ([extra], ch.on_device([extra])):
        assert as_bytes(synced(c, c.cell_isosurface(ms))[0]) == ref
    # slots listed twice, and the good call goes through
    with pytest.raises(spray.SprayRtError) as e:
        c.cell_isosurface_domains([1, 1], [good, good])
    assert e.value.code == ERR_ARG and "slot 1" in str(e.value)
    assert (export_all(c, 0), export_all(c, 1)) == before
    c.cell_isosurface_domains([0], [good])
    assert c.slot_export(0, c.SLOT_FACES).tobytes() == restated[ch.MIXED][3].tobytes()
    assert export_all(c, 1) == before[1]
    c.close()

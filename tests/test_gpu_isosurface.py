"""Isosurface extraction on the GPU (spray_rt_isosurface,
spray_rt_domains_isosurface).

References, each bit for bit: the host restatement (spray_rt_isosurface_host)
for the extracted arrays, a build_domains of those arrays in a second context
for the slot images, the oracle's brute force for queries, and an upload of
the same meshes for the scene launches.
"""
import ctypes as C

import numpy as np
import pytest

import build_helpers as bh
import iso_helpers as ih
import refit_helpers as rh

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5
SPHERE, TORUS, WAVELET, EMPTY = 2, 3, 5, 6


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def grids():
    return ih.gpu_grids()


@pytest.fixture(scope="module")
def restated(spray, grids):
    """(verts, normals, faces, colors) of every grid from the host restatement."""
    out = []
    for g in grids:
        v, n, f = spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"])
        col = None if g["color"] is None else np.full(len(v), g["color"], np.uint32)
        out.append((v, n, f, col))
    return out


def on_device(grids):
    import torch
    return [dict(g, values=torch.from_numpy(g["values"]).cuda()) for g in grids]


def as_bytes(mesh):
    v, n, f = mesh
    return (v.cpu().numpy().tobytes(), None if n is None else n.cpu().numpy().tobytes(),
            f.cpu().numpy().tobytes())


def test_batch_shapes(grids, restated):
    """The grids reach the paths they are there for."""
    assert grids[0]["values"].shape == (2, 2, 2) and len(restated[0][2]) > 0
    assert grids[4]["values"].size > 4 * 256                  # several blocks of points
    assert grids[WAVELET]["values"].size > 512 * 256          # more blocks than one scan stride
    assert len(restated[WAVELET][2]) > 10000
    assert len(restated[EMPTY][0]) == 0 and len(restated[EMPTY][2]) == 0


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_restatement(spray, grids, restated, device):
    c = spray.RtContext(0)
    gs = on_device(grids) if device else grids
    got = [as_bytes(m) for m in c.isosurface(gs)]
    for k, (v, n, f, _) in enumerate(restated):
        assert got[k] == (v.tobytes(), n.tobytes(), f.tobytes()), k
    # the same batch in reversed order, without normals: the same bytes per grid
    rev = [as_bytes(m) for m in c.isosurface(gs[::-1], normals=False)][::-1]
    for k in range(len(grids)):
        assert rev[k] == (got[k][0], None, got[k][2]), k
    c.close()


def test_count_only_form_and_short_capacity(spray, grids, restated):
    from spray_amd import _native, engine
    c = spray.RtContext(0)
    gs = on_device(grids)
    n = len(gs)
    arr, keep = engine._grid_table(gs)
    nv, nf = (C.c_size_t * n)(), (C.c_size_t * n)()
    rc = _native.lib().spray_rt_isosurface(c.h, n, arr, None, None, None, None, None, nv, nf)
    assert rc == 0
    assert [(nv[k], nf[k]) for k in range(n)] == [(len(r[0]), len(r[2])) for r in restated]
    v, _, f, _ = restated[TORUS]
    for cap in ((len(v) - 1, len(f)), (len(v), len(f) - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.isosurface([gs[SPHERE], gs[TORUS]], capacity=cap)
        assert e.value.code == ERR_LIMIT and "grid 1" in str(e.value)
        assert e.value.counts == [(len(restated[k][0]), len(restated[k][2]))
                                  for k in (SPHERE, TORUS)]
        c.sync()
        for bufs in e.value.buffers:   # zeroed before the call: untouched
            assert all(int(b.abs().max()) == 0 for b in bufs)
    # the exact capacity fits
    got = c.isosurface([gs[TORUS]], capacity=(len(v), len(f)))
    assert as_bytes(got[0])[0] == v.tobytes()
    c.close()


@pytest.fixture(scope="module")
def slots(spray, grids):
    """Slot k = the isosurface of grid k, all extracted and built in one call."""
    c = spray.RtContext(0)
    dev = on_device(grids)
    bounds = c.isosurface_domains(list(range(len(grids))), dev, bounds=True)
    yield c, bounds
    c.close()


def test_slot_images_equal_a_build_of_the_extracted_arrays(spray, grids, restated, slots):
    c, bounds = slots
    n = len(grids)
    B = spray.RtContext(0)
    cols = [[r[k] for r in restated] for k in (0, 2, 3, 1)]  # verts, faces, colors, normals
    ref_bounds = B.build_domains(list(range(n)), *cols, bounds=True)
    for k in range(n):
        assert bh.export_all(c, k) == bh.export_all(B, k), k
        assert c.slot_info(k) == B.slot_info(k)
        assert c.slot_info(k)["tris"] == len(restated[k][2])
        if len(restated[k][0]):
            v = restated[k][0]
            assert bounds[k].tobytes() == np.concatenate([v.min(0), v.max(0)]).tobytes()
    assert bounds.tobytes() == ref_bounds.tobytes()
    assert c.slot_info(EMPTY) == {"nodes": 0, "depth": 0, "tris": 0}
    # numpy fields, other slots, no normals: a build without them
    c2 = spray.RtContext(0)
    c2.isosurface_domains([7, 3], [grids[TORUS], grids[SPHERE]], normals=False)
    B.build_domains([7, 3], [restated[TORUS][0], restated[SPHERE][0]],
                    [restated[TORUS][2], restated[SPHERE][2]],
                    [restated[TORUS][3], restated[SPHERE][3]])
    for k in (7, 3):
        assert bh.export_all(c2, k) == bh.export_all(B, k), k
    c2.close()
    B.close()


@pytest.mark.parametrize("k", [SPHERE, TORUS], ids=["sphere", "torus"])
def test_queries_match_the_oracle(spray, oracle, restated, slots, k):
    v, n, f, col = restated[k]
    bh.check_queries(spray, oracle, slots[0], k, v, f, col, n, 500 + k)


def test_scene_launches_equal_uploaded_slots(spray, oracle, grids):
    ga = grids[SPHERE]
    gb = dict(grids[TORUS], origin=(9.0, -4.0, -5.0))  # beside the sphere
    doms = []
    for g in (ga, gb):
        v, n, f = spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"])
        doms.append((v, f, np.full(len(v), g["color"], np.uint32), n))
    A, B = spray.RtContext(0), spray.RtContext(0)
    dev = on_device([ga, gb])
    bounds = A.isosurface_domains([0, 1], dev, bounds=True)
    for i, d in enumerate(doms):
        B.upload_domain(i, *d)
        assert bounds[i].tobytes() == np.concatenate([d[0].min(0), d[0].max(0)]).tobytes()
    for rt in (A, B):
        rt.domain_bounds(bounds)
        for i in range(2):
            rt.map_domain(i, i)
    allv = np.concatenate([doms[0][0], doms[1][0]])
    allf = np.concatenate([doms[0][1], doms[1][1] + len(doms[0][0])]).astype(np.uint32)
    org, d = rh.refit_rays(np.random.default_rng(5), allv, allf)
    rays = spray.make_rays(org, d)
    cam = oracle.camera_init([10.0, 10.0, 40.0], [10.0, 4.0, 3.0], [0, 1, 0], 60, 64, 64)
    eo, ed, pix, _ = oracle.eye_rays_ooc(cam, 64, 1, (0, 0, 64, 64))
    eye = spray.make_rays(eo, ed)
    ra = bh.scene_results(spray, A, rays, eye, pix)
    rb = bh.scene_results(spray, B, rays, eye, pix)
    # not vacuous: hits in both domains and both occlusion outcomes
    hits = np.frombuffer(ra["intersect_scene"], spray.HIT_DTYPE)
    assert set(np.unique(hits["domain"])) >= {-1, 0, 1}
    occ = np.frombuffer(ra["occluded_scene_2"], np.uint8)
    assert 0 < occ.mean() < 1
    for k in ra:
        assert ra[k] == rb[k], k
    A.close()
    B.close()


def test_refit_replacement_and_release(spray, oracle, grids, restated):
    v, n, f, col = restated[TORUS]
    vs, ns, fs, cs = restated[SPHERE]
    c = spray.RtContext(0)
    c.isosurface_domains([3], [grids[TORUS]])
    built = bh.export_all(c, 3)
    # a later refit of the extracted slot, and back
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    c.refit_domains([3], [v1], [n1])
    bh.check_queries(spray, oracle, c, 3, v1, f, col, n1, 41)
    c.refit_domains([3], [v], [n])
    assert bh.export_all(c, 3) == built
    # replacement of loaded slots: the larger image's memory is reused, the smaller grows
    c.upload_domain(1, vs, fs, cs, ns)
    dev = on_device([grids[SPHERE], grids[TORUS]])
    c.isosurface_domains([3, 1], dev)
    B = spray.RtContext(0)
    B.build_domains([3, 1], [vs, v], [fs, f], [cs, col], [ns, n])
    for k in (3, 1):
        assert bh.export_all(c, k) == bh.export_all(B, k)
    bh.check_queries(spray, oracle, c, 1, v, f, col, n, 42)
    c.release_domain(3)
    with pytest.raises(spray.SprayRtError):
        c.slot_info(3)
    bh.check_queries(spray, oracle, c, 1, v, f, col, n, 43)
    # an empty surface into a loaded slot: the empty slot
    c.isosurface_domains([1], [grids[EMPTY]])
    assert c.slot_info(1) == {"nodes": 0, "depth": 0, "tris": 0}
    c.release_domain(1)
    B.close()
    c.close()


def test_failed_call_changes_nothing(spray, oracle, grids, restated):
    va, fa = rh.mesh("grid12", oracle)
    ca, na = rh.vertex_colors(len(va)), rh.vertex_normals(oracle, va, fa)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa, ca, na)
    c.isosurface_domains([1], [grids[SPHERE]])
    before = (bh.export_all(c, 0), bh.export_all(c, 1))
    good = grids[TORUS]

    def fails(code, slots, gs, names):
        with pytest.raises(spray.SprayRtError) as e:
            c.isosurface_domains(slots, gs)
        assert e.value.code == code
        assert "grid %d" % names in str(e.value)
        assert (bh.export_all(c, 0), bh.export_all(c, 1)) == before
        assert c.slot_info(0)["tris"] == len(fa)
        assert c.slot_info(1)["tris"] == len(restated[SPHERE][2])

    nan = good["values"].copy()
    nan[9, 3, 11] = np.nan
    for tgt in (0, 1):  # the bad grid aimed at either loaded slot, second in the call
        fails(ERR_ARG, [1 - tgt, tgt], [good, dict(good, values=nan)], 1)
        fails(ERR_ARG, [1 - tgt, tgt], on_device([good, dict(good, values=nan)]), 1)
    fails(ERR_ARG, [1, 1], [good, good], 1)                                  # a slot listed twice
    fails(ERR_ARG, [0, 1], [good, dict(good, values=good["values"][:, :, :1])], 1)  # dims < 2
    fails(ERR_ARG, [0, 1], [good, dict(good, spacing=(1.0, -1.0, 1.0))], 1)
    # an unquantizable box: coordinates near the largest float
    big = np.finfo(np.float32).max
    fails(ERR_LIMIT, [0, 1], [good, dict(good, origin=(big, big, big))], 1)
    # into a new slot as well: it stays unloaded
    fails(ERR_ARG, [5, 1], [good, dict(good, values=nan)], 1)
    with pytest.raises(spray.SprayRtError):
        c.slot_info(5)
    bh.check_queries(spray, oracle, c, 1, *[restated[SPHERE][k] for k in (0, 2, 3, 1)], 7)
    c.close()

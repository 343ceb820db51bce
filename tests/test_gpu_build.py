"""Device build of slots (spray_rt_domains_build) on the GPU.

Three references, each bit for bit: the host restatement
(spray_rt_bvh_build_device_host) for the slot image, the oracle's brute force
for queries, and an upload of the same meshes in a second context for the
scene launches (results do not depend on the tree).
"""
import numpy as np
import pytest

import build_helpers as bh
import refit_helpers as rh

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def meshes(oracle):
    """name -> (verts, faces, colors, normals)."""
    out = {}
    for m in bh.MESHES:
        v, f = bh.mesh(m, oracle)
        out[m] = (v, f, rh.vertex_colors(len(v)), rh.vertex_normals(oracle, v, f))
    return out


@pytest.fixture(scope="module")
def restated(meshes):
    return {m: bh.build_device_host(meshes[m][0], meshes[m][1]) for m in bh.MESHES}


def to_dev(x):
    """numpy -> GPU tensor (uint32 arrays travel as their int32 bits)."""
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def build_all(spray, meshes, device):
    """One context, slot k = mesh k of bh.MESHES, all built in one call."""
    c = spray.RtContext(0)
    cols = [[meshes[m][k] for m in bh.MESHES] for k in range(4)]
    if device:
        cols = [[to_dev(x) for x in col] for col in cols]
    bounds = c.build_domains(list(range(len(bh.MESHES))), *cols, bounds=True)
    return c, cols, bounds


@pytest.fixture(scope="module")
def ctx(spray, meshes):
    c, keep, bounds = build_all(spray, meshes, device=True)
    yield c
    c.close()


def assert_image(c, slot, want, normals):
    got = bh.export_all(c, slot)
    assert got["NODES"] == want["nodes"].tobytes()
    assert got["TRIS"] == want["tris"].tobytes()
    assert got["PRIMS"] == want["prims"].tobytes()
    assert got["QNODES4"] == want["qnodes4"].tobytes()
    assert got["QGRID"] == want["grid"].tobytes()
    assert got["NORMALS"] == normals.tobytes()
    info = c.slot_info(slot)
    assert info == {"nodes": len(want["nodes"]), "depth": want["depth"], "tris": len(want["prims"])}
    return got


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_slot_images_equal_the_host_restatement(spray, meshes, restated, device):
    c, cols, bounds = build_all(spray, meshes, device)
    first = []
    for k, m in enumerate(bh.MESHES):
        v, f, _, n = meshes[m]
        first.append(assert_image(c, k, restated[m], n))
        ref = v[np.unique(f)]
        assert bounds[k].tobytes() == np.concatenate([ref.min(0), ref.max(0)]).tobytes()
    # a second build, into the loaded slots and in another order: the same bytes
    order = list(range(len(bh.MESHES)))[::-1]
    c.build_domains(order, *[[col[k] for k in order] for col in cols])
    for k in range(len(bh.MESHES)):
        assert bh.export_all(c, k) == first[k]
    c.close()


@pytest.mark.parametrize("m", bh.MESHES)
def test_queries_match_the_oracle(spray, oracle, meshes, ctx, m):
    k = bh.MESHES.index(m)
    v, f, col, n = meshes[m]
    bh.check_queries(spray, oracle, ctx, k, v, f, col, n, 300 + k)


def test_scene_launches_equal_uploaded_slots(spray, oracle, meshes):
    va, fa, ca, na = meshes["wavelet0"]
    vb, fb, cb, _ = meshes["grid12"]
    vb = (vb + np.array([5.0, 0.0, 0.0], np.float32)).astype(np.float32)  # beside wavelet0
    nb = rh.vertex_normals(oracle, vb, fb)
    doms = [(va, fa, ca, na), (vb, fb, cb, nb)]
    A, B = spray.RtContext(0), spray.RtContext(0)
    dev = [[to_dev(d[k]) for d in doms] for k in range(4)]
    bounds = A.build_domains([0, 1], *dev, bounds=True)
    for i, d in enumerate(doms):
        B.upload_domain(i, *d)
        ref = d[0][np.unique(d[1])]
        assert bounds[i].tobytes() == np.concatenate([ref.min(0), ref.max(0)]).tobytes()
    for rt in (A, B):
        rt.domain_bounds(bounds)
        for i in range(2):
            rt.map_domain(i, i)
    allv = np.concatenate([va, vb])
    allf = np.concatenate([fa, fb + len(va)]).astype(np.uint32)
    org, d = rh.refit_rays(np.random.default_rng(5), allv, allf)
    rays = spray.make_rays(org, d)
    cam = oracle.camera_init([-5.0, 10.0, 25.0], [1.0, 0.0, 0.0], [0, 1, 0], 60, 64, 64)
    eo, ed, pix, _ = oracle.eye_rays_ooc(cam, 64, 1, (0, 0, 64, 64))
    eye = spray.make_rays(eo, ed)
    ra = bh.scene_results(spray, A, rays, eye, pix)
    rb = bh.scene_results(spray, B, rays, eye, pix)
    # not vacuous: hits in both domains, shadow rays, AO rays, both occlusion outcomes
    hits = np.frombuffer(ra["intersect_scene"], spray.HIT_DTYPE)
    assert set(np.unique(hits["domain"])) >= {-1, 0, 1}
    assert ra["shadow_pt"][3] > 0 and ra["ao"][1] > 0
    occ = np.frombuffer(ra["occluded_scene_2"], np.uint8)
    assert 0 < occ.mean() < 1
    for k in ra:
        assert ra[k] == rb[k], k
    A.close()
    B.close()


@pytest.mark.parametrize("m", ["tri1", "grid12", "wavelet0", "stairs"])
def test_refit_of_a_built_slot(spray, oracle, meshes, restated, m):
    v, f, col, n = meshes[m]
    c = spray.RtContext(0)
    c.build_domains([3], [v], [f], [col], [n])
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    c.refit_domains([3], [v1], [n1])
    got = bh.export_all(c, 3)
    b = restated[m]
    nodes = np.frombuffer(got["NODES"], rh.NODE_DTYPE)
    for k in ("left", "right"):  # topology kept
        assert np.array_equal(nodes[k], b["nodes"][k])
    assert got["PRIMS"] == b["prims"].tobytes()
    with np.errstate(invalid="ignore"):
        plo, phi, _ = rh.expected_boxes(b["nodes"], b["prims"], f, v1)
    assert np.stack([nodes["l_lo"], nodes["r_lo"]], 1).tobytes() == plo.tobytes()
    assert np.stack([nodes["l_hi"], nodes["r_hi"]], 1).tobytes() == phi.tobytes()
    assert got["TRIS"] == rh.expected_tris(b["prims"], f, v1).tobytes()
    assert got["NORMALS"] == n1.tobytes()
    q4 = np.frombuffer(got["QNODES4"], rh.QNODE4_DTYPE)
    assert np.array_equal(q4["child"], b["qnodes4"]["child"])
    bh.check_queries(spray, oracle, c, 3, v1, f, col, n1, 41)
    # and back: the built image again
    c.refit_domains([3], [v], [n])
    assert_image(c, 3, b, n)
    c.close()


def test_build_replaces_an_uploaded_slot_and_release_works(spray, oracle, meshes, restated):
    va, fa, ca, na = meshes["wavelet0"]
    vb, fb, cb, nb = meshes["tri5"]
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa, ca, na)   # the larger image first: its memory is reused
    c.upload_domain(1, vb, fb, cb, nb)   # the smaller: the build allocates
    c.build_domains([0, 1], [vb, va], [fb, fa], [cb, ca], [nb, na])
    assert_image(c, 0, restated["tri5"], nb)
    assert_image(c, 1, restated["wavelet0"], na)
    bh.check_queries(spray, oracle, c, 1, va, fa, ca, na, 9)
    c.release_domain(0)
    with pytest.raises(spray.SprayRtError):
        c.slot_info(0)
    bh.check_queries(spray, oracle, c, 1, va, fa, ca, na, 10)
    # an empty mesh: the empty slot an upload gives
    c.build_domains([0], [va[:0]], [fa[:0]])
    assert c.slot_info(0) == {"nodes": 0, "depth": 0, "tris": 0}
    c.release_domain(0)
    c.release_domain(1)
    c.close()


def test_failed_build_changes_nothing(spray, oracle, meshes):
    va, fa, ca, na = meshes["grid12"]
    vb, fb, cb, nb = meshes["tri5"]
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa, ca, na)
    c.build_domains([1], [vb], [fb], [cb], [nb])
    before = (bh.export_all(c, 0), bh.export_all(c, 1))
    v2, f2, c2, n2 = meshes["dups"]

    def unchanged():
        assert (bh.export_all(c, 0), bh.export_all(c, 1)) == before
        assert c.slot_info(0)["tris"] == len(fa) and c.slot_info(1)["tris"] == len(fb)
        bh.check_queries(spray, oracle, c, 0, va, fa, ca, na, 7)

    def fails(code, slots, v, f, col, n, names=None):
        with pytest.raises(spray.SprayRtError) as e:
            c.build_domains(slots, v, f, col, n)
        assert e.value.code == code
        if names is not None:
            assert "slot %d" % names in str(e.value)

    # a face index >= nverts in the SECOND slot of the call
    bad = f2.copy()
    bad[3, 1] = len(v2)
    for tgt in (0, 1):  # the bad mesh aimed at either loaded slot; the other is rebuilt validly
        other = 1 - tgt
        good = (va, fa, ca, na) if other == 0 else (vb, fb, cb, nb)
        fails(ERR_ARG, [other, tgt], [good[0], v2], [good[1], bad], [good[2], c2], [good[3], n2], tgt)
        unchanged()
    # a NaN in a referenced vertex
    nan = v2.copy()
    nan[f2[2, 1], 1] = np.nan
    fails(ERR_ARG, [0, 1], [va, nan], [fa, f2], [ca, c2], [na, n2], 1)
    unchanged()
    # a slot listed twice
    fails(ERR_ARG, [1, 1], [vb, v2], [fb, f2], [cb, c2], [nb, n2])
    unchanged()
    # coordinates near 3e38 (the largest float): finite vertices and edges, but the
    # padded boxes overflow and no grid holds them
    huge = np.full_like(v2, np.finfo(np.float32).max)
    fails(ERR_LIMIT, [0, 1], [va, huge], [fa, f2], [ca, c2], [na, n2], 1)
    unchanged()
    # into a new slot as well: it stays unloaded
    fails(ERR_ARG, [5, 1], [vb, nan], [fb, f2], [cb, c2], [nb, n2], 1)
    with pytest.raises(spray.SprayRtError):
        c.slot_info(5)
    unchanged()
    c.close()


def test_nan_in_unreferenced_vertex_is_accepted(spray, oracle, meshes, restated):
    v, f, _, _ = meshes["grid12"]
    v2 = np.concatenate([v, [[np.nan, 5.0, 5.0]]]).astype(np.float32)
    col2 = rh.vertex_colors(len(v2))
    n2 = rh.vertex_normals(oracle, v2, f)
    c = spray.RtContext(0)
    b = c.build_domains([0], [v2], [f], [col2], [n2], bounds=True)
    ref = v2[np.unique(f)]
    assert b[0].tobytes() == np.concatenate([ref.min(0), ref.max(0)]).tobytes()
    assert bh.export_all(c, 0)["NODES"] == restated["grid12"]["nodes"].tobytes()
    finite = v2.copy()
    finite[-1] = finite[0]
    bh.check_queries(spray, oracle, c, 0, v2, f, col2, n2, 11, ray_verts=finite)
    c.close()

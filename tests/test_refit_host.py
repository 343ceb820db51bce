"""Host restatement of the device refit (spray_rt_bvh_refit_host, no GPU).

The refit keeps the topology of the canonical build and recomputes boxes,
triangle records, the grid and the QNode4 child boxes from new vertices with
the builder's arithmetic.  Checked here against the build itself (identity)
and against independent numpy restatements (every deformation); the GPU
tests then hold the kernels to this function byte for byte.

The oracle's BVH walk builds its own tree and cannot be pointed at foreign
nodes, so closest hits over refitted trees are checked on the GPU only
(test_gpu_refit.py).
"""
import numpy as np
import pytest

import refit_helpers as rh


@pytest.fixture(scope="module")
def meshes(oracle):
    return {m: rh.mesh(m, oracle) for m in rh.MESHES}


@pytest.fixture(scope="module")
def built(meshes):
    return {m: rh.build_host(*meshes[m]) for m in rh.MESHES}


def test_mesh_shapes(built):
    """The meshes reach the paths they are there for."""
    n1 = built["tri1"]["nodes"]
    assert len(n1) == 1 and n1["r_lo"][0, 0] == np.inf and n1["left"][0] < 0
    assert len(built["tri4"]["nodes"]) == 1
    assert len(built["tri5"]["nodes"]) >= 1 and (built["tri5"]["nodes"]["left"] < 0).any()
    assert len(built["grid12"]["tris"]) == 288 and len(built["grid12"]["nodes"]) > 32
    assert len(built["grid12"]["qnodes4"]) > 8
    assert len(built["wavelet0"]["nodes"]) > 256  # more nodes than one workgroup has threads


@pytest.mark.parametrize("m", rh.MESHES)
def test_identity_refit_reproduces_the_build(meshes, built, m):
    v, f = meshes[m]
    r = rh.refit_host(v, v, f)
    b = built[m]
    for k in ("nodes", "tris", "grid", "qnodes4"):
        assert r[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("d", rh.DEFORMS)
@pytest.mark.parametrize("m", rh.MESHES)
def test_refit_matches_numpy_restatement(meshes, built, m, d):
    v, f = meshes[m]
    b = built[m]
    v1 = rh.deform(d, v)
    r = rh.refit_host(v, v1, f)
    nodes, q4 = r["nodes"], r["qnodes4"]
    # topology kept
    for k in ("left", "right", "pad"):
        assert np.array_equal(nodes[k], b["nodes"][k]), k
    assert np.array_equal(q4["child"], b["qnodes4"]["child"])
    # boxes: pad(exact min/max of the subtree's new vertices)
    with np.errstate(invalid="ignore"):
        plo, phi, rng = rh.expected_boxes(b["nodes"], b["prims"], f, v1)
    got_lo = np.stack([nodes["l_lo"], nodes["r_lo"]], 1)
    got_hi = np.stack([nodes["l_hi"], nodes["r_hi"]], 1)
    assert got_lo.tobytes() == plo.tobytes()
    assert got_hi.tobytes() == phi.tobytes()
    # triangle records
    assert r["tris"].tobytes() == rh.expected_tris(b["prims"], f, v1).tobytes()
    # every decoded QNode4 child box holds its source padded box with a whole
    # grid step to spare on both sides; empty children stay 0xFFFF
    key = {(int(rng[i, s, 0]), int(rng[i, s, 1])): (i, s)
           for i in range(len(nodes)) for s in range(2) if rng[i, s, 0] >= 0}
    qr = rh.q4_child_ranges(q4)
    scale = r["grid"][3:].astype(np.float64)
    assert (r["grid"][3:] > 0).all() and np.isfinite(r["grid"]).all()
    nchild = 0
    for i in range(len(q4)):
        for c in range(4):
            if qr[i, c, 0] < 0:
                assert (q4["q"][i, c] == 0xFFFF).all()
                continue
            ni, s = key[(int(qr[i, c, 0]), int(qr[i, c, 1]))]
            dlo = rh.decode_q(r["grid"], q4["q"][i, c, :3])
            dhi = rh.decode_q(r["grid"], q4["q"][i, c, 3:])
            assert (dlo + scale <= plo[ni, s].astype(np.float64)).all(), (i, c)
            assert (dhi - scale >= phi[ni, s].astype(np.float64)).all(), (i, c)
            nchild += 1
    assert nchild >= 1


def test_refit_rejects_what_an_upload_rejects(meshes):
    import spray_amd
    v, f = meshes["grid12"]
    bad = v.copy()
    bad[f[7, 1], 2] = np.nan
    with pytest.raises(spray_amd.SprayRtError) as e:
        spray_amd.bvh_refit_host(v, bad, f)
    assert e.value.code == -1  # SPRAY_RT_ERR_ARG
    # an unreferenced vertex may hold anything
    v2 = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    r = spray_amd.bvh_refit_host(v2, v2, f)
    assert np.isfinite(r["tris"]).all()
    # finite vertices and edges, but the padded boxes overflow: no grid holds them
    huge = np.full_like(v, np.finfo(np.float32).max)
    with pytest.raises(spray_amd.SprayRtError) as e:
        spray_amd.bvh_refit_host(v, huge, f)
    assert e.value.code == -5  # SPRAY_RT_ERR_LIMIT

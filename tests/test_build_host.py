"""Host restatement of the device build (spray_rt_bvh_build_device_host, no GPU).

The device build sorts the triangles by (Morton code of the box centroid,
face), splits ranges of the sorted order level by level and numbers nodes and
QNode4s in range order; boxes, records, grid and quantization are the refit's.
Checked here structurally and against independent numpy restatements; the GPU
tests then hold the kernels to this function byte for byte.
"""
import numpy as np
import pytest

import build_helpers as bh
import refit_helpers as rh


@pytest.fixture(scope="module")
def meshes(oracle):
    return {m: bh.mesh(m, oracle) for m in bh.MESHES}


@pytest.fixture(scope="module")
def built(meshes):
    return {m: bh.build_device_host(*meshes[m]) for m in bh.MESHES}


def test_mesh_shapes(meshes, built):
    """The meshes reach the paths they are there for."""
    n1 = built["tri1"]["nodes"]
    assert len(n1) == 1 and n1["r_lo"][0, 0] == np.inf and n1["left"][0] < 0
    assert n1["right"][0] == -1 and built["tri1"]["depth"] == 1
    assert len(built["tri4"]["nodes"]) == 1
    assert len(built["tri5"]["nodes"]) >= 1 and (built["tri5"]["nodes"]["left"] < 0).any()
    assert len(built["grid12"]["tris"]) == 288 and len(built["grid12"]["nodes"]) > 32
    # more nodes in all than one workgroup has threads; no BFS level is wider than
    # about 100 (levels beyond 512: build_cases.py)
    assert len(built["wavelet0"]["nodes"]) > 512
    # stairs: codes 2^k, k = 0..29, five zeros and the far corner
    v, f = meshes["stairs"]
    codes = np.sort(bh.sort_keys(v, f) >> np.uint64(32))
    want = np.array([0] * 5 + [1 << k for k in range(30)] + [(1 << 30) - 1], np.uint64)
    assert np.array_equal(codes, want)
    # ... so the bit splits alone would be 30 levels deep: the depth rule cuts in
    assert built["stairs"]["nmedian"] > 0 and built["stairs"]["depth"] <= bh.KMAXDEPTH
    assert built["stairs"]["depth"] > 20
    # dups: one code; no split is forced by the depth
    v, f = meshes["dups"]
    assert len(np.unique(bh.sort_keys(v, f) >> np.uint64(32))) == 1
    assert built["dups"]["nmedian"] == 0 and len(built["dups"]["nodes"]) > 8
    for m in rh.MESHES:
        assert built[m]["nmedian"] == 0, m


@pytest.mark.parametrize("m", bh.MESHES)
def test_order_is_the_sorted_key(meshes, built, m):
    v, f = meshes[m]
    b = built[m]
    assert np.array_equal(np.sort(b["prims"]), np.arange(len(f)))
    keys = bh.sort_keys(v, f)
    assert len(np.unique(keys)) == len(keys)
    assert np.array_equal(b["prims"], np.argsort(keys, kind="stable").astype(np.uint32))


@pytest.mark.parametrize("m", bh.MESHES)
def test_tree_structure(meshes, built, m):
    v, f = meshes[m]
    b = built[m]
    nodes = b["nodes"]
    nn = len(nodes)
    covered = np.zeros(len(f), np.int64)
    seen = np.zeros(nn, np.int64)
    seen[0] = 1
    for i in range(nn):
        for kl, kr in (("l_lo", "left"), ("r_lo", "right")):
            if nodes[kl][i, 0] == np.inf:
                assert nn == 1 and kr == "right"
                continue
            ref = int(nodes[kr][i])
            if ref < 0:
                first, cnt = rh._leaf(ref)
                assert 1 <= cnt <= bh.KLEAFMAX and first + cnt <= len(f)
                covered[first:first + cnt] += 1
            else:
                assert i < ref < nn
                seen[ref] += 1
    assert (covered == 1).all() and (seen == 1).all()
    assert (nodes["pad"] == 0).all()
    # depth: the deepest leaf, root range at depth 0
    depth = np.zeros(nn, np.int64)
    deepest = 0
    for i in range(nn):
        for kr in ("left", "right"):
            ref = int(nodes[kr][i])
            if ref >= 0:
                depth[ref] = depth[i] + 1
        deepest = max(deepest, depth[i] + 1)
    assert b["depth"] == deepest <= bh.KMAXDEPTH
    # breadth first: node depths never decrease with the index
    assert (np.diff(depth) >= 0).all()


@pytest.mark.parametrize("m", bh.MESHES)
def test_boxes_records_and_quantization(meshes, built, m):
    v, f = meshes[m]
    b = built[m]
    nodes, q4 = b["nodes"], b["qnodes4"]
    with np.errstate(invalid="ignore"):  # the never-hit box of a one-leaf root
        plo, phi, rng = rh.expected_boxes(nodes, b["prims"], f, v)
    assert np.stack([nodes["l_lo"], nodes["r_lo"]], 1).tobytes() == plo.tobytes()
    assert np.stack([nodes["l_hi"], nodes["r_hi"]], 1).tobytes() == phi.tobytes()
    assert b["tris"].tobytes() == rh.expected_tris(b["prims"], f, v).tobytes()
    # QNode4s: children after parents, their leaves tile the triangles, every
    # decoded box holds its source padded box with a grid step to spare
    assert 0 <= b["stack_bound"] <= bh.KQ4STACK
    key = {(int(rng[i, s, 0]), int(rng[i, s, 1])): (i, s)
           for i in range(len(nodes)) for s in range(2) if rng[i, s, 0] >= 0}
    qr = rh.q4_child_ranges(q4)
    scale = b["grid"][3:].astype(np.float64)
    assert (b["grid"][3:] > 0).all() and np.isfinite(b["grid"]).all()
    covered = np.zeros(len(f), np.int64)
    seen = np.zeros(len(q4), np.int64)
    seen[0] = 1
    for i in range(len(q4)):
        for c in range(4):
            ref = int(q4["child"][i, c])
            if ref == rh.KNOCHILD:
                assert (q4["q"][i, c] == 0xFFFF).all()
                continue
            if ref < 0:
                first, cnt = rh._leaf(ref)
                covered[first:first + cnt] += 1
            else:
                assert i < ref < len(q4)
                seen[ref] += 1
            ni, s = key[(int(qr[i, c, 0]), int(qr[i, c, 1]))]
            dlo = rh.decode_q(b["grid"], q4["q"][i, c, :3])
            dhi = rh.decode_q(b["grid"], q4["q"][i, c, 3:])
            assert (dlo + scale <= plo[ni, s].astype(np.float64)).all(), (i, c)
            assert (dhi - scale >= phi[ni, s].astype(np.float64)).all(), (i, c)
    assert (covered == 1).all() and (seen == 1).all()


@pytest.mark.parametrize("m", bh.MESHES)
def test_two_builds_give_the_same_bytes(meshes, built, m):
    again = bh.build_device_host(*meshes[m])
    for k in ("nodes", "tris", "prims", "grid", "qnodes4"):
        assert again[k].tobytes() == built[m][k].tobytes(), k
    for k in ("depth", "stack_bound", "nmedian"):
        assert again[k] == built[m][k]


def test_rejections_and_the_empty_mesh(meshes):
    import spray_amd
    v, f = meshes["grid12"]
    bad = f.copy()
    bad[5, 2] = len(v)
    with pytest.raises(spray_amd.SprayRtError) as e:
        spray_amd.bvh_build_device_host(v, bad)
    assert e.value.code == -1  # SPRAY_RT_ERR_ARG
    nan = v.copy()
    nan[f[7, 1], 2] = np.nan
    with pytest.raises(spray_amd.SprayRtError) as e:
        spray_amd.bvh_build_device_host(nan, f)
    assert e.value.code == -1
    v2 = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)  # unreferenced: accepted
    assert spray_amd.bvh_build_device_host(v2, f)["nodes"].tobytes() == \
        spray_amd.bvh_build_device_host(v, f)["nodes"].tobytes()
    with pytest.raises(spray_amd.SprayRtError) as e:
        spray_amd.bvh_build_device_host(np.full_like(v, np.finfo(np.float32).max), f)
    assert e.value.code == -5  # SPRAY_RT_ERR_LIMIT
    r = spray_amd.bvh_build_device_host(v, f[:0])
    assert len(r["nodes"]) == 0 and len(r["qnodes4"]) == 0 and r["depth"] == 0

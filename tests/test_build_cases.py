"""The classes of build_cases.py on the host (no GPU).

Every case must reach what it is there for: the widths, counts and outcomes are
asserted from the host restatement's image (spray_rt_bvh_build_device_host), so
a case that is edited away from its boundary fails here.  The restatement
itself is held to independent numpy: the key order, the structure of the tree,
boxes, records, QNode4 margins and tiling; the vectorised forms of
build_helpers that `million` needs are held equal to the per-node loops on every
case small enough for both.  test_gpu_build_cases.py then holds the kernels to
the restatement byte for byte.
"""
import numpy as np
import pytest

import build_cases as bc
import build_helpers as bh
import refit_helpers as rh

SMALL = sorted(bc.small())
BUILT = [n for n in SMALL if n not in bc.OUTCOME]


def restate(c):
    """The restatement's image of a case, or its error code."""
    import spray_amd
    try:
        return bh.build_device_host(c.verts, c.faces)
    except spray_amd.SprayRtError as e:
        return e.code


@pytest.fixture(scope="module")
def built():
    return {n: restate(c) for n, c in bc.small().items()}


@pytest.fixture(scope="module")
def million():
    c = bc.million()
    return c, bh.build_device_host(c.verts, c.faces)


def node_widths(b):
    return bh.level_widths(bh.node_refs(b["nodes"]))


def q_widths(b):
    return bh.level_widths(b["qnodes4"]["child"])


def chunks(width):
    return -(-width // bc.TREE_BLOCK)


def codes_of(c):
    with np.errstate(all="ignore"):
        return bh.sort_keys(c.verts, c.faces) >> np.uint64(32)


def refused(b):
    """QNode4s that keep an inner child although expanding it (two children for
    one) would still fit four: only the stack rule of collapse_node does that."""
    ch = b["qnodes4"]["child"]
    return int((((ch != rh.KNOCHILD).sum(1) <= 3) & (ch >= 0).any(1)).sum())


# ---- the cases reach their paths ----

def test_scale_cases_reach_their_boundaries(built):
    s = bc.small()
    assert len(s["level512"].faces) == bc.LEVEL512_N
    assert max(node_widths(built["level512"])) == 512      # one chunk, full
    assert max(node_widths(built["level513"])) == 513      # two chunks, the second of one node
    for n in ("level513", "level513_overlap"):
        assert node_widths(built[n])[10:] == [513, 5], n
        assert max(node_widths(built[n])) == 513 and built[n]["depth"] == 12
        assert len(s[n].faces) == bc.LEVEL513_CLUSTER + 15
        assert bh.carry_live(bh.node_refs(built[n]["nodes"]))
    assert (codes_of(s["level513"]) == 0).sum() == bc.LEVEL513_CLUSTER
    assert max(q_widths(built["qlevel512"])) == 512
    assert max(q_widths(built["qlevel513"])) == 513
    assert bc.find_qlevel.__defaults__ == (range(60, 70), 5) and bc.QLEVEL513 == (66, 8147)
    # a second chunk whose numbers depend on the first chunk's count
    assert bh.carry_live(bh.node_refs(built["level513"]["nodes"]))
    assert bh.carry_live(built["qlevel513"]["qnodes4"]["child"])
    for n in ("levels3", "check_16384", "two_cells", "deep_stack"):
        assert bh.carry_live(bh.node_refs(built[n]["nodes"])), n
        assert bh.carry_live(built[n]["qnodes4"]["child"]), n
    b = built["levels3"]
    assert len(s["levels3"].faces) == 20000 > bc.CHECK_TRIP
    assert (len(b["nodes"]), len(b["qnodes4"])) == (6582, 3105)
    assert (max(node_widths(b)), max(q_widths(b))) == (1200, 1347)
    assert chunks(max(node_widths(b))) == 3 and chunks(max(q_widths(b))) == 3
    assert len(s["check_16384"].faces) == 64 * 256 and len(s["check_16385"].faces) == 64 * 256 + 1
    for n in bc.scale_cases():
        assert built[n]["nmedian"] == 0, n


def test_million_reaches_its_boundaries(million):
    c, b = million
    assert len(c.faces) == 1051250 > bc.GRID_TRIP
    assert len(c.verts) == 527076 and 3 * len(c.verts) > bc.GRID_TRIP
    # refit_quant (a thread per QNode4 child) still covers it without a stride
    assert 4 * len(b["qnodes4"]) == 4 * 166531 < bc.GRID_TRIP
    assert b["depth"] == bh.KMAXDEPTH and b["nmedian"] == 112114
    assert chunks(max(node_widths(b))) > 3 and chunks(max(q_widths(b))) > 3


def test_key_cases_reach_their_regimes(built):
    s = bc.small()
    for n, c in bc.key_cases().items():
        want = bc.OUTCOME.get(n, 0)
        got = built[n] if isinstance(built[n], int) else 0
        assert got == want, n
        if n not in ("two_cells", "deep_stack", "stairs_wide"):
            assert 200 <= len(c.faces) <= 600, n

    def cells(name):
        c = s[name]
        tri = c.verts[c.faces]
        with np.errstate(all="ignore"):
            cen = ((tri.min(1) + tri.max(1)) * np.float32(0.5)).astype(np.float32)
            ext = cen.max(0) - cen.min(0)
            return cen, ext, np.float32(1024.0) / ext

    cen, ext, scale = cells("flat1")
    assert (ext > 0).tolist() == [True, True, False]
    cen, ext, scale = cells("flat2")
    assert (ext > 0).tolist() == [True, False, False]
    # tiny_extent: an infinite scale on z alone, subnormal differences, cells 0 and 1023
    cen, ext, scale = cells("tiny_extent")
    tiny = np.finfo(np.float32).tiny
    assert np.isinf(scale).tolist() == [False, False, True] and 1e-38 < ext[2] < 3e-38
    dz = cen[:, 2] - cen[:, 2].min()
    assert ((dz > 0) & (dz < tiny)).sum() > 50
    z = codes_of(s["tiny_extent"]) & np.uint64(0x9249249)   # the z bits of the code
    assert set(np.unique(z).tolist()) == {0, 0x9249249} and len(np.unique(codes_of(s["tiny_extent"]))) > 100
    cen, ext, scale = cells("tiny_all")
    assert np.isinf(scale).all() and len(np.unique(codes_of(s["tiny_all"]))) == 5
    assert (np.abs(s["subnormal"].verts) < tiny).all() and (s["subnormal"].verts != 0).any()
    cen, ext, scale = cells("huge")
    assert np.isfinite(ext).all() and ext.max() > 2e38 and np.abs(s["huge"].verts).max() > 1.1e38
    assert len(np.unique(codes_of(s["huge"]))) == 219      # 218 of the far half, one of the unit half
    v = s["overflow"].verts
    assert np.isfinite(v).all() and np.abs(v).min() > 2.9e38
    cen, ext, scale = cells("overflow")
    assert np.isinf(ext).all() and (scale == 0).all()
    with np.errstate(all="ignore"):
        assert np.isnan((cen - cen.min(0)) * scale).any()
    # ulps: centroids single floats apart, many equal codes
    cen, ext, scale = cells("ulps")
    step = np.unique(cen[:, 0])
    assert (np.diff(step) == np.spacing(np.float32(1e6))).all() and len(step) == 6
    k = codes_of(s["ulps"])
    assert len(np.unique(k)) < len(k) // 2 and float(scale[0]) * float(ext[0]) != 1024.0
    # at_hi: t = 1024 exactly, cell 1023
    cen, ext, scale = cells("at_hi")
    t = (cen - cen.min(0)) * scale
    assert ((t == 1024.0).sum(0) >= 40).all()
    # two_cells: two codes, the long run of one
    k = codes_of(s["two_cells"])
    assert len(np.unique(k)) == 2 and (k == 0).sum() == bc.TWO_CELLS_N
    assert built["two_cells"]["stack_bound"] >= 30 and built["two_cells"]["nmedian"] == 0
    # deep_stack: the stack rule's bound is reached, and it refuses
    b = built["deep_stack"]
    assert b["stack_bound"] == bh.KQ4STACK and refused(b) == 2047
    for n in BUILT:
        if n != "deep_stack":
            assert refused(built[n]) == 0, n
    # degenerate and twins
    c = s["degenerate"]
    tri = c.verts[c.faces].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area == 0).sum() == 80 and (area > 0).sum() == 392
    idx_equal = (c.faces[:, 0] == c.faces[:, 1]) | (c.faces[:, 0] == c.faces[:, 2])
    assert idx_equal.sum() == 48 and ((area == 0) & ~idx_equal).sum() == 32
    c = s["twins"]
    pts = np.sort(c.verts[c.faces].reshape(len(c.faces), 9).view([("", "<f4")] * 3), axis=1)
    same_points = len(c.faces) - len(np.unique(pts.view("<f4").reshape(-1, 9), axis=0))
    assert same_points == 210
    assert len(c.faces) - len(np.unique(c.faces, axis=0)) == 60   # listed twice, index for index
    # stairs_wide: the depth rule on a mesh beyond one block
    b = built["stairs_wide"]
    assert len(s["stairs_wide"].faces) == 3007 and b["nmedian"] == 511 and b["depth"] == bh.KMAXDEPTH
    assert built["level513"]["depth"] == 12


def test_batches():
    m = bc.mixed()
    assert [len(c.faces) for c in m] == [20000, 0, 1, 40, 4115, 5]
    orders = bc.mixed_orders()
    assert [c.name for c in orders["reversed"]] == [c.name for c in m][::-1]
    assert orders["rotated"][0].name == "tri1" and len(orders["rotated"]) == 6
    sizes = [len(c.faces) for c in bc.many_meshes()]
    assert tuple(sizes) == bc.MANY_SIZES and len(set(sizes)) == 12
    small = [n for n in sizes if n <= bc.SORT_SMALL]
    block = [n for n in sizes if bc.SORT_SMALL < n <= bc.SORT_BLOCK]
    radix = [n for n in sizes if n > bc.SORT_BLOCK]
    assert 0 in small and bc.SORT_SMALL in small and bc.SORT_SMALL + 1 in block
    assert bc.SORT_BLOCK in block and radix == [bc.SORT_BLOCK + 1]
    assert bc.MANY_CALLS == (3000, 2999)
    for n in bc.MANY_CALLS:
        assert {c.name for c in bc.many(n)} == {c.name for c in bc.many_meshes()}
    n = len(bc.levels3().faces)
    assert bc.poison_positions() == (0, 255, 256, 16383, 16384, n - 1)
    import spray_amd
    for tri in bc.poison_positions():
        for kind in ("face", "nan"):
            c = bc.poisoned(kind, tri)
            bad = (c.faces >= len(c.verts)).any(1) if kind == "face" else \
                np.isnan(c.verts[np.minimum(c.faces, len(c.verts) - 1)]).any((1, 2))
            assert np.nonzero(bad)[0].tolist() == [tri]
            with pytest.raises(spray_amd.SprayRtError) as e:
                spray_amd.bvh_build_device_host(c.verts, c.faces)
            assert e.value.code == bc.ERR_ARG


def test_queried_cases_stay_within_the_hit_rate(oracle):
    """bh.check_queries wants between 5 % and 95 % of its rays to hit: held
    here with the oracle's brute force alone, on the rays it will build."""
    for k, n in enumerate(bc.QUERIED):
        c = bc.small()[n]
        rv = bc.ray_verts(n)
        org, d = rh.refit_rays(np.random.default_rng(500 + k), c.verts if rv is None else rv,
                               c.faces)
        tri = oracle.prep_tris(c.verts, c.faces)
        _, _, _, p = oracle.brute_intersect(tri, org, d, np.full(len(org), 0.001, np.float32),
                                            np.full(len(org), np.inf, np.float32))
        assert 0.05 < (p != bh.INV).mean() < 0.95, n


# ---- the restatement against numpy ----

@pytest.mark.parametrize("n", BUILT)
def test_order_is_the_sorted_key(built, n):
    c = bc.small()[n]
    with np.errstate(all="ignore"):
        keys = bh.sort_keys(c.verts, c.faces)
    assert len(np.unique(keys)) == len(keys)
    assert np.array_equal(built[n]["prims"], np.argsort(keys, kind="stable").astype(np.uint32))


def expected_records(prims, f, v):
    """rh.expected_tris; where an edge is beyond 1e18 (`huge`: the products of
    Ng overflow, which fma_neg's fractions do not take) Ng is the float64 sum
    x y - fl(z w) rounded to float, which is exact about an overflow."""
    ff = f[prims]
    a, b, c = v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = (a - b).astype(np.float32), (c - a).astype(np.float32)
        far = np.maximum(np.abs(e1).max(1), np.abs(e2).max(1)) > 1e18
        out = np.zeros((len(ff), 12), np.float32)
        out[~far] = rh.expected_tris(prims[~far], f, v)
        out[far, 0:3], out[far, 3:6], out[far, 6:9] = a[far], e1[far], e2[far]
        x, y = e1[far].astype(np.float64), e2[far].astype(np.float64)
        for k, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            zw = (e1[far, j] * e2[far, i]).astype(np.float32).astype(np.float64)
            ng = x[:, i] * y[:, j] - zw
            assert (~np.isfinite(ng) | (np.abs(ng) > 1e40)).all()
            out[far, 9 + k] = ng.astype(np.float32)
    return out, int(far.sum())


def loop_depths(nodes):
    """test_build_host.test_tree_structure's depth loop."""
    depth = np.zeros(len(nodes), np.int64)
    deepest = 0
    for i in range(len(nodes)):
        for kr in ("left", "right"):
            ref = int(nodes[kr][i])
            if ref >= 0:
                depth[ref] = depth[i] + 1
        deepest = max(deepest, depth[i] + 1)
    return depth, deepest


@pytest.mark.parametrize("n", BUILT)
def test_structure_boxes_records_and_quantization(built, n):
    """The checks of test_build_host.py in their vectorised forms, and the
    vectorised forms equal to the per-node loops."""
    c, b = bc.small()[n], built[n]
    v, f, nodes, q4 = c.verts, c.faces, b["nodes"], b["qnodes4"]
    depth, deepest = bh.check_structure(nodes, len(f))
    ld, ldeep = loop_depths(nodes)
    assert np.array_equal(depth, ld) and deepest == ldeep == b["depth"] <= bh.KMAXDEPTH
    with np.errstate(invalid="ignore", over="ignore"):
        plo, phi, rng = bh.expected_boxes_by_level(nodes, b["prims"], f, v)
        llo, lhi, lrng = rh.expected_boxes(nodes, b["prims"], f, v)
    assert plo.tobytes() == llo.tobytes() and phi.tobytes() == lhi.tobytes()
    assert np.array_equal(rng, lrng)
    assert np.stack([nodes["l_lo"], nodes["r_lo"]], 1).tobytes() == plo.tobytes()
    assert np.stack([nodes["l_hi"], nodes["r_hi"]], 1).tobytes() == phi.tobytes()
    want, far = expected_records(b["prims"], f, v)
    assert b["tris"].tobytes() == want.tobytes() and (far > 0) == (n == "huge")
    assert 0 <= b["stack_bound"] <= bh.KQ4STACK
    assert np.array_equal(bh.q4_ranges_by_level(q4), rh.q4_child_ranges(q4))
    bh.check_qnodes4(q4, b["grid"], rng, plo, phi, len(f))


def test_million_against_numpy(million):
    """`million` in the vectorised forms alone; the records on a seeded sample
    of 20,000 triangles (fma_neg forms inexact sums with fractions)."""
    c, b = million
    v, f, nodes = c.verts, c.faces, b["nodes"]
    keys = bh.sort_keys(v, f)
    assert np.array_equal(b["prims"], np.argsort(keys, kind="stable").astype(np.uint32))
    depth, deepest = bh.check_structure(nodes, len(f))
    assert deepest == b["depth"] == bh.KMAXDEPTH
    plo, phi, rng = bh.expected_boxes_by_level(nodes, b["prims"], f, v)
    assert np.stack([nodes["l_lo"], nodes["r_lo"]], 1).tobytes() == plo.tobytes()
    assert np.stack([nodes["l_hi"], nodes["r_hi"]], 1).tobytes() == phi.tobytes()
    pick = np.sort(np.random.default_rng(7).choice(len(f), 20000, replace=False))
    assert b["tris"][pick].tobytes() == rh.expected_tris(b["prims"][pick], f, v).tobytes()
    ff = f[b["prims"]]
    assert np.array_equal(b["tris"][:, 0:3], v[ff[:, 0]])
    assert np.array_equal(b["tris"][:, 3:6], v[ff[:, 0]] - v[ff[:, 1]])
    assert np.array_equal(b["tris"][:, 6:9], v[ff[:, 2]] - v[ff[:, 0]])
    assert 0 <= b["stack_bound"] <= bh.KQ4STACK
    bh.check_qnodes4(b["qnodes4"], b["grid"], rng, plo, phi, len(f))


# ---- the refit restatement at scale ----

REFIT_MESHES = {"levels3": 100, "grid363": 363}


@pytest.fixture(scope="module")
def refit_built():
    out = {}
    for n, g in REFIT_MESHES.items():
        v, f = rh._grid(g)
        out[n] = (v, f, rh.build_host(v, f))
    return out


@pytest.mark.parametrize("d", ["sin", "shear", "flatten"])
@pytest.mark.parametrize("m", sorted(REFIT_MESHES))
def test_refit_restatement_at_scale(refit_built, m, d):
    """test_refit_host.test_refit_matches_numpy_restatement on 20,000 and
    263,538 triangles (depth 24 in the canonical build too), by level."""
    v, f, b = refit_built[m]
    v1 = rh.deform(d, v)
    r = rh.refit_host(v, v1, f)
    nodes, q4 = r["nodes"], r["qnodes4"]
    for k in ("left", "right", "pad"):
        assert np.array_equal(nodes[k], b["nodes"][k]), k
    assert np.array_equal(q4["child"], b["qnodes4"]["child"])
    plo, phi, rng = bh.expected_boxes_by_level(b["nodes"], b["prims"], f, v1)
    assert np.stack([nodes["l_lo"], nodes["r_lo"]], 1).tobytes() == plo.tobytes()
    assert np.stack([nodes["l_hi"], nodes["r_hi"]], 1).tobytes() == phi.tobytes()
    nt = len(f)
    pick = np.arange(nt) if nt <= 20000 else \
        np.sort(np.random.default_rng(8).choice(nt, 20000, replace=False))
    assert r["tris"][pick].tobytes() == rh.expected_tris(b["prims"][pick], f, v1).tobytes()
    ff = f[b["prims"]]
    assert np.array_equal(r["tris"][:, 0:3], v1[ff[:, 0]])
    assert np.array_equal(r["tris"][:, 3:6], v1[ff[:, 0]] - v1[ff[:, 1]])
    assert np.array_equal(r["tris"][:, 6:9], v1[ff[:, 2]] - v1[ff[:, 0]])
    bh.check_qnodes4(q4, r["grid"], rng, plo, phi, nt)
    if m == "levels3" and d == "sin":   # the by-level form on a depth-first numbering
        llo, lhi, lrng = rh.expected_boxes(b["nodes"], b["prims"], f, v1)
        assert plo.tobytes() == llo.tobytes() and phi.tobytes() == lhi.tobytes()
        assert np.array_equal(rng, lrng)
        assert np.array_equal(bh.q4_ranges_by_level(q4), rh.q4_child_ranges(q4))

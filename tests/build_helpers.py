"""Meshes, numpy restatements and query checks shared by the device-build tests
(test_build_host.py, test_gpu_build.py, and test_build_cases.py and
test_gpu_build_cases.py on the classes of build_cases.py)."""
import numpy as np

import refit_helpers as rh

F32 = np.float32
INV = 0xFFFFFFFF
KMAXDEPTH, KQ4STACK, KLEAFMAX = 24, 40, 4
MESHES = rh.MESHES + ("stairs", "dups")


def _tiny_tris(centers, e=1.0 / 16):
    """One triangle per row of centers whose box is center -+ e on every axis,
    so its box centroid is the center exactly (centers are multiples of 1/4)."""
    c = np.asarray(centers, np.float64)
    off = np.array([[-e, -e, -e], [e, -e, 0.0], [0.0, e, e]])
    v = (c[:, None, :] + off[None]).reshape(-1, 3).astype(F32)
    f = np.arange(3 * len(c), dtype=np.uint32).reshape(-1, 3)
    return v, f


def stairs():
    """36 tiny triangles whose Morton codes are 2^k, k = 0..29 (cell 2^j on one
    axis, cell 0 on the others), five in cell 0 and one at the far corner (the
    centroid bounds are [0, 1024]^3: one unit per cell).  Splitting at the
    highest differing bit peels one triangle per level, 30 levels deep: only
    the depth rule's median splits keep the tree within kMaxDepth."""
    cen = [[0, 0, 0], [.25, .25, .25], [.5, .25, .25], [.25, .5, .25], [.25, .25, .5]]
    for axis in range(3):
        for j in range(10):
            p = [.25, .25, .25]
            p[axis] = 2.0 ** j + .5
            cen.append(p)
    cen.append([1024.0, 1024.0, 1024.0])
    return _tiny_tris(cen)


def dups():
    """40 different triangles around one box centroid: equal codes, so every
    split is the median of the face order."""
    cen = np.tile([[1.0, 2.0, 3.0]], (40, 1))
    v, f = _tiny_tris(cen)
    v = v.reshape(40, 3, 3)
    # only coordinates strictly inside the box move: lo and hi stay
    k = np.arange(40, dtype=np.float64) / 64.0
    v[:, 1, 2] = (3.0 + k / 16).astype(F32)   # z of vertex 1: strictly inside (-e, e)
    v[:, 2, 0] = (1.0 - k / 16).astype(F32)   # x of vertex 2
    return v.reshape(-1, 3).copy(), f


def mesh(name, oracle):
    if name == "stairs":
        return stairs()
    if name == "dups":
        return dups()
    return rh.mesh(name, oracle)


# ---- numpy restatement of the sort key ----
def _spread3(c):
    out = np.zeros(len(c), np.uint64)
    for b in range(10):
        out |= ((c >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def sort_keys(v, f):
    """(code << 32) | face per face: box centroid (lo + hi) * 0.5 in float32,
    cell = clamp(trunc((c - lo) * (1024 / (hi - lo))), 0, 1023) per axis on the
    centroid bounds (0 on an axis without extent), x in the highest bit of
    each Morton triple."""
    tri = v[f]
    cen = ((tri.min(1) + tri.max(1)).astype(F32) * F32(0.5)).astype(F32)
    lo, hi = cen.min(0), cen.max(0)
    ext = (hi - lo).astype(F32)
    cells = np.zeros((len(f), 3), np.uint64)
    for j in range(3):
        if not ext[j] > 0:
            continue
        s = F32(1024.0) / ext[j]
        t = ((cen[:, j] - lo[j]).astype(F32) * s).astype(F32)
        cells[:, j] = np.clip(np.floor(np.where(t > 0, t, 0)), 0, 1023).astype(np.uint64)
    code = (_spread3(cells[:, 0]) << np.uint64(2)) | (_spread3(cells[:, 1]) << np.uint64(1)) \
        | _spread3(cells[:, 2])
    return (code << np.uint64(32)) | np.arange(len(f), dtype=np.uint64)


def build_device_host(v, f):
    """spray_amd.bvh_build_device_host with the records typed as rh.build_host's."""
    import spray_amd
    r = spray_amd.bvh_build_device_host(v, f)
    out = dict(r)
    out["nodes"] = r["nodes"].reshape(-1).view(rh.NODE_DTYPE)
    out["qnodes4"] = r["qnodes4"].reshape(-1).view(rh.QNODE4_DTYPE)
    return out


# ---- vectorised forms over the BFS levels (a million triangles in numpy) ----
def level_ranges(child):
    """[(first, end)] of the BFS levels of a tree numbered breadth first;
    child [n, k]: the refs of every node, inner ones >= 0."""
    inner = np.asarray(child) >= 0
    out, b, e = [], 0, min(1, len(inner))
    while b < e:
        out.append((b, e))
        b, e = e, e + int(inner[b:e].sum())
    return out


def level_widths(child):
    return [e - b for b, e in level_ranges(child)]


def carry_live(child, chunk=512):
    """Whether some level wider than `chunk` has inner children both among its
    first `chunk` nodes and after them: the numbering of the later ones then
    depends on the count carried over from the first chunk."""
    inner = np.asarray(child) >= 0
    return any(e - b > chunk and inner[b:b + chunk].any() and inner[b + chunk:e].any()
               for b, e in level_ranges(child))


def node_refs(nodes):
    return np.stack([nodes["left"], nodes["right"]], 1).astype(np.int64)


def check_structure(nodes, ntris):
    """test_build_host.test_tree_structure's checks without a loop over the
    nodes: leaves of 1..4 triangles tile [0, ntris) once, every node but the
    root is referred to once and after its parent, the numbering is breadth
    first.  -> (depth per node, depth of the tree)."""
    nn = len(nodes)
    refs = node_refs(nodes)
    live = np.stack([nodes["l_lo"][:, 0], nodes["r_lo"][:, 0]], 1) != np.inf
    assert live[:, 0].all() and (live[:, 1].all() or nn == 1)
    leaf = live & (refs < 0)
    u = (~refs[leaf]) & 0xFFFFFFFF
    first, cnt = np.sort(u >> 2), ((u & 3) + 1)[np.argsort(u >> 2, kind="stable")]
    assert first[0] == 0 and np.array_equal(first[1:], (first + cnt)[:-1])
    assert first[-1] + cnt[-1] == ntris and cnt.min() >= 1 and cnt.max() <= KLEAFMAX
    inner = live & (refs >= 0)
    assert np.array_equal(np.sort(refs[inner]), np.arange(1, nn))
    assert (refs[inner] > np.nonzero(inner)[0]).all()
    assert (nodes["pad"] == 0).all()
    # breadth first: the inner refs of a level, in node order, are the next level
    depth = np.zeros(nn, np.int64)
    levels = level_ranges(np.where(live, refs, -1))
    for d, (b, e) in enumerate(levels):
        depth[b:e] = d
        nxt = refs[b:e][inner[b:e]]
        end = levels[d + 1][1] if d + 1 < len(levels) else e
        assert np.array_equal(nxt, np.arange(e, end))
    assert levels[-1][1] == nn
    return depth, len(levels)


def _leaf_fold(first, cnt, lo_t, hi_t):
    """min / max over the triangles [first, first + cnt) of per-triangle boxes."""
    lo, hi = lo_t[first].copy(), hi_t[first].copy()
    for c in range(1, KLEAFMAX):
        k = first + np.minimum(c, cnt - 1)
        lo, hi = np.minimum(lo, lo_t[k]), np.maximum(hi, hi_t[k])
    return lo, hi


def tree_levels(refs, live):
    """The nodes of every depth as index arrays, root first, for any numbering
    (a breadth-first one gives consecutive ranges)."""
    out, idx = [], np.arange(min(1, len(refs)))
    while len(idx):
        out.append(idx)
        r = refs[idx]
        idx = r[live[idx] & (r >= 0)]
    return out


def expected_boxes_by_level(nodes, prims, f, v):
    """refit_helpers.expected_boxes bottom up, a level of the tree at a time:
    (plo, phi, rng) of the same shapes and bytes."""
    nn = len(nodes)
    refs = node_refs(nodes)
    live = np.stack([nodes["l_lo"][:, 0], nodes["r_lo"][:, 0]], 1) != np.inf
    pts = v[f[prims]]                      # [nt, 3, 3]
    lo_t, hi_t = pts.min(1), pts.max(1)
    lo = np.stack([nodes["l_lo"], nodes["r_lo"]], 1).astype(F32)   # the never-hit box stays
    hi = np.stack([nodes["l_hi"], nodes["r_hi"]], 1).astype(F32)
    rng = np.full((nn, 2, 2), -1, np.int64)
    for idx in tree_levels(refs, live)[::-1]:
        for side in range(2):
            r, lv = refs[idx, side], live[idx, side]
            leaf, inner = lv & (r < 0), lv & (r >= 0)
            u = (~r[leaf]) & 0xFFFFFFFF
            first, cnt = u >> 2, (u & 3) + 1
            lo[idx[leaf], side], hi[idx[leaf], side] = _leaf_fold(first, cnt, lo_t, hi_t)
            rng[idx[leaf], side] = np.stack([first, first + cnt], 1)
            c = r[inner]
            lo[idx[inner], side] = np.minimum(lo[c, 0], lo[c, 1])
            hi[idx[inner], side] = np.maximum(hi[c, 0], hi[c, 1])
            rng[idx[inner], side] = np.stack([rng[c, 0, 0], rng[c, 1, 1]], 1)
    plo, phi = rh.pad_np(lo, hi)
    plo[~live], phi[~live] = lo[~live], hi[~live]
    return plo, phi, rng


def q4_ranges_by_level(q4):
    """refit_helpers.q4_child_ranges bottom up, a level at a time."""
    child = q4["child"].astype(np.int64)
    rng = np.full((len(q4), 4, 2), -1, np.int64)
    big = np.iinfo(np.int64).max
    for idx in tree_levels(child, child != rh.KNOCHILD)[::-1]:
        for c in range(4):
            r = child[idx, c]
            leaf, inner = (r < 0) & (r != rh.KNOCHILD), r >= 0
            u = (~r[leaf]) & 0xFFFFFFFF
            rng[idx[leaf], c] = np.stack([u >> 2, (u >> 2) + (u & 3) + 1], 1)
            sub = rng[r[inner]]                # [k, 4, 2]
            rng[idx[inner], c] = np.stack([np.where(sub[:, :, 0] >= 0, sub[:, :, 0], big).min(1),
                                           sub[:, :, 1].max(1)], 1)
    return rng


def check_qnodes4(q4, grid, rng, plo, phi, ntris):
    """test_build_host's QNode4 checks without a loop over the nodes: children
    after parents and referred to once, leaves tile the triangles once, an
    empty child is all 0xFFFF, every decoded box holds the padded box of the
    BVH2 (node, side) of its range with a grid step to spare."""
    nq = len(q4)
    child = q4["child"].astype(np.int64)
    none = child == rh.KNOCHILD
    assert (q4["q"][none] == 0xFFFF).all()
    inner, leaf = child >= 0, (child < 0) & ~none
    assert np.array_equal(np.sort(child[inner]), np.arange(1, nq))
    assert (child[inner] > np.nonzero(inner)[0]).all()
    u = (~child[leaf]) & 0xFFFFFFFF
    o = np.argsort(u >> 2, kind="stable")
    first, cnt = (u >> 2)[o], ((u & 3) + 1)[o]
    assert first[0] == 0 and np.array_equal(first[1:], (first + cnt)[:-1])
    assert first[-1] + cnt[-1] == ntris
    assert (grid[3:] > 0).all() and np.isfinite(grid).all()
    # (range) -> BVH2 (node, side)
    nkey = (rng[:, :, 0] << 32 | rng[:, :, 1]).reshape(-1)
    order = np.argsort(nkey, kind="stable")
    qr = q4_ranges_by_level(q4)
    qkey = (qr[:, :, 0] << 32 | qr[:, :, 1])[~none]
    at = np.searchsorted(nkey[order], qkey)
    assert np.array_equal(nkey[order][at], qkey)
    src = order[at]
    slo, shi = plo.reshape(-1, 3)[src].astype(np.float64), phi.reshape(-1, 3)[src].astype(np.float64)
    scale = grid[3:].astype(np.float64)
    dlo = rh.decode_q(grid, q4["q"][:, :, :3][~none])
    dhi = rh.decode_q(grid, q4["q"][:, :, 3:][~none])
    assert (dlo + scale <= slo).all() and (dhi - scale >= shi).all()


# ---- GPU helpers (test_gpu_refit.py's, restated: that file stays as it is) ----
WHAT = ("NODES", "TRIS", "PRIMS", "QNODES4", "QGRID", "NORMALS")


def export_all(c, slot):
    return {w: c.slot_export(slot, getattr(c, "SLOT_" + w)).tobytes() for w in WHAT}


def rtc_records(spray, org, d, tnear=0.001, tfar=np.inf):
    r = np.zeros(len(org), spray.RTC_ISECT_DTYPE)
    r["org"], r["dir"], r["tnear"], r["tfar"] = org, d, tnear, tfar
    r["geomID"] = r["primID"] = r["instID"] = INV
    r["mask"] = 0xFFFFFFFF
    return r


def check_queries(spray, oracle, c, slot, v1, f, col, n1, seed, ray_verts=None):
    """intersect1M / occluded1M of a slot against the oracle's brute force on
    mesh (v1, f), bit for bit."""
    rng = np.random.default_rng(seed)
    org, d = rh.refit_rays(rng, v1 if ray_verts is None else ray_verts, f)
    tnear = np.full(len(org), 0.001, F32)
    tfar = np.full(len(org), np.inf, F32)
    recs = rtc_records(spray, org, d, tnear, tfar)
    before = recs.copy()
    c.intersect1M(slot, recs)
    tri = oracle.prep_tris(v1, f)
    t, u, vv, p = oracle.brute_intersect(tri, org, d, tnear, tfar)
    hit = p != INV
    assert 0.05 < hit.mean() < 0.95, hit.mean()
    assert np.array_equal(recs["primID"], p)
    assert np.array_equal(recs["geomID"][hit], np.zeros(hit.sum(), np.uint32))
    assert np.array_equal(recs["tfar"].view(np.uint32), t.view(np.uint32))
    assert np.array_equal(recs["u"][hit].view(np.uint32), u[hit].view(np.uint32))
    assert np.array_equal(recs["v"][hit].view(np.uint32), vv[hit].view(np.uint32))
    assert np.array_equal(recs["Ng"][hit].view(np.uint32), tri[p[hit], 9:12].view(np.uint32))
    ecol, ns = oracle.epilogue(f, col, n1, p, u, vv)
    assert np.array_equal(recs["color"][hit], ecol[hit])
    assert np.array_equal(recs["Ns"][hit].view(np.uint32), ns[hit].view(np.uint32))
    assert np.array_equal(recs[~hit].view(np.uint8), before[~hit].view(np.uint8))
    orec = rtc_records(spray, org, d, tnear, tfar)
    c.occluded1M(slot, orec)
    occ = oracle.brute_occluded(tri, org, d, tnear, tfar)
    assert np.array_equal(orec["geomID"] != INV, occ.astype(bool))


def scene_results(spray, rt, rays_np, eye, pix):
    """Every scene launch of the refit scene test, as bytes: closest hit, fused
    PT shadows, any hit in the three coherence modes, AO."""
    import torch
    out = {}
    rays = torch.from_numpy(rays_np.view(np.uint8)).cuda()
    n = len(rays_np)
    hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    rt.intersect_scene(rays, hits)
    rt.sync()
    out["intersect_scene"] = hits.cpu().numpy().tobytes()
    shade = np.array([-20, 20, 20, .2, .2, .2, 0.4, 0.4, 0.4, 10.0], np.float32)
    h2 = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    occ = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    sv = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    rt.intersect_scene_shadow_pt(rays, h2, shade, occ, sv, cnt)
    rt.sync()
    out["shadow_pt"] = (h2.cpu().numpy().tobytes(), occ.cpu().numpy().tobytes(),
                        sv.cpu().numpy().tobytes(), int(cnt.item()))
    for mode in (rt.RAYS_ADAPTIVE, rt.RAYS_COHERENT, rt.RAYS_INCOHERENT):
        rt.set_coherence(mode)
        o = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        rt.occluded_scene(rays, o)
        rt.sync()
        out["occluded_scene_%d" % mode] = o.cpu().numpy().tobytes()
    rt.set_coherence(rt.RAYS_ADAPTIVE)
    # AO: 4 samples over a 64 x 64 x 1 spp eye-ray batch
    er = torch.from_numpy(eye.view(np.uint8)).cuda()
    m, ns = len(eye), 4
    eh = torch.zeros(m * 48, dtype=torch.uint8, device="cuda")
    rt.intersect_scene(er, eh)
    pixid = torch.from_numpy(np.ascontiguousarray(pix)).cuda()
    pairs = torch.full((m * ns,), -1, dtype=torch.int32, device="cuda")
    acnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    aocc = torch.full((m * ns,), 9, dtype=torch.uint8, device="cuda")
    lv = torch.zeros((64 * 64 * ns, 4), dtype=torch.float32, device="cuda")
    rec = torch.zeros((m, 16), dtype=torch.float32, device="cuda")
    rt.occluded_ao(er, eh, pixid, m, ns, pairs, lv, rec, acnt, aocc)
    rt.sync()
    k = int(acnt.item())
    out["ao"] = (eh.cpu().numpy().tobytes(), k, pairs[:k].cpu().numpy().tobytes(),
                 aocc[:k].cpu().numpy().tobytes())
    return out

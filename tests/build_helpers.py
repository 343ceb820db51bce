"""Meshes, numpy restatements and query checks shared by the device-build tests
(test_build_host.py, test_gpu_build.py)."""
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

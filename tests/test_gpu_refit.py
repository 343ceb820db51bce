"""Device refit of resident slots (spray_rt_domains_refit) on the GPU.

Three references, each bit for bit: the host restatement
(spray_rt_bvh_refit_host) for the slot image, the oracle's brute force on the
deformed mesh for queries, and a fresh upload of the deformed mesh in a
second context for the scene launches.
"""
import numpy as np
import pytest

import refit_helpers as rh
from conftest import SCENES, WAVELET2

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
ERR_ARG, ERR_LIMIT = -1, -5
CASES = [(m, d) for m in rh.MESHES for d in rh.DEFORMS]


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def meshes(oracle):
    """name -> (verts, faces, colors, normals), the state slots are built from."""
    out = {}
    for m in rh.MESHES:
        v, f = rh.mesh(m, oracle)
        out[m] = (v, f, rh.vertex_colors(len(v)), rh.vertex_normals(oracle, v, f))
    return out


@pytest.fixture(scope="module")
def ctx(spray, meshes):
    """Slot k holds mesh k of rh.MESHES; tests leave it at any deformation."""
    c = spray.RtContext(0)
    for k, m in enumerate(rh.MESHES):
        c.upload_domain(k, *meshes[m])
    yield c
    c.close()


@pytest.fixture(scope="module")
def built_images(ctx):
    """The slot images right after the upload (before any refit)."""
    return {m: export_all(ctx, k) for k, m in enumerate(rh.MESHES)}


def export_all(c, slot):
    return {w: c.slot_export(slot, getattr(c, "SLOT_" + w)).tobytes()
            for w in ("NODES", "TRIS", "PRIMS", "QNODES4", "QGRID", "NORMALS")}


def rtc_records(spray, org, d, tnear=0.001, tfar=np.inf):
    r = np.zeros(len(org), spray.RTC_ISECT_DTYPE)
    r["org"], r["dir"], r["tnear"], r["tfar"] = org, d, tnear, tfar
    r["geomID"] = r["primID"] = r["instID"] = INV
    r["mask"] = 0xFFFFFFFF
    return r


def check_queries(spray, oracle, c, slot, v1, f, col, n1, seed, ray_verts=None):
    """intersect1M / occluded1M of a slot against the oracle's brute force on
    mesh (v1, f), as tests/test_gpu_parity.py::test_intersect1M_matches_oracle
    (ray_verts: the vertices the rays are built around, v1 unless it holds
    unreferenced non-finite ones)."""
    rng = np.random.default_rng(seed)
    org, d = rh.refit_rays(rng, v1 if ray_verts is None else ray_verts, f)
    tnear = np.full(len(org), 0.001, np.float32)
    tfar = np.full(len(org), np.inf, np.float32)
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


@pytest.mark.parametrize("m,d", CASES)
def test_refit_image_and_queries(spray, oracle, meshes, ctx, built_images, m, d):
    """The slot after a refit: its arrays equal the host restatement's byte
    for byte, and its queries equal the oracle on the deformed mesh."""
    k = rh.MESHES.index(m)
    v, f, col, _ = meshes[m]
    v1 = rh.deform(d, v)
    n1 = rh.vertex_normals(oracle, v1, f)
    ctx.refit_domains([k], [v1], [n1])
    got = export_all(ctx, k)
    want = spray.bvh_refit_host(v, v1, f)
    assert got["NODES"] == want["nodes"].tobytes()
    assert got["TRIS"] == want["tris"].tobytes()
    assert got["QGRID"] == want["grid"].tobytes()
    assert got["QNODES4"] == want["qnodes4"].tobytes()
    assert got["NORMALS"] == n1.tobytes()
    assert got["PRIMS"] == built_images[m]["PRIMS"]
    if d == "identity":  # the image the upload built, unchanged
        assert got == built_images[m]
    check_queries(spray, oracle, ctx, k, v1, f, col, n1, 100 + 10 * k + rh.DEFORMS.index(d))


def test_refit_and_back_restores_the_image(oracle, meshes, ctx, built_images):
    for k, m in enumerate(rh.MESHES):
        v, f, _, n = meshes[m]
        v1 = rh.deform("sin", v)
        ctx.refit_domains([k], [v1], [rh.vertex_normals(oracle, v1, f)])
        assert export_all(ctx, k)["NODES"] != built_images[m]["NODES"]
        ctx.refit_domains([k], [v], [n])
        assert export_all(ctx, k) == built_images[m]


def test_one_call_equals_two_and_bounds(spray, oracle, meshes, ctx):
    import torch
    ka, kb = rh.MESHES.index("grid12"), rh.MESHES.index("wavelet0")
    (va, fa, _, _), (vb, fb, _, _) = meshes["grid12"], meshes["wavelet0"]
    a1, b1 = rh.deform("shear", va), rh.deform("sin", vb)
    na, nb = rh.vertex_normals(oracle, a1, fa), rh.vertex_normals(oracle, b1, fb)
    ctx.refit_domains([ka], [a1], [na])
    ctx.refit_domains([kb], [b1], [nb])
    two = (export_all(ctx, ka), export_all(ctx, kb))
    ctx.refit_domains([ka, kb], [va, vb], [meshes["grid12"][3], meshes["wavelet0"][3]])
    # device pointers this time, in the other slot order
    dev = [torch.from_numpy(x).cuda() for x in (b1, a1, nb, na)]
    bounds = ctx.refit_domains([kb, ka], dev[:2], dev[2:], bounds=True)
    assert (export_all(ctx, ka), export_all(ctx, kb)) == two
    for row, (v1, f) in zip(bounds, ((b1, fb), (a1, fa))):
        ref = v1[np.unique(f)]
        assert row.tobytes() == np.concatenate([ref.min(0), ref.max(0)]).tobytes()


def sah_numpy(nodes):
    """spray_rt_slot_sah's definition on exported nodes."""
    n = nodes.reshape(-1).view(rh.NODE_DTYPE)
    total, root = 0.0, None
    lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    for kl, kh, kr in (("l_lo", "l_hi", "left"), ("r_lo", "r_hi", "right")):
        live = n[kl][:, 0] != np.inf
        with np.errstate(invalid="ignore"):  # the never-hit box: inf - inf, masked below
            e = (n[kh] - n[kl]).astype(np.float32)
        area = ((e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]).astype(np.float32)
        ref = n[kr].astype(np.int64)
        cnt = np.where(ref < 0, ((~ref) & 3) + 1, 1)
        total += float(np.sum(area[live].astype(np.float64) * cnt[live]))
        if live[0]:
            lo, hi = np.minimum(lo, n[kl][0]), np.maximum(hi, n[kh][0])
    e = (hi - lo).astype(np.float32)
    root = np.float32((e[0] * e[1] + e[1] * e[2]) + e[2] * e[0])
    return total / float(root)


def test_slot_sah(oracle, meshes, ctx):
    """Equal to numpy on the exported nodes within 1e-9 relative (fewer than
    10^4 double terms: the summation-order bound is ~n 2^-53 ~ 1e-12); an
    identity refit keeps the bits; shearing the grid mesh makes it worse."""
    for k, m in enumerate(rh.MESHES):
        v, f, _, n = meshes[m]
        ctx.refit_domains([k], [v], [n])
        s0 = ctx.slot_sah(k)
        ref = sah_numpy(ctx.slot_export(k, ctx.SLOT_NODES))
        assert abs(s0 - ref) <= 1e-9 * abs(ref), (m, s0, ref)
        ctx.refit_domains([k], [v], [n])
        assert np.float64(ctx.slot_sah(k)).tobytes() == np.float64(s0).tobytes()
        if m == "grid12":
            v1 = rh.deform("shear", v)
            ctx.refit_domains([k], [v1], [rh.vertex_normals(oracle, v1, f)])
            s1 = ctx.slot_sah(k)
            assert abs(s1 - sah_numpy(ctx.slot_export(k, ctx.SLOT_NODES))) <= 1e-9 * s1
            assert s1 > s0


def test_failed_refit_changes_nothing(spray, oracle, meshes, ctx):
    ka, kb = rh.MESHES.index("grid12"), rh.MESHES.index("tri5")
    (va, fa, ca, na), (vb, fb, _, nb) = meshes["grid12"], meshes["tri5"]
    ctx.refit_domains([ka, kb], [va, vb], [na, nb])
    before = (export_all(ctx, ka), export_all(ctx, kb))
    a1, b1 = rh.deform("sin", va), rh.deform("sin", vb)
    na1, nb1 = rh.vertex_normals(oracle, a1, fa), rh.vertex_normals(oracle, b1, fb)

    def unchanged():
        assert (export_all(ctx, ka), export_all(ctx, kb)) == before
        check_queries(spray, oracle, ctx, ka, va, fa, ca, na, 7)

    # a NaN in a referenced vertex of the SECOND slot: the first is not touched either
    bad = b1.copy()
    bad[fb[2, 1], 1] = np.nan
    with pytest.raises(spray.SprayRtError) as e:
        ctx.refit_domains([ka, kb], [a1, bad], [na1, nb1])
    assert e.value.code == ERR_ARG and "slot %d" % kb in str(e.value)
    unchanged()
    # padded boxes that overflow: no grid holds them
    with pytest.raises(spray.SprayRtError) as e:
        ctx.refit_domains([ka, kb], [a1, np.full_like(vb, np.finfo(np.float32).max)], [na1, nb1])
    assert e.value.code == ERR_LIMIT and "slot %d" % kb in str(e.value)
    unchanged()
    # a normals argument of the wrong length; normals missing for a slot that has them
    with pytest.raises(spray.SprayRtError) as e:
        ctx.refit_domains([ka, kb], [a1, b1], [na1, nb1[:-1]])
    assert e.value.code == ERR_ARG
    with pytest.raises(spray.SprayRtError) as e:
        ctx.refit_domains([ka, kb], [a1, b1], [na1])
    assert e.value.code == ERR_ARG
    with pytest.raises(spray.SprayRtError) as e:
        ctx.refit_domains([ka, kb], [a1, b1], None)
    assert e.value.code == ERR_ARG
    unchanged()
    # an unloaded slot, a slot listed twice
    with pytest.raises(spray.SprayRtError) as e:
        ctx.refit_domains([ka, 40], [a1, b1], [na1, nb1])
    assert e.value.code == ERR_ARG
    with pytest.raises(spray.SprayRtError) as e:
        ctx.refit_domains([ka, ka], [a1, a1], [na1, na1])
    assert e.value.code == ERR_ARG
    unchanged()


def test_nan_in_unreferenced_vertex_is_accepted(spray, oracle, meshes):
    v, f, col, _ = meshes["grid12"]
    v2 = np.concatenate([v, [[5.0, 5.0, 5.0]]]).astype(np.float32)
    col2 = rh.vertex_colors(len(v2))
    c = spray.RtContext(0)
    c.upload_domain(0, v2, f, col2, rh.vertex_normals(oracle, v2, f))
    v3 = rh.deform("scale", v2)
    v3[-1] = np.nan
    n3 = rh.vertex_normals(oracle, v3, f)
    b = c.refit_domains([0], [v3], [n3], bounds=True)
    ref = v3[np.unique(f)]
    assert b[0].tobytes() == np.concatenate([ref.min(0), ref.max(0)]).tobytes()
    finite = v3.copy()
    finite[-1] = finite[0]
    check_queries(spray, oracle, c, 0, v3, f, col2, n3, 11, ray_verts=finite)
    c.close()


# ---- refit vs fresh upload over two domains, the scene launches ----
def scene_results(spray, oracle, rt, rays_np, eye, pix):
    """Every scene launch the issue lists, as bytes."""
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


def test_refit_equals_fresh_upload_over_two_domains(spray, oracle):
    doms, _ = oracle.parse_spray(WAVELET2, SCENES)
    mesh0 = {}
    for dom in doms:
        v, f, c, n = oracle.load_domain_mesh(dom)
        mesh0[dom["id"]] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.uint32),
                            np.ascontiguousarray(c, np.uint32), np.ascontiguousarray(n, np.float32))
    boxes0 = np.array([dom["world_bound"] for dom in doms], np.float32).reshape(-1, 6)
    A, B = spray.RtContext(0), spray.RtContext(0)
    new, slots = {}, sorted(mesh0)
    for i in slots:
        v, f, c, n = mesh0[i]
        v1 = rh.deform("sin", v)
        new[i] = (v1, f, c, rh.vertex_normals(oracle, v1, f))
        A.upload_domain(i, v, f, c, n)
        B.upload_domain(i, *new[i])
    A.domain_bounds(boxes0)
    for i in slots:
        A.map_domain(i, i)
    bounds = A.refit_domains(slots, [new[i][0] for i in slots], [new[i][3] for i in slots],
                             bounds=True)
    for i, row in zip(slots, bounds):
        ref = new[i][0][np.unique(new[i][1])]
        assert row.tobytes() == np.concatenate([ref.min(0), ref.max(0)]).tobytes()
    for rt in (A, B):  # both set the new bounds (the call resets the domain map)
        rt.domain_bounds(bounds)
        for i in slots:
            rt.map_domain(i, i)
    allv = np.concatenate([new[i][0] for i in slots])
    allf = np.concatenate([new[i][1] + sum(len(new[j][0]) for j in slots if j < i)
                           for i in slots]).astype(np.uint32)
    org, d = rh.refit_rays(np.random.default_rng(5), allv, allf)
    rays = spray.make_rays(org, d)
    cam = oracle.camera_init([-5.0, 10.0, 15.0], [0.0, 0.0, 0.0], [0, 1, 0], 60, 64, 64)
    eo, ed, pix, _ = oracle.eye_rays_ooc(cam, 64, 1, (0, 0, 64, 64))
    eye = spray.make_rays(eo, ed)
    ra = scene_results(spray, oracle, A, rays, eye, pix)
    rb = scene_results(spray, oracle, B, rays, eye, pix)
    # not vacuous: hits, shadow rays, AO rays, both occlusion outcomes
    hits = np.frombuffer(ra["intersect_scene"], spray.HIT_DTYPE)
    assert 0.05 < (hits["domain"] >= 0).mean() < 0.95
    assert set(np.unique(hits["domain"])) >= {0, 1}
    assert ra["shadow_pt"][3] > 100 and ra["ao"][1] > 1000
    occ = np.frombuffer(ra["occluded_scene_2"], np.uint8)
    assert 0.05 < occ.mean() < 0.95
    for k in ra:
        assert ra[k] == rb[k], k
    A.close()
    B.close()

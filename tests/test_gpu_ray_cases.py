"""Every scene-path walk against the extended oracle on the hard ray classes
of ray_cases.py -- per-ray tnear / tfar in the 32-byte record, axis-parallel
and signed-zero directions, components around the direction clamp, rays in
lattice planes, rays at edges, origins on the surface, coincident triangles
in touching domains -- bit for bit: domain, prim, t, u, v, Ng, Ns, color,
occlusion bytes, untouched records on a miss.  The float64 reference of
test_ray_cases.py is also applied to the kernels' own output (packet closest
hit, 4-wide quantized any hit), so truth stands next to the kernel.

Rays per launch: 1024 per class, 7168 for `mixed` (the seven classes
interleaved, so that one wave holds several), at both scene positions."""
import numpy as np
import pytest

import ray_cases as RC

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
NAMES = RC.CLASSES + ("mixed",)
DEFAULT_EXTENTS = tuple(n for n in RC.CLASSES if n != "extents")
RAGGED = (1, 63, 64, 65, 129)  # one valid lane, a ragged last wave
SHADE = np.array([4.0, 30.0, 60.0, 1, 1, 1, 0.4, 0.4, 0.4, 10.0], np.float32)


class Env:
    pass


@pytest.fixture(scope="module", params=(0.0, RC.LARGE), ids=["origin", "large"])
def env(request, oracle):
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    e = Env()
    e.spray, e.oracle, e.torch = spray_amd, oracle, torch
    e.var = RC.variant(oracle, request.param)
    e.large = request.param != 0.0
    e.rt = spray_amd.RtContext(0)
    for i, (v, f) in enumerate(e.var["meshes"]):
        e.rt.upload_domain(i, v, f, e.var["colors"][i], e.var["normals"][i])
    e.rt.domain_bounds(e.var["boxes"])
    for i in range(RC.NDOM):
        e.rt.map_domain(i, i)
    e.bvh = [oracle.Bvh(v, f) for v, f in e.var["meshes"]]
    e.tri = [oracle.prep_tris(v, f) for v, f in e.var["meshes"]]
    yield e
    e.rt.close()


# ---- helpers ----
def host_rays(e, c, n=None):
    r = e.spray.make_rays(c["org"], c["dir"], c["tnear"], c["tfar"])
    return r if n is None else r[:n].copy()


def dev(e, a):
    return e.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def dev_rays(e, c, n=None):
    return dev(e, host_rays(e, c, n))


def sentinel_hits(e, n):
    return e.torch.full((n * 48,), 0xA5, dtype=e.torch.uint8, device="cuda")


def hits_of(e, t):
    return t.cpu().numpy().view(e.spray.HIT_DTYPE).reshape(-1)


def same_hits(got, ref, what):
    if got.tobytes() == ref.tobytes():
        return
    for k in ref.dtype.names:
        a = got[k].reshape(len(got), -1).view(np.uint32)
        b = ref[k].reshape(len(ref), -1).view(np.uint32)
        bad = np.flatnonzero((a != b).any(1))
        assert len(bad) == 0, (what, k, len(bad), bad[:8].tolist())
    raise AssertionError(what)


def same_occ(got, ref, what):
    bad = np.flatnonzero(np.asarray(got) != ref)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())


def masks_for(n, rng):
    """The adversarial masks of test_masked_occlusion_sparse_patterns."""
    return [np.ones(n, np.uint8), np.zeros(n, np.uint8),
            (np.arange(n) % 63 == 5).astype(np.uint8),
            (np.arange(n) == n // 2).astype(np.uint8),
            (rng.uniform(size=n) < 0.05).astype(np.uint8)]


def rtc_records(e, c):
    r = np.zeros(len(c["org"]), e.spray.RTC_ISECT_DTYPE)
    r["org"], r["dir"], r["tnear"], r["tfar"] = c["org"], c["dir"], c["tnear"], c["tfar"]
    r["geomID"] = r["primID"] = r["instID"] = INV
    r["mask"] = 0xFFFFFFFF
    return r


def expect_1m(e, slot, c, sel=slice(None)):
    """The records intersect1M must leave for slot `slot`, and occlusion."""
    v, f = e.var["meshes"][slot]
    org, d, tn, tf = c["org"][sel], c["dir"][sel], c["tnear"][sel], c["tfar"][sel]
    t, u, w, p, _ = e.bvh[slot].intersect(org, d, tn, tf)
    occ, _ = e.bvh[slot].occluded(org, d, tn, tf)
    want = rtc_records(e, dict(org=org, dir=d, tnear=tn, tfar=tf))
    hit = p != INV
    col, ns = e.oracle.epilogue(f, e.var["colors"][slot], e.var["normals"][slot], p, u, w)
    want["tfar"][hit] = t[hit]
    want["u"][hit], want["v"][hit] = u[hit], w[hit]
    want["Ng"][hit] = e.tri[slot][p[hit], 9:12]
    want["color"][hit], want["Ns"][hit] = col[hit], ns[hit]
    want["geomID"][hit], want["primID"][hit] = 0, p[hit]
    return want, occ


# ---- the forms: each runs class `name` and compares with the oracle ----
def form_1m(e, name):
    c = e.var["classes"][name]
    for slot in range(RC.NDOM):
        want, occ = expect_1m(e, slot, c)
        recs = rtc_records(e, c)
        e.rt.intersect1M(slot, recs)
        assert recs.tobytes() == want.tobytes(), (name, slot, np.flatnonzero(
            recs.view(np.uint8).reshape(len(recs), -1) != want.view(np.uint8).reshape(len(recs), -1))[:4])
        recs = rtc_records(e, c)
        before = recs.copy()
        e.rt.occluded1M(slot, recs)
        same_occ(recs["geomID"] != INV, occ.astype(bool), (name, slot, "occluded1M"))
        before["geomID"] = recs["geomID"]
        assert recs.tobytes() == before.tobytes()  # nothing else is written


def form_segments(e, name):
    c = e.var["classes"][name]
    n = len(c["org"])
    off = np.linspace(0, n, RC.NDOM + 1).astype(np.uint64)
    off[1:-1] += np.arange(1, RC.NDOM, dtype=np.uint64) % 3  # no multiples of the block
    parts = [expect_1m(e, s, c, slice(int(off[s]), int(off[s + 1]))) for s in range(RC.NDOM)]
    want = np.concatenate([p[0] for p in parts])
    occ = np.concatenate([p[1] for p in parts])
    recs = rtc_records(e, c)
    e.rt.intersect_segments(list(range(RC.NDOM)), off, recs)
    assert recs.tobytes() == want.tobytes(), name
    recs = rtc_records(e, c)
    e.rt.occluded_segments(list(range(RC.NDOM)), off, recs)
    same_occ(recs["geomID"] != INV, occ.astype(bool), (name, "occluded_segments"))


def modes(e):
    return (e.rt.RAYS_INCOHERENT, e.rt.RAYS_ADAPTIVE, e.rt.RAYS_COHERENT)


def form_intersect(e, name, lengths=(None,)):
    """The plain closest hit follows the context's coherence setting like the
    any hit: per lane, packets for coherent waves only, packets."""
    c = e.var["classes"][name]
    ref, _, cnt, _ = RC.oracle_results(e.var, name)
    try:
        for mode in modes(e):
            e.rt.set_coherence(mode)
            for n in lengths:
                m = len(ref) if n is None else n
                hits = sentinel_hits(e, m)
                e.rt.intersect_scene(dev_rays(e, c, n), hits)
                e.rt.sync()
                same_hits(hits_of(e, hits), ref[:m], (name, mode, n, "intersect_scene"))
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)
    return hits_of(e, hits)  # the packet walk's, full length


def form_intersect_counted(e, name):
    c = e.var["classes"][name]
    ref, _, cnt, _ = RC.oracle_results(e.var, name)
    k = e.torch.zeros(3, dtype=e.torch.int64, device="cuda")
    hits = sentinel_hits(e, len(ref))
    e.rt.intersect_scene(dev_rays(e, c), hits, counters=k)
    e.rt.sync()
    same_hits(hits_of(e, hits), ref, (name, "intersect_scene counted"))
    if name in DEFAULT_EXTENTS:
        assert k.cpu().tolist() == [cnt["nodes"], cnt["tris"], cnt["visits"]], name


def form_intersect_masked(e, name):
    c = e.var["classes"][name]
    ref, _, _, _ = RC.oracle_results(e.var, name)
    rays = dev_rays(e, c)
    try:
        for mode in modes(e):
            e.rt.set_coherence(mode)
            for q, mask in enumerate(masks_for(len(ref), np.random.default_rng(11))):
                hits = sentinel_hits(e, len(ref))
                e.rt.intersect_scene_masked(rays, dev(e, mask), hits)
                e.rt.sync()
                got = hits_of(e, hits)
                on = mask == 1
                same_hits(got[on], ref[on], (name, mode, q, "intersect_scene_masked"))
                assert (got[~on].view(np.uint8) == 0xA5).all(), (name, mode, q)
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)


def form_occluded(e, name, lengths=(None,)):
    c = e.var["classes"][name]
    _, ref, _, cnt = RC.oracle_results(e.var, name)
    out = {}
    for mode in modes(e):
        e.rt.set_coherence(mode)
        for n in lengths:
            m = len(ref) if n is None else n
            occ = e.torch.full((m,), 9, dtype=e.torch.uint8, device="cuda")
            e.rt.occluded_scene(dev_rays(e, c, n), occ)
            e.rt.sync()
            same_occ(occ.cpu().numpy(), ref[:m], (name, mode, n, "occluded_scene"))
        out[mode] = occ.cpu().numpy()
    e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)
    if name in DEFAULT_EXTENTS:  # the counting build: the canonical per-lane walk
        k = e.torch.zeros(3, dtype=e.torch.int64, device="cuda")
        occ = e.torch.full((len(ref),), 9, dtype=e.torch.uint8, device="cuda")
        e.rt.occluded_scene(dev_rays(e, c), occ, counters=k)
        e.rt.sync()
        same_occ(occ.cpu().numpy(), ref, (name, "occluded_scene counted"))
        assert k.cpu().tolist() == [cnt["nodes"], cnt["tris"], cnt["visits"]], name
    return out


def form_occluded_masked(e, name):
    c = e.var["classes"][name]
    _, ref, _, _ = RC.oracle_results(e.var, name)
    rays = dev_rays(e, c)
    for q, mask in enumerate(masks_for(len(ref), np.random.default_rng(11))):
        occ = e.torch.full((len(ref),), 9, dtype=e.torch.uint8, device="cuda")
        e.rt.occluded_scene_masked(rays, dev(e, mask), occ)
        e.rt.sync()
        o = occ.cpu().numpy()
        same_occ(o[mask == 1], ref[mask == 1], (name, q, "occluded_scene_masked"))
        assert (o[mask == 0] == 9).all(), (name, q)


def form_fused(e, name):
    """The hit records of the fused shadow launches are intersect_scene's."""
    c = e.var["classes"][name]
    ref, _, _, _ = RC.oracle_results(e.var, name)
    n = len(ref)
    T = e.torch
    rays = dev_rays(e, c)
    shade = SHADE.copy()
    shade[:3] += np.float32(e.var["boxes"][0, 0])  # the light moves with the scene
    plain = sentinel_hits(e, n)
    e.rt.intersect_scene(rays, plain)
    h1 = sentinel_hits(e, n)
    occ = T.full((n,), 9, dtype=T.uint8, device="cuda")
    sv = T.full((n,), 7, dtype=T.uint8, device="cuda")
    e.rt.intersect_scene_shadow_pt(rays, h1, shade, occ, sv, None)
    h2 = sentinel_hits(e, n)
    srays = T.zeros(n * 32, dtype=T.uint8, device="cuda")
    valid = T.full((n,), 7, dtype=T.uint8, device="cuda")
    e.rt.intersect_scene_spawn_pt(rays, h2, shade, srays, valid, None)
    e.rt.sync()
    same_hits(hits_of(e, plain), ref, (name, "intersect_scene"))
    assert h1.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), (name, "shadow_pt")
    assert h2.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), (name, "spawn_pt")
    v = sv.cpu().numpy()
    assert np.array_equal(v, valid.cpu().numpy()) and set(np.unique(v)) <= {0, 1}
    assert not v[ref["domain"] < 0].any()  # a miss spawns nothing


def form_ooc(e, name, slots):
    c = e.var["classes"][name]
    ref, ref_occ, _, _ = RC.oracle_results(e.var, name)
    n = len(ref)
    T = e.torch
    oc = e.spray.OocCache(e.rt, slots)
    try:
        for i, (v, f) in enumerate(e.var["meshes"]):
            oc.set_domain(i, v, f, e.var["colors"][i], e.var["normals"][i])
        rays = dev_rays(e, c)
        hits = sentinel_hits(e, n)
        oc.intersect(rays, hits)
        e.rt.sync()
        same_hits(hits_of(e, hits), ref, (name, slots, "ooc intersect"))
        mask = (np.arange(n) % 5 != 2).astype(np.uint8)
        for mode in (e.rt.RAYS_INCOHERENT, e.rt.RAYS_COHERENT):  # fp32 per-lane walk, packet
            e.rt.set_coherence(mode)
            occ = T.full((n,), 9, dtype=T.uint8, device="cuda")
            oc.occluded(rays, dev(e, mask), occ)
            e.rt.sync()
            o = occ.cpu().numpy()
            same_occ(o[mask == 1], ref_occ[mask == 1], (name, slots, mode, "ooc occluded"))
            assert (o[mask == 0] == 9).all(), (name, slots, mode)
        assert oc.stats()["drains"] > 0
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)
        oc.close()


def between(share, what):
    assert 0 < share < 1, (what, share)


def form_occluded_order(e, name):
    """occluded_scene_order: the identity (order = NULL), a seeded
    permutation, and a device count below the buffer length (the entries
    beyond it untouched), per lane and adaptive."""
    c = e.var["classes"][name]
    _, ref, _, _ = RC.oracle_results(e.var, name)
    n = len(ref)
    T = e.torch
    between(ref.mean(), (name, "occluded share"))
    rays = dev_rays(e, c)
    perm = np.random.default_rng(23).permutation(n).astype(np.int32)
    k = 2 * n // 3 + 1  # no multiple of the wave
    try:
        for mode in (e.rt.RAYS_ADAPTIVE, e.rt.RAYS_INCOHERENT):
            e.rt.set_coherence(mode)
            for order in (None, perm):
                for count in (n, k):
                    occ = T.full((n,), 9, dtype=T.uint8, device="cuda")
                    cnt = T.full((1,), count, dtype=T.int32, device="cuda")
                    e.rt.occluded_scene_order(rays, n, None if order is None else dev_i32(e, order),
                                              cnt, occ)
                    e.rt.sync()
                    o = occ.cpu().numpy()
                    done = np.zeros(n, bool)
                    done[np.arange(count) if order is None else order[:count]] = True
                    what = (name, mode, order is not None, count, "occluded_scene_order")
                    same_occ(o[done], ref[done], what)
                    assert (o[~done] == 9).all(), what
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)


def dev_i32(e, a):
    return e.torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def form_occluded_devcount(e, name):
    c = e.var["classes"][name]
    _, ref, _, _ = RC.oracle_results(e.var, name)
    n = len(ref)
    T = e.torch
    rays = dev_rays(e, c)
    for count in (0, 1, 65, n):
        occ = T.full((n,), 9, dtype=T.uint8, device="cuda")
        cnt = T.full((1,), count, dtype=T.int32, device="cuda")
        e.rt.occluded_scene_devcount(rays, n, cnt, occ)
        e.rt.sync()
        o = occ.cpu().numpy()
        same_occ(o[:count], ref[:count], (name, count, "occluded_scene_devcount"))
        assert (o[count:] == 9).all(), (name, count)


def scene_shade(e):
    shade = SHADE.copy()
    shade[:3] += np.float32(e.var["boxes"][0, 0])  # the light moves with the scene
    return shade


def form_spawn_pt(e, name):
    """spawn_shadows_pt on the oracle's hits of the class against the
    oracle's spawn (count, sources, rays bit for bit); the spawned rays'
    any hit against the oracle's."""
    c = e.var["classes"][name]
    hits, _, _, _ = RC.oracle_results(e.var, name)
    n = len(hits)
    T = e.torch
    shade = scene_shade(e)
    so, sd, src = e.oracle.spawn_shadows_pt(c["org"], c["dir"], hits, shade[0:3], shade[3:6],
                                            shade[6:9], shade[9])
    srays = T.zeros(n * 32, dtype=T.uint8, device="cuda")
    osrc = T.full((n,), -1, dtype=T.int32, device="cuda")
    cnt = T.full((1,), 123, dtype=T.int32, device="cuda")
    e.rt.spawn_shadows_pt(dev_rays(e, c), dev(e, hits), n, shade, srays, osrc, cnt)
    e.rt.sync()
    m = int(cnt.item())
    assert m == len(so) and 0 < m < n, (name, m, len(so))
    assert np.array_equal(osrc[:m].cpu().numpy(), src), name
    sr = srays[: m * 32].cpu().numpy().view(e.spray.RAY_DTYPE)
    assert np.array_equal(sr["org"].view(np.uint32), so.view(np.uint32)), name
    assert np.array_equal(sr["dir"].view(np.uint32), sd.view(np.uint32)), name
    assert (sr["tnear"] == RC.TNEAR).all() and np.isinf(sr["tfar"]).all()
    ref, _ = e.var["osc"].occluded(so, sd)
    between(ref.mean(), (name, "occluded shadow rays"))
    occ = T.full((m,), 9, dtype=T.uint8, device="cuda")
    e.rt.occluded_scene(srays[: m * 32], occ)
    e.rt.sync()
    same_occ(occ.cpu().numpy(), ref, (name, "occluded_scene of spawn_shadows_pt"))


def form_ao(e, name, ns):
    """The AO chain on the oracle's hits of the class, two rays per pixel:
    spawn_shadows_ao against the oracle's spawn; _ordered and _traced as
    permutations of it; occluded_scene_order on both; the pairs form
    (spawn_shadows_ao_pairs + occluded_ao_pairs, and occluded_ao) with the
    traced spawn's (source, sample) pairs and the written rays' occlusion."""
    c = e.var["classes"][name]
    hits, _, _, _ = RC.oracle_results(e.var, name)
    n = len(hits)
    T = e.torch
    pix = (np.arange(n) // 2).astype(np.int32)
    npix = int(pix[-1]) + 1
    so, sd, src = e.oracle.spawn_shadows_ao(c["org"], c["dir"], pix, hits, ns)
    m = len(so)
    assert m > ns * n // 4, (name, m)
    ref, _ = e.var["osc"].occluded(so, sd)
    between(ref.mean(), (name, ns, "occluded AO rays"))
    rays, h, pixid = dev_rays(e, c), dev(e, hits), dev_i32(e, pix)
    what = (name, ns)

    def spawn(**kw):
        out = T.zeros((n * ns, 8), dtype=T.float32, device="cuda")
        osrc = T.full((n * ns,), -1, dtype=T.int32, device="cuda")
        cnt = T.full((1,), 123, dtype=T.int32, device="cuda")
        e.rt.spawn_shadows_ao(rays, h, pixid, n, ns, out, osrc, cnt, **kw)
        e.rt.sync()
        assert int(cnt.item()) == m, (what, kw.keys(), int(cnt.item()), m)
        return out, osrc[:m].cpu().numpy(), cnt

    def any_hit(out, order, cnt):
        occ = T.full((n * ns,), 9, dtype=T.uint8, device="cuda")
        e.rt.occluded_scene_order(out, n * ns, order, cnt, occ)
        e.rt.sync()
        o = occ.cpu().numpy()
        assert (o[m:] == 9).all(), what
        return o[:m]

    out, osrc, cnt = spawn()
    g = out[:m].cpu().numpy()
    assert np.array_equal(osrc, src), what
    assert g[:, 0:3].tobytes() == np.ascontiguousarray(so).tobytes(), what
    assert g[:, 4:7].tobytes() == np.ascontiguousarray(sd).tobytes(), what
    assert (g[:, 3] == RC.TNEAR).all() and np.isinf(g[:, 7]).all(), what
    try:
        e.rt.set_coherence(e.rt.RAYS_INCOHERENT)
        same_occ(any_hit(out, None, cnt), ref, (what, "identity"))
        # ordered: the same rays and a permutation of [0, m) as trace order
        order = T.full((n * ns,), -1, dtype=T.int32, device="cuda")
        out2, osrc2, cnt2 = spawn(order=order)
        assert out2[:m].cpu().numpy().tobytes() == g.tobytes() and np.array_equal(osrc2, src), what
        ordh = order[:m].cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(ordh), np.arange(m)), what
        same_occ(any_hit(out2, order, cnt2), ref, (what, "ordered"))
        # traced: the rays written in that order
        out3, osrc3, cnt3 = spawn(traced=True)
        assert out3[:m].cpu().numpy().tobytes() == g[ordh].tobytes(), what
        assert np.array_equal(osrc3, src[ordh]), what
        same_occ(any_hit(out3, None, cnt3), ref[ordh], (what, "traced"))
        # pairs: the traced order's (source, sample) pairs, the rays made in the lanes
        first = np.searchsorted(src, src)  # a hit spawns its samples in order
        sample = (np.arange(m) - first)[ordh]
        for fused in (False, True):
            pairs = T.full((n * ns,), -1, dtype=T.int32, device="cuda")
            lv = T.full((npix * ns, 4), float("nan"), dtype=T.float32, device="cuda")
            rec = T.full((n, 16), float("nan"), dtype=T.float32, device="cuda")
            pcnt = T.full((1,), 123, dtype=T.int32, device="cuda")
            occ = T.full((n * ns,), 9, dtype=T.uint8, device="cuda")
            if fused:
                e.rt.occluded_ao(rays, h, pixid, n, ns, pairs, lv, rec, pcnt, occ)
            else:
                e.rt.spawn_shadows_ao_pairs(rays, h, pixid, n, ns, pairs, lv, rec, pcnt)
                e.rt.occluded_ao_pairs(n * ns, pairs, rec, lv, ns, pcnt, occ)
            e.rt.sync()
            assert int(pcnt.item()) == m, (what, fused)
            fp = pairs[:m].cpu().numpy().view(np.uint32)
            assert np.array_equal((fp >> 5).astype(np.int64), src[ordh]), (what, fused)
            per = np.bincount(src, minlength=n)
            if (per[per > 0] == ns).all():  # every hit spawned every sample
                assert np.array_equal((fp & 31).astype(np.int64), sample), (what, fused)
            key = (fp >> 5).astype(np.int64) * 64 + (fp & 31)  # each sample of a source once
            assert len(np.unique(key)) == m and ((fp & 31) < ns).all(), (what, fused)
            o = occ.cpu().numpy()
            same_occ(o[:m], ref[ordh], (what, fused, "pairs"))
            assert (o[m:] == 9).all(), (what, fused)
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)


# ---- the tests ----
def test_occluded_scene_order(env):
    for name in NAMES:
        form_occluded_order(env, name)


def test_occluded_scene_devcount(env):
    for name in NAMES:
        form_occluded_devcount(env, name)


def test_spawn_shadows_pt(env):
    for name in NAMES:
        form_spawn_pt(env, name)


@pytest.mark.parametrize("ns", [4, 16])
def test_ao_chain(env, ns):
    """On the hits of `surface` (origins on coincident triangles), `edge` and
    `mixed`: at 1e4 the AO origin and frame are where the pairs form's
    16-float record must reproduce the written ray's bits."""
    for name in ("surface", "edge", "mixed"):
        form_ao(env, name, ns)


def test_per_slot_streams(env):
    """intersect1M / occluded1M of every slot, every class."""
    for name in NAMES:
        form_1m(env, name)


def test_segments_over_all_slots(env):
    for name in NAMES:
        form_segments(env, name)


def test_intersect_scene_modes(env):
    """The closest hit per lane, adaptive and as packets; `mixed` also at
    ragged lengths.  The float64 reference is applied to the packet walk's
    own records."""
    for name in NAMES:
        got = form_intersect(env, name, RAGGED + (None,) if name == "mixed" else (None,))
        RC.check_against_f64(env.var, name, got["domain"] >= 0, got["t"].astype(np.float64))


def test_intersect_scene_counted(env):
    """The per-lane canonical walk (the counting build) and its counters."""
    for name in NAMES:
        form_intersect_counted(env, name)


def test_intersect_scene_masked(env):
    for name in NAMES:
        form_intersect_masked(env, name)


def test_occluded_scene_modes(env):
    """Per-lane 4-wide quantized walk, adaptive, packet; `mixed` at ragged
    lengths; the float64 reference on the quantized walk's own bytes."""
    for name in NAMES:
        out = form_occluded(env, name, RAGGED + (None,) if name == "mixed" else (None,))
        RC.check_against_f64(env.var, name, out[env.rt.RAYS_INCOHERENT].astype(bool))


def test_occluded_scene_masked(env):
    for name in NAMES:
        form_occluded_masked(env, name)


def test_fused_shadow_launches(env):
    for name in NAMES:
        form_fused(env, name)


@pytest.mark.parametrize("slots", [2, 3])
def test_out_of_core(env, slots):
    """2 and 3 cache slots for the 9 domains: the packet closest-hit drain,
    the fp32 postponed-leaf any hit and the packet any-hit drain."""
    for name in NAMES:
        form_ooc(env, name, slots)


def test_nonfinite_records(env):
    """Records with a NaN or an infinity in org / dir, an all-zero direction,
    a NaN tnear or a NaN tfar, every fourth record of a batch of hitting
    rays: every form returns the oracle's bytes -- a miss, not occluded, the
    1M record untouched -- and the records in between are unaffected.  (Every
    walk's trip count depends on the tree and the domain list only: the
    stack walks pop one entry or clear one mask bit per step, the out-of-core
    pass drains each queued domain once.)"""
    c = env.var["classes"]["nonfinite"]
    ref, occ, _, _ = RC.oracle_results(env.var, "nonfinite")
    pl = c["planted"] >= 0
    assert (ref["domain"][pl] == -1).all() and not occ[pl].any()
    assert (ref["domain"][~pl] >= 0).all()
    form_1m(env, "nonfinite")
    form_segments(env, "nonfinite")
    form_intersect(env, "nonfinite", (65, None))
    form_intersect_counted(env, "nonfinite")
    form_intersect_masked(env, "nonfinite")
    form_occluded(env, "nonfinite", (65, None))
    form_occluded_masked(env, "nonfinite")
    form_fused(env, "nonfinite")
    form_ooc(env, "nonfinite", 2)
    form_ooc(env, "nonfinite", 3)

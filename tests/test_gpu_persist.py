"""The persistent body of the scene kernel -- 64 work queues over bands of
the batch, chunks of 64 or SPRAY_CHUNK_* rays, the next packet prefetched
into LDS, the next chunk dequeued from inside a packet's walk, the per-wave
shadow queue -- against the oracle on the hard ray classes of ray_cases.py,
bit for bit.  The other scene-path tests trace up to about 65,000 rays, which
the launcher runs as a plain grid (one packet per wave); here every batch is
large enough to persist, and RtContext.scene_launch_info() proves it did.

A batch is a tiling (persist_helpers.tiling) of a class of a few thousand
rays: whole copies of the class (coherent waves) followed by a seeded draw
with repetition (incoherent waves, non-finite and masked records next to
ordinary ones).  The expected value of every positional output is ref[sel]
with ref the oracle's results on the unique rays, computed once; the tiling
and the comparison run on the device.  Nothing is compared with another
launch of the kernels, except the list position in the keys of
intersect_scene_keyed (labelled there).

Sizes (persist_helpers.sizes, from the launched instantiation's resident grid
and chunk, read at run time): M_small, just above the persistence threshold,
dealt in packets; M_big, from which chunks are dealt, with every band ending
64 rays into a chunk; both with 37 live lanes in the last packet.  Every
output buffer has 64 more records or bytes than the batch, which must stay
untouched.

Scenes: S9, the nine-domain ray-case scene at the origin and at 1e4 (W 1,
16 stack entries); S100, 5 x 5 x 4 domains (W 4); Sdeep, a chain of 40,000
slivers (a tree deeper than 16: kStack entries)."""
import numpy as np
import pytest

import persist_helpers as PH
import ray_cases as RC
from conftest import SCENES, random_rays
from test_gpu_ray_cases import (DEFAULT_EXTENTS, SHADE, Env, dev_i32, hits_of, masks_for,
                                same_hits, same_occ, sentinel_hits)

pytestmark = pytest.mark.gpu

PAD = 64                       # records / bytes past the batch that must stay untouched
CAP = 1 << 24                  # ray capacity from which an any hit persists (kPersistAhRays)
EPI_NONE, EPI_SPAWN, EPI_KEYS, EPI_SHADOW = 0, 1, 2, 3  # the kernel's epilogues
MISS_KEY = 0x7FFFFFFFFFFFFFFF
KSTACK = 24                    # stack entries of a launch over a tree deeper than 16
SEED = 31
SMALL_COUNTS = (1, 63, 4133)   # device counts that leave most of the 64 queues empty


class Batch:
    """A class of n unique rays with the oracle's results on them."""

    def __init__(self, name, c, hits, occ):
        self.name, self.c, self.hits, self.occ, self.n = name, c, hits, occ, len(hits)
        self.dev = {}


# ---- scenes ----
def finish(e, torch, spray, oracle, rt, osc, shade, W, STK):
    e.torch, e.spray, e.oracle, e.rt, e.osc = torch, spray, oracle, rt, osc
    e.shade, e.W, e.STK = np.asarray(shade, np.float32), W, STK
    e.batches, e.big = {}, None
    # the batches are tiled, filled and compared by torch on the device: the
    # launches run on its stream, in order with that work (the context's own
    # stream is not ordered with it, and the allocator may hand a block that
    # a launch still writes to the next tensor)
    rt.set_stream(torch.cuda.current_stream())
    e.trav ={rt.RAYS_INCOHERENT: 0, rt.RAYS_COHERENT: 1, rt.RAYS_ADAPTIVE: 2}
    return e


def unload(e):
    e.big = None
    e.batches.clear()
    e.torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=(0.0, RC.LARGE), ids=["origin", "large"])
def env(request, oracle):
    """S9, as test_gpu_ray_cases.py builds it."""
    import torch
    import spray_amd
    e = Env()
    e.var = RC.variant(oracle, request.param)
    rt = spray_amd.RtContext(0)
    for i, (v, f) in enumerate(e.var["meshes"]):
        rt.upload_domain(i, v, f, e.var["colors"][i], e.var["normals"][i])
    rt.domain_bounds(e.var["boxes"])
    for i in range(RC.NDOM):
        rt.map_domain(i, i)
    shade = SHADE.copy()
    shade[:3] += np.float32(e.var["boxes"][0, 0])  # the light moves with the scene
    finish(e, torch, spray_amd, oracle, rt, e.var["osc"], shade, 1, 16)
    for name in ("mixed", "nonfinite") + DEFAULT_EXTENTS:
        h, o, _, _ = RC.oracle_results(e.var, name)
        e.batches[name] = Batch(name, e.var["classes"][name], h, o)
    yield e
    unload(e)
    rt.close()


def default_extents(org, d):
    n = len(org)
    return dict(org=np.ascontiguousarray(org, np.float32), dir=np.ascontiguousarray(d, np.float32),
                tnear=np.full(n, RC.TNEAR, np.float32), tfar=np.full(n, RC.TFAR, np.float32))


def oracle_batch(e, name, org, d):
    c = default_extents(org, d)
    h, _ = e.osc.intersect(c["org"], c["dir"])
    o, _ = e.osc.occluded(c["org"], c["dir"])
    e.batches[name] = Batch(name, c, h, o)


@pytest.fixture(scope="module")
def s100(oracle, tmp_path_factory):
    """The 5 x 5 x 4 wavelet domains of test_scene_more_than_64_domains: a
    128 x 64 tile of its camera at 2 spp and 2,000 random rays."""
    import torch
    import spray_amd
    lines = ["light point 0 500 1000 1 1 1", ""]
    for i in range(5):
        for j in range(4):
            for k in range(5):
                lines += ["domain", "file wavelet.ply", "mtl diffuse 1 1 1",
                          "bound -10.000000 -10.000000 -10.000000 10.000000 9.324713 10.000000",
                          "face 5480", "vertex 2840",
                          "translate %f %f %f" % (20.0 * i, 19.324713 * j, 20.0 * k), ""]
    desc = tmp_path_factory.mktemp("persist") / "wavelets100.spray"
    desc.write_text("\n".join(lines))
    sc = spray_amd.Scene(str(desc), SCENES, cache_size=-1, device=0)
    osc, doms, _ = oracle.load_scene(str(desc), SCENES)
    assert len(doms) == 100
    e = finish(Env(), torch, spray_amd, oracle, sc.rt, osc,
               [0, 500, 1000, 1, 1, 1, 0.4, 0.4, 0.4, 10.0], 4, 16)
    cam = oracle.camera_init([150.0, 120.0, 150.0], [40.0, 28.0, 40.0], [0, 1, 0], 60.0, 512, 512)
    org, d, _, _ = oracle.eye_rays_ooc(cam, 512, 2, (192, 160, 128, 64))
    ro, rd = random_rays(np.random.default_rng(77), 2000, np.array([40.0, 29.0, 40.0]), 90.0)
    oracle_batch(e, "camera+random", np.concatenate([org, ro]), np.concatenate([d, rd]))
    yield e
    unload(e)
    sc.close()


@pytest.fixture(scope="module")
def sdeep(oracle):
    """The nested-sliver chain of test_quantized_any_hit_deep_stack with its
    8,192 rays along the chain (half inside every box, past every triangle)."""
    import torch
    import spray_amd
    n = 40000
    x = (np.arange(n, dtype=np.float64) ** 3 / n ** 2).astype(np.float32)
    v = np.zeros((3 * n, 3), np.float32)
    v[0::3, 0] = x
    v[1::3, 0] = x + 1e-3
    v[1::3, 1] = 1e-3
    v[2::3, 2] = 1e-3
    v[2::3, 0] = x
    f = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    rt = spray_amd.RtContext(0)
    osc = oracle.Scene(1)
    rt.upload_domain(0, v, f)
    box = np.concatenate([v.min(0), v.max(0)]).astype(np.float32)
    osc.set_domain(0, v, f, np.zeros(len(v), np.uint32), np.zeros_like(v), box)
    rt.domain_bounds(box[None])
    rt.map_domain(0, 0)
    assert rt.slot_info(0)["depth"] > 16
    e = finish(Env(), torch, spray_amd, oracle, rt, osc, SHADE, 1, KSTACK)
    rng = np.random.default_rng(8)
    m = 8192
    st = rng.uniform(0.02, 0.98, size=(m, 2))
    miss = np.arange(m) % 2 == 0
    st[miss] = 1.0 - st[miss] * 0.45  # s + t > 1.1
    st[~miss] *= 0.45                 # s + t < 0.9
    org = np.zeros((m, 3), np.float32)
    org[:, 0] = np.where(np.arange(m) % 4 < 2, -1.0, float(x[-1]) + 1.0)
    org[:, 1:] = (st * 1e-3).astype(np.float32)
    d = np.zeros((m, 3), np.float32)
    d[:, 0] = np.where(org[:, 0] < 0, 1.0, -1.0)
    d[:, 1:] = rng.normal(scale=1e-9, size=(m, 2)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    oracle_batch(e, "chain", org, d)
    yield e
    unload(e)
    rt.close()


# ---- device helpers ----
def rows(e, a):
    """Host records as a [n, bytes per record] uint8 tensor on the device."""
    a = np.ascontiguousarray(a)
    return e.torch.from_numpy(a.view(np.uint8).reshape(len(a), -1)).cuda()


def records(e, c):
    return e.spray.make_rays(c["org"], c["dir"], c["tnear"], c["tfar"])


def on_dev(e, b, what):
    """The unique rays / oracle hits / oracle occlusion of b on the device."""
    if what not in b.dev:
        b.dev[what] = rows(e, {"rays": lambda: records(e, b.c), "hits": lambda: b.hits,
                               "occ": lambda: b.occ.astype(np.uint8)}[what]())
    return b.dev[what]


def tiled(e, b, M, seed=SEED):
    """(sel, sel on the device, the M tiled rays as flat bytes)."""
    sel = PH.tiling(b.n, M, seed)
    sel_d = e.torch.from_numpy(sel).cuda()
    return sel, sel_d, on_dev(e, b, "rays")[sel_d].reshape(-1)


def filled(e, n, byte):
    return e.torch.full((n,), byte, dtype=e.torch.uint8, device="cuda")


def launched(e, **want):
    """The last launch's host decisions, asserted; returns all of them."""
    info = e.rt.scene_launch_info()
    assert {k: info[k] for k in want} == want, (info, want)
    return info


def probe(e, b, launch, **want):
    """Step 1 of every form: the form on 64 rays runs the plain grid and
    leaves its instantiation's resident grid and chunk to read."""
    launch(on_dev(e, b, "rays")[:64].reshape(-1), 64)
    e.rt.sync()
    info = launched(e, persist=0, W=e.W, STK=e.STK, **want)
    assert info["grid"] > 0 and info["chunk"] in (128, 256), info
    return info


def size_of(info, which):
    m_small, m_big = PH.sizes(info["grid"], info["chunk"])
    M = m_small if which == "small" else m_big
    assert M % 64 == PH.RESIDUE and PH.persists(M, info["grid"])
    assert PH.small(M, info["grid"], info["chunk"]) == (which == "small")
    return M


def same_rows(e, got, exp, what):
    """Two [M, k] byte tensors on the device, equal or the first bad rows."""
    if e.torch.equal(got, exp):
        return
    bad = (got != exp).reshape(len(exp), -1).any(1).nonzero().reshape(-1)
    raise AssertionError((what, int(bad.numel()), bad[:8].tolist()))


def check_hits(e, b, sel, sel_d, buf, M, what):
    got = buf[: M * 48].view(M, 48)
    if not e.torch.equal(got, on_dev(e, b, "hits")[sel_d]):
        same_hits(hits_of(e, buf[: M * 48]), b.hits[sel], what)  # names field and rays
        raise AssertionError(what)
    assert bool((buf[M * 48:] == 0xA5).all()), (what, "records past the batch")


def untouched(buf, start, byte, what):
    assert bool((buf[start:] == byte).all()), (what, "bytes past the batch")


# ---- closest-hit forms ----
def form_intersect(e, name, mode, which):
    b = e.batches[name]
    e.rt.set_coherence(mode)
    try:
        def launch(rays, m):
            out = sentinel_hits(e, m + PAD)
            e.rt.intersect_scene(rays, out[: m * 48])
            return out
        info = probe(e, b, launch, ANY=0, EPI=EPI_NONE, TRAV=e.trav[mode])
        M = size_of(info, which)
        sel, sel_d, rays = tiled(e, b, M)
        hits = launch(rays, M)
        launched(e, persist=1, W=e.W, STK=e.STK, TRAV=e.trav[mode], ANY=0, EPI=EPI_NONE)
        e.rt.sync()
        check_hits(e, b, sel, sel_d, hits, M, (name, mode, which, M, "intersect_scene"))
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)
    return M


def form_counted(e, name):
    """k whole copies of the class and a prefix of it through the counting
    build (per lane, persistent): the counters are k times the oracle's of
    the class plus the oracle's of the prefix."""
    b = e.batches[name]
    T = e.torch

    def launch(rays, m):
        out = sentinel_hits(e, m + PAD)
        k = T.zeros(3, dtype=T.int64, device="cuda")
        e.rt.intersect_scene(rays, out[: m * 48], counters=k)
        return out, k
    info = probe(e, b, launch, ANY=0, EPI=EPI_NONE, TRAV=0)
    M = size_of(info, "small")
    copies, p = PH.copies_and_prefix(b.n, M)
    assert copies >= 2 and 0 < p < b.n
    _, whole = e.osc.intersect(b.c["org"], b.c["dir"], tnear=b.c["tnear"], tfar=b.c["tfar"])
    _, part = e.osc.intersect(b.c["org"][:p], b.c["dir"][:p], tnear=b.c["tnear"][:p],
                              tfar=b.c["tfar"][:p])
    sel = np.arange(M, dtype=np.int64) % b.n
    sel_d = T.from_numpy(sel).cuda()
    hits, k = launch(on_dev(e, b, "rays")[sel_d].reshape(-1), M)
    launched(e, persist=1, W=e.W, STK=e.STK, TRAV=0, ANY=0, EPI=EPI_NONE)
    e.rt.sync()
    check_hits(e, b, sel, sel_d, hits, M, (name, M, "intersect_scene counted"))
    want = [copies * whole[key] + part[key] for key in ("nodes", "tris", "visits")]
    assert k.cpu().tolist() == want, (name, M, k.cpu().tolist(), want)


def form_masked(e, name, mode):
    """The masked closest hit selects the valid rays into an index list with
    a device count: every such launch persists, whatever the count."""
    b = e.batches[name]
    T = e.torch
    e.rt.set_coherence(mode)
    try:
        def plain(rays, m):
            e.rt.intersect_scene(rays, sentinel_hits(e, m))
        info = probe(e, b, plain, ANY=0, EPI=EPI_NONE, TRAV=e.trav[mode])
        M = size_of(info, "small")
        sel, sel_d, rays = tiled(e, b, M)
        ref = on_dev(e, b, "hits")[sel_d]
        for q, mask in enumerate(masks_for(M, np.random.default_rng(11))):
            what = (name, mode, q, M, "intersect_scene_masked")
            hits = sentinel_hits(e, M + PAD)
            valid = T.from_numpy(np.concatenate([mask, np.ones(PAD, np.uint8)])).cuda()
            e.rt.intersect_scene_masked(rays, valid[:M], hits[: M * 48])
            launched(e, persist=1, W=e.W, STK=e.STK, TRAV=e.trav[mode], ANY=0, EPI=EPI_NONE)
            e.rt.sync()
            want = T.where(valid[:M, None] != 0, ref, T.full_like(ref, 0xA5))
            same_rows(e, hits[: M * 48].view(M, 48), want, what)
            untouched(hits, M * 48, 0xA5, what)
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)


def shadow_ref(e, b):
    """Per unique ray, from the oracle alone: whether its hit spawns a shadow
    ray, that ray's record and its occlusion (as form_spawn_pt of
    test_gpu_ray_cases.py); 0x5A bytes / 9 where nothing is spawned."""
    if "valid" not in b.dev:
        s = e.shade
        so, sd, src = e.oracle.spawn_shadows_pt(b.c["org"], b.c["dir"], b.hits, s[0:3], s[3:6],
                                                s[6:9], s[9])
        occ, _ = e.osc.occluded(so, sd)
        valid = np.zeros(b.n, np.uint8)
        valid[src] = 1
        pos_occ = np.full(b.n, 9, np.uint8)
        pos_occ[src] = occ
        srays = np.full((b.n, 32), 0x5A, np.uint8)
        srays[src] = e.spray.make_rays(so, sd, RC.TNEAR, RC.TFAR).view(np.uint8).reshape(-1, 32)
        b.shadow = dict(valid=valid, occ=pos_occ, n=len(src), occluded=occ)
        b.dev["valid"], b.dev["socc"], b.dev["srays"] = rows(e, valid), rows(e, pos_occ), rows(e, srays)
    return b.shadow


def form_fused(e, name, which, shadow):
    """intersect_scene_spawn_pt (shadow False) / intersect_scene_shadow_pt."""
    b = e.batches[name]
    T = e.torch
    shadow_ref(e, b)
    api = "intersect_scene_shadow_pt" if shadow else "intersect_scene_spawn_pt"
    epi = EPI_SHADOW if shadow else EPI_SPAWN

    def launch(rays, m):
        o = dict(hits=sentinel_hits(e, m + PAD), valid=filled(e, m + PAD, 7),
                 cnt=T.full((1,), 123, dtype=T.int32, device="cuda"))
        if shadow:
            o["occ"] = filled(e, m + PAD, 9)
            e.rt.intersect_scene_shadow_pt(rays, o["hits"][: m * 48], e.shade, o["occ"][:m],
                                           o["valid"][:m], o["cnt"])
        else:
            o["srays"] = filled(e, (m + PAD) * 32, 0x5A)
            e.rt.intersect_scene_spawn_pt(rays, o["hits"][: m * 48], e.shade,
                                          o["srays"][: m * 32], o["valid"][:m], o["cnt"])
        return o
    info = probe(e, b, launch, ANY=0, EPI=epi, TRAV=1)
    M = size_of(info, which)
    sel, sel_d, rays = tiled(e, b, M)
    o = launch(rays, M)
    launched(e, persist=1, W=e.W, STK=e.STK, TRAV=1, ANY=0, EPI=epi)
    e.rt.sync()
    what = (name, which, M, api)
    check_hits(e, b, sel, sel_d, o["hits"], M, what)
    same_rows(e, o["valid"][:M, None], b.dev["valid"][sel_d], what + ("valid",))
    untouched(o["valid"], M, 7, what)
    spawned = int(b.shadow["valid"][sel].sum())
    assert 0 < spawned < M and int(o["cnt"].item()) == spawned, (what, int(o["cnt"].item()), spawned)
    if shadow:  # positional occlusion of the spawned rays; 9 where none was spawned
        same_rows(e, o["occ"][:M, None], b.dev["socc"][sel_d], what + ("occ",))
        untouched(o["occ"], M, 9, what)
    else:       # the positional shadow rays; 0x5A where none was spawned
        same_rows(e, o["srays"][: M * 32].view(M, 32), b.dev["srays"][sel_d], what + ("rays",))
        untouched(o["srays"], M * 32, 0x5A, what)


def form_keyed(e, name):
    b = e.batches[name]
    T = e.torch

    def launch(rays, m):
        hits = sentinel_hits(e, m + PAD)
        keys = T.full((m + PAD,), 0x1111111111111111, dtype=T.int64, device="cuda")
        e.rt.intersect_scene_keyed(rays, hits[: m * 48], keys[:m])
        return hits, keys
    info = probe(e, b, launch, ANY=0, EPI=EPI_KEYS, TRAV=1)
    M = size_of(info, "small")
    # the keys of the unique rays, from a plain-grid launch of the same kernel
    _, ukeys = launch(on_dev(e, b, "rays").reshape(-1), b.n)
    launched(e, persist=0, EPI=EPI_KEYS)
    sel, sel_d, rays = tiled(e, b, M)
    hits, keys = launch(rays, M)
    launched(e, persist=1, W=e.W, STK=e.STK, TRAV=1, ANY=0, EPI=EPI_KEYS)
    e.rt.sync()
    what = (name, M, "intersect_scene_keyed")
    check_hits(e, b, sel, sel_d, hits, M, what)
    # against the oracle: t bits and domain of a hit's key, the miss key
    k = keys[:M].cpu().numpy()
    ref = b.hits[sel]
    hit = ref["domain"] >= 0
    assert hit.any() and not hit.all()
    assert (k[~hit] == MISS_KEY).all(), what
    assert np.array_equal(k[hit] & 0xFFFF, ref["domain"][hit].astype(np.int64)), what
    assert np.array_equal((k[hit] >> 32).astype(np.uint32), ref["t"][hit].view(np.uint32)), what
    # consistency between the two bodies of the kernel, not a comparison with
    # the oracle: the whole key, list position included, is the plain grid's
    assert T.equal(keys[:M], ukeys[: b.n][sel_d]), what
    assert bool((keys[M:] == 0x1111111111111111).all()), what


# ---- any-hit forms (a device count over a buffer of CAP rays: persistent) ----
def big_rays(e):
    if e.big is None:
        e.big = e.torch.empty(CAP * 32, dtype=e.torch.uint8, device="cuda")
    return e.big


def any_hit(e, b, api, count, seed=SEED):
    """One launch over `count` tiled rays; returns its launch info.
    api: devcount | order (order = None) | perm (count of count + PAD rays, in
    the order of a seeded permutation: the entries it leaves out stay 9)."""
    T = e.torch
    L = count + PAD if api == "perm" else count
    sel, sel_d, rays = tiled(e, b, L, seed)
    big = big_rays(e)
    big[: L * 32] = rays
    occ = filled(e, CAP, 9)
    cnt = T.full((1,), count, dtype=T.int32, device="cuda")
    ref = on_dev(e, b, "occ")[sel_d].reshape(-1)
    if api == "devcount":
        e.rt.occluded_scene_devcount(big, CAP, cnt, occ)
    elif api == "order":
        e.rt.occluded_scene_order(big, CAP, None, cnt, occ)
    else:
        perm = np.random.default_rng(23).permutation(L).astype(np.int32)
        e.rt.occluded_scene_order(big, CAP, dev_i32(e, perm), cnt, occ)
        done = T.zeros(L, dtype=T.bool, device="cuda")
        done[T.from_numpy(perm[:count].astype(np.int64)).cuda()] = True
        ref = T.where(done, ref, T.full_like(ref, 9))
    info = e.rt.scene_launch_info()
    e.rt.sync()
    what = (b.name, api, count)
    if not T.equal(occ[:L], ref):
        same_occ(occ[:L].cpu().numpy(), ref.cpu().numpy(), what)
    untouched(occ, L, 9, what)
    return info


def form_any_hit(e, name, mode, api, big=False):
    b = e.batches[name]
    e.rt.set_coherence(mode)
    want = dict(W=e.W, STK=e.STK, TRAV=e.trav[mode], ANY=1, EPI=EPI_NONE)
    try:
        # below CAP rays and without a count: the plain grid
        e.rt.occluded_scene(on_dev(e, b, "rays")[:64].reshape(-1), filled(e, 64, 9))
        launched(e, persist=0, **want)
        sizes = None
        for count in SMALL_COUNTS + ("small",) + (("big",) if big else ()):
            if isinstance(count, str):
                count = size_of(sizes, count)
            info = any_hit(e, b, api, count)
            assert {k: info[k] for k in want} == want and info["persist"] == 1, (info, want)
            assert info["grid"] > 0 and info["chunk"] in (128, 256), info
            sizes = info  # the persistent launches computed the instantiation's grid
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)


# ---- the tests: S9 ----
S9 = ("mixed", "nonfinite")
MODES = ("incoherent", "adaptive", "coherent")


def mode_of(e, m):
    return {"incoherent": e.rt.RAYS_INCOHERENT, "adaptive": e.rt.RAYS_ADAPTIVE,
            "coherent": e.rt.RAYS_COHERENT}[m]


@pytest.mark.parametrize("mode", MODES)
def test_intersect_scene(env, mode):
    """Per lane, adaptive, packets at M_small; the packets also at M_big: the
    in-chunk LDS prefetch and the band end inside a chunk."""
    for name in S9:
        form_intersect(env, name, mode_of(env, mode), "small")
        if mode == "coherent":
            form_intersect(env, name, mode_of(env, mode), "big")


def test_intersect_scene_counted(env):
    for name in ("axis_lattice", "random"):
        assert name in DEFAULT_EXTENTS
        form_counted(env, name)


@pytest.mark.parametrize("mode", MODES)
def test_intersect_scene_masked(env, mode):
    for name in S9:
        form_masked(env, name, mode_of(env, mode))


@pytest.mark.parametrize("which", ["small", "big"])
def test_intersect_scene_spawn_pt(env, which):
    for name in S9:
        form_fused(env, name, which, shadow=False)


@pytest.mark.parametrize("which", ["small", "big"])
def test_intersect_scene_shadow_pt(env, which):
    """The per-wave shadow queue with partial packets and its flush at the
    end of the wave."""
    for name in S9:
        form_fused(env, name, which, shadow=True)


def test_intersect_scene_keyed(env):
    for name in S9:
        form_keyed(env, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("api", ["devcount", "order", "perm"])
def test_occluded_scene_counts(env, api, mode):
    """occluded_scene_devcount, occluded_scene_order with order = None and
    with a seeded permutation, at device counts 1, 63, 4,133, M_small and
    (packets and per lane) M_big of the any-hit chunk."""
    for name in S9:
        form_any_hit(env, name, mode_of(env, mode), api, big=mode != "adaptive")


# ---- S100: four mask words ----
def test_s100_intersect_scene(s100):
    for which in ("small", "big"):
        form_intersect(s100, "camera+random", s100.rt.RAYS_COHERENT, which)


def test_s100_shadow_pt(s100):
    for which in ("small", "big"):
        form_fused(s100, "camera+random", which, shadow=True)


def test_s100_occluded_devcount(s100):
    form_any_hit(s100, "camera+random", s100.rt.RAYS_COHERENT, "devcount", big=True)


# ---- Sdeep: kStack stack entries ----
@pytest.mark.parametrize("mode", ["coherent", "incoherent"])
def test_sdeep_intersect_scene(sdeep, mode):
    form_intersect(sdeep, "chain", mode_of(sdeep, mode), "small")


@pytest.mark.parametrize("mode", MODES)
def test_sdeep_occluded_devcount(sdeep, mode):
    form_any_hit(sdeep, "chain", mode_of(sdeep, mode), "devcount")


# ---- the batches are what the forms are there for ----
def shapes(e, name, sizes, domains=None, past=None):
    b = e.batches[name]
    shadow_ref(e, b)
    for M in sizes:
        assert M % 64 == 37  # a last packet with 37 live lanes
        sel = PH.tiling(b.n, M, SEED)
        for part in PH.halves(b.n, M):
            dom = b.hits["domain"][sel[part]]
            assert (dom < 0).any() and (dom >= 0).any(), (name, M)
            if domains:
                assert len(np.unique(dom[dom >= 0])) >= domains, (name, M)
            if past:
                assert (dom >= past).sum() > 1000, (name, M)
            assert 0 < b.occ[sel[part]].mean() < 1, (name, M)
            v = b.shadow["valid"][sel[part]]
            assert 0 < v.sum() < len(v), (name, M)
            so = b.shadow["occ"][sel[part]][v == 1]
            assert 0 < so.mean() < 1, (name, M)


def grid_sizes(e, name, mode, any_hit_=False):
    """(M_small, M_big) of the plain closest hit's or the any hit's
    instantiation, from a launch that computes its grid."""
    b = e.batches[name]
    e.rt.set_coherence(mode)
    try:
        if any_hit_:
            info = any_hit(e, b, "devcount", 1)
        else:
            e.rt.intersect_scene(on_dev(e, b, "rays")[:64].reshape(-1), sentinel_hits(e, 64))
            info = e.rt.scene_launch_info()
    finally:
        e.rt.set_coherence(e.rt.RAYS_ADAPTIVE)
    assert info["grid"] > 0
    return PH.sizes(info["grid"], info["chunk"])


def test_batch_shapes(env):
    """Both parts of every S9 batch hold hits in at least 8 domains and
    misses, both occlusion outcomes, rays that spawn a shadow ray and rays
    that do not, occluded and unoccluded shadow rays; `nonfinite` keeps every
    kind of planted record in both parts."""
    ch = grid_sizes(env, "mixed", env.rt.RAYS_COHERENT)
    ah = grid_sizes(env, "mixed", env.rt.RAYS_COHERENT, any_hit_=True)
    for name in S9:
        shapes(env, name, ch + ah, domains=8)
    planted = env.var["classes"]["nonfinite"]["planted"]
    for M in ch + ah:
        sel = PH.tiling(len(planted), M, SEED)
        for part in PH.halves(len(planted), M):
            assert set(planted[sel[part]].tolist()) == set(range(-1, len(RC.PLANTS))), M


def test_batch_shapes_s100(s100):
    """Hits in the domains past the first mask word in both parts."""
    ch = grid_sizes(s100, "camera+random", s100.rt.RAYS_COHERENT)
    ah = grid_sizes(s100, "camera+random", s100.rt.RAYS_COHERENT, any_hit_=True)
    shapes(s100, "camera+random", ch + ah, past=64)


def test_batch_shapes_sdeep(sdeep):
    """The window of test_quantized_any_hit_deep_stack on the occluded share,
    on the tiled batch."""
    b = sdeep.batches["chain"]
    ch = grid_sizes(sdeep, "chain", sdeep.rt.RAYS_COHERENT)
    ah = grid_sizes(sdeep, "chain", sdeep.rt.RAYS_COHERENT, any_hit_=True)
    for M in (ch[0], ah[0]):
        assert M % 64 == 37
        sel = PH.tiling(b.n, M, SEED)
        assert 0.3 < b.occ.mean() < 0.7 and 0.3 < b.occ[sel].mean() < 0.7
        assert 0 < (b.hits["domain"][sel] >= 0).mean() < 1

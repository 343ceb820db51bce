"""CPU tests of the scene oracle's per-ray extents and of the hard ray
classes of ray_cases.py: the oracle -- whose bytes the HIP kernels must
reproduce -- is held to a float64 brute force on every class, not only on
random rays over one mesh (test_oracle.py)."""
import os

import numpy as np
import pytest

import ray_cases as RC
from conftest import SCENES, WAVELETS64, axis_rays, edge_rays, random_rays

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INV = 0xFFFFFFFF
OFFSETS = (0.0, RC.LARGE)


@pytest.fixture(scope="module", params=OFFSETS, ids=["origin", "large"])
def var(request, oracle):
    return RC.variant(oracle, request.param)


# ---- the extension itself ----
def test_null_extents_reproduce_golden_vectors(oracle):
    """NULL extents, and the defaults passed per ray, give the bytes of the
    two golden vector files."""
    g = np.load(os.path.join(GOLDEN, "vectors_wavelets64.npz"))
    sc, _, _ = oracle.load_scene(WAVELETS64, SCENES)
    n = len(g["org"])
    for tn, tf in ((None, None), (np.full(n, 0.001, np.float32), np.full(n, np.inf, np.float32))):
        h, _ = sc.intersect(g["org"], g["dir"], tnear=tn, tfar=tf)
        assert np.array_equal(h.view(np.uint8).reshape(-1, 48), g["hits"])
    m = len(g["shadow_org"])
    for tn, tf in ((None, None), (np.full(m, 0.001, np.float32), np.full(m, np.inf, np.float32))):
        o, _ = sc.occluded(g["shadow_org"], g["shadow_dir"], tnear=tn, tfar=tf)
        assert np.array_equal(o, g["occluded"])
    # the single-domain vectors through a one-domain scene
    g = np.load(os.path.join(GOLDEN, "vectors_wavelet.npz"))
    v, f, c = oracle.load_ply(os.path.join(SCENES, "wavelet.ply"))
    one = oracle.Scene(1)
    one.set_domain(0, v, f, c, np.zeros_like(v), np.concatenate([v.min(0), v.max(0)]))
    h, _ = one.intersect(g["org"], g["dir"])
    assert np.array_equal(h["prim"], g["prim"])
    hit = g["prim"] != INV
    assert np.isinf(h["t"][~hit]).all()
    for k in ("t", "u", "v"):
        assert np.array_equal(h[k][hit].view(np.uint32), g[k][hit].view(np.uint32)), k
    o, _ = one.occluded(g["org"], g["dir"])
    assert np.array_equal(o, g["occluded"])


def test_one_domain_scene_equals_bvh_with_extents(oracle):
    """On a one-domain scene the extended queries are Bvh.intersect /
    Bvh.occluded with the same extents, bit for bit (a miss: t = +inf in the
    scene record, the ray's tfar in the Bvh's)."""
    v, f, c = oracle.load_ply(os.path.join(SCENES, "wavelet.ply"))
    rng = np.random.default_rng(41)
    ctr = (v.min(0) + v.max(0)) / 2
    o1, d1 = random_rays(rng, 3000, ctr, 25.0)
    o2, d2 = edge_rays(rng, v, f, 1500)
    o3, d3 = axis_rays(v, 300)
    org, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    n = len(org)
    bvh = oracle.Bvh(v, f)
    t0, _, _, p0, _ = bvh.intersect(org, d)
    tnear = np.full(n, 0.001, np.float32)
    tfar = np.full(n, np.inf, np.float32)
    tnear[::7] = 5.0
    tfar[::5] = 30.0
    k = np.arange(n)
    tfar[k % 6 == 1] = t0[k % 6 == 1]                           # t == tfar
    tfar[k % 6 == 2] = np.nextafter(t0[k % 6 == 2], np.float32(0))
    tnear[k % 6 == 3] = np.where(np.isfinite(t0[k % 6 == 3]), t0[k % 6 == 3], 0.001)
    one = oracle.Scene(1)
    one.set_domain(0, v, f, c, np.zeros_like(v), np.concatenate([v.min(0), v.max(0)]))
    h, hc = one.intersect(org, d, tnear=tnear, tfar=tfar)
    bt, bu, bv, bp, bc = bvh.intersect(org, d, tnear, tfar)
    hit = bp != INV
    assert 0.2 < hit.mean() < 0.9
    assert np.array_equal(h["prim"], bp) and np.array_equal(h["domain"] >= 0, hit)
    for a, b in ((h["t"], bt), (h["u"], bu), (h["v"], bv)):
        assert np.array_equal(a[hit].view(np.uint32), b[hit].view(np.uint32))
    assert np.isinf(h["t"][~hit]).all() and np.array_equal(bt[~hit], tfar[~hit])
    o, _ = one.occluded(org, d, tnear=tnear, tfar=tfar)
    bo, _ = bvh.occluded(org, d, tnear, tfar)
    assert np.array_equal(o, bo) and np.array_equal(o.astype(bool), hit)


# ---- the classes ----
def test_scene_is_what_the_classes_need(var):
    meshes, boxes = var["meshes"], var["boxes"]
    assert len(meshes) == RC.NDOM and all(90 <= len(f) <= 130 for _, f in meshes)
    tri = [set(map(lambda t: tuple(sorted(map(tuple, t))), v[f].tolist())) for v, f in meshes[:8]]
    shared = sum(len(tri[a] & tri[b]) > 0 for a in range(8) for b in range(a + 1, 8))
    assert shared >= 8  # coincident triangles in pairs of touching domains
    for v, f in meshes[:8]:
        assert np.array_equal(v, np.round(v))
        assert len(set(map(lambda t: tuple(sorted(map(tuple, t))), v[f].tolist()))) <= len(f)
    assert any(boxes[a, 3 + ax] == boxes[b, ax] for a in range(8) for b in range(8)
               for ax in range(3))  # boxes touching in a plane


# the largest ambiguous share a class may have (0.70: at least 30 % robust)
CAPS = {"axis_off": 0.01, "tiny": 0.01, "surface": 0.01, "extents": 0.01, "random": 0.01,
        "axis_lattice": 0.70, "edge": 0.70, "mixed": None}
BOUNDARY = (0, 1, 2)  # EXTENT_CASES whose extent sits on a hit by construction


@pytest.mark.parametrize("name", RC.CLASSES + ("mixed",))
def test_oracle_matches_float64_on_class(var, name):
    """Robust rays: the oracle's hit or miss is the float64 reference's and
    its t is within 1e-4 relative.  The ambiguous share is capped, so that
    the classification cannot hide a failure: at most 1 % of axis_off, tiny,
    surface, extents and random, at least 30 % robust of axis_lattice and
    edge.

    Measured ambiguous shares (seed 7, 1024 rays per class; scene at the
    origin / translated by 1e4): axis_off 0 / 0.10 %, tiny 0 / 0.20 %,
    surface 0.10 % / 0.10 %, random 0.20 % / 0, axis_lattice 59.6 % / 59.6 %,
    edge 40.6 % / 27.9 %, mixed 19.8 % / 18.0 % (no cap); no mismatch on a
    robust ray, worst relative t error 6.7e-7.  Hit shares: axis_off 48 %,
    axis_lattice 59 %, tiny 48 %, edge 96 %, surface 72 %, extents 62 %,
    random 68 %, mixed 65 %.

    extents: the sub-cases tfar = t1, tfar = nextafter(t1, 0) and tnear = t1
    put an extent exactly on a hit, which the reference's own rule (a hit
    within 1e-4 relative of an extent) makes ambiguous, all of them; they are
    decided exactly by test_extents_class_semantics instead, and the 1 % cap
    is asserted over the other five sub-cases (measured 0 / 0.16 %)."""
    c = var["classes"][name]
    h, o, _, _ = RC.oracle_results(var, name)
    hit = h["domain"] >= 0
    assert np.array_equal(o.astype(bool), hit)  # any hit == closest hit exists
    amb = RC.check_against_f64(var, name, hit, h["t"].astype(np.float64))
    if name == "extents":
        by_design = np.isin(c["case"], BOUNDARY)
        assert amb[by_design].all()
        amb = amb[~by_design]
    share = amb.mean()
    print("%s: %d rays, hit share %.3f, ambiguous share %.4f" % (name, len(hit), hit.mean(), share))
    if CAPS[name] is not None:
        assert share <= CAPS[name], (name, share)
    if name == "edge":  # aimed at the surface: nearly every ray hits
        assert 0 < hit.sum() < len(hit)
    else:
        assert 0.05 < hit.mean() < 0.95, (name, hit.mean())


def test_extents_class_semantics(oracle, var):
    """What each sub-case of `extents` must give, stated from the oracle's
    own hits under the default extents (bit for bit)."""
    c = var["classes"]["extents"]
    osc = var["osc"]
    h, o, _, _ = RC.oracle_results(var, "extents")
    h1, _ = osc.intersect(c["org"], c["dir"])
    assert np.array_equal(h1["t"], c["t1"])
    case = c["case"]
    hit = h["domain"] >= 0
    assert np.array_equal(o.astype(bool), hit)
    for k in (0, 6, 7):  # tfar = t1 accepted; tnear = 0 / -1: the default hit
        s = case == k
        assert s.sum() > 50 and h[s].tobytes() == h1[s].tobytes(), RC.EXTENT_CASES[k]
    for k in (1, 4, 5):  # tfar just below t1, tfar < tnear, tfar = 0: misses
        s = case == k
        assert s.sum() > 50 and not hit[s].any(), RC.EXTENT_CASES[k]
    s = case == 2  # tnear = t1 is strict: the next surface, or none
    assert s.sum() > 50 and (h["t"][s] > c["t1"][s]).all() and hit[s].mean() > 0.5
    s = case == 3  # a hit of a later list entry only
    ids, _, cnt, _ = oracle.domain_query(c["org"][s], c["dir"][s], var["boxes"], RC.NDOM)
    assert s.sum() > 50 and hit[s].all()
    assert ((h["t"][s] > c["tnear"][s]) & (h["t"][s] <= c["tfar"][s])).all()
    pos = np.array([list(ids[r, :cnt[r]]).index(d) for r, d in enumerate(h["domain"][s])])
    assert (pos >= 1).all() and (h["domain"][s] != h1["domain"][s]).all()


def test_classes_reach_the_cross_domain_tie_rule(oracle, var):
    """The coincident triangles of touching domains are hit: winning hits
    with the same t, bit for bit, in two domains, and among them ties that
    the smaller domain id does not win (the earlier entry of the domain list
    does).  Measured (scene at the origin / translated): 130 / 115 ties,
    59 / 50 of them won by the larger id; the floors asserted are about half
    of that, enough for the rule to be exercised on every run."""
    bvh = [oracle.Bvh(v, f) for v, f in var["meshes"]]
    ties = by_list = 0
    for name in RC.CLASSES:
        c = var["classes"][name]
        h, _, _, _ = RC.oracle_results(var, name)
        per = [b.intersect(c["org"], c["dir"], c["tnear"], c["tfar"]) for b in bvh]
        same = np.stack([(p[0] == h["t"]) & (p[3] != INV) for p in per], 1)
        tie = (h["domain"] >= 0) & (same.sum(1) >= 2)
        assert same[np.flatnonzero(h["domain"] >= 0), h["domain"][h["domain"] >= 0]].all()
        ties += tie.sum()
        by_list += (tie & (same.argmax(1) != h["domain"])).sum()
    print("ties %d, won by the larger id %d" % (ties, by_list))
    assert ties >= 60 and by_list >= 20


def test_nonfinite_records_miss_and_leave_neighbours_alone(var):
    """A record with a NaN or an infinity in it, an all-zero direction, a
    NaN tnear or a NaN tfar is a miss and not occluded; the records around
    it keep the results they have without it."""
    c = var["classes"]["nonfinite"]
    osc = var["osc"]
    h, o, _, _ = RC.oracle_results(var, "nonfinite")
    pl = c["planted"] >= 0
    assert pl.sum() >= len(RC.PLANTS) * 8 and set(c["planted"][pl]) == set(range(len(RC.PLANTS)))
    miss = np.zeros(1, h.dtype)
    miss["t"], miss["prim"], miss["domain"] = np.inf, INV, -1
    assert h[pl].tobytes() == np.repeat(miss, pl.sum()).tobytes()
    assert not o[pl].any()
    keep = ~pl
    h2, _ = osc.intersect(c["org"][keep], c["dir"][keep])
    o2, _ = osc.occluded(c["org"][keep], c["dir"][keep])
    assert h[keep].tobytes() == h2.tobytes() and np.array_equal(o[keep], o2)
    assert (h2["domain"] >= 0).all()

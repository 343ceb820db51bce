"""The host restatements of the glyph filter (spray_rt_glyphs_host,
spray_rt_glyph_sphere_host) against numpy, byte for byte, and the properties
of the meshes: no GPU.

The numpy side (glyph_helpers.py) is written from the rule in
include/spray_rt.h and counts the paths the cases reach.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import glyph_helpers as gh

F32, F64 = np.float32, np.float64
ERR_ARG, ERR_LIMIT = -1, -5


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def cases():
    return gh.small_cases()


def colour_modes(S, G, seed):
    """The set and glyph with a mapped colour, a constant colour and none."""
    return ((gh.with_color(S, seed), G), (S, dict(G, color=0x00123456 + seed)), (S, dict(G, color=None)))


def test_both_shapes_equal_numpy_byte_for_byte(spray, cases):
    st = collections.Counter()
    shapes = collections.Counter()
    for seed, name in enumerate(sorted(cases)):
        S0, G0 = cases[name]
        for S, G in colour_modes(S0, G0, seed):
            ref = gh.glyphs_numpy(S, G, spray, stats=st)
            for _ in range(2):   # twice
                got = spray.glyphs_host(S, G)
                for k, (a, b) in enumerate(zip(ref, got)):
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, k)
            v, n, c, f, ids = spray.glyphs_host(S, G, normals=False, point_ids=False)
            assert n is None and ids is None
            assert (v.tobytes(), c.tobytes(), f.tobytes()) == (ref[0].tobytes(), ref[2].tobytes(),
                                                             ref[3].tobytes()), name
            assert spray.glyphs_host(S, G, count_only=True) == (len(ref[0]), len(ref[3]))
            V, F = gh.per_glyph(G)
            assert len(ref[0]) == V * len(ref[4]) and len(ref[3]) == F * len(ref[4])
            shapes[G["shape"], G.get("level"), G.get("nsides")] += len(ref[4])
    # every path of the rule is reached
    for key in ("off_stride", "select_on_lo", "select_on_hi", "select_out", "s_zero", "s_overflow",
                "s_subnormal", "speed_low", "speed_overflow", "square_underflow", "axis_tie",
                "axis_0", "axis_1", "axis_2", "kept"):
        assert st[key] > 0, key
    for lv in range(4):
        assert shapes[gh.SPHERE, lv, None] > 0
    for ns in range(3, 17):
        assert shapes[gh.ARROW, None, ns] > 0


def test_keep_rule_cases(spray, cases):
    ids = lambda name: list(spray.glyphs_host(*cases[name])[4])
    assert ids("n0") == [] and ids("n0_arrow") == [] and ids("n1") == [0] and ids("n1_arrow") == [0]
    assert ids("all_dropped") == [] and ids("first_only") == [0] and ids("last_only") == [6]
    assert ids("stride1") == list(range(7)) and ids("stride2") == [0, 2, 4, 6]
    assert ids("stride3") == [0, 3, 6] and ids("stride8") == [0]
    assert ids("stride3_arrow") == [0, 3, 6]
    assert ids("select_edges") == [1, 2, 3, 4, 5]        # lo and hi themselves are inside
    assert ids("select_point") == [1, 3, 6]              # lo == hi
    assert ids("select_zero") == [0, 1, 6] and ids("select_negzero") == [0, 1, 6]   # -0.0 == 0.0
    assert ids("scales") == [1, 2, 3, 6]                 # 0 and -0 dropped, subnormal kept, overflow dropped
    assert ids("scales_arrow") == [1, 2, 3, 6]
    # the speed one float below the smallest min_speed is dropped, at it and above kept
    # (0, 3 dropped), d overflowing dropped (5), a large d that does not kept (6), zero dropped (10)
    assert ids("speeds_0") == [1, 2, 4, 6, 7, 8, 9] and ids("speeds_1") == [1, 2, 4, 6, 7, 8, 9]
    # 1e27 * 1e19 overflows, 1e-33 * 2e-19 underflows to zero, 1e-33 * 1e10 does not
    assert ids("length_range") == [2, 3]
    assert len(ids("ties_0")) == len(gh.tie_vectors())


def test_empty_results_and_sizes(spray, cases):
    for name in ("n0", "n0_arrow", "all_dropped"):
        v, n, c, f, ids = spray.glyphs_host(*cases[name])
        assert v.shape == (0, 3) and n.shape == (0, 3) and c.shape == (0,) and f.shape == (0, 3)
        assert ids.shape == (0,)


@pytest.mark.parametrize("level", range(4))
def test_sphere_table(spray, level):
    v, f = spray.glyph_sphere(level)
    assert v.dtype == F32 and f.dtype == np.uint32
    assert v.shape == (10 * 4 ** level + 2, 3) and f.shape == (20 * 4 ** level, 3)
    ok, chi = gh.closed_oriented(f, len(v))
    assert ok and chi == 2 and len(np.unique(f)) == len(v)
    ng = gh.geometric_normals(v, f)
    centre = v[f].astype(F64).mean(1)
    assert (np.einsum("ij,ij->i", ng, centre) > 0).all()
    # within 1 ulp (of float32, at 1) of unit length, in float64 terms, after the cast
    assert np.abs(np.linalg.norm(v.astype(F64), axis=1) - 1.0).max() <= 2.0 ** -23
    if level:   # a subdivision keeps the vertices of the level below, in place
        v0, _ = spray.glyph_sphere(level - 1)
        assert v[:len(v0)].tobytes() == v0.tobytes()
    assert spray.glyph_sphere(level)[0].tobytes() == v.tobytes()


def test_sphere_table_errors(spray):
    for level in (-1, 4):
        with pytest.raises(spray.SprayRtError) as e:
            spray.glyph_sphere(level)
        assert e.value.code == ERR_ARG


def arrow_sets():
    tv = gh.tie_vectors()
    p = gh.cloud(40, 9)
    out = [(gh.pset(gh.cloud(len(tv), 4), vectors=tv), gh.arrow(0.5, ns, ns % 2 == 1)) for ns in (3, 4, 16)]
    out += [(gh.pset(p, vectors=gh.swirl(p, ns)), gh.arrow(0.75, ns, ns % 2 == 0)) for ns in range(3, 17)]
    return out


def test_arrows_are_closed_and_point_outward(spray):
    for S, G in arrow_sets():
        ns = G["nsides"]
        V, F = gh.per_glyph(G)
        v, n, c, f, ids = spray.glyphs_host(S, G)
        assert len(ids) == len(S["points"])
        vec = S["vectors"].astype(F64)
        T = vec / np.linalg.norm(vec, axis=1, keepdims=True)
        for g in range(len(ids)):
            fg = f[g * F:(g + 1) * F].astype(np.int64) - g * V
            assert fg.min() == 0 and fg.max() == V - 1
            vg = v[g * V:(g + 1) * V]
            # the ns tip vertices share one position: one vertex of the surface
            assert len({vg[3 * ns + k].tobytes() for k in range(ns)}) == 1
            weld = np.where((fg >= 3 * ns) & (fg < 4 * ns), 3 * ns, fg)
            ok, chi = gh.closed_oriented(weld, V)
            assert ok and chi == 2
            ng = gh.geometric_normals(vg, fg)
            ng /= np.linalg.norm(ng, axis=1, keepdims=True)
            centre = vg[fg].astype(F64).mean(1) - S["points"][g].astype(F64)
            radial = centre - (centre @ T[g])[:, None] * T[g]
            radial /= np.linalg.norm(radial, axis=1, keepdims=True)
            away = np.einsum("ij,ij->i", ng, radial)
            along = ng @ T[g]
            shaft, annulus = slice(0, 2 * ns), slice(2 * ns, 4 * ns)
            cone, tail = slice(4 * ns, 5 * ns), slice(5 * ns, 6 * ns)
            assert (away[shaft] > 0.8).all() and (np.abs(along[shaft]) < 1e-3).all()
            assert (away[cone] > 0.9).all() and (along[cone] > 0.1).all()
            assert (along[annulus] < -0.999).all() and (along[tail] < -0.999).all()
            # vertex normals: unit, away from the axis or along -T
            nn = n[g * V:(g + 1) * V].astype(F64)
            assert np.abs(np.linalg.norm(nn, axis=1) - 1).max() < 1e-5
            assert np.abs(nn[4 * ns] + T[g]).max() < 1e-6


def relative_error(a, b, scale):
    return float((np.abs(a.astype(F64) - b.astype(F64)).max(1) / scale).max())


def test_positions_within_four_times_the_float32_error(spray):
    """Sphere vertices lie at distance s from their point, arrow tips at
    p + L T.  The yardstick is the float32 numpy restatement measured against
    the float64 one, on coordinates of the radius's order; the host form is
    held to four times that figure (the margin of the streamline rotation
    test)."""
    rng = np.random.default_rng(5)
    n = 400
    p = rng.uniform(-1, 1, (n, 3)).astype(F32)
    scales = rng.uniform(0.5, 2.0, n).astype(F32)
    # spheres: | |v - p| - s | / s
    S, G = gh.pset(p, scales=scales), gh.sphere(1.0, 2)
    V, _ = gh.per_glyph(G)
    s = np.repeat(scales.astype(F64), V)
    centre = np.repeat(p.astype(F64), V, 0)
    off = lambda v: np.abs(np.linalg.norm(v.astype(F64) - centre, axis=1) - s) / s
    v32 = gh.glyphs_numpy(S, G, spray)[0]
    v64 = gh.glyphs_numpy(S, G, spray, F64)[0]
    fig = max(float(off(v32).max()), relative_error(v32, v64, s))
    print("sphere: float32 restatement off by %.3g of s (float64: %.3g)" % (fig, off(v64).max()))
    assert 0 < fig < 1e-6
    host = spray.glyphs_host(S, G)[0]
    assert off(host).max() <= 4 * fig
    # arrows: the tip against p + L T of the float64 restatement
    vec = gh.swirl(p, 3)
    for sbv in (False, True):
        S, G = gh.pset(p, vectors=vec, scales=scales), gh.arrow(1.0, 7, sbv)
        V, _ = gh.per_glyph(G)
        kept = gh.keep_numpy(S, G)[0]
        assert kept.all()
        tip = lambda v: v.reshape(n, V, 3)[:, 3 * 7:4 * 7]
        t64 = tip(gh.glyphs_numpy(S, G, spray, F64, kept=kept)[0])
        L = scales.astype(F64) * (np.linalg.norm(vec.astype(F64), axis=1) if sbv else 1.0)
        Tdir = vec.astype(F64) / np.linalg.norm(vec.astype(F64), axis=1, keepdims=True)
        exact = p.astype(F64) + L[:, None] * Tdir
        assert np.abs(t64[:, 0] - exact).max() < 1e-6   # the float64 restatement is the statement
        err = lambda v: float((np.abs(tip(v).astype(F64) - t64).max((1, 2)) / L).max())
        fig = err(gh.glyphs_numpy(S, G, spray)[0])
        print("arrow tip (scale_by_vector %d): float32 restatement off by %.3g of L" % (sbv, fig))
        assert 0 < fig < 1e-6
        assert err(spray.glyphs_host(S, G)[0]) <= 4 * fig


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/cpp/glyph_host_check.cpp with glyphs.cpp's host restatement
    (SPRAY_RT_GLYPH_HOST_ONLY: nothing that needs the HIP runtime), built by
    g++ under the address and undefined-behaviour sanitizers and run as a plain
    executable, as test_job_arena.py does for its header."""
    from spray_amd import build
    root = build.ROOT
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    exe = str(tmp_path / "glyph_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                        "-DSPRAY_RT_GLYPH_HOST_ONLY", "-I" + os.path.join(rocm, "include"),
                        "-I" + os.path.join(root, "include"), "-I" + build.CSRC,
                        os.path.join(build.CSRC, "glyphs.cpp"),
                        os.path.join(root, "tests", "cpp", "glyph_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures")


# ---- errors ----

def raw_host(spray, set_kw, glyph_kw, color_kw=None, count=True):
    """spray_rt_glyphs_host through ctypes on raw records -> (rc, nverts, nfaces)."""
    from spray_amd._native import Glyph, PointSet, lib
    from spray_amd.engine import _GridColor
    S, G, K = PointSet(), Glyph(), _GridColor()
    keep = []
    for rec, kw in ((S, set_kw), (G, glyph_kw), (K, color_kw or {})):
        for k, x in kw.items():
            if isinstance(x, np.ndarray):
                keep.append(x)
                x = x.ctypes.data
            setattr(rec, k, x)
    nv, nf = C.c_size_t(7), C.c_size_t(7)
    rc = lib().spray_rt_glyphs_host(C.addressof(S), C.addressof(G), C.addressof(K) if color_kw else None,
                                    C.byref(nv), C.byref(nf), None, None, None, None, None)
    return rc, nv.value, nf.value


P5 = gh.cloud(5, 11)
V5 = gh.swirl(P5)
GOOD_SET = dict(points=P5, npoints=5, stride=1)
GOOD_SPHERE = dict(shape=0, size=0.5, level=1)
GOOD_ARROW = dict(shape=1, size=0.5, nsides=5, min_speed=1e-6)


def test_good_raw_records(spray):
    assert raw_host(spray, GOOD_SET, GOOD_SPHERE) == (0, 5 * 42, 5 * 80)
    assert raw_host(spray, dict(GOOD_SET, vectors=V5), GOOD_ARROW) == (0, 5 * 21, 5 * 30)
    # the select range is read with select only
    assert raw_host(spray, dict(GOOD_SET, select_lo=2.0, select_hi=1.0), GOOD_SPHERE)[0] == 0
    assert raw_host(spray, dict(GOOD_SET, select_lo=np.nan), GOOD_SPHERE)[0] == 0


def test_argument_errors(spray):
    nan, inf = float("nan"), float("inf")
    sel = np.linspace(0, 1, 5).astype(F32)
    table = np.arange(4, dtype=np.uint32)
    arrows = dict(GOOD_SET, vectors=V5)
    bad = [
        (dict(GOOD_SET, points=None), GOOD_SPHERE, None),
        (dict(GOOD_SET, stride=0), GOOD_SPHERE, None),
        (arrows, dict(GOOD_ARROW, shape=2), None),
        (arrows, dict(GOOD_ARROW, shape=-1), None),
        (GOOD_SET, dict(GOOD_SPHERE, level=-1), None),
        (GOOD_SET, dict(GOOD_SPHERE, level=4), None),
        (arrows, dict(GOOD_ARROW, nsides=2), None),
        (arrows, dict(GOOD_ARROW, nsides=17), None),
        (GOOD_SET, GOOD_ARROW, None),                       # arrows without vectors
    ]
    bad += [(GOOD_SET, dict(GOOD_SPHERE, size=x), None) for x in (0.0, -1.0, nan, inf)]
    bad += [(arrows, dict(GOOD_ARROW, min_speed=x), None) for x in (0.0, -1.0, 1e-20, 1e20, nan, inf)]
    bad += [(dict(GOOD_SET, select=sel, select_lo=lo, select_hi=hi), GOOD_SPHERE, None)
            for lo, hi in ((1.0, 0.5), (nan, 1.0), (0.0, nan), (-inf, 1.0), (0.0, inf))]
    good_map = dict(field=sel, table_rgb=table, ntable=4, lo=0.0, hi=1.0)
    bad += [(GOOD_SET, GOOD_SPHERE, dict(good_map, **kw)) for kw in
            (dict(table_rgb=None), dict(ntable=0), dict(ntable=4097), dict(lo=1.0), dict(lo=2.0),
             dict(hi=inf), dict(lo=nan), dict(lo=0.0, hi=1e-44))]
    for S, G, K in bad:
        assert raw_host(spray, S, G, K) == (ERR_ARG, 0, 0), (S, G, K)
    assert raw_host(spray, GOOD_SET, GOOD_SPHERE, good_map)[0] == 0
    from spray_amd._native import lib
    assert lib().spray_rt_glyphs_host(None, None, None, None, None, None, None, None, None, None) == ERR_ARG


def test_check_pass_errors(spray):
    """One bad element per call, in every array the call uses, at the first and
    at the last element."""
    sel = np.linspace(0, 1, 5).astype(F32)
    S = gh.with_color(gh.pset(P5, vectors=V5, scales=np.ones(5), select=sel, select_range=(0.0, 1.0)), 3)
    for G, arrays in ((gh.sphere(0.5), ("points", "scales", "select", "cfield")),
                      (gh.arrow(0.5), ("points", "vectors", "scales", "select", "cfield"))):
        assert len(spray.glyphs_host(S, G)[4]) == 5
        for key in arrays:
            values = (np.nan, np.inf, -np.inf) + ((-1.0, -1e-45) if key == "scales" else ())
            for x in values:
                for at in (0, S[key].size - 1):
                    T = dict(S)
                    T[key] = S[key].copy()
                    T[key].reshape(-1)[at] = x
                    with pytest.raises(spray.SprayRtError) as e:
                        spray.glyphs_host(T, G)
                    assert e.value.code == ERR_ARG and e.value.counts == (0, 0), (key, x, at)
    # a point the stride or the select range leaves out is checked all the same
    T = dict(S, stride=2)
    T["points"] = S["points"].copy()
    T["points"][1, 1] = np.nan
    with pytest.raises(spray.SprayRtError):
        spray.glyphs_host(T, gh.sphere(0.5))
    # a sphere set may carry vectors: they are not read
    T = dict(S)
    T["vectors"] = np.full((5, 3), np.nan, F32)
    ref = spray.glyphs_host(S, gh.sphere(0.5))
    assert [a.tobytes() for a in spray.glyphs_host(T, gh.sphere(0.5))] == [a.tobytes() for a in ref]
    # FLT_MAX-scale values and subnormals are finite: accepted
    T = dict(S)
    T["points"] = S["points"].copy()
    T["points"][0] = (3e38, -3e38, 1e-45)
    T["scales"] = np.array([1e-45, 3e38, 1, 1, 1], F32)
    T["vectors"] = S["vectors"].copy()
    T["vectors"][4] = (1e-45, 1.0, -1e-45)
    for G in (gh.sphere(0.5), gh.arrow(0.5)):
        got = spray.glyphs_host(T, G)
        ref = gh.glyphs_numpy(T, G, spray)
        assert [a.tobytes() for a in got] == [a.tobytes() for a in ref]


def test_limits_from_the_counts_alone(spray):
    """npoints >= 2^31 and 2^29 faces are rejected before a byte of the arrays
    is read: the arrays here hold one point."""
    one = np.zeros((1, 3), F32)
    lv3 = dict(shape=0, size=0.5, level=3)       # 1280 faces, 642 vertices a glyph
    n = 2 ** 29 // 1280 + 1                      # 419431 spheres: 2^29 faces and more
    assert (n - 1) * 1280 < 2 ** 29 <= n * 1280
    for npoints in (2 ** 31, 2 ** 31 + 5, 2 ** 40):
        assert raw_host(spray, dict(points=one, npoints=npoints, stride=1), lv3) == (ERR_LIMIT, 0, 0)
        assert raw_host(spray, dict(points=one, vectors=one, npoints=npoints, stride=7),
                        GOOD_ARROW) == (ERR_LIMIT, 0, 0)
    assert raw_host(spray, dict(points=one, npoints=n, stride=1), lv3) == (ERR_LIMIT, n * 642, n * 1280)
    assert raw_host(spray, dict(points=one, npoints=2 * n - 1, stride=2), lv3) == (ERR_LIMIT, n * 642, n * 1280)
    assert raw_host(spray, dict(points=one, npoints=2 ** 31 - 1, stride=1),
                    dict(shape=0, size=0.5, level=0))[0] == ERR_LIMIT
    # one glyph fewer passes (the arrays are real now), and a set whose count
    # needs its arrays reaches the limit after the count
    p = np.zeros((n, 3), F32)
    assert raw_host(spray, dict(points=p, npoints=n - 1, stride=1), lv3) == (0, (n - 1) * 642, (n - 1) * 1280)
    ones = np.ones(n, F32)
    assert raw_host(spray, dict(points=p, npoints=n, stride=1, select=ones, select_lo=0.5, select_hi=1.0),
                    lv3) == (ERR_LIMIT, n * 642, n * 1280)
    assert raw_host(spray, dict(points=p, npoints=n, stride=1, select=ones, select_lo=1.5, select_hi=2.0),
                    lv3) == (0, 0, 0)

"""The streamline filter's host forms (spray_rt_streamlines_host,
spray_rt_stream_tubes_host, spray_rt_tube_ring_host; no GPU) against the numpy
restatement of the rule (stream_helpers.py), byte for byte, and the properties
the rule promises: exact points on a dyadic field, the accuracy of RK4 on a
rigid rotation, closed and outward-oriented tubes, the errors.

Of the limits, 2^32 points of lines and 2^32 vertices are not reached here: the
first needs 4 * 10^9 RK4 steps on the host, the second cannot be reached before
2^29 faces.
"""
import collections
import ctypes as C

import numpy as np
import pytest

import stream_helpers as sh

F32 = np.float32
ERR_ARG, ERR_LIMIT = -1, -5
CASES = sh.small_cases()
DIRECTIONS = (sh.FORWARD, sh.BACKWARD, sh.BOTH)


@pytest.fixture(scope="module")
def spray():
    from spray_amd import build
    build.build()
    import spray_amd
    return spray_amd


def host_lines(spray, f):
    return spray.streamlines_host(*sh.host_args(f), **sh.host_kw(f))


def host_tubes(spray, f, radius, nsides, **kw):
    return spray.stream_tubes_host(*sh.host_args(f), radius, nsides, cfield=f.get("cfield"),
                                   cmap=f.get("cmap"), **sh.host_kw(f), **kw)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_cases_reach_their_paths():
    """From the numpy side: every path of the rule the cases are there for."""
    stats = collections.Counter()
    lines = {k: sh.lines_numpy(f, stats=stats) for k, f in CASES.items()}
    for key in ("upper_face", "seed_outside", "speed_low", "speed_overflow", "no_motion",
                "repick", "tangent_kept", "empty_back", "empty_fwd", "line_1", "line_2", "line_3"):
        assert stats[key] > 0, key
    per = {k: collections.Counter() for k in CASES}
    for k, f in CASES.items():
        sh.lines_numpy(f, stats=per[k])
    assert per["turn"]["repick"] and per["underflow"]["no_motion"] and per["huge"]["speed_overflow"]
    assert per["slow"]["speed_low"] and per["zero"]["speed_low"] and per["sink"]["tangent_kept"]
    assert per["ends"]["empty_back"] and per["ends"]["empty_fwd"]
    assert CASES["cell2"]["vectors"].shape == (2, 2, 2, 3)
    assert {CASES[k]["vectors"].shape[:3] for k in ("abc322", "abc232", "abc223")} == \
        {(2, 2, 3), (2, 3, 2), (3, 2, 2)}
    for k in ("abc322", "abc232", "abc223"):   # -0.0, a lattice point, just outside on each side
        s = CASES[k]["seeds"]
        assert np.signbit(s[5, 0]) and s[5, 0] == 0 and per[k]["seed_outside"] == 3
        assert per[k]["upper_face"] > 3
    assert len(lines["steps0"]["points"]) == 3 and (lines["steps0"]["info"][:, 0] == 0).all()
    ends = lines["sink"]["info"][:, 1]
    assert sh.SPEED in (ends & 255) or sh.SPEED in (ends >> 8)


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_forms_equal_numpy(spray, name, direction):
    f = sh.with_color(dict(CASES[name], direction=direction), 5)
    L = sh.lines_numpy(f)
    for _ in range(2):
        p, off, info = host_lines(spray, f)
        assert same(p, L["points"]) and same(off, L["off"]) and same(info, L["info"])
    ring = spray.tube_ring(5)
    plain = dict(f, cfield=None, cmap=None)
    refs = (sh.tubes_numpy(f, L, 0.0625, 5, ring),
            sh.tubes_numpy(plain, L, 0.0625, 5, ring, color=0x00A1B2C3),
            sh.tubes_numpy(plain, L, 0.0625, 5, ring))
    for _ in range(2):
        got = (host_tubes(spray, f, 0.0625, 5),
               host_tubes(spray, plain, 0.0625, 5, color=0x00A1B2C3, normals=False),
               host_tubes(spray, plain, 0.0625, 5))
        for k, ((v, n, c, fc), (rv, rn, rc, rf)) in enumerate(zip(got, refs)):
            assert same(v, rv) and same(c, rc) and same(fc, rf), k
            assert n is None if k == 1 else same(n, rn), k
    assert host_tubes(spray, f, 0.0625, 5, count_only=True) == (len(refs[0][0]), len(refs[0][3]))
    if name == "spaced":
        assert len(np.unique(refs[0][2])) > 3 and len(refs[0][0]) > 100


@pytest.mark.parametrize("nsides", [3, 16])
def test_other_side_counts_equal_numpy(spray, nsides):
    f = sh.with_color(CASES["spaced"], 9)
    L = sh.lines_numpy(f)
    ref = sh.tubes_numpy(f, L, 0.03125, nsides, spray.tube_ring(nsides))
    got = host_tubes(spray, f, 0.03125, nsides)
    assert all(same(a, b) for a, b in zip(got, ref))


def test_uniform_dyadic_field_is_exact(spray):
    p, off, info = host_lines(spray, CASES["dyadic"])
    want = np.zeros((8, 3), F32)
    want[:, 0] = 0.25 + 0.5 * np.arange(8)
    want[:, 1:] = 0.5
    assert same(p, want)
    assert off.tolist() == [0, 8] and info.tolist() == [[0, sh.STEPS | sh.GRID << 8]]


def test_rigid_rotation_keeps_its_radius(spray):
    """Orbits about the centre of a 9^3 grid: the host form's radius against the
    same rule in float64 numpy.  The bound is four times the difference between
    the float32 and the float64 numpy restatements, which involves none of the
    code under test: measured 2.05e-06 (radii 1 to 3, 50 steps of 0.125, the
    RK4 truncation error is common to both)."""
    seeds = [[4 + r, 4, 4 + 0.5 * r] for r in (1.0, 2.0, 3.0)] + [[4, 4 - 2.5, 1]]
    f = sh.field(sh.rotation(9), seeds, 0.125, 50, sh.BOTH)
    radius = lambda p: np.hypot(p[:, 0].astype(np.float64) - 4, p[:, 1].astype(np.float64) - 4)
    L32, L64 = sh.lines_numpy(f), sh.lines_numpy(f, F=np.float64)
    assert same(L32["off"], L64["off"]) and len(L32["points"]) == 4 * 101
    measured = np.abs(radius(L32["points"]) - radius(L64["points"])).max()
    print("float32 against float64 restatement: %.3g" % measured)
    assert 0 < measured < 1e-5
    p, off, info = host_lines(spray, f)
    assert same(off, L64["off"])
    assert np.abs(radius(p) - radius(L64["points"])).max() <= 4 * measured
    # and the orbit is a circle to RK4's accuracy: h^5 / 120 per step
    r0 = np.repeat(radius(np.asarray(seeds, F32)), 101)
    assert np.abs(radius(p) - r0).max() < 50 * 3.0 * 0.125 ** 5 / 120 + 1e-5


def edges_of(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)


@pytest.mark.parametrize("name", ["spaced", "sink", "turn", "cell2"])
def test_tubes_are_closed_oriented_manifolds(spray, name):
    f = dict(CASES[name])
    p, off, info = host_lines(spray, f)
    m = np.diff(off.astype(np.int64))
    nlines = int((m >= 2).sum())
    ns, r = 6, 0.25   # a radius of the coordinates' order: their rounding stays below 1e-5 r
    v, n, c, fc = host_tubes(spray, f, r, ns)
    assert nlines > 0 and len(v) == (m[m >= 2] * ns + 2).sum() and len(fc) == (2 * ns * m[m >= 2]).sum()
    e = edges_of(fc)
    key = e[:, 0] * len(v) + e[:, 1]
    rev = e[:, 1] * len(v) + e[:, 0]
    assert len(np.unique(key)) == len(key)              # every directed edge once ...
    assert np.array_equal(np.sort(key), np.sort(rev))   # ... and its reverse once
    assert len(v) - len(key) // 2 + len(fc) == 2 * nlines
    assert fc.max() == len(v) - 1 and len(np.unique(fc)) == len(v)
    # ring vertices lie at the radius from their point, normals are unit offsets
    v0 = 0
    for l in np.flatnonzero(m >= 2):
        pts = p[off[l]:off[l + 1]].astype(np.float64)
        ring = v[v0:v0 + m[l] * ns].astype(np.float64).reshape(m[l], ns, 3)
        d = np.linalg.norm(ring - pts[:, None, :], axis=2)
        assert np.abs(d - r).max() <= 1e-5 * r
        nr = n[v0:v0 + m[l] * ns].astype(np.float64)
        assert np.abs(np.linalg.norm(nr, axis=1) - 1).max() < 1e-5
        assert same(v[v0 + m[l] * ns], p[off[l]]) and same(v[v0 + m[l] * ns + 1], p[off[l + 1] - 1])
        v0 += m[l] * ns + 2


def test_faces_point_away_from_the_axis(spray):
    f = sh.field(sh.rotation(9, 1.0, 0.25), [[6, 4, 1], [4, 2.5, 2], [5, 5, 0.5]], 0.0625, 40,
                 sh.BOTH)
    p, off, info = host_lines(spray, f)
    ns, r = 5, 0.03125
    v, n, c, fc = host_tubes(spray, f, r, ns)
    v64 = v.astype(np.float64)
    a, b, cc = (v64[fc[:, k]] for k in range(3))
    ng = np.cross(a - b, cc - a)
    cen = (a + b + cc) / 3
    m = np.diff(off.astype(np.int64))
    f0 = v0 = 0
    for l in range(len(m)):
        assert m[l] >= 40
        pts = p[off[l]:off[l + 1]].astype(np.float64)
        nside = 2 * ns * (m[l] - 1)
        seg = np.arange(nside) // (2 * ns)
        mid = (pts[seg] + pts[seg + 1]) / 2
        out = cen[f0:f0 + nside] - mid
        assert (np.einsum("ij,ij->i", ng[f0:f0 + nside], out) > 0).all()
        t0, t1 = pts[1] - pts[0], pts[-1] - pts[-2]
        assert (ng[f0 + nside:f0 + nside + ns] @ -t0 > 0).all()
        assert (ng[f0 + nside + ns:f0 + nside + 2 * ns] @ t1 > 0).all()
        # the stored normals of the caps and of the rings agree with the faces' side
        assert n[v0 + m[l] * ns] @ -t0 > 0 and n[v0 + m[l] * ns + 1] @ t1 > 0
        f0 += nside + 2 * ns
        v0 += m[l] * ns + 2
    assert f0 == len(fc) and v0 == len(v)


@pytest.mark.parametrize("nsides", [3, 5, 6, 16])
def test_volume_of_a_straight_tube(spray, nsides):
    f = dict(CASES["dyadic"])
    r, length = 0.25, 3.5
    v, n, c, fc = host_tubes(spray, f, r, nsides)
    v64 = v.astype(np.float64)
    a, b, cc = (v64[fc[:, k]] for k in range(3))
    # Ng = (v0 - v1) x (v2 - v0) points outward: the usual orientation's inverse
    vol = -np.einsum("ij,ij->i", a, np.cross(b, cc)).sum() / 6
    want = nsides / 2 * np.sin(2 * np.pi / nsides) * r * r * length
    assert abs(vol - want) <= 1e-5 * want


def test_ring_table(spray):
    for ns in range(3, 17):
        got = spray.tube_ring(ns)
        a = 2 * np.pi * np.arange(ns) / ns
        want = np.stack([np.cos(a), np.sin(a)], 1).astype(F32)
        assert got.shape == (ns, 2) and got.dtype == F32
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), ns
    for ns in (2, 17, 0, -1):
        with pytest.raises(spray.SprayRtError) as e:
            spray.tube_ring(ns)
        assert e.value.code == ERR_ARG


def fails(spray, code, f, radius=0.1, nsides=6, tubes_only=False, **kw):
    if not tubes_only:
        with pytest.raises(spray.SprayRtError) as e:
            host_lines(spray, f)
        assert e.value.code == code
    with pytest.raises(spray.SprayRtError) as e:
        host_tubes(spray, f, radius, nsides, **kw)
    assert e.value.code == code


def test_argument_errors(spray):
    good = sh.with_color(CASES["spaced"], 3)
    host_lines(spray, good)
    host_tubes(spray, good, 0.1, 6)
    inf, nan = np.inf, np.nan
    for key, bad in (("spacing", (1, 0, 1)), ("spacing", (1, -1, 1)), ("spacing", (inf, 1, 1)),
                     ("spacing", (1, 1, nan)), ("origin", (0, nan, 0)), ("origin", (inf, 0, 0)),
                     ("step", 0.0), ("step", -0.5), ("step", inf), ("step", nan),
                     ("max_steps", -1), ("max_steps", 65536), ("direction", 3), ("direction", -1),
                     ("min_speed", 0.0), ("min_speed", -1.0), ("min_speed", 1e-20),
                     ("min_speed", 1e20), ("min_speed", nan)):
        fails(spray, ERR_ARG, dict(good, **{key: bad}))
    host_lines(spray, dict(good, max_steps=65535, step=1e-9, min_speed=1.1e-19))
    for dims in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        fails(spray, ERR_ARG, dict(good, vectors=np.zeros(dims + (3,), F32), cfield=None))
    for where in ((0, 0, 0, 0), (4, 4, 4, 2), (2, 3, 1, 1)):
        for val in (nan, inf, -inf):
            v = good["vectors"].copy()
            v[where] = val
            fails(spray, ERR_ARG, dict(good, vectors=v))
    s = good["seeds"].copy()
    s[3, 1] = nan
    fails(spray, ERR_ARG, dict(good, seeds=s))
    s[3, 1] = -inf
    fails(spray, ERR_ARG, dict(good, seeds=s))
    # the tube and the colour map
    for radius in (0.0, -1.0, inf, nan):
        fails(spray, ERR_ARG, good, radius=radius, tubes_only=True)
    for nsides in (2, 17, 0, -3):
        fails(spray, ERR_ARG, good, nsides=nsides, tubes_only=True)
    g = good["cfield"].copy()
    g[1, 2, 3] = nan
    fails(spray, ERR_ARG, dict(good, cfield=g), tubes_only=True)
    tab = good["cmap"][0]
    for cmap in (None, (np.zeros(0, np.uint32), 0.0, 1.0), (np.zeros(4097, np.uint32), 0.0, 1.0),
                 (tab, 1.0, 1.0), (tab, nan, 1.0), (tab, -3e38, 3e38), (tab, 0.0, 1e-45)):
        fails(spray, ERR_ARG, dict(good, cmap=cmap), tubes_only=True)
    # a colour field does not matter to the polylines
    host_lines(spray, dict(good, cfield=g))
    # null pointers
    from spray_amd import engine
    from spray_amd._native import lib
    arr, tarr, carr, keep = engine._stream_tables([good], dict(radius=0.1, nsides=6))
    n = C.c_size_t()
    L = lib()
    assert L.spray_rt_streamlines_host(None, C.byref(n), None, None, None) == ERR_ARG
    assert L.spray_rt_stream_tubes_host(C.addressof(arr), None, None, None, None, None, None,
                                        None, None) == ERR_ARG
    seeds = arr[0].seeds
    arr[0].seeds = None
    assert L.spray_rt_streamlines_host(C.addressof(arr), C.byref(n), None, None, None) == ERR_ARG
    arr[0].seeds, vec = seeds, arr[0].vectors
    arr[0].vectors = None
    assert L.spray_rt_streamlines_host(C.addressof(arr), C.byref(n), None, None, None) == ERR_ARG
    arr[0].vectors = vec
    assert L.spray_rt_streamlines_host(C.addressof(arr), C.byref(n), None, None, None) == 0
    arr[0].nseeds, arr[0].seeds = 0, None       # no seeds: no pointer needed
    assert L.spray_rt_streamlines_host(C.addressof(arr), C.byref(n), None, None, None) == 0
    assert n.value == 0


def test_limits(spray):
    from spray_amd import engine
    from spray_amd._native import lib
    L = lib()
    good = CASES["spaced"]
    arr, tarr, carr, keep = engine._stream_tables([good], dict(radius=0.1, nsides=6))
    n = C.c_size_t()
    call = lambda: L.spray_rt_streamlines_host(C.addressof(arr), C.byref(n), None, None, None)
    assert call() == 0
    arr[0].dims = (C.c_int32 * 3)(2048, 1024, 1024)     # rejected before a sample is read
    assert call() == ERR_LIMIT
    arr[0].dims = (C.c_int32 * 3)(5, 5, 5)
    arr[0].nseeds = 1 << 31                             # ... and before a seed is
    assert call() == ERR_LIMIT
    # 2^29 faces: 129 orbits of 131,071 points at 16 sides, counted without the arrays
    seeds = np.zeros((129, 3), F32)
    seeds[:, 0] = 4 + 1 + 2 * np.arange(129) / 129
    seeds[:, 1:] = 4
    f = sh.field(sh.rotation(9), seeds, 0.01, 65535, sh.BOTH)
    with pytest.raises(spray.SprayRtError) as e:
        host_tubes(spray, f, 0.1, 16, count_only=True)
    assert e.value.code == ERR_LIMIT
    assert e.value.counts == (129 * 131071 * 16 + 2 * 129, 2 * 16 * 129 * 131071)
    assert e.value.counts[1] >= 1 << 29 > 2 * 16 * 128 * 131071   # one line fewer would fit

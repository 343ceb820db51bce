"""The hard classes of stream_cases.py on the host (no GPU): the host forms
(spray_rt_streamlines_host, spray_rt_stream_tubes_host) against the numpy
restatement byte for byte on every arithmetic class, on the gap fields and on
the 509 distinct seeds of the chunk fields; from the numpy side and from the
inputs, that each class reaches what it is there for; the closed forms of the
two long fields.  test_gpu_stream_cases.py holds the kernels to the host forms
on the same inputs.
"""
import collections

import numpy as np
import pytest

import color_helpers as ch
import stream_cases as sc
import stream_helpers as sh
from test_streamlines_host import edges_of, host_lines, host_tubes, same

F32 = np.float32
ARITH = sc.arithmetic()
GAPS = sc.gaps()
DISTINCT = sc.chunks(distinct=True)
SMALL = dict(ARITH, **GAPS, **DISTINCT)
EXITS = ("grid_q2", "grid_q3", "grid_q4", "grid_pn")


@pytest.fixture(scope="module")
def spray():
    from spray_amd import build
    build.build()
    import spray_amd
    return spray_amd


def stats_of(f):
    st = collections.Counter()
    return sh.lines_numpy(f, stats=st), st


def runs_of(m):
    """[(value, length)] of the runs of m."""
    cut = np.flatnonzero(np.diff(m)) + 1
    start = np.concatenate([[0], cut])
    return list(zip(m[start].tolist(), np.diff(np.concatenate([start, [len(m)]])).tolist()))


def test_arithmetic_classes_reach_their_paths():
    per = {k: stats_of(f) for k, f in ARITH.items()}
    # all four stages at which a step leaves the grid, at a lower and an upper
    # face of every axis, forward and backward
    assert len(sc.exits()) == 13
    st = per["exit_bent"][1]
    assert st["grid_q2"] and st["grid_q3"] and st["grid_q4"]
    for k in sorted(sc.exits())[1:]:
        assert all(per[k][1][e] > 0 for e in EXITS), (k, per[k][1])
        assert (per[k][1]["upper_face"] > 0) == ("+" in k)   # only the upper face is inside
        seeds = ARITH[k]["seeds"]
        axis = "xyz".index(k[5])
        assert ((seeds[:, axis] >= 1.0).all() if "+" in k else (seeds[:, axis] <= 2.0).all())
    # both sides of the frame threshold, and the flip between adjacent floats
    for k in sc.threshold():
        L, st = per[k]
        assert len(L["points"]) == 3 and st["repick"] + st["carried"] == 2
        if k.startswith("turn_pair"):
            continue
        angle = float(k[5:])
        assert (st["repick"] == 1) == (angle > 60.0), k
    lo, hi, s = sc.threshold_pair()
    assert np.nextafter(lo, F32(1)) == hi
    assert per["turn_pair_repick"][1]["repick"] == 1 and per["turn_pair_carried"][1]["repick"] == 0
    # ... where the carried side sits on the threshold itself: |w|^2 == 0.25f
    L = per["turn_pair_carried"][0]
    N0, T1 = L["normals"][0], L["tangents"][1]
    w = N0 - sh.dot(N0, T1) * T1
    assert sh.dot(w, w) == F32(0.25)
    # exact ties of the axis rule, each axis picked, the lowest of a tie
    ties = sc.zeros_and_ties()
    picked = collections.Counter()
    for k in ties:
        st = per[k][1]
        assert st["axis_tie"] == st["axis_0"] + st["axis_1"] + st["axis_2"] > 0, k
        picked.update({a: st[a] for a in ("axis_0", "axis_1", "axis_2")})
    assert picked["axis_0"] and picked["axis_1"]
    for k in ("tie_yz_same", "tie_yz_opp", "zero_00", "zero_01", "zero_10", "zero_11", "axis_0+"):
        assert per[k][1]["axis_1"] and not per[k][1]["axis_2"], k   # y and z tie: y
    assert {tuple(np.signbit(ARITH["zero_%d%d" % (a, b)]["vectors"][0, 0, 0, 1:]))
            for a in (0, 1) for b in (0, 1)} == {(False, False), (False, True), (True, False),
                                                 (True, True)}
    # a subnormal tangent component decides the axis, without a tie
    for k, axis in (("sub_z0", 2), ("sub_zy", 2), ("sub_x", 0), ("sub_y", 1)):
        L, st = per[k]
        T = np.abs(L["tangents"][0])
        assert st["axis_%d" % axis] and not st["axis_tie"], k
        sub = (T > 0) & (T < sc.FLT_MIN)
        assert sub.any() and np.argmin(T) == axis, k
        # flushed to zero, the components would tie or the normal lose its small part
        flushed = np.where(sub, 0, T)
        assert (flushed == flushed[axis]).sum() > 1 or sub[axis], k
    assert per["sub_zy"][0]["tangents"][0, 1] > per["sub_zy"][0]["tangents"][0, 2] > 0
    # the speed limit from both sides at the smallest min_speed, squares that underflow
    ms = sc.MIN_SPEED
    assert ms * ms >= sc.FLT_MIN > np.nextafter(ms, F32(0)) * np.nextafter(ms, F32(0))
    assert per["slowest_at"][1]["speed_low"] == 0 and len(per["slowest_at"][0]["points"]) > 8
    assert per["slowest_up"][1]["speed_low"] == 0 and len(per["slowest_up"][0]["points"]) > 8
    assert per["slowest_dn"][1]["speed_low"] == 4 and len(per["slowest_dn"][0]["points"]) == 2
    v = ARITH["tiny"]["vectors"][0, 0, 0]
    assert 0 < v[1] * v[1] < sc.FLT_MIN and v[2] * v[2] == 0 and 0 < abs(v[2]) < sc.FLT_MIN
    assert len(per["tiny"][0]["points"]) > 8
    g = ARITH["sub_colour"]["cfield"]
    assert (np.abs(g) < sc.FLT_MIN).all() and (g != 0).all()
    sampled = per["sub_colour"][0]["scalars"]
    assert (np.abs(sampled) < sc.FLT_MIN).all()
    assert len(np.unique(ch.colormap_numpy(sampled, *ARITH["sub_colour"]["cmap"]))) == 4
    # the stall: SPEED by no motion after steps, the tangent a unit vector still
    L, st = per["stall"]
    assert st["no_motion"] >= 4 and st["tangent_kept"] == 0
    ends = L["info"][:5, 1]
    assert ((ends & 255) == sh.SPEED).sum() + ((ends >> 8) == sh.SPEED).sum() >= 4
    assert (np.diff(L["off"].astype(np.int64))[:5] > 20).all()
    # the fast fields take steps below the overflow and none above it
    assert per["fast_over"][1]["speed_overflow"] == 4
    for k in ("fast_x", "fast_xyz", "fast_rotation"):
        assert per[k][1]["speed_overflow"] == 0 and len(per[k][0]["points"]) >= 20, k
    # off the lattice: seeds on, below and above every face, a coarse float grid
    for k in sc.offlattice():
        L, st = per[k]
        assert st["seed_outside"] >= 6 and st["upper_face"] >= 3, (k, st)
        assert len(ARITH[k]["seeds"]) == 12 + 18
    f = ARITH["off_0"]
    assert np.spacing(F32(f["origin"][0])) == 0.0625 and float(F32(f["spacing"][0])) != 0.1
    assert max(len(per[k][0]["points"]) for k in ARITH) < 300   # small grids, short lines


def test_scale_classes_sit_on_the_boundaries():
    cf = sc.chunks()
    assert [sc.nblocks(cf[k]) for k in sorted(cf)] == [256, 257, 513]
    assert [sc.nlanes(cf[k]) for k in sorted(cf)] == [65536, 65538, 131073]
    # one, two and three chunks of the scan's loop over 256 blocks
    assert [(sc.nblocks(cf[k]) + sc.CHUNK - 1) // sc.CHUNK for k in sorted(cf)] == [1, 2, 3]
    L, st = stats_of(DISTINCT["chunks256"])
    m = np.diff(L["off"].astype(np.int64))
    assert st["seed_outside"] == 3 and (m == 0).sum() == 3 and (m == 1).sum() >= 1
    assert sc.PERIOD % 2 == 1 and all(sc.PERIOD % p for p in range(3, 23, 2))
    # fullblock: block 0 is 256 forward lanes of 65,536 points
    f = sc.fullblock()["fullblock"]
    assert sc.nlanes(f) == 257 and f["direction"] == sh.FORWARD and f["max_steps"] == 65535
    assert sc.LANES * (f["max_steps"] + 1) == 1 << 24
    assert len({tuple(s) for s in f["seeds"].tolist()}) == 257
    # gaps: the runs as laid out, each empty run of 300 across a block boundary
    for k, f in GAPS.items():
        L, st = stats_of(f)
        m = np.diff(L["off"].astype(np.int64))
        assert np.array_equal(m, f["want"]), k
        assert 1400 <= len(m) <= 1600
        runs, at = runs_of(m), 0
        empty = []
        for val, n in runs:
            if val == 0 and n >= 299:
                empty.append((at, n))
                assert at // sc.LANES != (at + n - 1) // sc.LANES
            at += n
        assert len(empty) >= 2 and any(n > sc.LANES for _, n in empty), k
        tubes = np.flatnonzero(m >= 2)
        if "_base_" in k:
            assert empty[0][0] == 0 and empty[-1][0] + empty[-1][1] == len(m) and len(empty) == 3
            assert (1, 300) in runs and {2, 3, 40} <= set(m.tolist())
        if "_first_" in k:
            assert tubes[0] == 0 and len(tubes) > 1
        if "_last_" in k:
            assert tubes[-1] == len(m) - 1 and len(tubes) > 1
        if "_only0_" in k:
            assert tubes.tolist() == [0]
        if "_onlyN_" in k:
            assert tubes.tolist() == [len(m) - 1]
    assert sorted(f["tube"]["nsides"] for f in GAPS.values()) == list(range(3, 17))
    assert {k.split("_")[1] for k in GAPS} == {"base", "first", "last", "only0", "onlyN"}


def test_probe_positions_lie_in_every_trip():
    """The check pass covers 64 blocks x 256 threads = 16,384 elements per trip
    of its grid-stride loops (kCheckBlocks, kCheckBlock of stream_kernels.hip)."""
    assert sc.TRIP == 64 * 256 == 16384
    f = sc.probe()
    sizes = {"vectors": 51975, "cfield": 17325, "seeds": 18000}
    for key, trips in (("vectors", 4), ("cfield", 2), ("seeds", 2)):
        n = f[key].size
        pos = sc.probe_positions(n)
        assert n == sizes[key] and (n + sc.TRIP - 1) // sc.TRIP == trips
        assert pos[0] == 0 and pos[1] == 16383 and pos[2] == 16384 and pos[4] == n - 1
        assert pos == sorted(set(pos))
        assert {p // sc.TRIP for p in pos} == set(range(trips))   # the first, a second, every later one
        assert pos[3] // sc.TRIP == max(trips - 2, 1) and pos[3] % sc.TRIP not in (0, sc.TRIP - 1)
    g = sc.probe_control(f)
    for key, _ in sc.PROBE_KINDS:
        a = g[key].reshape(-1)[sc.probe_positions(g[key].size)]
        assert np.isfinite(g[key]).all() and (np.abs(a) > 1e38).sum() == 3
        assert ((a != 0) & (np.abs(a) < sc.FLT_MIN)).sum() == 2


@pytest.mark.parametrize("name", sorted(SMALL))
def test_host_forms_equal_numpy(spray, name):
    f = SMALL[name]
    t = sc.tube_of(f, sorted(SMALL).index(name))
    ns, r = t["nsides"], t["radius"]
    if f.get("cfield") is None:
        f = sh.with_color(f, 5)
    L = sh.lines_numpy(f)
    p, off, info = host_lines(spray, f)
    assert same(p, L["points"]) and same(off, L["off"]) and same(info, L["info"])
    ring = spray.tube_ring(ns)
    plain = dict(f, cfield=None, cmap=None)
    refs = (sh.tubes_numpy(f, L, r, ns, ring),
            sh.tubes_numpy(plain, L, r, ns, ring, color=0x00A1B2C3),
            sh.tubes_numpy(plain, L, r, ns, ring))
    got = (host_tubes(spray, f, r, ns),
           host_tubes(spray, plain, r, ns, color=0x00A1B2C3, normals=False),
           host_tubes(spray, plain, r, ns))
    for k, ((v, n, c, fc), (rv, rn, rc, rf)) in enumerate(zip(got, refs)):
        assert same(v, rv) and same(c, rc) and same(fc, rf), k
        assert n is None if k == 1 else same(n, rn), k
    assert host_tubes(spray, f, r, ns, count_only=True) == (len(refs[0][0]), len(refs[0][3]))


@pytest.mark.parametrize("name", [c[0] for c in sc.CHUNK_FIELDS])
def test_tiled_chunks_equal_the_tiled_restatement(spray, name):
    """The host form of a whole chunk field is the restatement of its 509
    distinct seeds, tiled: every copy of a seed yields the same line bytes."""
    f = sc.chunks()[name]
    L = sh.lines_numpy(DISTINCT[name])
    idx = np.arange(len(f["seeds"])) % sc.PERIOD
    assert same(f["seeds"], DISTINCT[name]["seeds"][idx])
    p, off, info = host_lines(spray, f)
    m = np.diff(L["off"].astype(np.int64))[idx]
    want_off = np.concatenate([[0], np.cumsum(m)])
    assert same(off, want_off.astype(np.uint32)) and same(info, L["info"][idx])
    src = np.repeat(L["off"].astype(np.int64)[idx] - want_off[:-1], m) + np.arange(want_off[-1])
    assert same(p, L["points"][src])
    assert 150000 < len(p) < 400000


def test_fullblock_is_its_closed_form(spray):
    f = sc.fullblock()["fullblock"]
    pick = [0, 131, 256]
    sub = dict(f, seeds=f["seeds"][pick])
    p, off, info = host_lines(spray, sub)
    want = np.zeros((3, 65536, 3), F32)
    want[:, :, 0] = np.arange(65536)
    want[:, :, 1:] = f["seeds"][pick, None, 1:]
    assert same(p, want.reshape(-1, 3))
    assert off.tolist() == [0, 65536, 131072, 196608]
    assert info.tolist() == [[0, sh.STEPS | sh.STEPS << 8]] * 3
    L = sh.lines_numpy(dict(sub, seeds=sub["seeds"][:1], max_steps=40))
    assert same(L["points"], want[0, :41])   # the restatement agrees on the first steps
    # all 257 lines, counted without the arrays: block 0 holds 2^24 points
    ns = f["tube"]["nsides"]
    nv, nf = host_tubes(spray, f, f["tube"]["radius"], ns, count_only=True)
    assert (nv, nf) == (257 * 65536 * ns + 2 * 257, 2 * ns * 257 * 65536)
    assert (nv - 2 * 257) // ns - 65536 == 1 << 24


def test_longest_is_its_closed_form_and_a_closed_tube(spray):
    f = sc.longest()["longest"]
    p, off, info = host_lines(spray, f)
    assert off.tolist() == [0, 131071, 131073]
    assert info.tolist() == [[65535, sh.GRID | sh.STEPS << 8], [1, sh.GRID | sh.GRID << 8]]
    want = np.zeros((131073, 3), F32)
    want[:131071, 0] = np.arange(131071)
    want[131071:] = [[1000, 0.25, 1], [1000, 1, 1]]
    assert same(p, want)
    L = sh.lines_numpy(dict(f, max_steps=30))
    assert same(L["points"][:61], want[65535 - 30:65535 + 31]) and same(L["points"][61:], want[131071:])
    t = f["tube"]
    v, n, c, fc = host_tubes(spray, f, t["radius"], t["nsides"])
    assert len(v) == 131071 * 16 + 2 + 2 * 16 + 2 and len(fc) == 2 * 16 * 131073
    assert len(v) - (2 * 16 + 2) == 2097138 and len(fc) - 2 * 16 * 2 == 4194272
    e = edges_of(fc)
    key = np.sort(e[:, 0] * len(v) + e[:, 1])
    rev = np.sort(e[:, 1] * len(v) + e[:, 0])
    assert (np.diff(key) > 0).all()                     # every directed edge once ...
    assert np.array_equal(key, rev)                     # ... and its reverse once
    assert len(v) - len(key) // 2 + len(fc) == 2 * 2    # chi = 2 per line
    seen = np.zeros(len(v), bool)
    seen[fc.reshape(-1)] = True
    assert seen.all()

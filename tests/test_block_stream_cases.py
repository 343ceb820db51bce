"""The hard classes of block_stream_cases.py on the host (no GPU): from the
counters of its numpy restatement and from the inputs, that each class reaches
the path it is there for; the host forms (spray_rt_block_streamlines_host,
spray_rt_block_stream_tubes_host) against the restatement byte for byte on every
class small enough for numpy, point blocks included; the closed forms of the
long sets; the host forms' refusal of every bad element of the check-pass sets.
The box of the miss path by brute force is in tests/cpp/block_stream_host_check.cpp,
built and run by test_block_streamlines_host.py.  test_gpu_block_stream_cases.py
holds the kernels to the host forms on the same inputs.
"""
import collections
import functools

import numpy as np
import pytest

import block_stream_cases as bc
import block_stream_helpers as bs
import stream_cases as sc
from test_block_streamlines_host import ERR_ARG, host_lines, host_tubes, same

F32 = np.float32
SMALL = bc.small()
NAMES = sorted(SMALL)
OUT = bs.SEED | bs.SEED << 8


@pytest.fixture(scope="module")
def spray():
    from spray_amd import build
    build.build()
    import spray_amd
    return spray_amd


@functools.lru_cache(maxsize=None)
def restated(name):
    near = "seed" if name.startswith("hb_") else "all" if name.startswith("land_") else None
    return bc.restate(SMALL[name], near)


def total(names):
    st = collections.Counter()
    for k in names:
        st.update({a: b for a, b in restated(k)[1].items() if a != "scan_max"})
    return st


def test_hard_boxes_sit_on_their_faces():
    hb = bc.hard_boxes()
    assert len(hb) == bc.HB_COUNT == 40
    info = [s["hb"] for s in hb.values()]
    assert {(h["spacing"], h["origin"] if h["origin"] else str(h["origin"])) for h in info} == \
        {(n, o if o else str(o)) for n, _ in bc.HB_SPACINGS for o in bc.HB_ORIGINS}
    assert {h["joint"] for h in info} == set(bc.HB_JOINTS) and {h["axis"] for h in info} == {0, 1, 2}
    assert {h["n"] for h in info} == {2, 3, 4, 5}
    assert {len(s["blocks"]) for s in hb.values()} == {2, 3}
    assert {s["max_steps"] for s in hb.values()} == {0, 1, 2, 3}
    inexact = 0
    for name, s in hb.items():
        h = s["hb"]
        # the neighbour starts at the face computed in float, a float below or a float above it
        k = {"coincide": 0, "overlap": -1, "gap": 1}[h["joint"]]
        for face, start in zip(h["faces"], h["starts"][1:]):
            assert bc.fkey(start) - bc.fkey(face) == k, name
            assert np.isfinite(face)
        sp = F32(s["blocks"][0]["spacing"][h["axis"]])
        inexact += float(np.float64(h["faces"][0] - h["starts"][0]) / np.float64(sp)) != h["n"] - 1
        # seven seeds about every face of every axis; some inside, some outside
        nfaces = 4 + len(s["blocks"]) + 1
        assert len(s["seeds"]) == 7 * nfaces, name
        L, st = restated(name)
        assert 0 < st["seed_outside"] < len(s["seeds"]), name
        # seeds that are inside while the float next to them, or the one after, is not
        assert st["near_seed"] > 0, name
    assert inexact >= 20           # the far face is not (n - 1) spacings from the origin as a real number
    st = total(hb)
    assert st["near_seed"] > 7 * len(hb)      # more than a face's seeds a set
    assert st["miss"] > 500 and st["switch"] > 100 and st["full_scan"] > 100 and st["hit_last"] > 50
    assert st["sticky_over_lower"] > 0 and st["in_several"] > 50 and st["on_shared_face"] > 50
    assert st["switch_q2"] and st["switch_q4"] and st["grid_q2"] and st["grid_q4"]
    assert st["end_%d" % bs.GRID] > 100 and st["end_%d" % bs.STEPS] > 100
    # subnormal and huge bounds are in there: p - origin below FLT_MIN, and above 1e38
    sub = [s for s in hb.values() if s["hb"]["spacing"] == "sub" and s["hb"]["origin"] == 0.0][0]
    assert 0 < float(sub["hb"]["faces"][0]) < float(sc.FLT_MIN) * 4
    assert 0 < sub["step"] < float(sc.FLT_MIN)
    huge = [s for s in hb.values() if s["hb"]["spacing"] == "huge"]
    assert all(float(s["hb"]["faces"][-1]) > 5e37 for s in huge)
    assert float(F32(1e6) + F32(0.1)) != 1e6 + 0.1 and np.spacing(F32(1e6)) == 0.0625


def test_landings_decide_within_two_floats_of_a_bound():
    la = bc.landings()
    assert len(la) >= 18
    assert {k[:7] for k in la} == {"land_%d%d" % (a, b) for a in range(3) for b in range(3)}
    for k, s in la.items():
        L, st = restated(k)
        assert st["near_pn"] > 0 and len(L["points"]) >= 2, k
    st = total(la)
    assert st["switch_pn"] > 0 and st["end_%d" % bs.STEPS] > 0
    ends = collections.Counter(int(restated(k)[0]["info"][0, 1]) >> 8 for k in la)
    assert len(ends) >= 2          # on one side of a bound the line goes on, on the other it ends


def test_many_blocks_scan_every_box():
    mb = bc.many_blocks()
    assert [len(mb["row_%d" % n]["blocks"]) for n in bc.ROW_SIZES] == [255, 256, 257, 4097, 65535]
    assert bc.MAX_BLOCKS == 65535 and len({id(b["vectors"]) for b in mb["row_65535"]["blocks"]}) == 16
    for n in bc.ROW_SIZES:
        L, st = restated("row_%d" % n)
        seed_at = L["off"][:-1] + L["info"][:, 0]
        inside = L["info"][:, 1] != OUT
        assert inside.tolist() == [True] * 5 + [False] * 2
        # the first, the middle, the last but one, the last block; on the last plane the lower block
        assert L["blocks"][seed_at[:5]].tolist() == [0, n // 2, n - 2, n - 1, n - 2]
        # two seeds outside: two full scans; a half that leaves the last block: a miss after all n
        assert st["seed_full_scan"] == 2 and st["seed_scanned"] >= 2 * n + n - 1
        assert st["full_scan"] >= 2 and st["scan_max"] == n
        assert st["hit_last"] >= 2          # a half that enters the last block from the one before
        assert st["scanned"] > st["miss"] * n // 4
    L, st = restated("row_4097_long")
    assert len(np.unique(L["blocks"])) > 600 and st["switch"] > 600
    assert L["info"].tolist() == [[600, bs.STEPS | bs.STEPS << 8]] and len(L["points"]) == 1201
    assert (np.diff(L["blocks"].astype(int)) >= 0).all()
    x = L["points"][:, 0]
    assert ((L["blocks"] <= x) & (x <= L["blocks"] + 1)).all()      # the unit block that holds x
    # the stack: 64 blocks hold every point, block 0 samples it; reversed, block 0 has other data
    L, st = restated("stack64")
    R, rst = restated("stack64_reversed")
    assert st["in_several"] > 30 and not L["blocks"].any() and not R["blocks"].any()
    assert not same(L["points"], R["points"])
    assert st["miss"] == st["full_scan"] and st["seed_scanned"] == 5   # no miss but to leave all 64
    # the reversed row: a seed on a shared plane starts in the block listed first, the upper one
    L, st = restated("row_257_reversed")
    seed_at = L["off"][:-1] + L["info"][:, 0]
    assert L["blocks"][seed_at[-3:]].tolist() == [256 - 1, 256 - 128, 256 - 256]
    F, _ = restated("row_257")
    assert L["blocks"][seed_at[4]] == 0 and F["blocks"][F["off"][4] + F["info"][4, 0]] == 255


def test_probe_positions_lie_in_every_trip(spray):
    """The check pass covers 64 x 256 = 16,384 elements per trip of its
    grid-stride loops (kCheckBlocks, kCheckBlock of block_stream_kernels.hip)."""
    s = bc.probe33()
    b = s["blocks"][0]
    sizes = {"vectors": b["vectors"].size, "cfield": b["cfield"].size, "seeds": s["seeds"].size}
    assert sizes == {"vectors": 107811, "cfield": 35937, "seeds": 18000} and bc.TRIP == 16384
    for key, trips in (("vectors", 7), ("cfield", 3), ("seeds", 2)):
        pos = bc.probe_positions(sizes[key])
        assert (sizes[key] + bc.TRIP - 1) // bc.TRIP == trips and len(pos) == trips + 1
        assert [p // bc.TRIP for p in pos[:-1]] == list(range(trips))     # a bad element in every trip
        assert pos[-1] == sizes[key] - 1 and pos == sorted(set(pos))
        assert pos[0] == 0 and (trips < 4 or pos[1:3] == [2 * bc.TRIP - 1, 2 * bc.TRIP])
        for j, p in enumerate(pos):   # the host forms refuse each
            bad = bc.probed(s, key, p, bc.PROBE_VALUES[j % 3])
            with pytest.raises(spray.SprayRtError) as e:
                host_tubes(spray, bad, 0.0625, 4)
            assert e.value.code == ERR_ARG
            if key != "cfield":
                with pytest.raises(spray.SprayRtError) as e:
                    host_lines(spray, bad)
                assert e.value.code == ERR_ARG
    p, off, info, blk = host_lines(spray, s)
    assert len(p) > 12000 and not blk.any()


def test_bad_blocks_of_the_row(spray):
    s = bc.row300()
    assert len(s["blocks"]) == 300 and s["blocks"][0]["cfield"] is not None
    assert bc.ROW300_BAD == (((299,), ()), ((17, 299), ()), ((299, 17, 250), ()), ((9,), (3,)))
    for vec, col in bc.ROW300_BAD:
        bad = bc.row300_bad(vec, col)
        for k, b in enumerate(bad["blocks"]):
            assert np.isfinite(b["vectors"]).all() == (k not in vec)
            assert np.isfinite(b["cfield"]).all() == (k not in col)
        with pytest.raises(spray.SprayRtError) as e:
            host_tubes(spray, bad, 0.0625, 4)
        assert e.value.code == ERR_ARG
    p, off, info, blk = host_lines(spray, bc.row300_bad((), (3,)))   # colour: nothing to the polylines
    assert len(p) > 20


def test_orbits_are_their_closed_form(spray):
    """513 lines of 2 x 4,100 + 1 points on closed orbits through eight blocks."""
    s = bc.orbits()
    S = bc.ORBIT_STEPS
    assert bc.nlanes(s) == 1026 and (bc.nlanes(s) + bc.LANES - 1) // bc.LANES == 5
    assert len(s["blocks"]) == 8 and all(b["vectors"].shape == (9, 9, 9, 3) for b in s["blocks"])
    # a full workgroup holds 128 forward halves with their seeds and 128 backward ones
    assert 128 * (S + 1) + 128 * S > 1 << 20
    p, off, info, blk = host_lines(spray, s)
    assert off.tolist() == [(2 * S + 1) * l for l in range(514)]
    assert info.tolist() == [[S, bs.STEPS | bs.STEPS << 8]] * 513
    r = np.hypot(p[:, 0] - 8.0, p[:, 1] - 8.0)
    assert 1.4 < r.min() and r.max() < 7.01
    # the block of a point off the shared planes is its octant
    octant = (p[:, 0] > 8).astype(int) + 2 * (p[:, 1] > 8) + 4 * (p[:, 2] > 8)
    off_plane = (p != 8.0).all(1)
    assert off_plane.mean() > 0.999 and np.array_equal(blk[off_plane], octant[off_plane])
    lines = blk.reshape(513, 2 * S + 1).astype(int)
    crossings = (np.diff(lines, axis=1) != 0).sum(1)
    assert crossings.min() >= 4 * 18      # four blocks a revolution, some twenty revolutions a half
    # the first steps of 40 of the lines against the restatement
    sub = dict(s, seeds=s["seeds"][::13], max_steps=12)
    L = bc.lines_numpy(sub)
    q, qoff, qinfo, qblk = host_lines(spray, sub)
    assert same(q, L["points"]) and same(qblk, L["blocks"]) and same(qinfo, L["info"])
    full = p.reshape(513, 2 * S + 1, 3)[::13, S - 12:S + 13]
    assert same(np.ascontiguousarray(full).reshape(-1, 3), q)


def test_fullblock_is_its_closed_form(spray):
    s = bc.fullblock()
    assert bc.nlanes(s) == 257 and bc.LANES * (s["max_steps"] + 1) == 1 << 24
    assert [b["origin"][0] for b in s["blocks"]] == [0.0, 32768.0]
    pick = [0, 131, 256]
    sub = dict(s, seeds=s["seeds"][pick])
    p, off, info, blk = host_lines(spray, sub)
    want = np.zeros((3, 65536, 3), F32)
    want[:, :, 0] = np.arange(65536)
    want[:, :, 1:] = s["seeds"][pick, None, 1:]
    assert same(p, want.reshape(-1, 3))
    assert off.tolist() == [0, 65536, 131072, 196608]
    assert info.tolist() == [[0, bs.STEPS | bs.STEPS << 8]] * 3
    # block 0 holds the line up to and on its upper face
    assert same(blk, np.tile(np.arange(65536) > 32768, 3).astype(np.uint32))
    L = bc.lines_numpy(dict(sub, seeds=[[32760.0, 0.25, 0.5]], max_steps=20))
    h = host_lines(spray, dict(sub, seeds=[[32760.0, 0.25, 0.5]], max_steps=20))
    assert same(h[0], L["points"]) and same(h[3], L["blocks"]) and L["blocks"].tolist() == [0] * 9 + [1] * 12
    ns = s["tube"]["nsides"]
    nv, nf = host_tubes(spray, s, s["tube"]["radius"], ns, count_only=True)
    assert (nv, nf) == (257 * 65536 * ns + 2 * 257, 2 * ns * 257 * 65536)


def test_longest_is_its_closed_form(spray):
    s = bc.longest()
    p, off, info, blk = host_lines(spray, s)
    assert off.tolist() == [0, 131071, 131073]
    assert info.tolist() == [[65535, bs.GRID | bs.STEPS << 8], [1, bs.GRID | bs.GRID << 8]]
    want = np.zeros((131073, 3), F32)
    want[:131071, 0] = np.arange(131071)
    want[131071:] = [[1000, 0.25, 1], [1000, 1, 1]]
    assert same(p, want)
    # the seed (x = 65535) and the plane point stay in block 0; both halves start there
    assert same(blk, np.concatenate([np.arange(131071) > 65536, [0, 0]]).astype(np.uint32))
    L = bc.lines_numpy(dict(s, max_steps=30))
    assert same(L["points"][:61], want[65535 - 30:65535 + 31])
    assert same(L["blocks"][:61], blk[65535 - 30:65535 + 31])


def test_gaps_keep_their_runs():
    for k in bc.GAP_PICK:
        s = SMALL[k]
        L, st = restated(k)
        m = np.diff(L["off"].astype(np.int64))
        assert np.array_equal(m, sc.gaps()[k]["want"]), k
        assert len(s["blocks"]) == 2 and [b["vectors"].shape[2] for b in s["blocks"]] == [21, 21]
        assert st["switch"] > 0 and (bc.nlanes(s) + bc.LANES - 1) // bc.LANES >= 6
        # an empty run longer than a workgroup
        assert (np.diff(np.flatnonzero(np.concatenate([[True], m != 0, [True]]))) - 1).max() > bc.LANES


def test_mid_step_classes_reach_their_paths():
    mid = bc.mid_steps()
    assert len(mid) == 24
    for d, direction in (("fwd", bs.FORWARD), ("back", bs.BACKWARD)):
        names = [k for k in mid if k.endswith(d)]
        assert all(mid[k]["direction"] == direction for k in names)
        st = total(names)
        for c in bc.MID_CLASSES:
            assert st[c] >= 3, (d, c, st[c])
        for stage in bc.STAGES:
            assert st["switch_" + stage] > 0 and st["grid_" + stage] > 0, (d, stage)
        assert st["gap_q2"] and st["gap_q3"] and st["gap_q4"] and st["gap_pn"]
        assert st["three_blocks_in_step"] > 0 and st["sticky_over_lower"] > 0
        for layout in bc.MID_LAYOUTS:   # every layout changes block in mid-step
            assert total([k for k in names if "_%s_" % layout in k])["changes_2"] > 0
    # the mirror runs the same points backward
    for k in mid:
        if k.endswith("fwd"):
            F, B = restated(k)[0], restated(k[:-3] + "back")[0]
            assert same(F["off"], B["off"])
            for a, b in zip(F["off"][:-1], F["off"][1:]):
                assert same(F["points"][a:b], np.ascontiguousarray(B["points"][a:b][::-1]))
            assert restated(k)[1]["only_q3"] == restated(k[:-3] + "back")[1]["only_q3"]


def test_carried_fields_cross_their_plane():
    ca = bc.carried()
    assert len(ca) == 36 and all(len(s["blocks"]) == 2 for s in ca.values())
    st = total(ca)
    for key in ("switch", "speed_low", "speed_overflow", "no_motion", "axis_tie", "axis_0", "axis_1",
                "axis_2", "on_shared_face", "sticky_over_lower"):
        assert st[key] > 0, key
    # the stall converges on the shared plane x = 1: the last points are on it, in both blocks
    L, st = restated("split_stall")
    assert st["no_motion"] >= 4 and st["on_shared_face"] > 0 and set(L["blocks"]) == {0, 1}
    # the frame threshold pair still flips between adjacent floats, now with the turn in block 1
    a, b = restated("split_turn_pair_repick")[0], restated("split_turn_pair_carried")[0]
    assert a["blocks"].tolist() == [0, 1, 1] and not same(a["normals"], b["normals"])
    for k in ("split_sub_z0", "split_sub_zy", "split_sub_x", "split_sub_y"):
        T = np.abs(restated(k)[0]["tangents"][0])
        assert ((T > 0) & (T < sc.FLT_MIN)).any(), k
    assert restated("split_fast_over")[1]["speed_overflow"] == 4
    assert len(restated("split_tiny")[0]["points"]) > 8


@pytest.mark.parametrize("name", NAMES)
def test_host_forms_equal_numpy(spray, name):
    i = NAMES.index(name)
    s = bc.with_colors(SMALL[name], 50 + i) if i % 3 else SMALL[name]
    L = bc.lines_numpy(s)
    p, off, info, blk = host_lines(spray, s)
    assert same(p, L["points"]) and same(off, L["off"]) and same(info, L["info"])
    assert same(blk, L["blocks"])
    t = bc.tube_of(s, i)
    color = t["color"] if t["color"] is not None else 0
    ring = spray.tube_ring(t["nsides"])
    ref = bs.tubes_numpy(s, L, t["radius"], t["nsides"], ring, color=color)
    v, n, c, fc = host_tubes(spray, s, t["radius"], t["nsides"], color=color)
    assert same(v, ref[0]) and same(n, ref[1]) and same(c, ref[2]) and same(fc, ref[3])
    assert host_tubes(spray, s, t["radius"], t["nsides"], count_only=True) == (len(v), len(fc))

"""The multi-block streamline filter's host forms
(spray_rt_block_streamlines_host, spray_rt_block_stream_tubes_host; no GPU)
against the numpy restatement of the block rule (block_stream_helpers.py), byte
for byte on every case, and the two properties the rule promises: (P1) a set of
one block gives the single-grid forms' bytes, (P2) index sub-boxes of a grid at
origin 0 with power-of-two spacing give the unsplit grid's bytes as long as no
located point lies on a shared plane, which the restatement counts.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import block_stream_helpers as bs
import stream_helpers as sh

F32 = np.float32
ERR_ARG, ERR_LIMIT = -1, -5
NAMES = sorted(bs.cases())
SPLITS = ("rotation_both", "rotation_fwd", "rotation_back", "abc_both", "abc_fwd", "abc_back")


@pytest.fixture(scope="module")
def spray():
    from spray_amd import build
    build.build()
    import spray_amd
    return spray_amd


def host_lines(spray, s):
    return spray.block_streamlines_host(*bs.host_args(s), **bs.host_kw(s))


def host_tubes(spray, s, radius, nsides, **kw):
    return spray.block_stream_tubes_host(*bs.host_args(s), radius, nsides, cmap=s.get("cmap"),
                                         **bs.host_kw(s), **kw)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_cases_reach_their_paths():
    """From the numpy side: every path of the block rule the cases are there for."""
    st = {k: bs.restated(k)[1] for k in NAMES}
    L = {k: bs.restated(k)[0] for k in NAMES}
    cases = bs.cases()
    assert [len(cases[k]["blocks"]) for k in SPLITS] == [8] * 6
    assert all(b["vectors"].shape == (5, 5, 5, 3) for b in cases["abc_both"]["blocks"])
    assert {cases[k]["direction"] for k in SPLITS} == {bs.FORWARD, bs.BACKWARD, bs.BOTH}
    assert len(cases["rotation_both"]["seeds"]) == 130         # 260 lanes: two workgroups
    for k in ("rotation_both", "rotation_fwd", "rotation_back"):
        # lines that cross and return: many more switches than lines
        assert st[k]["switch"] > 3 * len(cases[k]["seeds"]), k
    assert all(st[k]["switch"] > 0 and st[k]["on_shared_face"] == 0 for k in SPLITS)
    # seeds on a shared plane and at the corner of eight blocks start in the lowest block
    on = L["on_planes"]
    seed_at = on["off"][:-1] + on["info"][:, 0]
    assert on["blocks"][seed_at].tolist() == [0, 0, 4, 7, 0] and st["on_planes"]["on_shared_face"] >= 3
    rv = L["reversed"]
    assert rv["blocks"][(rv["off"][:-1] + rv["info"][:, 0])[12:]].tolist() == [6, 0, 1, 0, 7]
    # stickiness: points of the overlap sampled in block 1 although block 0 holds them
    ov = L["overlap"]
    assert st["overlap"]["sticky_over_lower"] > 0
    x = ov["points"][:, 0]
    assert ((ov["blocks"] == 1) & (x >= 3) & (x <= 5)).any() and ((ov["blocks"] == 0) & (x >= 3)).any()
    assert st["refined"]["switch"] > 0 and set(L["refined"]["blocks"]) == {0, 1}
    g = L["gap"]
    assert g["info"][0, 1] >> 8 == bs.GRID and g["info"][1].tolist() == [0, bs.SEED | bs.SEED << 8]
    assert st["gap"]["switch"] == 0 and st["gap"]["seed_outside"] == 1
    # a float beyond a face of the set is outside, on it and a float before it inside
    fu = L["face_ulps"]["info"][:, 1] == (bs.SEED | bs.SEED << 8)
    lower, upper, inner = [False, False, True], [False, True, False], [False] * 3
    assert fu.tolist() == lower + inner + upper + (lower + upper) * 2
    assert st["hop3"]["three_blocks_in_step"] > 0
    assert all(b["vectors"].shape == (2, 2, 2, 3) for b in cases["hop3"]["blocks"])
    assert st["aligned"]["on_shared_face"] > 10 and st["aligned"]["switch"] > 0
    assert len(L["steps0"]["points"]) == 5 and (L["steps0"]["info"][:, 0] == 0).all()
    assert np.diff(L["steps1_fwd"]["off"].astype(int)).tolist() == [2, 2]
    assert len(L["no_seeds"]["points"]) == 0 and L["no_seeds"]["off"].tolist() == [0]
    assert len(cases["one_block"]["blocks"]) == 1
    assert bs.case("abc_both")["cmap"][0].size == 37


@pytest.mark.parametrize("name", NAMES)
def test_host_forms_equal_numpy(spray, name):
    s = bs.case(name)
    L = bs.restated(name)[0]
    for _ in range(2):
        p, off, info, blk = host_lines(spray, s)
        assert same(p, L["points"]) and same(off, L["off"]) and same(info, L["info"])
        assert same(blk, L["blocks"])
    ring = spray.tube_ring(5)
    ref = bs.tubes_numpy(s, L, 0.03125, 5, ring, color=0x00A1B2C3)
    v, n, c, fc = host_tubes(spray, s, 0.03125, 5, color=0x00A1B2C3)
    assert same(v, ref[0]) and same(n, ref[1]) and same(c, ref[2]) and same(fc, ref[3])
    if len(fc):
        assert host_tubes(spray, s, 0.03125, 5, count_only=True) == (len(v), len(fc))
        assert host_tubes(spray, s, 0.03125, 5, normals=False)[1] is None
    if name in bs.COLORED:
        assert len(np.unique(c)) > 3


def test_one_block_equals_the_single_grid_forms(spray):
    """P1."""
    s = bs.case("one_block")
    f = bs.as_field(s)
    p, off, info, blk = host_lines(spray, s)
    gp, goff, ginfo = spray.streamlines_host(*sh.host_args(f), **sh.host_kw(f))
    assert len(p) > 100 and same(p, gp) and same(off, goff) and same(info, ginfo)
    assert not blk.any()
    for kw in (dict(color=0x00C0FFEE), dict()):
        got = host_tubes(spray, s, 0.0625, 7, **kw)
        ref = spray.stream_tubes_host(*sh.host_args(f), 0.0625, 7, cfield=f["cfield"],
                                      cmap=f["cmap"], **sh.host_kw(f), **kw)
        assert all(same(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("name", SPLITS)
def test_plane_sharing_splits_equal_the_unsplit_grid(spray, name):
    """P2; the third condition is asserted from the restatement's count."""
    s = bs.cases()[name]
    assert bs.restated(name)[1]["on_shared_face"] == 0
    assert all(float(x) == 0.25 for x in bs.SPACING)
    for b in s["blocks"]:
        assert all(float(o) / 0.25 == int(float(o) / 0.25) for o in b["origin"])
    f = bs.unsplit(s, name.split("_")[0])
    p, off, info, blk = host_lines(spray, s)
    gp, goff, ginfo = spray.streamlines_host(*sh.host_args(f), **sh.host_kw(f))
    assert len(p) > 80 and same(p, gp) and same(off, goff) and same(info, ginfo)
    assert len(np.unique(blk)) > 3
    got = host_tubes(spray, s, 0.015625, 6, color=0x00204060)
    ref = spray.stream_tubes_host(*sh.host_args(f), 0.015625, 6, color=0x00204060, **sh.host_kw(f))
    assert all(same(a, b) for a, b in zip(got, ref))


def test_points_on_shared_planes_follow_the_rule_not_the_unsplit_grid(spray):
    """The aligned case's points are the unsplit grid's here as well (a uniform
    field is the same in every cell); its blocks are the rule's: the block a
    line is in holds a point on its upper face, the next one takes over only
    beyond it."""
    s = bs.cases()["aligned"]
    p, off, info, blk = host_lines(spray, s)
    x = p[off[0]:off[1], 0]
    b = blk[off[0]:off[1]]
    assert (x == 1.0).any() and b[x == 1.0].tolist() == [0] and set(b[x > 1.0]) == {1}
    # backward from a seed in block 1 the plane point stays in block 1
    x, b = p[off[3]:off[4], 0], blk[off[3]:off[4]]
    assert b[x == 1.0].tolist() == [1] and set(b[x < 1.0]) == {0}


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """tests/cpp/block_stream_host_check.cpp with the host restatements of
    streamlines.cpp and block_streamlines.cpp (SPRAY_RT_STREAM_HOST_ONLY:
    nothing that needs the HIP runtime), built by g++ under the address and
    undefined-behaviour sanitizers and run as a plain executable.  It also
    holds the box of the miss path to the division by brute force."""
    from spray_amd import build
    root = build.ROOT
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    exe = str(tmp_path / "block_stream_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-DSPRAY_RT_STREAM_HOST_ONLY",
                        "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(root, "include"),
                        "-I" + build.CSRC, os.path.join(build.CSRC, "streamlines.cpp"),
                        os.path.join(build.CSRC, "block_streamlines.cpp"),
                        os.path.join(root, "tests", "cpp", "block_stream_host_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures")


# ---- errors ----

def raw(spray, s, tube=None, patch=None):
    """The host forms through ctypes on records patch(arr, blocks, carr) may
    change -> the return code (of the tube form where tube is given)."""
    from spray_amd import engine
    from spray_amd._native import lib
    arr, tarr, carr, keep = engine._block_tables([s], tube)
    if patch:
        patch(arr[0], keep[0], carr[0])
    n, m = C.c_size_t(7), C.c_size_t(7)
    if tube is None:
        return lib().spray_rt_block_streamlines_host(C.addressof(arr), C.byref(n), None, None,
                                                     None, None)
    return lib().spray_rt_block_stream_tubes_host(C.addressof(arr), C.addressof(tarr),
                                                  C.addressof(carr), C.byref(n), C.byref(m), None,
                                                  None, None, None)


def fails(spray, code, s, radius=0.1, nsides=6, tubes_only=False):
    if not tubes_only:
        with pytest.raises(spray.SprayRtError) as e:
            host_lines(spray, s)
        assert e.value.code == code
    with pytest.raises(spray.SprayRtError) as e:
        host_tubes(spray, s, radius, nsides)
    assert e.value.code == code


def with_block(s, k, **kw):
    blocks = list(s["blocks"])
    blocks[k] = dict(blocks[k], **kw)
    return dict(s, blocks=blocks)


def test_argument_errors(spray):
    good = bs.case("abc_both")
    plain = bs.cases()["abc_both"]
    tube = dict(radius=0.1, nsides=6)
    assert raw(spray, good) == 0 and raw(spray, good, tube) == 0 and raw(spray, plain, tube) == 0
    inf, nan = np.inf, np.nan
    # the set
    fails(spray, ERR_ARG, dict(good, blocks=[]))
    for t in (None, tube):
        def nblocks(v):
            return lambda rec, blocks, crec: setattr(rec, "nblocks", v)
        assert raw(spray, good, t, nblocks(0)) == ERR_ARG
        assert raw(spray, good, t, nblocks(-1)) == ERR_ARG
        assert raw(spray, good, t, nblocks(65536)) == ERR_ARG     # rejected before a block is read
        assert raw(spray, good, t, lambda rec, blocks, crec: setattr(rec, "blocks", None)) == ERR_ARG
        assert raw(spray, good, t, lambda rec, blocks, crec: setattr(rec, "seeds", None)) == ERR_ARG
        for k in (0, 7):
            assert raw(spray, good, t,
                       lambda rec, blocks, crec: setattr(blocks[k], "vectors", None)) == ERR_ARG
    for key, bad in (("step", 0.0), ("step", nan), ("max_steps", -1), ("max_steps", 65536),
                     ("direction", 3), ("min_speed", 0.0), ("min_speed", 1e-20)):
        fails(spray, ERR_ARG, dict(good, **{key: bad}))
    # a block: the last one, so that every block is looked at
    for key, bad in (("spacing", (1, 0, 1)), ("spacing", (inf, 1, 1)), ("origin", (0, nan, 0))):
        fails(spray, ERR_ARG, with_block(good, 7, **{key: bad}))
    fails(spray, ERR_ARG, with_block(good, 7, vectors=np.zeros((5, 1, 5, 3), F32), cfield=None))
    for k, where in ((0, (0, 0, 0, 0)), (7, (4, 4, 4, 2))):
        v = good["blocks"][k]["vectors"].copy()
        v[where] = nan
        fails(spray, ERR_ARG, with_block(good, k, vectors=v))
    s = good["seeds"].copy()
    s[3, 1] = -inf
    fails(spray, ERR_ARG, dict(good, seeds=s))
    # colour fields on some blocks but not on all, either way round
    fails(spray, ERR_ARG, with_block(good, 5, cfield=None))
    fails(spray, ERR_ARG, with_block(plain, 7, cfield=good["blocks"][7]["cfield"]))
    # a table for a set without colour fields; colour fields without a usable table
    fails(spray, ERR_ARG, dict(plain, cmap=good["cmap"]), tubes_only=True)
    tab = good["cmap"][0]
    for cmap in (None, (np.zeros(0, np.uint32), 0.0, 1.0), (np.zeros(4097, np.uint32), 0.0, 1.0),
                 (tab, 1.0, 1.0), (tab, nan, 1.0)):
        fails(spray, ERR_ARG, dict(good, cmap=cmap), tubes_only=True)
    g = good["blocks"][7]["cfield"].copy()
    g[4, 4, 4] = nan
    fails(spray, ERR_ARG, with_block(good, 7, cfield=g), tubes_only=True)
    host_lines(spray, with_block(good, 7, cfield=g))     # it does not matter to the polylines
    for radius in (0.0, nan):
        fails(spray, ERR_ARG, good, radius=radius, tubes_only=True)
    fails(spray, ERR_ARG, good, nsides=17, tubes_only=True)
    from spray_amd._native import lib
    n = C.c_size_t()
    assert lib().spray_rt_block_streamlines_host(None, C.byref(n), None, None, None, None) == ERR_ARG


def test_limits(spray):
    good = bs.cases()["abc_both"]

    def dims(k, d):
        return lambda rec, blocks, crec: setattr(blocks[k], "dims", (C.c_int32 * 3)(*d))
    assert raw(spray, good, None, dims(7, (2048, 1024, 1024))) == ERR_LIMIT   # no sample is read
    assert raw(spray, good, None, dims(0, (1 << 11, 1 << 10, 1 << 10))) == ERR_LIMIT
    assert raw(spray, good, None, lambda rec, blocks, crec: setattr(rec, "nseeds", 1 << 31)) \
        == ERR_LIMIT

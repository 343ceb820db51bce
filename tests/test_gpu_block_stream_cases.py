"""The multi-block streamline kernels at their scale limits and on the hard
boxes of block_stream_cases.py (spray_rt_block_streamlines,
spray_rt_block_stream_tubes, spray_rt_domains_block_stream_tubes).

References, each bit for bit and none a second GPU run: the host forms (held to
numpy on the same inputs by test_block_stream_cases.py) in every array, the
block of every point included, and the closed forms of the long sets; a
build_domains of the restated arrays in a second context for the slot images.

What the inputs execute that test_gpu_block_streamlines.py does not: the box of
the miss path against the device's division where quotients round, at subnormal
and at huge bounds and at origins where p - origin rounds; a miss path of up to
65,535 boxes, its last box hit and all of them missed; the second and every
later trip of the check pass's loops and its atomicMin among several bad
blocks; five workgroups of lines of 8,201 points, a workgroup sum of 2^24 and a
line with 65,535 points behind its seed, each across blocks; every stage of a
step in another block than the one before it, and in a gap.
"""
import numpy as np
import pytest

import block_stream_cases as bc
import block_stream_helpers as bs
import refit_helpers as rh
from test_gpu_block_streamlines import (ERR_ARG, ERR_LIMIT, as_bytes, export_all, ref_bytes,
                                        slot_colors, synced)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


def on_device(sets):
    """The sets with their arrays as tensors on the GPU; an array that several
    blocks share is one tensor."""
    import torch
    made = {}

    def put(x):
        if x is None:
            return None
        if id(x) not in made:
            made[id(x)] = (x, torch.from_numpy(np.ascontiguousarray(x)).cuda())
        return made[id(x)][1]
    return [dict(s, seeds=put(s["seeds"]),
                 blocks=[dict(b, vectors=put(b["vectors"]), cfield=put(b.get("cfield")))
                         for b in s["blocks"]]) for s in sets]


def host_forms(spray, sets, tubes, meshes=True):
    lines, out = [], []
    for s, t in zip(sets, tubes):
        lines.append(spray.block_streamlines_host(*bs.host_args(s), **bs.host_kw(s)))
        if meshes:
            out.append(spray.block_stream_tubes_host(*bs.host_args(s), t["radius"], t["nsides"],
                                                     color=t["color"], cmap=s.get("cmap"),
                                                     **bs.host_kw(s)))
    return lines, out


def small_sets():
    """(names, sets, tubes) of the hard boxes, the landings, the mid-step sets
    and the carried fields; two in three get colour fields."""
    cases = dict(bc.hard_boxes(), **bc.landings(), **bc.mid_steps(), **bc.carried())
    names = sorted(cases)
    sets = [bc.with_colors(cases[k], 70 + i) if i % 3 else cases[k] for i, k in enumerate(names)]
    return names, sets, [bc.tube_of(s, i) for i, s in enumerate(sets)]


@pytest.fixture(scope="module")
def batch():
    return small_sets()


@pytest.fixture(scope="module")
def restated(spray, batch):
    names, sets, tubes = batch
    return host_forms(spray, sets, tubes)


def raises(spray, call, code, *words):
    with pytest.raises(spray.SprayRtError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    return e.value


def untouched(c, err):
    c.sync()
    for bufs in err.buffers:
        assert all(int(b.abs().max()) == 0 for b in bufs)


def test_batch_shapes(batch, restated):
    names, sets, tubes = batch
    lines, meshes = restated
    assert len(sets) == len(bc.hard_boxes()) + len(bc.landings()) + 24 + 36 and len(sets) > 115
    assert {len(s["blocks"]) for s in sets} == {2, 3}
    assert sum(len(l[0]) for l in lines) > 5000 and sum(len(m[3]) for m in meshes) > 50000
    assert sum(s["blocks"][0].get("cfield") is not None for s in sets) > len(sets) // 2
    assert any((l[3] == 2).any() for l in lines)


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_small_sets_equal_the_host_forms(spray, batch, restated, device):
    """One batched call over every hard-box, landing, mid-step and carried set."""
    names, sets, tubes = batch
    lines, meshes = restated
    c = spray.RtContext(0)
    ss = on_device(sets) if device else sets
    got = [as_bytes(x) for x in synced(c, c.block_streamlines(ss))]
    assert [names[k] for k, ref in enumerate(lines) if got[k] != ref_bytes(ref)] == []
    tub = [as_bytes(x) for x in synced(c, c.block_stream_tubes(ss, tubes))]
    assert [names[k] for k, ref in enumerate(meshes) if tub[k] != ref_bytes(ref)] == []
    # reversed, without normals: the same bytes per set
    rev = [as_bytes(x) for x in synced(c, c.block_streamlines(ss[::-1]))][::-1]
    assert rev == got
    rev = [as_bytes(x) for x in
           synced(c, c.block_stream_tubes(ss[::-1], tubes[::-1], normals=False))][::-1]
    for k in range(len(sets)):
        assert rev[k] == (tub[k][0], None, tub[k][2], tub[k][3]), names[k]
    assert c.block_streamlines(ss, count_only=True) == [len(l[0]) for l in lines]
    assert c.block_stream_tubes(ss, tubes, count_only=True) == \
        [(len(m[0]), len(m[3])) for m in meshes]
    c.close()


@pytest.mark.parametrize("name", sorted(bc.many_blocks()))
def test_many_blocks_equal_the_host_forms(spray, name):
    """One call a set; 65,535 blocks as polylines only."""
    s = bc.many_blocks()[name]
    t = bs.tube_of(3)
    tubes = len(s["blocks"]) < bc.MAX_BLOCKS
    (lines,), meshes = host_forms(spray, [s], [t], tubes)
    c = spray.RtContext(0)
    dev = on_device([s])
    assert as_bytes(synced(c, c.block_streamlines(dev))[0]) == ref_bytes(lines), name
    if tubes:
        assert as_bytes(synced(c, c.block_stream_tubes(dev, [t]))[0]) == ref_bytes(meshes[0]), name
    if name in ("row_257", "stack64", "row_65535"):     # from host arrays as well
        assert as_bytes(synced(c, c.block_streamlines([s]))[0]) == ref_bytes(lines), name
    if name == "row_65535":
        seed_at = lines[1][:-1] + lines[2][:, 0]
        assert lines[3][seed_at[:5]].tolist() == [0, 32767, 65533, 65534, 65533]
    c.close()


def test_orbits_equal_the_host_form(spray):
    """513 lines of 8,201 points in five workgroups, four of them above 2^20 points."""
    s = bc.orbits()
    S = bc.ORBIT_STEPS
    total = 513 * (2 * S + 1)
    (lines,), _ = host_forms(spray, [s], [None], False)
    assert len(lines[0]) == total and lines[2][:, 0].tolist() == [S] * 513
    c = spray.RtContext(0)
    dev = on_device([s])
    assert c.block_streamlines(dev, count_only=True) == [total]
    err = raises(spray, lambda: c.block_streamlines(dev, capacity=total - 1), ERR_LIMIT, "set 0")
    assert err.counts == [total]
    untouched(c, err)
    del err
    got, = synced(c, c.block_streamlines(dev, capacity=total))
    assert as_bytes(got) == ref_bytes(lines)
    c.close()


def test_fullblock_equals_its_closed_form(spray):
    """257 forward lanes of 65,535 steps across two blocks: workgroup 0 sums to
    exactly 2^24 points and 2^24 tube points, lane 256 starts at 2^24."""
    import torch
    s = bc.fullblock()
    t = s["tube"]
    total = 257 * 65536
    c = spray.RtContext(0)
    dev = on_device([s])
    assert c.block_streamlines(dev, count_only=True) == [total]
    ns = t["nsides"]
    assert c.block_stream_tubes(dev, [t], count_only=True) == [(total * ns + 2 * 257, 2 * ns * total)]
    err = raises(spray, lambda: c.block_streamlines(dev, capacity=total - 1), ERR_LIMIT, "set 0")
    assert err.counts == [total]
    untouched(c, err)
    del err
    (p, off, info, blk), = synced(c, c.block_streamlines(dev, capacity=total))
    assert tuple(p.shape) == (total, 3)
    want = torch.empty((257, 65536, 3), dtype=torch.float32, device=p.device)
    want[:, :, 0] = torch.arange(65536, dtype=torch.float32, device=p.device)
    want[:, :, 1:] = dev[0]["seeds"][:, None, 1:]
    assert torch.equal(p.view(torch.int32), want.view(total, 3).view(torch.int32))
    # block 0 up to and on its upper face x = 32768, block 1 beyond
    wantb = (torch.arange(65536, device=p.device) > 32768).to(torch.int32).repeat(257)
    assert torch.equal(blk, wantb)
    assert off.cpu().numpy().view(np.uint32).tolist() == [65536 * l for l in range(258)]
    assert info.cpu().numpy().tolist() == [[0, bs.STEPS | bs.STEPS << 8]] * 257
    c.close()


def test_longest_line_equals_the_host_form(spray):
    """One line of 131,071 points with nback = 65535 across two blocks, then one of two points."""
    s = bc.longest()
    t = s["tube"]
    (lines,), (mesh,) = host_forms(spray, [s], [t])
    assert lines[1].tolist() == [0, 131071, 131073] and lines[2][0, 0] == 65535
    assert set(lines[3].tolist()) == {0, 1}
    nv, nf = len(mesh[0]), len(mesh[3])
    c = spray.RtContext(0)
    dev = on_device([s])
    got, = synced(c, c.block_streamlines(dev))
    assert as_bytes(got) == ref_bytes(lines)
    for cap in ((nv - 1, nf), (nv, nf - 1)):
        err = raises(spray, lambda: c.block_stream_tubes(dev, [t], capacity=cap), ERR_LIMIT, "set 0")
        assert err.counts == [(nv, nf)]
        untouched(c, err)
        del err
    got, = synced(c, c.block_stream_tubes(dev, [t], capacity=(nv, nf)))
    assert as_bytes(got) == ref_bytes(mesh)
    c.close()


def test_gap_runs_equal_the_host_forms(spray):
    """Empty runs longer than a workgroup, over two blocks; capacities one short."""
    g = bc.gaps()
    names = sorted(g)
    sets, tubes = [g[k] for k in names], [g[k]["tube"] for k in names]
    lines, meshes = host_forms(spray, sets, tubes)
    c = spray.RtContext(0)
    dev = on_device(sets)
    npts = [len(l[0]) for l in lines]
    err = raises(spray, lambda: c.block_streamlines(dev, capacity=max(npts) - 1), ERR_LIMIT)
    assert err.counts == npts
    untouched(c, err)
    del err
    got = synced(c, c.block_streamlines(dev, capacity=max(npts)))
    assert [as_bytes(x) for x in got] == [ref_bytes(l) for l in lines]
    nv, nf = [len(m[0]) for m in meshes], [len(m[3]) for m in meshes]
    for cap in ((max(nv) - 1, max(nf)), (max(nv), max(nf) - 1)):
        err = raises(spray, lambda: c.block_stream_tubes(dev, tubes, capacity=cap), ERR_LIMIT)
        assert err.counts == list(zip(nv, nf))
        untouched(c, err)
        del err
    got = synced(c, c.block_stream_tubes(dev, tubes, capacity=(max(nv), max(nf))))
    assert [as_bytes(x) for x in got] == [ref_bytes(m) for m in meshes]
    c.close()


def loaded(spray, oracle, good, tube):
    """A context with an uploaded slot 0 and the good set's tubes in slot 1."""
    c = spray.RtContext(0)
    va, fa = rh.mesh("grid12", oracle)
    c.upload_domain(0, va, fa)
    c.block_stream_tubes_domains([1], [good], [tube])
    return c, (export_all(c, 0), export_all(c, 1))


def test_check_pass_finds_a_bad_element_in_every_trip(spray, oracle):
    """One NaN, +inf or -inf in each trip of the check pass's loops over a block
    of 33^3 points (seven trips over its vectors, three over its colour field)
    and over 6,000 seeds (two), and at each array's last element."""
    import torch
    s = bc.probe33()
    t = dict(radius=0.0625, nsides=4, color=None)
    good, gt = bs.case("rotation_fwd"), bs.tube_of(1)
    c, before = loaded(spray, oracle, good, gt)
    dev, gdev = on_device([s])[0], on_device([good])[0]
    ncalls = 0
    for key, word in bc.PROBE_KINDS:
        size = s["seeds"].size if key == "seeds" else s["blocks"][0][key].size
        pos = bc.probe_positions(size)
        assert {p // bc.TRIP for p in pos} == set(range((size + bc.TRIP - 1) // bc.TRIP))
        for j, p in enumerate(pos):
            bad = bc.probed(s, key, p, bc.PROBE_VALUES[j % 3])
            if key == "seeds":
                bdev = dict(dev, seeds=torch.from_numpy(bad["seeds"]).cuda())
            else:
                bdev = dict(dev, blocks=[dict(dev["blocks"][0], **{
                    key: torch.from_numpy(bad["blocks"][0][key]).cuda()})])
            raises(spray, lambda: c.block_stream_tubes([bdev], [t]), ERR_ARG, "set 0", word)
            if key != "cfield":   # the polylines do not read the colour field
                raises(spray, lambda: c.block_streamlines([bdev]), ERR_ARG, "set 0", word)
            if j % 3:
                continue
            # from host arrays; second in a call of two sets into the loaded slots
            raises(spray, lambda: c.block_stream_tubes([bad], [t]), ERR_ARG, "set 0", word)
            for slots in ((1, 0), (0, 1)):
                raises(spray, lambda: c.block_stream_tubes_domains(list(slots), [gdev, bdev], [gt, t]),
                       ERR_ARG, "set 1, slot %d" % slots[1], word)
            assert (export_all(c, 0), export_all(c, 1)) == before, (key, p)
            ncalls += 1
    assert ncalls == 3 + 2 + 1
    # the good set still goes through
    (lines,), (mesh,) = host_forms(spray, [s], [t])
    assert as_bytes(synced(c, c.block_streamlines([dev]))[0]) == ref_bytes(lines)
    assert as_bytes(synced(c, c.block_stream_tubes([dev], [t]))[0]) == ref_bytes(mesh)
    c.close()


def test_check_pass_reports_the_lowest_bad_block(spray, oracle):
    """Bad vectors in blocks {299}, {17, 299}, {299, 17, 250} of 300; a bad
    colour in block 3 with a bad vector in block 9; the bad set first, in the
    middle and last in a batch of good ones."""
    s = bc.row300()
    t = bs.tube_of(2)
    good, gt = bs.case("rotation_fwd"), bs.tube_of(1)
    c, before = loaded(spray, oracle, good, gt)
    (lines, glines), (mesh, gmesh) = host_forms(spray, [s, good], [t, gt])
    at = 0
    for (vec, col), lowest in zip(bc.ROW300_BAD, (299, 17, 17, 3)):
        bad = bc.row300_bad(vec, col)
        for bset in (bad, on_device([bad])[0]):
            for k, batch in enumerate(([bset, good, s], [good, bset, s], [good, s, bset])):
                tubes = [gt if x is good else t for x in batch]
                word = "set %d, block %d)" % (k, lowest)
                err = raises(spray, lambda: c.block_stream_tubes(batch, tubes), ERR_ARG, word,
                             "vector")
                # with both kinds in the set the block named is the lowest of either kind
                assert ("colour" in str(err)) == bool(col), str(err)
                # the polylines do not read the colour fields: their lowest bad block has a bad vector
                raises(spray, lambda: c.block_streamlines(batch), ERR_ARG,
                       "set %d, block %d)" % (k, min(vec)))
                if k == at % 3:
                    slots = [5, 6, 7]
                    slots[k] = at % 2            # the bad set aimed at a loaded slot
                    raises(spray, lambda: c.block_stream_tubes_domains(slots, batch, tubes), ERR_ARG,
                           "set %d, slot %d, block %d)" % (k, slots[k], lowest))
                    assert (export_all(c, 0), export_all(c, 1)) == before
            at += 1
    assert min(bc.ROW300_BAD[3][0]) == 9 and bc.ROW300_BAD[3][1] == (3,)
    # the good sets' outputs are produced by the good call that follows
    got = synced(c, c.block_streamlines([good, s]))
    assert [as_bytes(x) for x in got] == [ref_bytes(glines), ref_bytes(lines)]
    got = synced(c, c.block_stream_tubes(on_device([s, good]), [t, gt]))
    assert [as_bytes(x) for x in got] == [ref_bytes(mesh), ref_bytes(gmesh)]
    c.block_stream_tubes_domains([1, 0], [s, good], [t, gt])
    B = spray.RtContext(0)
    B.build_domains([1, 0], [mesh[0], gmesh[0]], [mesh[3], gmesh[3]],
                    [slot_colors(s, t, mesh[2]), slot_colors(good, gt, gmesh[2])],
                    [mesh[1], gmesh[1]])
    for k in (0, 1):
        assert export_all(c, k) == export_all(B, k)
    assert export_all(c, 0) != before[0]
    c.close()
    B.close()


SLOT_PICK = ("hb_03", "hb_07", "hb_18", "mid_gap_7_fwd", "mid_overlap_3_back", "split_stall",
             "split_sub_colour", "land_11_+0")


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, batch, restated):
    names, sets, tubes = batch
    lines, meshes = restated
    pick = [names.index(k) for k in SLOT_PICK]
    many = bc.many_blocks()
    extra = [many["row_4097_long"], many["stack64_reversed"], bc.gaps()["gaps_first_4"]]
    etubes = [bs.tube_of(4), bs.tube_of(5), extra[2]["tube"]]
    _, emeshes = host_forms(spray, extra, etubes)
    ss = [sets[k] for k in pick] + extra
    tt = [tubes[k] for k in pick] + etubes
    mm = [meshes[k] for k in pick] + emeshes
    n = len(ss)
    assert sum(len(m[3]) > 0 for m in mm) >= n - 2
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds, nf = c.block_stream_tubes_domains(list(range(n)), on_device(ss), tt, bounds=True)
    assert nf == [len(m[3]) for m in mm]
    cols = [slot_colors(s, t, m[2]) for s, t, m in zip(ss, tt, mm)]
    ref_bounds = B.build_domains(list(range(n)), [m[0] for m in mm], [m[3] for m in mm], cols,
                                 [m[1] for m in mm], bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), k
        assert c.slot_info(k) == B.slot_info(k), k
    assert bounds.tobytes() == ref_bounds.tobytes()
    c.close()
    B.close()

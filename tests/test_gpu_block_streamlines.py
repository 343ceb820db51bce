"""Streamlines across blocks on the GPU (spray_rt_block_streamlines,
spray_rt_block_stream_tubes, spray_rt_domains_block_stream_tubes).

References, each bit for bit: the host restatements
(spray_rt_block_streamlines_host, spray_rt_block_stream_tubes_host, themselves
held to numpy by test_block_streamlines_host.py) for the polylines, the block of
every point and the tube arrays, a build_domains of the restated arrays in a
second context for the slot images, the oracle's brute force for queries.
"""
import ctypes as C

import numpy as np
import pytest

import block_stream_helpers as bs
import build_helpers as bh
import refit_helpers as rh

pytestmark = pytest.mark.gpu

F32 = np.float32
ERR_ARG, ERR_LIMIT = -1, -5
WHAT = bh.WHAT + ("COLORS", "FACES")


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def batch():
    """(names, sets, tubes): every case of block_stream_helpers in one call."""
    names = sorted(bs.cases())
    return names, [bs.case(k) for k in names], [bs.tube_of(k) for k in range(len(names))]


@pytest.fixture(scope="module")
def restated(spray, batch):
    """Per set: (points, offsets, info, point blocks) and (verts, normals,
    colors, faces) of the host forms."""
    names, sets, tubes = batch
    lines, meshes = [], []
    for s, t in zip(sets, tubes):
        lines.append(spray.block_streamlines_host(*bs.host_args(s), **bs.host_kw(s)))
        meshes.append(spray.block_stream_tubes_host(*bs.host_args(s), t["radius"], t["nsides"],
                                                    color=t["color"], cmap=s.get("cmap"),
                                                    **bs.host_kw(s)))
    return lines, meshes


def on_device(sets):
    import torch
    put = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return [dict(s, seeds=put(s["seeds"]),
                 blocks=[dict(b, vectors=put(b["vectors"]), cfield=put(b.get("cfield")))
                         for b in s["blocks"]]) for s in sets]


def synced(c, x):
    c.sync()
    return x


def as_bytes(arrays):
    return tuple(None if x is None else x.cpu().numpy().tobytes() for x in arrays)


def ref_bytes(arrays):
    return tuple(None if x is None else x.tobytes() for x in arrays)


def export_all(c, slot, what=WHAT):
    return {w: c.slot_export(slot, getattr(c, "SLOT_" + w)).tobytes() for w in what}


def slot_colors(s, t, col):
    colored = s["blocks"][0].get("cfield") is not None
    return col if colored or t["color"] is not None else None


def test_batch_shapes(batch, restated):
    names, sets, tubes = batch
    lines, meshes = restated
    lanes = [len(s["seeds"]) * (2 if s["direction"] == bs.BOTH else 1) for s in sets]
    assert max(lanes) == 260 and 0 in lanes              # two workgroups; a set without seeds
    assert {len(s["blocks"]) for s in sets} >= {1, 2, 6, 8}
    assert sum(len(l[0]) for l in lines) > 5000
    crossings = sum(int((np.diff(l[3][a:b].astype(int)) != 0).sum())
                    for l in lines for a, b in zip(l[1][:-1], l[1][1:]))
    assert crossings > 500
    assert any(len(np.unique(m[2])) > 8 for m in meshes)


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_forms(spray, batch, restated, device):
    names, sets, tubes = batch
    lines, meshes = restated
    c = spray.RtContext(0)
    ss = on_device(sets) if device else sets
    for _ in range(2):   # twice on one context: the same bytes
        got = [as_bytes(x) for x in synced(c, c.block_streamlines(ss))]
        for k, ref in enumerate(lines):
            assert got[k] == ref_bytes(ref), names[k]
        tub = [as_bytes(x) for x in synced(c, c.block_stream_tubes(ss, tubes))]
        for k, ref in enumerate(meshes):
            assert tub[k] == ref_bytes(ref), names[k]
    # the same batch in reversed order, without normals: the same bytes per set
    rev = [as_bytes(x) for x in synced(c, c.block_streamlines(ss[::-1]))][::-1]
    assert rev == got
    rev = [as_bytes(x) for x in
           synced(c, c.block_stream_tubes(ss[::-1], tubes[::-1], normals=False))][::-1]
    for k in range(len(sets)):
        assert rev[k] == (tub[k][0], None, tub[k][2], tub[k][3]), names[k]
    c.close()


def test_a_batch_of_one_block_eight_blocks_and_no_seeds(spray, batch, restated):
    names, sets, tubes = batch
    lines, meshes = restated
    pick = [names.index(k) for k in ("one_block", "abc_both", "no_seeds")]
    assert [len(sets[k]["blocks"]) for k in pick] == [1, 8, 8] and len(sets[pick[2]]["seeds"]) == 0
    c = spray.RtContext(0)
    got = synced(c, c.block_streamlines(on_device([sets[k] for k in pick])))
    assert [as_bytes(x) for x in got] == [ref_bytes(lines[k]) for k in pick]
    got = synced(c, c.block_stream_tubes([sets[k] for k in pick], [tubes[k] for k in pick]))
    assert [as_bytes(x) for x in got] == [ref_bytes(meshes[k]) for k in pick]
    # the one block alone: the single-grid kernels' bytes (P1)
    f = bs.as_field(sets[pick[0]])
    one = synced(c, c.streamlines([f]))[0]
    assert as_bytes(one) == ref_bytes(lines[pick[0]][:3])
    t = tubes[pick[0]]
    assert as_bytes(synced(c, c.stream_tubes([f], [t]))[0]) == ref_bytes(meshes[pick[0]])
    c.close()


def test_counts_and_short_capacities(spray, batch, restated):
    names, sets, tubes = batch
    lines, meshes = restated
    c = spray.RtContext(0)
    ss = on_device(sets)
    assert c.block_streamlines(ss, count_only=True) == [len(l[0]) for l in lines]
    assert c.block_stream_tubes(ss, tubes, count_only=True) == \
        [(len(m[0]), len(m[3])) for m in meshes]
    pick = [names.index("rotation_both"), names.index("reversed")]
    sub, subt = [ss[k] for k in pick], [tubes[k] for k in pick]
    npts = [len(lines[k][0]) for k in pick]
    with pytest.raises(spray.SprayRtError) as e:
        c.block_streamlines(sub, capacity=max(npts) - 1)
    assert e.value.code == ERR_LIMIT and "set 0" in str(e.value) and e.value.counts == npts
    c.sync()
    for bufs in e.value.buffers:   # zeroed before the call: untouched
        assert all(int(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.block_streamlines(sub, capacity=max(npts)))   # the exact capacity fits
    assert [as_bytes(x) for x in got] == [ref_bytes(lines[k]) for k in pick]
    nv = [len(meshes[k][0]) for k in pick]
    nf = [len(meshes[k][3]) for k in pick]
    for cap in ((max(nv) - 1, max(nf)), (max(nv), max(nf) - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.block_stream_tubes(sub, subt, capacity=cap)
        assert e.value.code == ERR_LIMIT and e.value.counts == list(zip(nv, nf))
        c.sync()
        for bufs in e.value.buffers:
            assert all(int(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.block_stream_tubes(sub, subt, capacity=(max(nv), max(nf))))
    assert [as_bytes(x) for x in got] == [ref_bytes(meshes[k]) for k in pick]
    c.close()


def test_phase_times(spray, batch):
    names, sets, tubes = batch
    c = spray.RtContext(0)
    assert c.block_stream_phase_times() == [0.0, 0.0, 0.0]
    k = names.index("rotation_fwd")
    c.block_streamlines([sets[k]])
    t = c.block_stream_phase_times()
    assert t[0] > 0 and t[1] > 0 and t[2] == 0
    c.block_stream_tubes_domains([3], [sets[k]], [tubes[k]])
    t = c.block_stream_phase_times()
    assert min(t) > 0 and max(t) < 10000
    c.block_streamlines([sets[k]], count_only=True)
    t = c.block_stream_phase_times()
    assert t[0] > 0 and t[1] == 0 and t[2] == 0
    assert c.stream_phase_times() == [0.0, 0.0, 0.0]    # the single-grid calls' times are their own
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, batch, restated):
    names, sets, tubes = batch
    lines, meshes = restated
    n = len(sets)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds, nf = c.block_stream_tubes_domains(list(range(n)), on_device(sets), tubes, bounds=True)
    assert nf == [len(m[3]) for m in meshes]
    cols = [slot_colors(s, t, m[2]) for s, t, m in zip(sets, tubes, meshes)]
    ref_bounds = B.build_domains(list(range(n)), [m[0] for m in meshes], [m[3] for m in meshes],
                                 cols, [m[1] for m in meshes], bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), names[k]
        assert c.slot_info(k) == B.slot_info(k)
        assert c.slot_export(k, c.SLOT_FACES).tobytes() == meshes[k][3].tobytes()
        got = c.slot_export(k, c.SLOT_COLORS)
        assert got.tobytes() == (b"" if cols[k] is None else cols[k].tobytes()), names[k]
    assert bounds.tobytes() == ref_bounds.tobytes()
    # numpy sets, other slots, no normals
    a, b = names.index("refined"), names.index("hop3")
    c.block_stream_tubes_domains([40, 38], [sets[a], sets[b]], [tubes[a], tubes[b]], normals=False)
    B.build_domains([40, 38], [meshes[a][0], meshes[b][0]], [meshes[a][3], meshes[b][3]],
                    [cols[a], cols[b]])
    for k in (40, 38):
        assert export_all(c, k) == export_all(B, k), k
    c.close()
    B.close()


def test_slots_answer_queries(spray, oracle, batch):
    names, sets, tubes = batch
    a, b = names.index("abc_both"), names.index("rotation_fwd")
    assert sets[a]["blocks"][0].get("cfield") is not None
    c = spray.RtContext(0)
    va, fa = rh.mesh("grid12", oracle)
    c.upload_domain(1, va, fa)                         # replaced by the call below
    ta = dict(tubes[a], radius=0.0625)
    tb = dict(tubes[b], radius=0.03125, color=0x00334455)
    c.block_stream_tubes_domains([1, 4], on_device([sets[a], sets[b]]), [ta, tb])
    for slot, k, t, seed in ((1, a, ta, 71), (4, b, tb, 72)):
        s = sets[k]
        v, n, col, fc = spray.block_stream_tubes_host(*bs.host_args(s), t["radius"], t["nsides"],
                                                      color=t["color"], cmap=s.get("cmap"),
                                                      **bs.host_kw(s))
        assert c.slot_info(slot)["tris"] == len(fc) > 0
        bh.check_queries(spray, oracle, c, slot, v, fc, col, n, seed)
    c.close()


def raw_call(spray, c, s, patch):
    """spray_rt_block_streamlines through ctypes on records patch(set record,
    block records) may change -> the return code."""
    from spray_amd import engine
    from spray_amd._native import lib
    arr, _, _, keep = engine._block_tables([s])
    patch(arr[0], keep[0])
    n = (C.c_size_t * 1)()
    return lib().spray_rt_block_streamlines(c.h, 1, arr, None, None, None, None, None, n)


def test_failed_calls_change_nothing(spray, oracle, batch):
    names, sets, tubes = batch
    good, tube = sets[names.index("rotation_fwd")], tubes[names.index("rotation_fwd")]
    other = sets[names.index("abc_both")]                # eight blocks with colour fields
    plain = bs.cases()["abc_both"]
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.block_stream_tubes_domains([1], [good], [tube])
    before = (export_all(c, 0), export_all(c, 1))

    def with_block(s, k, **kw):
        blocks = list(s["blocks"])
        blocks[k] = dict(blocks[k], **kw)
        return dict(s, blocks=blocks)

    def fails(ss, slots=(0, 1), names_="set 1, slot", code=ERR_ARG, forms=True, also=""):
        with pytest.raises(spray.SprayRtError) as e:
            c.block_stream_tubes_domains(list(slots), ss, [tube] * len(ss))
        assert e.value.code == code and names_ in str(e.value) and also in str(e.value), str(e.value)
        assert "slot %d" % slots[1] in str(e.value)
        assert (export_all(c, 0), export_all(c, 1)) == before
        if forms:
            for call in (lambda: c.block_stream_tubes(ss, [tube] * len(ss)),
                         lambda: c.block_streamlines(ss)):
                with pytest.raises(spray.SprayRtError) as e:
                    call()
                assert e.value.code == code and "set 1" in str(e.value) and also in str(e.value)

    # a non-finite sample in the last block, a non-finite seed: found by the check pass
    vec = other["blocks"][7]["vectors"].copy()
    vec[4, 4, 4, 2] = np.nan
    seeds = other["seeds"].copy()
    seeds[11, 0] = np.inf
    for tgt in (0, 1):   # the bad set aimed at either loaded slot, second in the call
        fails([good, with_block(other, 7, vectors=vec)], (1 - tgt, tgt), also="block 7")
        fails(on_device([good, with_block(other, 7, vectors=vec)]), (1 - tgt, tgt), also="block 7")
        fails([good, dict(other, seeds=seeds)], (1 - tgt, tgt), also="seed")
    col = other["blocks"][7]["cfield"].copy()
    col[0, 0, 0] = -np.inf
    fails(on_device([good, with_block(other, 7, cfield=col)]), forms=False, also="colour")
    with pytest.raises(spray.SprayRtError) as e:
        c.block_stream_tubes([good, with_block(other, 7, cfield=col)], [tube] * 2)
    assert e.value.code == ERR_ARG and "set 1, block 7" in str(e.value)
    c.block_streamlines([good, with_block(other, 7, cfield=col)])   # nothing to the polylines
    # the argument errors of the blocks
    fails([good, dict(other, blocks=[])], also="nblocks")
    tiny = bs.hop_blocks(1)[0]
    fails([good, dict(plain, blocks=[tiny] * 65536)], also="nblocks")
    fails([good, with_block(other, 5, cfield=None)], also="block 5")
    fails([good, with_block(plain, 7, cfield=other["blocks"][7]["cfield"])], also="block 7")
    fails([good, dict(plain, cmap=other["cmap"])], forms=False, also="colour table")
    fails([good, dict(other, cmap=None)], forms=False, also="colour")
    fails([good, with_block(other, 7, spacing=(0.25, 0.0, 0.25))], also="block 7")
    fails([good, dict(other, step=0.0)])
    assert raw_call(spray, c, other, lambda rec, blocks: setattr(rec, "blocks", None)) == ERR_ARG
    assert raw_call(spray, c, other, lambda rec, blocks: setattr(blocks[7], "vectors", None)) == ERR_ARG
    from spray_amd._native import lib
    assert b"set 0, block 7" in lib().spray_rt_last_error(c.h)
    assert raw_call(spray, c, other, lambda rec, blocks: setattr(
        blocks[7], "dims", (C.c_int32 * 3)(2048, 1024, 1024))) == ERR_LIMIT
    fails([good, other], (0, -1), "set 1", forms=False)            # a bad slot
    fails([good, other], (1, 1), "set 1", forms=False, also="twice")   # a slot listed twice
    with pytest.raises(spray.SprayRtError) as e:
        c.block_stream_tubes_domains([0, 1], [good, other], [tube, dict(tube, nsides=17)])
    assert e.value.code == ERR_ARG and "set 1, slot 1" in str(e.value)
    assert (export_all(c, 0), export_all(c, 1)) == before
    # and the good call goes through
    B = spray.RtContext(0)
    c.block_stream_tubes_domains([0, 1], [good, other], [tube, tube])
    B.block_stream_tubes_domains([0, 1], on_device([good, other]), [tube, tube])
    for s in (0, 1):
        assert export_all(c, s) == export_all(B, s)
    assert export_all(c, 0) != before[0]
    c.close()
    B.close()

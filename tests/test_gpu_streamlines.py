"""Streamlines on the GPU (spray_rt_streamlines, spray_rt_stream_tubes,
spray_rt_domains_stream_tubes).

References, each bit for bit: the host restatements (spray_rt_streamlines_host,
spray_rt_stream_tubes_host, themselves held to numpy by
test_streamlines_host.py) for the polylines and the tube arrays, a
build_domains of the restated arrays in a second context for the slot images,
the oracle's brute force for queries.
"""
import numpy as np
import pytest

import build_helpers as bh
import refit_helpers as rh
import stream_helpers as sh

pytestmark = pytest.mark.gpu

F32 = np.float32
ERR_ARG, ERR_LIMIT = -1, -5
WHAT = bh.WHAT + ("COLORS", "FACES")
KEPT = tuple(w for w in WHAT if w != "COLORS")


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


def batch_fields():
    """(names, fields, tubes): the host test's small cases, then the block-scan
    boundaries, ragged waves, an empty field in the middle, seeds all outside."""
    small = sh.small_cases()
    names = sorted(small)
    fields = [sh.with_color(small[k], 20 + i) if i % 3 != 1 else small[k]
              for i, k in enumerate(names)]
    flow = sh.abc(9)
    for i, (n, d) in enumerate(((1, sh.BOTH), (255, sh.FORWARD), (256, sh.BACKWARD),
                                (257, sh.FORWARD), (600, sh.BOTH), (256, sh.BOTH))):
        names.append("seeds%d_%d" % (n, d))
        f = sh.field(flow, sh.random_seeds(n, (9, 9, 9), 40 + i), 0.0625, 12 + 3 * i, d)
        fields.append(sh.with_color(f, 50 + i) if i % 2 else f)
        if n == 1:
            names.append("noseeds")
            fields.append(sh.field(flow, np.zeros((0, 3), F32), 0.0625, 10, sh.BOTH))
    # a wave whose lines are ragged: a stagnant centre next to full-length orbits
    seeds = np.zeros((64, 3), F32)
    seeds[:] = 8.0
    seeds[1:, 0] += 0.5 + 6.5 * np.arange(63) / 63
    seeds[1::2, 2] = 3.0
    names.append("ragged")
    fields.append(sh.with_color(sh.field(sh.rotation(17), seeds, 0.05, 300, sh.BOTH), 7))
    names.append("outside")
    out = sh.random_seeds(70, (9, 9, 9), 3) + F32(8.5)
    fields.append(sh.field(flow, out, 0.0625, 10, sh.BOTH))
    tubes = [dict(radius=0.03125 * (1 + i % 4), nsides=3 + (5 * i) % 14,
                  color=None if i % 3 == 1 else 0x00102030 + i) for i in range(len(fields))]
    return names, fields, tubes


@pytest.fixture(scope="module")
def batch():
    return batch_fields()


@pytest.fixture(scope="module")
def restated(spray, batch):
    """Per field: (points, offsets, info) and (verts, normals, colors, faces) of
    the host forms."""
    names, fields, tubes = batch
    lines, meshes = [], []
    for f, t in zip(fields, tubes):
        lines.append(spray.streamlines_host(*sh.host_args(f), **sh.host_kw(f)))
        meshes.append(spray.stream_tubes_host(*sh.host_args(f), t["radius"], t["nsides"],
                                              color=t["color"], cfield=f.get("cfield"),
                                              cmap=f.get("cmap"), **sh.host_kw(f)))
    return lines, meshes


def on_device(fields):
    import torch
    out = []
    for f in fields:
        g = dict(f)
        for k in ("vectors", "seeds", "cfield"):
            if g.get(k) is not None:
                g[k] = torch.from_numpy(np.ascontiguousarray(g[k])).cuda()
        out.append(g)
    return out


def synced(c, x):
    c.sync()
    return x


def as_bytes(arrays):
    return tuple(None if x is None else x.cpu().numpy().tobytes() for x in arrays)


def ref_bytes(arrays):
    return tuple(None if x is None else x.tobytes() for x in arrays)


def export_all(c, slot, what=WHAT):
    return {w: c.slot_export(slot, getattr(c, "SLOT_" + w)).tobytes() for w in what}


def slot_colors(f, t, col):
    return col if f.get("cfield") is not None or t["color"] is not None else None


def test_batch_shapes(batch, restated):
    names, fields, tubes = batch
    lines, meshes = restated
    at = names.index
    lanes = [len(f["seeds"]) * (2 if f["direction"] == sh.BOTH else 1) for f in fields]
    assert {1 * 2, 255, 256, 257, 1200, 512} <= set(lanes) and 0 in lanes
    assert 0 < at("noseeds") < len(names) - 1 and len(lines[at("noseeds")][0]) == 0
    assert len(lines[at("outside")][0]) == 0 and len(fields[at("outside")]["seeds"]) == 70
    m = np.diff(lines[at("ragged")][1].astype(np.int64))
    assert m[0] == 1 and (m[1:] == 601).all()        # stagnant next to full-length lines
    assert sum(len(l[0]) for l in lines) > 60000
    assert {t["nsides"] for t in tubes} >= {3, 16}
    assert any(len(np.unique(mesh[2])) > 8 for mesh in meshes)


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_forms(spray, batch, restated, device):
    names, fields, tubes = batch
    lines, meshes = restated
    c = spray.RtContext(0)
    fs = on_device(fields) if device else fields
    for _ in range(2):   # twice on one context
        got = [as_bytes(x) for x in synced(c, c.streamlines(fs))]
        for k, ref in enumerate(lines):
            assert got[k] == ref_bytes(ref), names[k]
        tub = [as_bytes(x) for x in synced(c, c.stream_tubes(fs, tubes))]
        for k, ref in enumerate(meshes):
            assert tub[k] == ref_bytes(ref), names[k]
    # the same batch in reversed order, without normals: the same bytes per field
    rev = [as_bytes(x) for x in synced(c, c.streamlines(fs[::-1]))][::-1]
    assert rev == got
    rev = [as_bytes(x) for x in synced(c, c.stream_tubes(fs[::-1], tubes[::-1], normals=False))][::-1]
    for k in range(len(fields)):
        assert rev[k] == (tub[k][0], None, tub[k][2], tub[k][3]), names[k]
    c.close()


def test_counts_and_short_capacities(spray, batch, restated):
    names, fields, tubes = batch
    lines, meshes = restated
    c = spray.RtContext(0)
    fs = on_device(fields)
    assert c.streamlines(fs, count_only=True) == [len(l[0]) for l in lines]
    assert c.stream_tubes(fs, tubes, count_only=True) == [(len(m[0]), len(m[3])) for m in meshes]
    pick = [names.index("seeds600_2"), names.index("ragged")]
    sub, subt = [fs[k] for k in pick], [tubes[k] for k in pick]
    npts = [len(lines[k][0]) for k in pick]
    with pytest.raises(spray.SprayRtError) as e:
        c.streamlines(sub, capacity=max(npts) - 1)
    assert e.value.code == ERR_LIMIT and "field" in str(e.value) and e.value.counts == npts
    c.sync()
    for bufs in e.value.buffers:   # zeroed before the call: untouched
        assert all(int(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.streamlines(sub, capacity=max(npts)))   # the exact capacity fits
    assert [as_bytes(x) for x in got] == [ref_bytes(lines[k]) for k in pick]
    nv = [len(meshes[k][0]) for k in pick]
    nf = [len(meshes[k][3]) for k in pick]
    for cap in ((max(nv) - 1, max(nf)), (max(nv), max(nf) - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.stream_tubes(sub, subt, capacity=cap)
        assert e.value.code == ERR_LIMIT and e.value.counts == list(zip(nv, nf))
        c.sync()
        for bufs in e.value.buffers:
            assert all(int(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.stream_tubes(sub, subt, capacity=(max(nv), max(nf))))
    assert [as_bytes(x) for x in got] == [ref_bytes(meshes[k]) for k in pick]
    c.close()


def test_phase_times(spray, batch):
    names, fields, tubes = batch
    c = spray.RtContext(0)
    assert c.stream_phase_times() == [0.0, 0.0, 0.0]
    k = names.index("ragged")
    c.streamlines([fields[k]])
    t = c.stream_phase_times()
    assert t[0] > 0 and t[1] > 0 and t[2] == 0
    c.stream_tubes_domains([3], [fields[k]], [tubes[k]])
    t = c.stream_phase_times()
    assert min(t) > 0 and max(t) < 10000
    c.streamlines([fields[k]], count_only=True)
    t = c.stream_phase_times()
    assert t[0] > 0 and t[1] == 0 and t[2] == 0
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, batch, restated):
    names, fields, tubes = batch
    lines, meshes = restated
    n = len(fields)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds, nf = c.stream_tubes_domains(list(range(n)), on_device(fields), tubes, bounds=True)
    assert nf == [len(m[3]) for m in meshes]
    cols = [slot_colors(f, t, m[2]) for f, t, m in zip(fields, tubes, meshes)]
    ref_bounds = B.build_domains(list(range(n)), [m[0] for m in meshes], [m[3] for m in meshes],
                                 cols, [m[1] for m in meshes], bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), names[k]
        assert c.slot_info(k) == B.slot_info(k)
        assert c.slot_export(k, c.SLOT_FACES).tobytes() == meshes[k][3].tobytes()
        got = c.slot_export(k, c.SLOT_COLORS)
        assert got.tobytes() == (b"" if cols[k] is None else cols[k].tobytes()), names[k]
    assert bounds.tobytes() == ref_bounds.tobytes()
    # numpy fields, other slots, no normals
    a, b = names.index("ragged"), names.index("turn")
    c.stream_tubes_domains([40, 38], [fields[a], fields[b]], [tubes[a], tubes[b]], normals=False)
    B.build_domains([40, 38], [meshes[a][0], meshes[b][0]], [meshes[a][3], meshes[b][3]],
                    [cols[a], cols[b]])
    for k in (40, 38):
        assert export_all(c, k) == export_all(B, k), k
    c.close()
    B.close()


def test_slots_answer_queries_refit_and_recolor(spray, oracle, batch, restated):
    import torch
    names, fields, tubes = batch
    lines, meshes = restated
    a, b = names.index("seeds255_0"), names.index("seeds256_1")
    assert fields[a].get("cfield") is not None and fields[b].get("cfield") is None
    c = spray.RtContext(0)
    va, fa = rh.mesh("grid12", oracle)
    c.upload_domain(1, va, fa)                         # replaced by the call below
    ta = dict(tubes[a], radius=0.25)
    tb = dict(tubes[b], radius=0.125, color=0x00334455)
    c.stream_tubes_domains([1, 4], on_device([fields[a], fields[b]]), [ta, tb])
    for slot, k, t, seed in ((1, a, ta, 71), (4, b, tb, 72)):
        f = fields[k]
        v, n, col, fc = spray.stream_tubes_host(*sh.host_args(f), t["radius"], t["nsides"],
                                                color=t["color"], cfield=f.get("cfield"),
                                                cmap=f.get("cmap"), **sh.host_kw(f))
        assert c.slot_info(slot)["tris"] == len(fc)
        bh.check_queries(spray, oracle, c, slot, v, fc, col, n, seed)
    # a refit of the tube slot, then new colours for it
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, fc)
    c.refit_domains([4], [v1], [n1])
    bh.check_queries(spray, oracle, c, 4, v1, fc, col, n1, 73)
    new = rh.vertex_colors(len(v))
    before = export_all(c, 4, KEPT)
    c.recolor_domains([4], [torch.from_numpy(new.view(np.int32)).cuda()])
    assert c.slot_export(4, c.SLOT_COLORS).tobytes() == new.tobytes()
    assert export_all(c, 4, KEPT) == before
    bh.check_queries(spray, oracle, c, 4, v1, fc, new, n1, 74)
    c.close()


def test_failed_calls_change_nothing(spray, oracle, batch):
    names, fields, tubes = batch
    k = names.index("seeds257_0")
    good, tube = fields[k], tubes[k]
    other = sh.with_color(fields[names.index("seeds600_2")], 4)
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.stream_tubes_domains([1], [good], [tube])
    before = (export_all(c, 0), export_all(c, 1))

    def fails(fs, slots=(0, 1), names_="field 1, slot", code=ERR_ARG, forms=True):
        with pytest.raises(spray.SprayRtError) as e:
            c.stream_tubes_domains(list(slots), fs, [tube] * len(fs))
        assert e.value.code == code and names_ in str(e.value), str(e.value)
        assert "slot %d" % slots[1] in str(e.value)
        assert (export_all(c, 0), export_all(c, 1)) == before
        if forms:
            for call in (lambda: c.stream_tubes(fs, [tube] * len(fs)), lambda: c.streamlines(fs)):
                with pytest.raises(spray.SprayRtError) as e:
                    call()
                assert e.value.code == code and "field 1" in str(e.value)

    vec = other["vectors"].copy()
    vec[8, 8, 8, 2] = np.nan
    seeds = other["seeds"].copy()
    seeds[599, 0] = np.inf
    for tgt in (0, 1):   # the bad field aimed at either loaded slot, second in the call
        for bad in (dict(other, vectors=vec), dict(other, seeds=seeds)):
            fails([good, bad], (1 - tgt, tgt))
            fails(on_device([good, bad]), (1 - tgt, tgt))
    col = other["cfield"].copy()
    col[0, 0, 0] = -np.inf
    with pytest.raises(spray.SprayRtError) as e:
        c.stream_tubes_domains([0, 1], on_device([good, dict(other, cfield=col)]), [tube] * 2)
    assert e.value.code == ERR_ARG and "field 1, slot 1" in str(e.value)
    assert "colour" in str(e.value)
    assert (export_all(c, 0), export_all(c, 1)) == before
    fails([good, other], (0, -1), "field 1", forms=False)            # a bad slot
    fails([good, other], (1, 1), "field 1", forms=False)             # a slot listed twice
    fails([good, dict(other, step=0.0)], (0, 1))
    with pytest.raises(spray.SprayRtError) as e:
        c.stream_tubes_domains([0, 1], [good, other], [tube, dict(tube, nsides=17)])
    assert e.value.code == ERR_ARG and "field 1, slot 1" in str(e.value)
    assert (export_all(c, 0), export_all(c, 1)) == before
    # and the good call goes through
    B = spray.RtContext(0)
    c.stream_tubes_domains([0, 1], [good, other], [tube, tube])
    B.stream_tubes_domains([0, 1], on_device([good, other]), [tube, tube])
    for s in (0, 1):
        assert export_all(c, s) == export_all(B, s)
    assert export_all(c, 0) != before[0]
    c.close()
    B.close()

"""The streamline kernels at their scale limits and on the hard fields of
stream_cases.py (spray_rt_streamlines, spray_rt_stream_tubes,
spray_rt_domains_stream_tubes).

References, each bit for bit and none a second GPU run: the host forms
(held to numpy on the same inputs by test_stream_cases.py) and the closed forms
of the two long fields; a build_domains of the restated arrays in a second
context for the slot images; the oracle's brute force for queries.

What the inputs execute that test_gpu_streamlines.py does not: the scan's chunk
loop twice and three times (257 and 513 blocks), a block sum of exactly 2^24 in
both 25-bit fields of the packed scan word, a lane count of 65,536 and nback of
65,535, a second and a later trip of each loop of the check pass, empty runs
longer than a block in the expansion's search, and the arithmetic classes where
a GPU differs from a CPU (subnormals, signed zeros, ties, the frame threshold).
"""
import collections

import numpy as np
import pytest

import build_helpers as bh
import refit_helpers as rh
import stream_cases as sc
import stream_helpers as sh
from test_gpu_streamlines import (ERR_ARG, ERR_LIMIT, as_bytes, export_all, on_device, ref_bytes,
                                  slot_colors, synced)

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


def small_fields():
    """(names, fields, tubes) of the arithmetic classes and the gap fields;
    two in three of the fields without a colour field get one."""
    cases = dict(sc.arithmetic(), **sc.gaps())
    names = sorted(cases)
    fields = [cases[k] if cases[k].get("cfield") is not None or i % 3 == 1
              else sh.with_color(cases[k], 60 + i) for i, k in enumerate(names)]
    return names, fields, [sc.tube_of(f, i) for i, f in enumerate(fields)]


def batch_fields():
    """The small fields, then the chunk fields with a field of one seed between
    them: 256 blocks, 1, 513, 257."""
    names, fields, tubes = small_fields()
    ch = sc.chunks()
    one = sh.field(sc.chunk_flow(), [[4.0, 4.5, 3.25]], 0.0625, 7, sh.BOTH)
    for k, f in (("chunks256", ch["chunks256"]), ("oneseed", one), ("chunks513", ch["chunks513"]),
                 ("chunks257", ch["chunks257"])):
        names.append(k)
        fields.append(f)
        tubes.append(sc.tube_of(f, len(names)))
    return names, fields, tubes


def host_forms(spray, fields, tubes):
    lines, meshes = [], []
    for f, t in zip(fields, tubes):
        lines.append(spray.streamlines_host(*sh.host_args(f), **sh.host_kw(f)))
        meshes.append(spray.stream_tubes_host(*sh.host_args(f), t["radius"], t["nsides"],
                                              color=t["color"], cfield=f.get("cfield"),
                                              cmap=f.get("cmap"), **sh.host_kw(f)))
    return lines, meshes


@pytest.fixture(scope="module")
def batch():
    return batch_fields()


@pytest.fixture(scope="module")
def restated(spray, batch):
    names, fields, tubes = batch
    return host_forms(spray, fields, tubes)


def test_batch_shapes(batch, restated):
    names, fields, tubes = batch
    lines, meshes = restated
    blocks = [sc.nblocks(f) for f in fields]
    at = names.index("oneseed")
    assert blocks[at - 1:at + 3] == [256, 1, 513, 257]
    assert sc.nlanes(fields[at - 1]) == 65536 and fields[at + 2]["direction"] == sh.BOTH
    npts, ntris = sum(len(l[0]) for l in lines), sum(len(m[3]) for m in meshes)
    print("fields %d, points %d, triangles %d" % (len(fields), npts, ntris))
    assert len(fields) == 101 and npts > 750000 and ntris > 4000000
    assert {t["nsides"] for t in tubes} == set(range(3, 17))
    # the expansion's search meets lines without a tube on either side of a block boundary
    k = names.index("gaps_base_3")
    m = np.diff(lines[k][1].astype(np.int64))
    assert (m[:300] == 0).all() and (m[-300:] == 0).all() and (m >= 2).sum() == 6
    # the paths of the rule the arithmetic classes are there for, from the numpy side
    st = collections.Counter()
    for f in sc.arithmetic().values():
        sh.lines_numpy(f, stats=st)
    for key in ("grid_q2", "grid_q3", "grid_q4", "grid_pn", "repick", "carried", "axis_tie",
                "axis_0", "axis_1", "axis_2", "no_motion", "speed_low", "speed_overflow",
                "seed_outside", "upper_face", "empty_back", "empty_fwd"):
        assert st[key] > 0, key


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
    # the count-only forms
    assert c.streamlines(fs, count_only=True) == [len(l[0]) for l in lines]
    assert c.stream_tubes(fs, tubes, count_only=True) == [(len(m[0]), len(m[3])) for m in meshes]
    c.close()


def test_fullblock_equals_its_closed_form(spray):
    """257 forward lanes of 65,535 steps: block 0 sums to exactly 2^24 points
    and 2^24 tube points, lane 256 starts at 2^24."""
    import torch
    f = sc.fullblock()["fullblock"]
    t = f["tube"]
    total = 257 * 65536
    assert sc.nlanes(f) == 257 and sc.LANES * (f["max_steps"] + 1) == 1 << 24
    c = spray.RtContext(0)
    fs = on_device([f])
    assert c.streamlines(fs, count_only=True) == [total]
    ns = t["nsides"]
    assert c.stream_tubes(fs, [t], count_only=True) == [(total * ns + 2 * 257, 2 * ns * total)]
    # a capacity one short: the counts, nothing written
    with pytest.raises(spray.SprayRtError) as e:
        c.streamlines(fs, capacity=total - 1)
    assert e.value.code == ERR_LIMIT and e.value.counts == [total]
    c.sync()
    for bufs in e.value.buffers:
        assert all(int(b.abs().max()) == 0 for b in bufs)
    del e
    # the exact capacity fits; compared on the device
    (p, off, info), = synced(c, c.streamlines(fs, capacity=total))
    assert tuple(p.shape) == (total, 3)
    seeds = fs[0]["seeds"]
    want = torch.empty((257, 65536, 3), dtype=torch.float32, device=p.device)
    want[:, :, 0] = torch.arange(65536, dtype=torch.float32, device=p.device)
    want[:, :, 1:] = seeds[:, None, 1:]
    assert torch.equal(p.view(torch.int32), want.view(total, 3).view(torch.int32))
    assert off.cpu().numpy().view(np.uint32).tolist() == [65536 * l for l in range(258)]
    assert off.cpu().numpy().view(np.uint32)[256] == 1 << 24
    assert info.cpu().numpy().tolist() == [[0, sh.STEPS | sh.STEPS << 8]] * 257
    c.close()


def test_longest_line_equals_the_host_form(spray):
    """One line of 131,071 points with nback = 65535, then one of two points:
    2,097,172 vertices and 4,194,336 faces at 16 sides."""
    f = sc.longest()["longest"]
    t = f["tube"]
    (lines,), (mesh,) = host_forms(spray, [f], [t])
    assert lines[1].tolist() == [0, 131071, 131073] and lines[2][0, 0] == 65535
    assert len(mesh[0]) == 2097138 + 2 * 16 + 2 and len(mesh[3]) == 4194272 + 2 * 16 * 2
    c = spray.RtContext(0)
    fs = on_device([f])
    got, = synced(c, c.streamlines(fs))
    assert as_bytes(got) == ref_bytes(lines)
    got, = synced(c, c.stream_tubes(fs, [t]))
    assert as_bytes(got) == ref_bytes(mesh)
    c.close()


def test_check_pass_finds_one_bad_element_anywhere(spray, oracle):
    """One NaN, +inf or -inf at the first element, on either side of the first
    trip of the check pass, in a later trip and at the last element of the
    vectors, the seeds and the colour field."""
    import torch
    f = sc.probe()
    t = f["tube"]
    good = sh.field(sh.abc(5), sh.random_seeds(9, (5, 5, 5), 3), 0.125, 6, sh.BOTH)
    gt = dict(radius=0.0625, nsides=5, color=0x00506070)
    c = spray.RtContext(0)
    va, fa = rh.mesh("grid12", oracle)
    c.upload_domain(0, va, fa)
    c.stream_tubes_domains([1], [good], [gt])
    before = (export_all(c, 0), export_all(c, 1))
    dev, gdev = on_device([f])[0], on_device([good])[0]

    def raises(call, *words):
        with pytest.raises(spray.SprayRtError) as e:
            call()
        assert e.value.code == ERR_ARG, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    ncalls = 0
    for key, kind in sc.PROBE_KINDS:
        # a position in every trip of the loop: 64 blocks x 256 threads cover 16,384 elements
        trips = (f[key].size + sc.TRIP - 1) // sc.TRIP
        assert trips >= 2 and {p // sc.TRIP for p in sc.probe_positions(f[key].size)} == set(range(trips))
        for j, pos in enumerate(sc.probe_positions(f[key].size)):
            for i, value in enumerate(sc.PROBE_VALUES):
                bad = sc.probed(f, key, pos, value)
                bdev = dict(dev, **{key: torch.from_numpy(bad[key]).cuda()})
                raises(lambda: c.stream_tubes([bdev], [t]), "field 0", kind)
                if key != "cfield":   # the polylines do not read the colour field
                    raises(lambda: c.streamlines([bdev]), "field 0", kind)
                if (i + j) % 3:
                    continue
                # numpy arrays; then second in a call of two fields into loaded slots
                raises(lambda: c.stream_tubes([bad], [t]), "field 0", kind)
                for slots in ((1, 0), (0, 1)):
                    raises(lambda: c.stream_tubes_domains(list(slots), [gdev, bdev], [gt, t]),
                           "field 1, slot %d" % slots[1], kind)
                    raises(lambda: c.stream_tubes_domains(list(slots), [good, bad], [gt, t]),
                           "field 1, slot %d" % slots[1], kind)
                assert (export_all(c, 0), export_all(c, 1)) == before, (key, pos)
                ncalls += 1
    assert ncalls == 15
    # the control: values of FLT_MAX's scale and subnormals at the same places
    g = sc.probe_control(f)
    (lines,), (mesh,) = host_forms(spray, [g], [t])
    for fs in (on_device([g]), [g]):
        got, = synced(c, c.streamlines(fs))
        assert as_bytes(got) == ref_bytes(lines)
        got, = synced(c, c.stream_tubes(fs, [t]))
        assert as_bytes(got) == ref_bytes(mesh)
    assert len(lines[0]) > 6000 and len(mesh[3]) > 10000
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, oracle):
    names, fields, tubes = small_fields()
    lines, meshes = host_forms(spray, fields, tubes)
    n = len(fields)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds, nf = c.stream_tubes_domains(list(range(n)), on_device(fields), tubes, bounds=True)
    assert nf == [len(m[3]) for m in meshes]
    cols = [slot_colors(f, t, m[2]) for f, t, m in zip(fields, tubes, meshes)]
    ref_bounds = B.build_domains(list(range(n)), [m[0] for m in meshes], [m[3] for m in meshes],
                                 cols, [m[1] for m in meshes], bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), names[k]
        assert c.slot_info(k) == B.slot_info(k), names[k]
    assert bounds.tobytes() == ref_bounds.tobytes()
    # rays against the oracle's brute force on two slots with tubes of ordinary size
    for name, seed in (("sub_colour", 81), ("fast_rotation", 82)):
        k = names.index(name)
        v, nr, col, fc = meshes[k]
        assert len(fc) > 500 and cols[k] is not None
        bh.check_queries(spray, oracle, c, k, v, fc, cols[k], nr, seed)
    c.close()
    B.close()

"""Glyphs on the GPU (spray_rt_glyphs, spray_rt_domains_glyphs).

References, each bit for bit: the host restatement (spray_rt_glyphs_host,
itself held to numpy by test_glyphs_host.py) for the five arrays, a
build_domains of the restated arrays in a second context for the slot images,
the oracle's brute force for queries.
"""
import numpy as np
import pytest

import build_helpers as bh
import glyph_helpers as gh
import refit_helpers as rh

pytestmark = pytest.mark.gpu

F32 = np.float32
ERR_ARG, ERR_LIMIT = -1, -5
WHAT = bh.WHAT + ("COLORS", "FACES")
KEPT = tuple(w for w in WHAT if w != "COLORS")
ARRAYS = ("points", "vectors", "scales", "select", "cfield")


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


def batch_sets():
    """(names, sets, glyphs): the host test's small cases, then the block-scan
    boundaries, an empty set in the middle, a set with every point dropped,
    kept points in runs with long dropped runs across block boundaries, and one,
    two and three chunks of the scan."""
    small = gh.small_cases()
    names = sorted(small)
    sets = [gh.with_color(small[k][0], 20 + i) if i % 3 != 1 else small[k][0]
            for i, k in enumerate(names)]
    glyphs = [dict(small[k][1], color=None if i % 3 == 2 else 0x00102030 + i)
              for i, k in enumerate(names)]
    for i, n in enumerate((1, 255, 256, 257, 600)):
        p = gh.cloud(n, 40 + i, 8.0)
        arrows = i % 2 == 1
        S = gh.pset(p, vectors=gh.swirl(p, i), scales=np.linspace(0.5, 2.0, n), stride=1 + i % 2)
        names.append("points%d" % n)
        sets.append(gh.with_color(S, 50 + i) if i % 2 else S)
        glyphs.append(gh.arrow(0.4, 3 + 3 * i, i == 3, color=0x00405060) if arrows
                      else gh.sphere(0.2, i // 2, 0x00405060 + i))
        if n == 1:
            names.append("empty_mid")
            sets.append(gh.pset(np.zeros((0, 3))))
            glyphs.append(gh.sphere(0.5, 1))
    names.append("none_kept")
    sets.append(gh.pset(gh.cloud(700, 7), scales=np.zeros(700)))
    glyphs.append(gh.sphere(0.5, 1))
    runs = dict(first=[(0, 1)], last=[(1499, 1500)], both_ends=[(0, 1), (1499, 1500)],
                runs=[(300, 420), (800, 1100)], runs_arrows=[(290, 300), (700, 1030)])
    for i, (k, r) in enumerate(sorted(runs.items())):
        S, G = gh.runs_case(1500, r, 60 + i, arrows=k.endswith("arrows") or k == "last")
        names.append(k)
        sets.append(gh.with_color(S, 70 + i) if i % 2 else S)
        glyphs.append(dict(G, color=0x00112233))
    for k, (n, prime, stride) in (("chunks2", (65537, 251, 1)), ("chunks3", (131073, 257, 2))):
        S, G = gh.tiled_case(n, prime, 80, stride)
        names.append(k)
        sets.append(S)
        glyphs.append(G)
    return names, sets, glyphs


@pytest.fixture(scope="module")
def batch():
    return batch_sets()


@pytest.fixture(scope="module")
def restated(spray, batch):
    """Per set: (verts, normals, colors, faces, point_ids) of the host form."""
    names, sets, glyphs = batch
    return [spray.glyphs_host(S, G) for S, G in zip(sets, glyphs)]


def on_device(sets):
    import torch
    out = []
    for S in sets:
        T = dict(S)
        for k in ARRAYS:
            if T.get(k) is not None:
                T[k] = torch.from_numpy(np.ascontiguousarray(T[k])).cuda()
        out.append(T)
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


def slot_colors(S, G, col):
    return col if S.get("cfield") is not None or G["color"] is not None else None


def test_batch_shapes(spray, batch, restated):
    names, sets, glyphs = batch
    at = names.index
    npts = [len(S["points"]) for S in sets]
    assert {1, 255, 256, 257, 600, 65537, 131073} <= set(npts)
    assert 0 < at("empty_mid") < len(names) - 1 and npts[at("empty_mid")] == 0
    assert npts[at("none_kept")] == 700 and len(restated[at("none_kept")][4]) == 0
    assert list(restated[at("first")][4]) == [0] and list(restated[at("last")][4]) == [1499]
    assert list(restated[at("both_ends")][4]) == [0, 1499]
    ids = restated[at("runs")][4].astype(np.int64)
    gaps = np.diff(np.concatenate([[-1], ids, [1500]])) - 1     # dropped runs
    assert (gaps > 256).sum() == 3 and gaps[0] > 256 and gaps[-1] > 256
    assert glyphs[at("last")]["shape"] == gh.ARROW and glyphs[at("first")]["shape"] == gh.SPHERE
    # one, two and three chunks of glyph_scan (256 blocks of 256 points a chunk)
    blocks = lambda n: -(-n // 256)
    assert blocks(npts[at("chunks2")]) == 257 and blocks(npts[at("chunks3")]) == 513
    assert max(blocks(n) for n in npts[:at("chunks2")]) <= 256
    for k in ("chunks2", "chunks3"):   # the tiled sets against the tiled numpy restatement
        S, G = sets[at(k)], glyphs[at(k)]
        assert len(np.unique(S["points"], axis=0)) in (251, 257)
        assert ref_bytes(restated[at(k)]) == ref_bytes(gh.glyphs_numpy(S, G, spray))
        assert len(restated[at(k)][4]) == 65537
    assert {G["shape"] for G in glyphs} == {gh.SPHERE, gh.ARROW}
    assert any(len(np.unique(m[2])) > 8 for m in restated)


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_form(spray, batch, restated, device):
    names, sets, glyphs = batch
    c = spray.RtContext(0)
    ss = on_device(sets) if device else sets
    for _ in range(2):   # twice on one context
        got = [as_bytes(x) for x in synced(c, c.glyphs(ss, glyphs))]
        for k, ref in enumerate(restated):
            assert got[k] == ref_bytes(ref), names[k]
    # the same batch in reversed order, without normals: the same bytes per set
    rev = [as_bytes(x) for x in synced(c, c.glyphs(ss[::-1], glyphs[::-1], normals=False))][::-1]
    for k in range(len(sets)):
        assert rev[k] == (got[k][0], None) + got[k][2:], names[k]
    c.close()


def test_counts_and_short_capacities(spray, batch, restated):
    names, sets, glyphs = batch
    c = spray.RtContext(0)
    ss = on_device(sets)
    assert c.glyphs(ss, glyphs, count_only=True) == [(len(m[0]), len(m[3])) for m in restated]
    pick = [names.index("points600"), names.index("runs_arrows")]
    sub, subg = [ss[k] for k in pick], [glyphs[k] for k in pick]
    nv = [len(restated[k][0]) for k in pick]
    nf = [len(restated[k][3]) for k in pick]
    assert min(nv) > 0
    for cap in ((max(nv) - 1, max(nf)), (max(nv), max(nf) - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.glyphs(sub, subg, capacity=cap)
        assert e.value.code == ERR_LIMIT and "set" in str(e.value)
        assert e.value.counts == list(zip(nv, nf))
        c.sync()
        for bufs in e.value.buffers:   # zeroed before the call: untouched
            assert all(int(b.abs().max()) == 0 for b in bufs)
    got = synced(c, c.glyphs(sub, subg, capacity=(max(nv), max(nf))))   # the exact capacity fits
    assert [as_bytes(x) for x in got] == [ref_bytes(restated[k]) for k in pick]
    # single arrays
    only = synced(c, c.glyphs(sub, subg, arrays=("point_ids",)))
    assert [as_bytes(x) for x in only] == [(None,) * 4 + (restated[k][4].tobytes(),) for k in pick]
    only = synced(c, c.glyphs(sub, subg, arrays=("faces",)))
    assert [as_bytes(x)[3] for x in only] == [restated[k][3].tobytes() for k in pick]
    c.close()


def test_phase_times(spray, batch):
    names, sets, glyphs = batch
    c = spray.RtContext(0)
    assert c.glyph_phase_times() == [0.0, 0.0, 0.0]
    k = names.index("points600")
    c.glyphs([sets[k]], [glyphs[k]])
    t = c.glyph_phase_times()
    assert all(np.isfinite(t)) and t[0] > 0 and t[1] > 0 and t[2] == 0
    c.glyphs_domains([3], [sets[k]], [glyphs[k]])
    t = c.glyph_phase_times()
    assert all(np.isfinite(t)) and min(t) > 0 and max(t) < 10000
    c.glyphs([sets[k]], [glyphs[k]], count_only=True)
    t = c.glyph_phase_times()
    assert t[0] > 0 and t[1] == 0 and t[2] == 0
    c.close()


def buildable(names):
    """The sets whose meshes have an extent: a glyph of subnormal size is a
    point, which the byte comparisons above cover."""
    skip = ("scales", "scales_arrow", "speeds_0", "speeds_1", "length_range", "chunks2", "chunks3")
    return [k for k, name in enumerate(names) if name not in skip]


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, batch, restated):
    names, sets, glyphs = batch
    pick = buildable(names)
    n = len(pick)
    ss, gs, ms = [sets[k] for k in pick], [glyphs[k] for k in pick], [restated[k] for k in pick]
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds, nf = c.glyphs_domains(list(range(n)), on_device(ss), gs, bounds=True)
    assert nf == [len(m[3]) for m in ms]
    cols = [slot_colors(S, G, m[2]) for S, G, m in zip(ss, gs, ms)]
    ref_bounds = B.build_domains(list(range(n)), [m[0] for m in ms], [m[3] for m in ms], cols,
                                 [m[1] for m in ms], bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), names[pick[k]]
        assert c.slot_info(k) == B.slot_info(k)
        assert c.slot_export(k, c.SLOT_FACES).tobytes() == ms[k][3].tobytes()
        got = c.slot_export(k, c.SLOT_COLORS)
        assert got.tobytes() == (b"" if cols[k] is None else cols[k].tobytes()), names[pick[k]]
    assert bounds.tobytes() == ref_bounds.tobytes()
    # numpy sets, other slots, no normals; a set that keeps nothing gives an empty slot
    a, b, e = (pick.index(names.index(x)) for x in ("runs_arrows", "level2", "none_kept"))
    c.glyphs_domains([40, 38, 39], [ss[a], ss[b], ss[e]], [gs[a], gs[b], gs[e]], normals=False)
    B.build_domains([40, 38, 39], [ms[a][0], ms[b][0], ms[e][0]], [ms[a][3], ms[b][3], ms[e][3]],
                    [cols[a], cols[b], cols[e]])
    for k in (40, 38, 39):
        assert export_all(c, k) == export_all(B, k), k
    assert c.slot_info(39)["tris"] == 0
    c.close()
    B.close()


def test_slots_answer_queries_move_and_recolor(spray, oracle, batch, restated):
    """About 3,000 rays per slot against the oracle's brute force on a sphere
    slot and an arrow slot; the moving-particle recipe (verts and normals
    alone, then a refit) and the recolour recipe (colors alone, then a
    recolour); the replacement of an uploaded slot."""
    import torch
    names, sets, glyphs = batch
    a, b = names.index("points257"), names.index("points256")
    assert glyphs[a]["shape"] == gh.ARROW and glyphs[b]["shape"] == gh.SPHERE
    assert sets[a].get("cfield") is not None
    c = spray.RtContext(0)
    va, fa = rh.mesh("grid12", oracle)
    c.upload_domain(1, va, fa)                         # replaced by the call below
    Sa, Sb = sets[a], gh.with_color(sets[b], 5)
    Ga, Gb = glyphs[a], glyphs[b]
    c.glyphs_domains([1, 4], on_device([Sa, Sb]), [Ga, Gb])
    for slot, S, G, seed in ((1, Sa, Ga, 71), (4, Sb, Gb, 72)):
        v, n, col, fc, ids = spray.glyphs_host(S, G)
        assert c.slot_info(slot)["tris"] == len(fc)
        bh.check_queries(spray, oracle, c, slot, v, fc, col, n, seed)
    # the particles move, the kept set does not: verts and normals alone, a refit
    for slot, S, G, seed in ((1, Sa, Ga, 73), (4, Sb, Gb, 74)):
        rng = np.random.default_rng(seed)
        moved = dict(S, points=(S["points"] + rng.normal(size=S["points"].shape) * 0.3).astype(F32))
        if S.get("vectors") is not None:   # the directions turn, the speeds stay usable
            moved["vectors"] = (S["vectors"][:, [1, 2, 0]] * F32(1.25)).astype(F32)
        v1, n1, col, fc, ids = spray.glyphs_host(moved, G)
        assert np.array_equal(ids, spray.glyphs_host(S, G)[4])
        (gv, gn, gc, gf, gi), = c.glyphs(on_device([moved]), [G], arrays=("verts", "normals"))
        assert gc is None and gf is None and gi is None
        c.sync()
        assert gv.cpu().numpy().tobytes() == v1.tobytes() and gn.cpu().numpy().tobytes() == n1.tobytes()
        c.refit_domains([slot], [gv], [gn])
        bh.check_queries(spray, oracle, c, slot, v1, fc, col, n1, seed + 10)
        # what section 10 promises of a refit against a fresh extraction: the
        # arrays in vertex order and every query (both equal the oracle's)
        c.glyphs_domains([9], on_device([moved]), [G])
        for w in ("NORMALS", "COLORS", "FACES"):
            assert export_all(c, slot, (w,)) == export_all(c, 9, (w,)), w
        assert c.slot_info(slot)["tris"] == c.slot_info(9)["tris"]
        bh.check_queries(spray, oracle, c, 9, v1, fc, col, n1, seed + 10)
        # another colour field: colors alone, a recolour
        other = gh.with_color(moved, seed + 20, ntable=11)
        new = spray.glyphs_host(other, G)[2]
        assert new.tobytes() != col.tobytes()
        before = export_all(c, slot, KEPT)
        (_, _, gc, _, _), = c.glyphs(on_device([other]), [G], arrays=("colors",))
        c.recolor_domains([slot], [gc])
        assert c.slot_export(slot, c.SLOT_COLORS).tobytes() == new.tobytes()
        assert export_all(c, slot, KEPT) == before
        bh.check_queries(spray, oracle, c, slot, v1, fc, new, n1, seed + 30)
    c.close()


# ---- the check pass ----

PROBE = 16500


def check_trip(npoints):
    """Elements one trip of the check pass covers: a block of 256 threads per
    1,024 coordinates of the call's largest set, 2,048 blocks at most."""
    blocks = -(-npoints // 256)
    return 256 * min(max((3 * blocks + 3) // 4, 1), 2048)


def probe_set():
    """A set whose arrays take more than one trip of the check pass (49 blocks
    of 256 threads for 16,500 points: 12,544 elements a trip, so four trips
    over the coordinates and two over the per-point arrays) with all five
    arrays in use."""
    n = PROBE
    p = gh.cloud(n, 90, 32.0)
    S = gh.pset(p, vectors=gh.swirl(p, 1), scales=np.linspace(0.5, 1.0, n),
                select=np.linspace(0.0, 1.0, n), select_range=(0.25, 0.75), stride=3)
    return gh.with_color(S, 91)


KIND = dict(points="point", vectors="vector", scales="scale", select="select", cfield="colour")


def spots(size):
    """Element 0, a block boundary, the check pass's trip boundary, the last."""
    trip = check_trip(PROBE)
    return (0, 255, 256, trip - 1, trip, size - 1)


def bad_elements():
    """(shape, array, flat index, value): one bad element per call; every bad
    value at element 0, at a block boundary, at the check pass's trip boundary
    and at the last element of each array in use."""
    out = []
    for shape, arrays in ((gh.SPHERE, ("points", "scales", "select", "cfield")),
                          (gh.ARROW, ("points", "vectors", "scales", "select", "cfield"))):
        for key in arrays:
            size = PROBE * (3 if key in ("points", "vectors") else 1)
            values = [np.nan, np.inf, -np.inf] + ([-1.0] if key == "scales" else [])
            out += [(shape, key, at, x) for at in spots(size) for x in values]
    return out


def test_check_pass_errors(spray, oracle):
    S = probe_set()
    G = {gh.SPHERE: gh.sphere(0.25, 0, 0x00334455), gh.ARROW: gh.arrow(0.5, 4, color=0x00334455)}
    good_S, good_G = gh.pset(gh.cloud(300, 3)), gh.sphere(0.5, 1, 0x00556677)
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.glyphs_domains([1], [good_S], [good_G])
    before = (export_all(c, 0), export_all(c, 1))
    cases = bad_elements()
    assert check_trip(PROBE) == 12544 and len(cases) == 174
    for i, (shape, key, at, x) in enumerate(cases):
        T = dict(S)
        T[key] = S[key].copy()
        T[key].reshape(-1)[at] = x
        kind = "negative scale" if x == -1.0 else KIND[key]
        forms = [on_device([T])] + ([[T]] if i % 3 == 0 else [])
        for ts in forms:
            with pytest.raises(spray.SprayRtError) as e:
                c.glyphs(ts, [G[shape]])
            assert e.value.code == ERR_ARG and "set 0" in str(e.value) and kind in str(e.value), \
                (shape, key, at, x, str(e.value))
        with pytest.raises(spray.SprayRtError):
            spray.glyphs_host(T, G[shape])
        if i % 3 == 0:   # second in a two-set domains call, aimed at either loaded slot
            tgt = (i // 3) % 2
            with pytest.raises(spray.SprayRtError) as e:
                c.glyphs_domains([1 - tgt, tgt], on_device([good_S, T]), [good_G, G[shape]])
            assert e.value.code == ERR_ARG and "set 1, slot %d" % tgt in str(e.value)
            assert kind in str(e.value)
            assert (export_all(c, 0), export_all(c, 1)) == before
    # the control: FLT_MAX-scale values and subnormals at the same elements
    T = {k: (None if S[k] is None else np.array(S[k])) for k in ARRAYS}
    T = dict(S, **T)
    for key in ARRAYS:
        flat = T[key].reshape(-1)
        for j, at in enumerate(spots(flat.size)):
            flat[at] = (3e38, 1e-45, -1e-45, -3e38)[j % 4] if key != "scales" else (3e38, 1e-45)[j % 2]
    for shape in (gh.SPHERE, gh.ARROW):
        ref = spray.glyphs_host(T, G[shape])
        got, = c.glyphs(on_device([T]), [G[shape]])
        c.sync()
        assert as_bytes(got) == ref_bytes(ref)
    # a sphere set that carries non-finite vectors: the array is not in use
    T = dict(S, vectors=np.full((PROBE, 3), np.nan, F32))
    ref = spray.glyphs_host(S, G[gh.SPHERE])
    got, = c.glyphs(on_device([T]), [G[gh.SPHERE]])
    c.sync()
    assert as_bytes(got) == ref_bytes(ref) and len(ref[4]) > 1000
    c.close()


def test_failed_calls_change_nothing(spray, oracle):
    good_S, good_G = gh.pset(gh.cloud(300, 3)), gh.sphere(0.5, 1, 0x00556677)
    p = gh.cloud(500, 4)
    other = gh.pset(p, vectors=gh.swirl(p))
    arrows = gh.arrow(0.5, 6, color=0x00010203)
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.glyphs_domains([1], [good_S], [good_G])
    before = (export_all(c, 0), export_all(c, 1))

    def fails(S, G, slots=(0, 1), names_="set 1, slot", code=ERR_ARG):
        with pytest.raises(spray.SprayRtError) as e:
            c.glyphs_domains(list(slots), [good_S, S], [good_G, G])
        assert e.value.code == code and names_ in str(e.value), str(e.value)
        assert (export_all(c, 0), export_all(c, 1)) == before

    fails(other, arrows, (0, -1), "set 1")                   # a bad slot
    fails(other, arrows, (1, 1), "set 1")                    # a slot listed twice
    fails(dict(other, stride=0), arrows)
    fails(dict(other, vectors=None), arrows)                 # arrows without vectors
    fails(other, dict(arrows, nsides=17))
    fails(other, dict(arrows, size=0.0))
    fails(other, dict(arrows, min_speed=0.0))
    fails(other, gh.sphere(0.5, 4))
    fails(dict(other, select=np.ones(500, F32), select_range=(1.0, 0.0)), arrows)
    fails(dict(gh.with_color(other, 1), cmap=(np.arange(3, dtype=np.uint32), 1.0, 1.0)), arrows)
    # and the good call goes through
    B = spray.RtContext(0)
    c.glyphs_domains([0, 1], [good_S, other], [good_G, arrows])
    B.glyphs_domains([0, 1], on_device([good_S, other]), [good_G, arrows])
    for s in (0, 1):
        assert export_all(c, s) == export_all(B, s)
    assert export_all(c, 0) != before[0]
    c.close()
    B.close()

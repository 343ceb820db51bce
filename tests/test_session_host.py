"""The session of session_helpers.py satisfies, on the host forms alone, every
condition test_gpu_session.py relies on: which calls follow which, what the
shared scratch has to hold from step to step, where slots are empty, where
the engine's cache keys match over changed geometry and where they must not,
which calls are rejected.  Without these the GPU comparisons could pass
without ever laying a small call over a larger one's bytes.

`pytest -s` prints the per-step table (bytes laid out in d_isomesh, buffers
that grow)."""
import numpy as np
import pytest

import session_helpers as S


@pytest.fixture(scope="module")
def ses(oracle):
    return S.session(oracle)


def good_steps(ses):
    return [k for k, st in enumerate(ses) if S.good(st)]


def flat(ses, rejected=False):
    """[(step, op)] in call order."""
    out = []
    for k, st in enumerate(ses):
        ops = st["ops"] if S.good(st) else (st["reject"]["ops"] if rejected else [])
        order = []
        for o in ops:
            if o["kind"] not in order:
                order.append(o["kind"])
        out += [(k, o) for kind in order for o in ops if o["kind"] == kind]
    return out


def test_domains_boxes_and_names(ses):
    names = [o["name"] for _, o in flat(ses[:-1], rejected=True)]
    assert len(names) == len(set(names))
    assert S.maps(ses, 0).keys() == {0, 1, 2, 3, 4}        # domain 5 starts unmapped
    slack = S.slack_boxes(ses)
    assert slack.shape == (S.NDOM, 6) and np.isfinite(slack).all()
    for k in good_steps(ses):
        b = S.boxes(ses, k)
        assert b.shape == (S.NDOM, 6)
        for d, s in S.maps(ses, k).items():
            m = S.content(ses, k, s)
            assert m is not None, (k, d, s)                 # a mapped slot is live
            if len(m[1]):
                e = S.exact_box(m[0], m[1])
                assert (b[d, :3] <= e[:3]).all() and (e[3:] <= b[d, 3:]).all(), (k, d)
                assert (slack[d, :3] < e[:3]).all() and (e[3:] < slack[d, 3:]).all(), (k, d)
    # the regions do not overlap: a ray's domain order is the same on every walk
    for d in range(S.NDOM):
        for e in range(d):
            assert ((slack[d, 3:] < slack[e, :3]) | (slack[e, 3:] < slack[d, :3])).any(), (d, e)


def test_every_kind_after_and_before_a_larger_call_that_shares_scratch(ses):
    ops = flat(ses)
    kinds = {o["kind"] for _, o in ops}
    assert kinds >= set(S.KINDS)

    def larger_other(o, others):
        return [p["name"] for _, p in others
                if p["kind"] in S.SCRATCH and p["kind"] != o["kind"]
                and S.SCRATCH[p["kind"]] & S.SCRATCH[o["kind"]]
                and S.mesh_bytes(p) > S.mesh_bytes(o)]

    for kind in S.KINDS:
        mine = [i for i, (_, o) in enumerate(ops) if o["kind"] == kind]
        assert any(larger_other(ops[i][1], ops[:i]) for i in mine), ("after", kind)
        assert any(larger_other(ops[i][1], ops[i + 1:]) for i in mine), ("before", kind)


def grown(ses, device=True):
    """[(step, buffer, bytes)]: d_isomesh (never under 1 MiB) and the glyph
    arena's pinned mirror (never under 64 KiB) each time they must grow."""
    out, iso_cap, mirror_cap = [], 0, 0
    for k, st in enumerate(ses):
        if not S.good(st):
            continue
        need = S.step_isomesh_bytes(st, device)
        if need > iso_cap:
            iso_cap = max(need, S.MIB)
            out.append((k, "d_isomesh", iso_cap))
        for o in st["ops"]:
            if o["kind"] in ("glyphs", "glyph_buffers") or (o["kind"] == "refit" and "set" in o):
                n = len(o["sets"]) if o["kind"] == "glyph_buffers" else \
                    sum(1 for p in st["ops"] if p["kind"] == o["kind"])
                head = S.glyph_head_bytes(n)
                if head > mirror_cap:
                    mirror_cap = max(head, S.MIRROR0)
                    out.append((k, "glyph arena mirror", mirror_cap))
    return out


def test_isomesh_is_small_then_over_a_mebibyte_then_small(ses):
    gs = good_steps(ses)
    need = {k: S.step_isomesh_bytes(ses[k]) for k in gs}
    print()
    for k in gs:
        print("step %2d %-20s d_isomesh %8d B" % (k, ses[k]["name"], need[k]))
    for k, what, nbytes in grown(ses):
        print("step %2d grows %s to %d B" % (k, what, nbytes))
    assert 0 < need[gs[0]] < S.MIRROR0
    assert need[S.LARGE] > S.MIB and S.LARGE in gs
    assert max(need[k] for k in gs if k != S.LARGE) < S.MIB    # nothing larger is needed
    after = gs[gs.index(S.LARGE) + 1]
    assert need[after] < S.MIRROR0
    assert S.step_isomesh_bytes(ses[after], device=False) < S.MIRROR0
    # the reallocation happens while slots made from the old buffer are live
    made = [s for s in S.live_slots(ses, S.LARGE - 1)
            if S.chain(ses, S.LARGE - 1, s)[0]["kind"] in S.EXTRACTIONS
            and s not in S.written(ses[S.LARGE])]
    assert made
    assert [g for g in grown(ses) if g[1] == "d_isomesh"] == \
        [(0, "d_isomesh", S.MIB), (S.LARGE, "d_isomesh", need[S.LARGE])]


def test_pinned_mirror_outgrows_its_first_size_then_one_small_job(ses):
    ops = flat(ses, rejected=True)
    glyphy = [(k, o) for k, o in ops if o["kind"] in ("glyphs", "glyph_buffers")
              or (o["kind"] == "refit" and "set" in o)]
    at = [i for i, (_, o) in enumerate(glyphy) if o["kind"] == "glyph_buffers"]
    assert len(at) == 1
    k, o = glyphy[at[0]]
    assert len(o["sets"]) >= 200 and all(len(s["points"]) == 1 for s in o["sets"])
    assert len(o["sets"]) * S.GLYPH_HEAD_PER_JOB > S.MIRROR0
    assert all(len(m[4]) == 1 for m in S.restate_buffers(o))       # every set keeps its point
    k2, nxt = glyphy[at[0] + 1]
    assert k2 > k and nxt["kind"] == "glyphs"
    assert sum(1 for p in ses[k2]["ops"] if p["kind"] == "glyphs") == 1   # a single job
    assert S.glyph_head_bytes(1) < 4096 and 0 < S.mesh_bytes(nxt) < S.MIRROR0
    assert max(S.glyph_head_bytes(1), *(S.glyph_head_bytes(
        sum(1 for p in ses[j]["ops"] if p["kind"] == "glyphs")) for j in range(k))) < S.MIRROR0


def pairs(ses, first, second):
    """[(bytes of kind `first` in a step, bytes of kind `second` in the next good step)]."""
    gs = good_steps(ses)
    size = lambda k, kind: sum(S.mesh_bytes(o) for o in ses[k]["ops"] if o["kind"] == kind)
    return [(size(a, first), size(b, second)) for a, b in zip(gs, gs[1:])
            if size(a, first) and size(b, second)]


@pytest.mark.parametrize("a,b", [("surface", "clip"), ("tet", "build")])
def test_scratch_leftovers_both_ways(ses, a, b):
    assert any(x > y for x, y in pairs(ses, a, b)), (a, "then a smaller", b)
    assert any(x > y for x, y in pairs(ses, b, a)), (b, "then a smaller", a)


def test_empty_slots_are_mapped_for_a_step_and_refilled_by_another_filter(ses):
    gs = good_steps(ses)
    found = []
    for k, nxt in zip(gs, gs[1:]):
        empties = [o for o in ses[k]["ops"] if o["kind"] in S.EXTRACTIONS
                   and len(S.restate(o)[1]) == 0]
        if {o["kind"] for o in empties} >= {"iso", "glyphs"}:
            found.append(k)
            mapped = set(S.maps(ses, k).values())
            for o in empties:
                assert o["slot"] in mapped
                assert S.content(ses, k, o["slot"])[1].shape == (0, 3)
                again = [p for p in ses[nxt]["ops"] if p.get("slot") == o["slot"]]
                assert len(again) == 1 and again[0]["kind"] in S.EXTRACTIONS
                assert again[0]["kind"] != o["kind"] and len(S.restate(again[0])[1]) > 0
                assert o["slot"] in set(S.maps(ses, nxt).values())
    assert found


def same_scene(ses, a, b):
    return S.boxes(ses, a).tobytes() == S.boxes(ses, b).tobytes() and S.maps(ses, a) == S.maps(ses, b)


def test_same_key_step_moves_geometry_under_identical_boxes_and_maps(ses):
    gs = good_steps(ses)
    k, prev = S.SAMEKEY, gs[gs.index(S.SAMEKEY) - 1]
    assert same_scene(ses, k, prev)
    kinds = {}
    for o in ses[k]["ops"]:
        base = S.chain(ses, k, o["slot"])[0]
        kinds[o["kind"]] = base["kind"]
        before, after = S.content(ses, prev, o["slot"]), S.content(ses, k, o["slot"])
        assert S.mesh_image(before) != S.mesh_image(after)
        assert before[1].tobytes() == after[1].tobytes()                     # topology stays
        assert o["slot"] in set(S.maps(ses, k).values())
        # the new content stays inside the unchanged box
        d = [d for d, s in S.maps(ses, k).items() if s == o["slot"]][0]
        e, b = S.exact_box(after[0], after[1]), S.boxes(ses, k)[d]
        assert (b[:3] <= e[:3]).all() and (e[3:] <= b[3:]).all()
    assert kinds == {"refit": "glyphs", "recolor": "surface"}
    assert "set" in [o for o in ses[k]["ops"] if o["kind"] == "refit"][0]    # glyphs(arrays=...)


def test_key_change_steps(ses):
    gs = good_steps(ses)
    steps = list(zip(gs, gs[1:]))
    boxes_change = [b for a, b in steps if S.boxes(ses, a).tobytes() != S.boxes(ses, b).tobytes()]
    assert len(boxes_change) >= 2 and any(ses[b].get("boxes") == "exact" for b in boxes_change)
    gained = [b for a, b in steps if S.boxes(ses, a).tobytes() == S.boxes(ses, b).tobytes()
              and set(S.maps(ses, b)) - set(S.maps(ses, a))]
    assert S.MAP5 in gained
    assert set(S.maps(ses, S.MAP5)) - set(S.maps(ses, S.MAP5 - 1)) == {5}
    assert len(S.content(ses, S.MAP5, S.maps(ses, S.MAP5)[5])[1]) > 0
    released = []
    for a, b in steps:
        lost = set(S.maps(ses, a)) - set(S.maps(ses, b))
        for d in lost:
            slot = S.maps(ses, a)[d]
            if any(o["kind"] == "release" and o["slot"] == slot for o in ses[b]["ops"]):
                released.append((b, d))
                assert S.content(ses, b, slot) is None
    assert released
    # and the domain comes back later
    b, d = released[0]
    assert any(d in S.maps(ses, k) for k in gs if k > b)


def test_rejected_calls_sit_between_good_steps_with_the_bad_element_second(ses):
    import spray_amd as spray
    rej = [k for k, st in enumerate(ses) if not S.good(st)]
    assert {ses[k]["reject"]["kind"] for k in rej} >= {"glyphs", "build", "cell"}
    for k in rej:
        assert 0 < k < len(ses) - 1 and S.good(ses[k - 1]) and S.good(ses[k + 1])
        r = ses[k]["reject"]
        ok, bad = r["ops"]
        assert S.mesh_bytes(ok) > 0                                    # the first job is valid
        assert "slot %d" % bad["slot"] in r["expect"][0]
        if r["kind"] == "build":
            assert bad["faces"].max() >= len(bad["verts"]) > ok["faces"].max()
        else:
            with pytest.raises(spray.SprayRtError):
                S.corrupted(bad, bad)
        # both targets are live: a failed call could damage them
        assert S.content(ses, k, ok["slot"]) is not None


def test_round_trip(ses):
    assert all(a is b for a, b in zip(ses[-1]["ops"], ses[0]["ops"]))
    assert len(ses[-1]["ops"]) == len(ses[0]["ops"])
    for s in S.written(ses[0]):
        assert S.mesh_image(S.content(ses, len(ses) - 1, s)) == S.mesh_image(S.content(ses, 0, s))


def test_anchor_step_has_every_domain_with_colours_and_normals(ses):
    """What the oracle's whole-scene frame needs of the step it is compared on."""
    m = S.maps(ses, S.ANCHOR)
    assert sorted(m) == list(range(S.NDOM))
    for d, s in m.items():
        v, f, c, n = S.content(ses, S.ANCHOR, s)
        assert len(f) > 0 and c is not None and n is not None, (d, s)
        assert len(c) == len(v) == len(n)


def test_colour_maps_give_more_than_eight_colours(ses):
    for k in good_steps(ses):
        cols = [S.content(ses, k, s)[2] for s in S.maps(ses, k).values()]
        assert len(np.unique(np.concatenate([c for c in cols if c is not None]))) > 8, k


def test_the_comparison_reports_step_and_slot_when_state_is_carried(ses):
    """Carried state, simulated on the restated side: the same-key step's
    slots paired with the previous step's inputs (a refit or a recolour that
    never arrived), and one operation restated from another's inputs."""
    gs = good_steps(ses)
    k, prev = S.SAMEKEY, gs[gs.index(S.SAMEKEY) - 1]
    want = {s: S.mesh_image(S.content(ses, k, s)) for s in S.live_slots(ses, k)}
    S.compare_slots(dict(want), want, k)
    stale = {s: S.mesh_image(S.content(ses, prev, s)) for s in S.live_slots(ses, k)}
    moved = S.written(ses[k])
    with pytest.raises(AssertionError) as e:
        S.compare_slots(stale, want, k)
    assert str([(k, s) for s in moved]) in str(e.value)
    # a batch neighbour's inputs in place of the slot's own
    a, b = ses[0]["ops"][0], ses[0]["ops"][1]
    assert a["kind"] == b["kind"]
    got = dict(want)
    got[a["slot"]] = S.mesh_image(S.corrupted(a, b))
    with pytest.raises(AssertionError) as e:
        S.compare_slots(got, {**want, a["slot"]: S.mesh_image(S.restate(a))}, 0)
    assert str([(0, a["slot"])]) in str(e.value)
    # a missing slot (released on one side only) is a difference too
    with pytest.raises(AssertionError) as e:
        S.compare_slots({s: v for s, v in want.items() if s != moved[0]}, want, k)
    assert str((k, moved[0])) in str(e.value)

"""One context and one live in-situ engine through the time-step session of
session_helpers.py (test_session_host.py proves its conditions on the CPU):
every filter writes slots of the same context step after step, the boxes and
maps move, and the engine created before the first step renders after each.

After every step the session context A is compared with its twin, a fresh
context on which each live slot's chain was replayed alone, one single-slot
call at a time (session_helpers.replay).  The twin has no history and another
batch composition, so a difference is carried state or batch dependence: a
scratch word read before it is written, a pointer kept over a buffer that
grew, a table that was not rebuilt.  Everything is byte equality; the
independent anchors are the host restatements of the slots' arrays, the
oracle's brute force on the last two steps and its whole-scene frame on one
step (records bit for bit, totals exactly, the image within the film's
summation order: rtol 1e-5, atol 1e-6, as test_gpu_insitu_ray_cases.check).

The frames: trace_camera through the replicated steps (the camera tables
under cam_key, with a mapped flag per domain), trace_image (img_key),
trace_frame, render_tiles (ftab_key) and render_tile, 64 x 64 at spp 2, a
point-light PT shader and an AO shader.  One rank's image-parallel frame wants
every domain resident and refuses the steps in which a domain is unmapped;
the refusal is asserted, on both contexts.

The walk runs once per parametrisation (device arrays; host arrays with jobs
that mix host and device arrays) and records what the tests below assert."""
import os

import numpy as np
import pytest

import build_helpers as bh
import clip_helpers as clh
import insitu_helpers as H
import refit_helpers as rh
import session_helpers as S
import stream_helpers as sth
import surface_helpers as sfh

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
IMG, SPP = 64, 2
EYE, LOOKAT, FOV = (13.0, 12.0, 36.0), (13.0, 9.0, 2.0), 58.0   # both rows of domains in view
LIGHTS = [(0, 14.0, 50.0, 60.0, 1.0, 1.0, 1.0)]
SHADERS = {"pt": ("pt", 1, 1), "ao": ("ao", 1, 4)}
FRAMES = ("camera", "image", "frame")


def full_export(c, slot):
    out = bh.export_all(c, slot)
    out["FACES"] = c.slot_export(slot, c.SLOT_FACES).tobytes()
    out["COLORS"] = c.slot_export(slot, c.SLOT_COLORS).tobytes()
    out["INFO"] = c.slot_info(slot)
    return out


def exports(c, slots):
    return {s: full_export(c, s) for s in slots}


def render(spray, insitu, torch, c, eng, eye):
    """Every frame form on context c and its engine -> {name: (records, totals,
    image bytes)}; images start zeroed."""
    cam = spray.camera_init(EYE, LOOKAT, [0.0, 1.0, 0.0], FOV, IMG, IMG)
    org, d, pix, sam = eye
    rays = H.rays_tensor(org, d).cuda()
    gpix, gsam = torch.from_numpy(pix).cuda(), torch.from_numpy(sam).cuda()
    n = len(org)
    out = {}
    for sname, (kind, bounces, samples) in SHADERS.items():
        sh = spray.frame.make_shader(kind, bounces, samples, lights=LIGHTS)
        for how in FRAMES:
            recs = insitu.InsituRecords(n * bounces + 16)
            image = torch.zeros(IMG * IMG * 4, dtype=torch.float32, device="cuda")
            try:
                if how == "camera":
                    # the replicated steps (prepare_camera's tables under cam_key);
                    # without the switch one rank's camera frame is the image frame
                    os.environ["SPRAY_INSITU_REPLICATED"] = "1"
                    try:
                        tot = eng.trace_camera(sh, cam, IMG, IMG, SPP, image, recs)
                    finally:
                        del os.environ["SPRAY_INSITU_REPLICATED"]
                elif how == "image":
                    tot = eng.trace_image(sh, cam, IMG, IMG, SPP, image, 1, recs)
                else:
                    tot = eng.trace_frame(sh, rays, gpix, gsam, SPP, image, recs)
            except spray.SprayRtError as e:   # a refusal is a result too: the twin's must equal it
                out["%s-%s" % (how, sname)] = ("refused", e.code, str(e))
                continue
            torch.cuda.synchronize()
            r = recs.numpy()
            out["%s-%s" % (how, sname)] = ({k: v.tobytes() for k, v in r.items()}, tuple(tot),
                                           image.cpu().numpy().tobytes())
            if how == "camera":
                out["domains-" + sname] = sorted(set(r["hits"].view(np.int32)[:, 11].tolist()))
    # the frame layer: the footprint-culled batch of tiles, and tile by tile
    sh = spray.frame.make_shader("pt", 1, 1, lights=LIGHTS)
    tiles = [t for t in spray.frame.tile_list(IMG, IMG, SPP, 1, 0, 1500) if t[2] * t[3]]
    many = torch.zeros(IMG * IMG * 4, dtype=torch.float32, device="cuda")
    c.frame_stats(reset=True)
    c.render_tiles(sh, cam, IMG, SPP, tiles, many)
    cnt = c.frame_stats(reset=True)
    torch.cuda.synchronize()
    out["render_tiles"] = ({}, tuple(cnt), many.cpu().numpy().tobytes())
    one = torch.zeros_like(many)
    for t in tiles:
        c.render_tile(sh, cam, IMG, SPP, t, one)
    cnt = c.frame_stats(reset=True)
    torch.cuda.synchronize()
    out["render_tile"] = ({}, tuple(cnt), one.cpu().numpy().tobytes())
    assert len(tiles) > 3
    return out


def buffer_forms(spray, torch, A, ses):
    """glyphs, stream_tubes, cell_clip and cell_surface into caller buffers,
    back to back on A with device inputs, the large one first, one sync at
    the end -> [(name, got bytes, host bytes)]."""
    big = ses[S.LARGE]["ops"][0]
    tube_op = ses[S.FIRST]["ops"][4]
    clip_op = [o for o in ses[S.ANCHOR]["ops"] if o["kind"] == "clip"][0]
    surf_op = [o for o in ses[S.MAP5]["ops"] if o["kind"] == "surface"][0]
    g = A.glyphs(S.on_device([big["set"]]), [big["glyph"]])
    t = A.stream_tubes(S.on_device([tube_op["field"]]), [tube_op["tube"]])
    cl = A.cell_clip(S.on_device([clip_op["mesh"]]), [clip_op["invert"]])
    su = A.cell_surface(S.on_device([surf_op["mesh"]]))
    A.sync()
    f = tube_op["field"]
    want = {
        "glyphs": spray.glyphs_host(big["set"], big["glyph"]),
        "stream_tubes": spray.stream_tubes_host(
            *sth.host_args(f), tube_op["tube"]["radius"], tube_op["tube"]["nsides"],
            color=tube_op["tube"].get("color"), cfield=f.get("cfield"), cmap=f.get("cmap"),
            **sth.host_kw(f)),
        "cell_clip": clh.host_clip(spray, clip_op["mesh"], clip_op["invert"]),
        "cell_surface": sfh.host_surface(spray, surf_op["mesh"]),
    }
    got = {"glyphs": g[0], "stream_tubes": t[0], "cell_clip": cl[0], "cell_surface": su[0]}
    tob = lambda x: int(x) if np.isscalar(x) else (
        None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)).tobytes())
    return [(name, tuple(tob(x) for x in got[name]), tuple(tob(x) for x in want[name]))
            for name in got]


def scene_rays(ses, k):
    """refit_helpers.refit_rays over the merged restated meshes, and over every
    mapped domain's own mesh (a few triangles among many thousands would
    otherwise see no ray)."""
    rng = np.random.default_rng(100 + k)
    parts = [rh.refit_rays(rng, *S.merged(ses, k))]
    for d, s in sorted(S.maps(ses, k).items()):
        v, f = S.content(ses, k, s)[:2]
        if len(f):
            parts.append(rh.refit_rays(rng, v, f, n=400))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def run_session(oracle, device):
    import torch
    import spray_amd as spray
    from spray_amd import insitu
    ses = S.session(oracle)
    cam = oracle.camera_init(EYE, LOOKAT, [0.0, 1.0, 0.0], FOV, IMG, IMG)
    eye = oracle.eye_rays_insitu(cam, IMG, SPP, (0, 0, IMG, IMG), (0, 0, IMG, IMG))
    eo, ed, epix, _ = oracle.eye_rays_ooc(cam, IMG, 1, (0, 0, IMG, IMG))
    eye1 = spray.make_rays(eo, ed)
    A = spray.RtContext(0)
    A.set_stream(torch.cuda.current_stream())
    A.domain_bounds(S.slack_boxes(ses))     # the domain count is fixed from the start
    eng = insitu.InsituEngine(A, 1, 0, transport="rccl")
    good = [k for k, st in enumerate(ses) if S.good(st)]
    log, images = [], {}
    for k, step in enumerate(ses):
        rec = dict(k=k, name=step["name"])
        log.append(rec)
        if not S.good(step):
            rec["error"] = S.attempt(A, step, device)
            rec["A"] = exports(A, S.live_slots(ses, k))
            rec["before"] = dict(images)
            continue
        rec["before"] = dict(images)
        bounds, outs, rec["boxes"] = S.apply(A, ses, k, device)
        A.sync()
        rec["buffers"] = [(o["name"], [[None if x is None else x.cpu().numpy().tobytes()
                                        for x in r] for r in res]) for o, res in outs]
        rec["bounds"] = bounds
        live = S.live_slots(ses, k)
        images = exports(A, live)
        rec["A"] = dict(images)
        B = spray.RtContext(0)
        B.set_stream(torch.cuda.current_stream())
        rec["boxes_twin"] = S.replay(B, ses, k, device)
        B.sync()
        rec["B"] = exports(B, live)
        rays = spray.make_rays(*scene_rays(ses, k))
        rec["scene_A"] = bh.scene_results(spray, A, rays, eye1, epix)
        rec["scene_B"] = bh.scene_results(spray, B, rays, eye1, epix)
        before = eng.stats()
        rec["frames_A"] = render(spray, insitu, torch, A, eng, eye)
        rec["stats"] = {key: v - before[key] for key, v in eng.stats().items()}
        twin = insitu.InsituEngine(B, 1, 0, transport="rccl")
        rec["frames_B"] = render(spray, insitu, torch, B, twin, eye)
        twin.close()
        B.close()
        if k in good[-2:]:   # the oracle's brute force on every non-empty slot
            rec["queries"] = []
            for s in live:
                v, f, c, n = S.content(ses, k, s)
                if len(f):
                    bh.check_queries(spray, oracle, A, s, v, f, c, n, 40 + s)
                    rec["queries"].append(s)
    log[-1]["buffer_forms"] = buffer_forms(spray, torch, A, ses)
    eng.close()
    A.close()
    return ses, log


@pytest.fixture(scope="module", params=[True, False], ids=["device", "host-mixed"])
def walk(request, oracle):
    return run_session(oracle, request.param)


def good_records(log):
    return [r for r in log if "error" not in r]


def test_slots_equal_the_twin_and_the_restated_arrays(walk):
    ses, log = walk
    for r in good_records(log):
        k = r["k"]
        S.compare_slots(r["A"], r["B"], k, "session against twin:")
        wrote = S.written(ses[k])
        S.compare_slots({s: v for s, v in r["A"].items() if s not in wrote},
                        {s: v for s, v in r["before"].items()
                         if s not in wrote and s in r["A"]}, k, "slots the step did not write:")
        assert sorted(r["A"]) == S.live_slots(ses, k)
        for s in wrote:
            if s not in r["A"]:
                continue   # released
            v, f, c, n = S.content(ses, k, s)
            got = r["A"][s]
            want = S.mesh_image((v, f, c, n))
            S.compare_slots({s: {w: got[w] for w in ("FACES", "COLORS", "NORMALS")}},
                            {s: {w: want[w] for w in ("FACES", "COLORS", "NORMALS")}}, k,
                            "restated arrays:")
            assert got["INFO"]["tris"] == len(f), (k, s)
            if len(f) and s in r["bounds"]:
                assert r["bounds"][s].tobytes() == S.exact_box(v, f).tobytes(), (k, s)
        assert r["boxes"].tobytes() == r["boxes_twin"].tobytes() == S.boxes(ses, k).tobytes(), k
    last, first = good_records(log)[-1], log[S.FIRST]
    S.compare_slots({s: last["A"][s] for s in S.written(ses[S.FIRST])},
                    {s: first["A"][s] for s in S.written(ses[S.FIRST])}, last["k"],
                    "round trip:")


def test_rejected_calls_name_the_job_and_change_nothing(walk):
    ses, log = walk
    rejected = [r for r in log if "error" in r]
    assert len(rejected) >= 3
    for r in rejected:
        e, want = r["error"], ses[r["k"]]["reject"]
        assert e.code == ERR_ARG, (r["name"], str(e))
        for text in want["expect"]:
            assert text in str(e), (r["name"], str(e))
        S.compare_slots(r["A"], r["before"], r["k"], "after a rejected call:")
        nxt = log[r["k"] + 1]
        assert "error" not in nxt and nxt["A"]   # the next step ran, and is compared above


def test_caller_buffer_forms_back_to_back(walk):
    ses, log = walk
    forms = log[-1]["buffer_forms"]
    assert [f[0] for f in forms] == ["glyphs", "stream_tubes", "cell_clip", "cell_surface"]
    for name, got, want in forms:
        assert len(got) == len(want), name
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, i)
    assert len(forms[0][1][0]) > S.MIB // 4         # the large one came first
    # the several hundred one-point sets of the session itself
    done = [(r["k"], b) for r in good_records(log) for b in r["buffers"]]
    assert len(done) == 1
    k, (name, res) = done[0]
    o = [o for o in ses[k]["ops"] if o["name"] == name][0]
    want = S.restate_buffers(o)
    assert len(res) == len(want) >= 200
    for i, (g, w) in enumerate(zip(res, want)):
        assert g == [None if x is None else np.asarray(x).tobytes() for x in w], (name, i)


def test_scene_walks_equal_the_twin(walk):
    import spray_amd as spray
    ses, log = walk
    for r in good_records(log):
        k = r["k"]
        ra, rb = r["scene_A"], r["scene_B"]
        for key in ra:
            assert ra[key] == rb[key], (k, key)
        hits = np.frombuffer(ra["intersect_scene"], spray.HIT_DTYPE)
        full = {d for d, s in S.maps(ses, k).items() if len(S.content(ses, k, s)[1])}
        assert set(np.unique(hits["domain"]).tolist()) == full | {-1}, k
        assert ra["shadow_pt"][3] > 0 and ra["ao"][1] > 0, k
        for mode in (0, 1, 2):
            occ = np.frombuffer(ra["occluded_scene_%d" % mode], np.uint8)
            assert 0 < occ.mean() < 1, (k, mode)
        assert len(np.unique(hits["color"][hits["domain"] >= 0])) > 8, k


def test_live_engine_frames_equal_a_fresh_engine_on_the_twin(walk):
    ses, log = walk
    recs = good_records(log)
    for r in recs:
        k = r["k"]
        fa, fb = r["frames_A"], r["frames_B"]
        assert fa.keys() == fb.keys()
        for name in fa:
            assert fa[name] == fb[name], (k, name)
        # the image-parallel frame wants every domain resident; nothing else is refused
        refused = sorted(name for name in fa if fa[name][0] == "refused")
        unmapped = sorted(set(range(S.NDOM)) - set(S.maps(ses, k)))
        assert refused == (["image-ao", "image-pt"] if unmapped else []), (k, refused)
        for name in refused:
            assert fa[name][1] == ERR_STATE and "domain %d is not" % unmapped[0] in fa[name][2]
        for name in fa:   # no frame is black, not even the step of the smallest meshes
            if name.split("-")[0] in FRAMES + ("render_tiles", "render_tile") and name not in refused:
                assert (np.frombuffer(fa[name][2], np.float32) > 0).any(), (k, name)
        assert fa["render_tiles"][1:] == fa["render_tile"][1:], k
    by_k = {r["k"]: r for r in recs}
    order = [r["k"] for r in recs]
    prev = lambda k: by_k[order[order.index(k) - 1]]
    # a matching key over geometry that changed: the frames still move
    same = by_k[S.SAMEKEY]
    assert len(S.maps(ses, S.SAMEKEY)) == S.NDOM     # so every frame form runs
    for name in same["frames_A"]:
        if not name.startswith("domains"):
            assert same["frames_A"][name][2] != prev(S.SAMEKEY)["frames_A"][name][2], name
    # keys that must stop matching: the newly mapped domain contributes ...
    for sname in SHADERS:
        assert 5 not in prev(S.MAP5)["frames_A"]["domains-" + sname]
        assert 5 in by_k[S.MAP5]["frames_A"]["domains-" + sname]
    # ... and no frame shades a domain that is unmapped (the released one among them)
    assert [k for k in order if 4 not in S.maps(ses, k)]
    for k in order:
        for sname in SHADERS:
            assert set(by_k[k]["frames_A"]["domains-" + sname]) <= set(S.maps(ses, k)), k
    # new boxes: every step whose boxes changed still equals its twin (above)
    assert any(by_k[a]["boxes"].tobytes() != by_k[b]["boxes"].tobytes()
               for a, b in zip(order, order[1:]))


def test_independent_anchors(walk, oracle):
    """The oracle's brute force on every non-empty slot after the last two
    steps (run inside the walk), and its whole-scene frame of the merged
    restated meshes on one mid-session step."""
    ses, log = walk
    recs = good_records(log)
    for r in recs[-2:]:
        want = [s for s in S.live_slots(ses, r["k"]) if len(S.content(ses, r["k"], s)[1])]
        assert r["queries"] == want and len(want) >= 6
    r = log[S.ANCHOR]
    osc = oracle.Scene(S.NDOM)
    boxes = S.boxes(ses, S.ANCHOR)
    for d, s in S.maps(ses, S.ANCHOR).items():
        v, f, c, n = S.content(ses, S.ANCHOR, s)
        osc.set_domain(d, v, f, c, n, boxes[d])
    cam = oracle.camera_init(EYE, LOOKAT, [0.0, 1.0, 0.0], FOV, IMG, IMG)
    org, d, pix, sam = oracle.eye_rays_insitu(cam, IMG, SPP, (0, 0, IMG, IMG), (0, 0, IMG, IMG))
    for sname, (kind, bounces, samples) in SHADERS.items():
        sh = oracle.shader(kind, bounces, samples, (0.4, 0.4, 0.4), 10.0, LIGHTS)
        ref, ref_img, ref_tot = H.reference_frame_rays(oracle, sh, list(S.BSDFS), osc, org, d, pix,
                                                       sam, IMG, IMG, SPP)
        raw, tot, img = r["frames_A"]["frame-" + sname]
        got = {"samid": np.frombuffer(raw["samid"], np.int32),
               "bounce": np.frombuffer(raw["bounce"], np.int32),
               "hits": np.frombuffer(raw["hits"], np.float32).reshape(-1, 12),
               "svalid": np.frombuffer(raw["svalid"], np.uint64),
               "occluded": np.frombuffer(raw["occluded"], np.uint64)}
        assert tuple(tot) == tuple(ref_tot), (sname, tot, ref_tot)
        H.compare_records(H.records_dict(got), ref)
        # the reference itself is not vacuous: shaded samples in every domain,
        # and for AO both outcomes of the occlusion rays
        doms = [int(np.frombuffer(v[0], oracle.HIT_DTYPE)["domain"][0]) for v in ref.values()]
        assert min(np.bincount(doms, minlength=S.NDOM)) >= 10, (sname, np.bincount(doms))
        spawned = sum(bin(v[1]).count("1") for v in ref.values())
        blocked = sum(bin(v[2]).count("1") for v in ref.values())
        assert spawned > 0 and (ref_img > 0).any(), sname
        if kind == "ao":
            assert 0 < blocked < spawned, (blocked, spawned)
        np.testing.assert_allclose(np.frombuffer(img, np.float32), ref_img, rtol=1e-5, atol=1e-6,
                                   err_msg=sname)

"""The in-situ engine and its stand-alone consumers on the hard ray classes of
ray_cases.py (test_insitu_ray_cases.py pins the rule on the CPU): the
nine-domain scene of touching boxes and coincident triangles, at the origin
and at 1e4, its contexts built with upload_domain / map_domain /
domain_bounds / set_owners / set_bsdfs.

Every expected value is the whole-scene reference frame's
(ray_cases.frame_reference: the oracle's closest hit -> shade -> any hit ->
film on the same eye rays): the shaded samples' records bit for bit
(insitu_helpers.compare_records), the totals exactly, the image within the
film's summation order (rtol 1e-5, atol 1e-6, as test_gpu_insitu._check).

  world 1, one-rank RCCL transport: the `mixed` class (7168 rays, axis-parallel
    and signed-zero directions, rays in lattice planes, origins on surfaces)
    and `nonfinite` through trace (all-local and the whole protocol with its
    wire records), trace_frame (all-local and the replicated steps, both key
    forms), PT 1 bounce, AO 4 samples, PT 3 bounces x 2 samples (trace);
  world 2, two processes on the one GPU over the host transport (one GPU
    cannot hold an RCCL group of two ranks): `mixed` under OWNER_CHECKER
    (every pair of domains with coincident triangles split: cross-rank exact
    t ties) and OWNER_ONE, trace and trace_frame (both key forms),
    trace_camera, and trace_image with every domain on both ranks;
  stand-alone: intersect_scene_keyed and route of a rank's context against
    the CPU rule, every class; trace_camera / trace_image with the eye in a
    plane the touching boxes share and inside a domain's box."""
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

import insitu_helpers as H
import ray_cases as RC
from test_gpu_insitu import _rendezvous_file, same_collectives

pytestmark = pytest.mark.gpu

OFFSETS = pytest.mark.parametrize("offset", (0.0, RC.LARGE), ids=["origin", "large"])
PARTITIONS = {"checker": RC.OWNER_CHECKER, "one": RC.OWNER_ONE}
NAMES = RC.CLASSES + ("mixed",)
RAGGED = (1, 63, 64, 65, 129)
IMG, SPP = 64, 2  # the camera frames
# (a) the eye exactly in the plane x = 4 the touching boxes share; (b) the eye
# inside domain 0's box [0, 4]^3 (outside its cubes).  Both look at the scene
# centre; each reference has more than 500 lit pixels where it stands (821 /
# 819 and 544 / 543 at the two offsets), so neither was moved.
CAMERAS = {"cam_a": ((4.0, 4.0, 20.0), 60.0), "cam_b": ((0.5, 3.9, 3.0), 90.0)}
REP, PROTO = {"SPRAY_INSITU_REPLICATED": "1"}, {"SPRAY_INSITU_LOCAL": "0"}


def camera(make, offset, name):
    eye, fov = CAMERAS[name]
    off = float(offset)
    return make([e + off for e in eye], [4.0 + off] * 3, [0.0, 1.0, 0.0], fov, IMG, IMG)


def inputs_of(po, var, offset, source):
    """The eye rays of `source`: a ray class as a frame, or a camera's."""
    if source not in CAMERAS:
        return RC.frame_inputs(var, source)
    key = ("inputs", source)
    if key not in var["ref"]:
        org, d, pix, sam = po.eye_rays_insitu(camera(po.camera_init, offset, source), IMG, SPP,
                                              (0, 0, IMG, IMG), (0, 0, IMG, IMG))
        var["ref"][key] = dict(org=org, dir=d, pix=pix, sam=sam, w=IMG, h=IMG, spp=SPP)
    return var["ref"][key]


def rank_context(spray, var, owner, rank, resident=None):
    """insitu.setup_rank_context from meshes in memory: every box, the owner
    map, the rank's own domains (resident: others too) in slots 0..k-1."""
    rt = spray.RtContext(0)
    rt.domain_bounds(var["boxes"])
    mine = [d for d in range(RC.NDOM) if owner[d] == rank] if resident is None else resident
    for slot, d in enumerate(mine):
        v, f = var["meshes"][d]
        rt.upload_domain(slot, v, f, var["colors"][d], var["normals"][d])
        rt.map_domain(d, slot)
    rt.set_owners(np.asarray(owner, np.int32))
    rt.set_bsdfs(list(RC.BSDFS))
    return rt


def run_jobs(rank, world, offset, part, jobs, dist=None):
    """One rank's engine frames.  part: "checker" / "one" (world 2), "all"
    (every domain resident on every rank: the image frames; the owner map is
    OWNER_CHECKER's at world 2).
    jobs: [(label, source, case, how, env)], how = "trace" (this rank's share of
    the eye rays), "frame" (trace_frame, every eye ray), "camera", "image";
    env: the engine's switches that are read per frame.  Returns {label:
    (records, totals, image, stats of that frame)}."""
    import spray_amd
    from spray_amd import insitu
    from oracle import pyoracle as po
    var = RC.variant(po, offset)
    if part == "all" or world == 1:
        owner = [0] * RC.NDOM if world == 1 else RC.OWNER_CHECKER
        resident = list(range(RC.NDOM))
    else:
        owner, resident = PARTITIONS[part], None
    rt = rank_context(spray_amd, var, owner, rank, resident)
    rt.set_stream(torch.cuda.current_stream())
    eng = insitu.InsituEngine(rt, world, rank, dist=dist,
                              transport="rccl" if world == 1 else "host")
    out = {}
    for label, source, case, how, env in jobs:
        fi = inputs_of(po, var, offset, source)
        n = len(fi["org"])
        lo, hi = (0, n) if how != "trace" or world == 1 else \
            ((0, n // 2) if rank == 0 else (n // 2, n))  # whole pixels: n // 2 is even
        rays = H.rays_tensor(fi["org"][lo:hi], fi["dir"][lo:hi]).cuda()
        pix = torch.from_numpy(np.ascontiguousarray(fi["pix"][lo:hi])).cuda()
        sam = torch.from_numpy(np.ascontiguousarray(fi["sam"][lo:hi])).cuda()
        sh = RC.frame_shader(spray_amd.frame.make_shader, offset, case)
        recs = insitu.InsituRecords(n * RC.SHADING[case][1] + 16)
        image = torch.zeros(fi["w"] * fi["h"] * 4, dtype=torch.float32, device="cuda")
        before = eng.stats()
        os.environ.update(env)
        try:
            if how == "trace":
                tot = eng.trace(sh, rays, pix, sam, fi["spp"], image, recs)
            elif how == "frame":
                tot = eng.trace_frame(sh, rays, pix, sam, fi["spp"], image, recs)
            else:
                cam = camera(spray_amd.camera_init, offset, source)
                if how == "camera":
                    tot = eng.trace_camera(sh, cam, IMG, IMG, SPP, image, recs)
                else:
                    tot = eng.trace_image(sh, cam, IMG, IMG, SPP, image, 1, recs)
        finally:
            for k in env:
                del os.environ[k]
        torch.cuda.synchronize()
        st = {k: v - before[k] for k, v in eng.stats().items()}
        st["clog"] = eng.collective_log()
        out[label] = (recs.numpy(), tot, image.cpu().numpy(), st)
    eng.close()
    rt.close()
    return out


def _rank_main(rank, world, port, out, offset, part, jobs):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        res = run_jobs(rank, world, offset, part, jobs, dist)
        with open(os.path.join(out, "r%d.pkl" % rank), "wb") as fh:
            pickle.dump(res, fh)
    finally:
        dist.destroy_process_group()


def spawned(world, offset, part, jobs):
    """run_jobs in `world` fresh processes sharing the GPU (a fresh process
    also reads SPRAY_INSITU_SPLIT_KEYS anew: the engine reads it once)."""
    with tempfile.TemporaryDirectory() as out:
        torch.multiprocessing.spawn(_rank_main,
                                    args=(world, _rendezvous_file(), out, offset, part, jobs),
                                    nprocs=world)
        res = []
        for r in range(world):
            with open(os.path.join(out, "r%d.pkl" % r), "rb") as fh:
                res.append(pickle.load(fh))
    return res


def check(oracle, var, offset, job, results):
    """One job's results of every rank against the whole-scene reference
    frame.  Returns (merged records, reference records)."""
    label, source, case, how, env = job
    fi = inputs_of(oracle, var, offset, source)
    ref, ref_img, ref_tot = RC.frame_reference(oracle, var, offset, source, case, inputs=fi)
    merged = []
    for r in results:
        recs, tot, _, _ = r[label]
        assert tuple(tot) == tuple(ref_tot), (label, tot, ref_tot)
        merged += [(b, s) + v for (b, s), v in H.records_dict(recs).items()]
    got = H.records_dict(merged)  # raises on a sample shaded on two ranks
    try:
        H.compare_records(got, ref)
    except AssertionError as e:
        raise AssertionError((label, e.args)) from None
    # the image frame gathers the other ranks' rows into rank 0's image
    total = results[0][label][2] if how == "image" else \
        np.sum([r[label][2] for r in results], axis=0)
    assert (ref_img > 0).sum() > 500, label
    if source in CAMERAS:  # more than 500 lit pixels (three entries each; alpha stays 0)
        assert (ref_img.reshape(-1, 4)[:, :3] > 0).any(1).sum() > 500, label
    np.testing.assert_allclose(total, ref_img, rtol=1e-5, atol=1e-6, err_msg=label)
    return got, ref


W1_JOBS = [("trace-%s" % c, None, c, "trace", {}) for c in ("pt1", "ao4", "pt3")] + \
          [("proto-%s" % c, None, c, "trace", PROTO) for c in ("pt1", "ao4", "pt3")] + \
          [("frame-%s" % c, None, c, "frame", {}) for c in ("pt1", "ao4")] + \
          [("rep-%s" % c, None, c, "frame", REP) for c in ("pt1", "ao4")]


def jobs_for(jobs, source):
    return [(lb, source, c, how, env) for lb, _, c, how, env in jobs]


def check_nonfinite(var, got):
    """The records with a non-finite or all-zero origin / direction shade
    nothing; a NaN tnear / tfar is not part of a radiance ray (the default
    extents), so those samples shade like their neighbours."""
    pl = var["classes"]["nonfinite"]["planted"]
    dead = set(np.flatnonzero((pl >= 0) & (pl < 7)).tolist())
    assert len(dead) > 150
    assert not [k for k in got if k[1] in dead]
    assert len({k[1] for k in got if k[0] == 0}) == len(pl) - len(dead)


@OFFSETS
@pytest.mark.parametrize("source", ["mixed", "nonfinite"])
def test_world1_frames(oracle, offset, source):
    """World 1 through the one-rank RCCL transport: trace all-local and with
    the whole protocol (SPRAY_INSITU_LOCAL=0: k_pack_rad / k_unpack_rad, the
    wire records), trace_frame all-local and with the replicated steps
    (SPRAY_INSITU_REPLICATED=1: k_rep_cull, the keyed closest hit's list
    positions, the shadow rays built in the lanes)."""
    var = RC.variant(oracle, offset)
    jobs = jobs_for(W1_JOBS, source)
    res = run_jobs(0, 1, offset, "all", jobs)
    for job in jobs:
        got, ref = check(oracle, var, offset, job, [res])
        st = res[job[0]][3]
        if job[4] == PROTO:
            assert st["exchanges"] > 0, job[0]
        else:
            assert st["exchanges"] == 0, job[0]
        if job[4] == REP:
            assert st["collectives"] >= 3, (job[0], st)
        if job[0] == "rep-pt1":  # the split keys: a MIN of the t bits, then of a byte
            ops = [op for op, _, _ in st["clog"]]
            assert "allreduce_min_u8" in ops and "allreduce_min_u64" not in ops, ops
        if source == "nonfinite":
            check_nonfinite(var, got)
        else:
            hits, shadows, occluded = RC.bounce_counts(ref, 0)
            assert shadows > 3000 and occluded > 1500, (job[0], hits, shadows, occluded)
            if job[2] == "pt3":
                assert RC.bounce_counts(ref, 2)[0] > 1000


U64_JOBS = [("rep-pt1-mixed", "mixed", "pt1", "frame", REP),
            ("rep-pt1-nonfinite", "nonfinite", "pt1", "frame", REP),
            ("camrep-cam_a", "cam_a", "pt1", "camera", REP),
            ("camrep-cam_b", "cam_b", "pt1", "camera", REP)]


@OFFSETS
def test_world1_replicated_steps_u64_keys(oracle, offset, monkeypatch):
    """The 64-bit key MIN (SPRAY_INSITU_SPLIT_KEYS=0) of the replicated PT
    frames at world 1, in a fresh process (the engine reads the switch once
    per process)."""
    monkeypatch.setenv("SPRAY_INSITU_SPLIT_KEYS", "0")
    var = RC.variant(oracle, offset)
    res = spawned(1, offset, "all", U64_JOBS)
    for job in U64_JOBS:
        got, _ = check(oracle, var, offset, job, res)
        ops = [op for op, _, _ in res[0][job[0]][3]["clog"]]
        assert "allreduce_min_u64" in ops and "allreduce_min_u8" not in ops, (job[0], ops)
        if job[1] == "nonfinite":
            check_nonfinite(var, got)


W2_JOBS = [("trace-pt1", "mixed", "pt1", "trace", {}), ("trace-ao4", "mixed", "ao4", "trace", {}),
           ("frame-pt1", "mixed", "pt1", "frame", {}), ("frame-ao4", "mixed", "ao4", "frame", {})]
W2_CAMERA_JOBS = [("%s-%s" % (how, c), c, "pt1", how, {}) for c in sorted(CAMERAS)
                  for how in ("camera", "frame")]
W2_IMAGE_JOBS = [("%s-%s" % (lb, c), c, "pt1", "image", env) for c in sorted(CAMERAS)
                 for lb, env in (("image", {}), ("whole", {"SPRAY_IMAGE_CULL": "0"}))]


@OFFSETS
@pytest.mark.parametrize("part,keys", [("checker", "split"), ("checker", "u64"), ("one", "split"),
                                       ("one", "u64"), ("all", "split")])
def test_world2_frames(oracle, offset, part, keys, monkeypatch):
    """Two processes sharing the GPU over the host transport: trace (each
    rank half the eye rays) and trace_frame on `mixed`, under OWNER_CHECKER
    also trace_camera of both cameras and trace_frame on their eye rays; with
    every domain resident on both ranks ("all", the owner map OWNER_CHECKER's)
    trace_image of both cameras, the footprint cull on and off (the packed
    gather of the footprints' pixels against the gather of whole bands).
    keys "u64": the PT frames with the 64-bit key MIN.  The cross-rank exact
    t ties, counted from the oracle, are among the merged records (which
    compare equal to the reference's)."""
    var = RC.variant(oracle, offset)
    jobs = list(W2_JOBS)
    if keys == "u64":
        monkeypatch.setenv("SPRAY_INSITU_SPLIT_KEYS", "0")
        jobs = [j for j in jobs if j[0] == "frame-pt1"]
    if part == "checker":
        jobs += W2_CAMERA_JOBS
    if part == "all":
        jobs = W2_IMAGE_JOBS
    res = spawned(2, offset, part, jobs)
    for job in jobs:
        label, source = job[0], job[1]
        same_collectives([(None, None, None, r[label][3]) for r in res])
        got, ref = check(oracle, var, offset, job, res)
        if job[3] in ("frame", "camera"):  # the whole film on rank 0
            assert not res[1][label][2].any() and res[0][label][2].any(), label
            assert all(r[label][3]["exchanges"] == 0 for r in res), label
            ops = [op for op, _, _ in res[0][label][3]["clog"]]
            if job[2] == "pt1":
                assert ("allreduce_min_u64" in ops) == (keys == "u64"), (label, ops)
        if job[3] == "image":  # each rank its own rows, shaded there
            assert all(len(r[label][0]["samid"]) > 300 for r in res), label
            for r in res:
                assert r[label][3]["exchanges"] == 0 and r[label][3]["host_count_reads"] == 0
        elif part == "one":  # rank 0 holds rays only
            assert len(res[0][label][0]["samid"]) == 0 and len(res[1][label][0]["samid"]) == len(ref)
            if job[3] == "trace":
                assert res[0][label][3]["bytes_sent"] > 0
        else:
            assert all(len(r[label][0]["samid"]) > 300 for r in res), label
            fi = inputs_of(oracle, var, offset, source)
            ties = RC.cross_rank_ties(oracle, var, RC.OWNER_CHECKER, fi["org"], fi["dir"])
            if source == "mixed":
                assert len(ties) >= 50  # measured: 110 / 95
            assert all((0, int(fi["sam"][i])) in got for i in ties), label
    for c in sorted(CAMERAS) if part == "all" else ():  # the cull decides no pixel
        for r in range(2):
            a, b = res[r]["image-" + c], res[r]["whole-" + c]
            assert H.records_dict(a[0]) == H.records_dict(b[0]) and a[1] == b[1], (c, r)
            np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    for c in sorted(CAMERAS) if part == "checker" else ():  # the camera frame: trace_frame's
        cam, frame = [[H.records_dict(r[how + "-" + c][0]) for r in res] for how in ("camera", "frame")]
        assert cam == frame, c
        np.testing.assert_allclose(res[0]["camera-" + c][2], res[0]["frame-" + c][2], rtol=1e-5,
                                   atol=1e-6)


@OFFSETS
def test_keyed_hit_and_route_of_a_rank(oracle, offset):
    """intersect_scene_keyed and route of a context that holds rank r's
    domains under OWNER_CHECKER against the CPU rule (OracleLocal: the
    oracle's hit within the record's own extents, the list position from the
    domain query, which ignores them), every class and `mixed`, `mixed` at
    ragged lengths too."""
    import spray_amd
    var = RC.variant(oracle, offset)
    meshes = (var["meshes"], var["boxes"], var["colors"], var["normals"])
    for rank in (0, 1):
        ref = H.OracleLocal(oracle, RC.OWNER_CHECKER, rank, meshes=meshes)
        rt = rank_context(spray_amd, var, RC.OWNER_CHECKER, rank)
        seen = set()
        for name in NAMES:
            c = var["classes"][name]
            host = spray_amd.make_rays(c["org"], c["dir"], c["tnear"], c["tfar"])
            cpu = torch.from_numpy(host.view(np.float32).reshape(-1, 8).copy())
            rh, rk = ref.intersect_keyed(cpu, extents=True)
            rm = ref.route(cpu)
            for n in (RAGGED if name == "mixed" else ()) + (len(host),):
                rays = cpu[:n].contiguous().cuda()
                m = torch.full((n,), -7, dtype=torch.int64, device="cuda")
                hits = torch.full((n, 12), float("nan"), dtype=torch.float32, device="cuda")
                keys = torch.full((n,), -7, dtype=torch.int64, device="cuda")
                rt.route(rays, m)
                rt.intersect_scene_keyed(rays, hits, keys)
                rt.sync()
                assert (m.cpu() == rm[:n]).all(), (name, rank, n, "route")
                bad = np.flatnonzero((keys.cpu() != rk[:n]).numpy())
                assert len(bad) == 0, (name, rank, n, "keys", len(bad), bad[:8])
                assert hits.cpu().numpy().tobytes() == rh[:n].numpy().tobytes(), (name, rank, n)
            seen |= set(np.unique(rm.numpy()).tolist())
            k = rk.numpy()
            assert 0 < (k != H.MISS_KEY).sum() < len(k), name
            if name == "mixed":  # list positions beyond the first decide too
                assert (((k[k != H.MISS_KEY] >> 16) & 0xFFFF) > 0).sum() > 100
        assert seen == {0, 1, 2, 3}
        rt.close()


CAM_JOBS = [(how + "-" + c, c, "pt1", kind, env) for c in sorted(CAMERAS) for how, kind, env in
            (("camera", "camera", {}), ("camrep", "camera", REP), ("image", "image", {}),
             ("whole", "image", {"SPRAY_IMAGE_CULL": "0"}), ("frame", "frame", {}),
             ("rep", "frame", REP))]


@OFFSETS
def test_camera_and_image_frames_world1(oracle, offset):
    """trace_camera (the image frame at world 1, and the replicated camera
    steps) and trace_image (the eye rays of the boxes' footprints only, and
    the bands whole) at 64 x 64 x 2, PT 1 bounce, with the eye in the plane
    the touching boxes share and inside a domain's box: the records, totals
    and image of trace_frame on the same camera's eye rays and of the
    whole-scene reference frame; the image frame bit-equal with the footprint
    cull on and off (the footprints are conservative at 1e4 too)."""
    var = RC.variant(oracle, offset)
    res = run_jobs(0, 1, offset, "all", CAM_JOBS)
    for job in CAM_JOBS:
        check(oracle, var, offset, job, [res])
    for c in sorted(CAMERAS):
        frame = res["frame-" + c]
        for how in ("camera", "camrep", "image", "whole", "rep"):
            r = res[how + "-" + c]
            assert H.records_dict(r[0]) == H.records_dict(frame[0]), (how, c)
            assert r[1] == frame[1], (how, c)
            np.testing.assert_allclose(r[2], frame[2], rtol=1e-5, atol=1e-6, err_msg=how + c)
        np.testing.assert_array_equal(res["image-" + c][2].view(np.uint32),
                                      res["whole-" + c][2].view(np.uint32))
        # the all-local frame's film on stored eye rays: the image frame's bits
        np.testing.assert_array_equal(res["image-" + c][2].view(np.uint32),
                                      frame[2].view(np.uint32))

"""The in-situ engine's camera, image and film frames off the square,
spp-divides-64 grid: 90x50 and 50x90 images of the bench camera (widths and
heights that are no multiple of 4 or of 64, rows that the ranks and bands do
not divide), spp 1, 3, 4, 16, 32 and 64.  What turns (x, y, sample) into
addresses is what goes wrong there: the RGB pack / unpack and the band copies
of the image frame's gather, the rows of a band, the footprint rows of the
camera frame, the film's pixel runs across wave edges.

Everything is compared with the whole-scene oracle at the same (w, h, spp):
records bit for bit, totals exactly, the image within the summation-order
tolerance.  That tolerance (rtol 1e-5, atol 1e-6) is derived, not tuned: both
sides add a pixel's n = spp x shadow-slots non-negative terms in different
orders, each result within (n - 1) 2^-24 relative of the exact sum, so they
differ by at most 2 (n - 1) 2^-24 -- below 1e-5 while n <= 64, which every
case here keeps (PT with one light up to spp 64, AO with 4 samples at spp 3).
The gather itself is a copy and is checked without any tolerance."""
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

import insitu_helpers as H
import test_gpu_insitu as T
from conftest import SCENES, WAVELETS64

pytestmark = pytest.mark.gpu

WIDE = (90, 50)
TALL = (50, 90)
NAMES = {WIDE: "wide", TALL: "tall"}
LIGHT1 = [(0, 0.0, 500.0, 1000.0, 1.0, 1.0, 1.0)]
ERR_ARG = -1  # SPRAY_RT_ERR_ARG


def pt1(shape, spp):
    return ("pt", 1, 1, shape, spp, LIGHT1)


def ao4(shape, spp):
    return ("ao", 1, 4, shape, spp, LIGHT1)


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


def band_rows(h, world, bands, rank):
    """The rows of rank's bands: band b = rows [b h / bt, (b + 1) h / bt)."""
    bt = world * bands
    rows = np.zeros(h, bool)
    for b in range(rank, bt, world):
        rows[b * h // bt:(b + 1) * h // bt] = True
    return rows


@pytest.fixture(scope="module")
def coverage(oracle):
    """Per shape, on the CPU: U (the union of the 64 boxes' footprints) and
    the pixels whose spp-1 eye ray hits, as [h, w] masks.  Recorded:
        shape  |U| / pixels  rows x columns of U  hit pixels  hits outside U
        90x50  1146 / 4500   40 x 43              680         0
        50x90  2685 / 4500   68 x 50              2073        0
    so the cull removes pixels at both shapes and U's rows and columns
    differ in count."""
    from spray_amd import insitu
    sc, doms, _ = oracle.load_scene(WAVELETS64, SCENES)
    boxes = np.array([dm["world_bound"] for dm in doms], np.float32)
    c = H.BENCH_CAMERA
    out = {}
    for w, h in (WIDE, TALL):
        cam = oracle.camera_init(c["pos"], c["lookat"], c["up"], c["fov"], w, h)
        U = np.zeros((h, w), bool)
        for b in boxes:
            kind, x0, x1 = insitu.box_rows(cam, w, h, b)
            assert kind == 1
            for y in np.flatnonzero(x0 <= x1):
                U[y, x0[y]:x1[y] + 1] = True
        org, d, pix, _ = oracle.eye_rays_insitu(cam, w, 1, (0, 0, w, h), (0, 0, w, h))
        hits, _ = sc.intersect(np.ascontiguousarray(org), np.ascontiguousarray(d))
        hit = np.zeros(w * h, bool)
        hit[pix[hits["domain"] >= 0]] = True
        hit = hit.reshape(h, w)
        assert 0 < U.sum() < w * h
        assert U.any(1).sum() != U.any(0).sum()
        assert hit.sum() > 500 and not (hit & ~U).any()
        out[(w, h)] = (U, hit)
    return out


_REFS = {}


def reference(oracle, spec):
    """(records, image, totals) of the whole-scene oracle, computed once."""
    key = (spec[0], spec[2], spec[3], spec[4])
    if key not in _REFS:
        _REFS[key] = T._image_reference(oracle, spec)
    return _REFS[key]


# ---- B: eye rays of a stripe off the origin ----
@pytest.mark.parametrize("shape,block,stripe", [(WIDE, (7, 5, 71, 40), (19, 13, 40, 17)),
                                                (TALL, (5, 7, 40, 71), (11, 23, 27, 31))],
                         ids=["wide", "tall"])
def test_eye_rays_insitu_off_origin(spray, oracle, shape, block, stripe):
    """A blocking tile and a stripe that start off the origin and are
    narrower than the image (and the stripe than the tile): rays, pixel ids
    (image_w y + x) and sample ids (tile-relative) equal the oracle's bit
    for bit, at spp 1 (pixel corners) and spp 3 (jittered)."""
    w, h = shape
    c = H.BENCH_CAMERA
    cam = oracle.camera_init(c["pos"], c["lookat"], c["up"], c["fov"], w, h)
    rt = spray.RtContext(0)
    for spp in (1, 3):
        org, d, pix, sam = oracle.eye_rays_insitu(cam, w, spp, block, stripe)
        n = len(org)
        assert n == stripe[2] * stripe[3] * spp
        rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        p = torch.empty(n, dtype=torch.int32, device="cuda")
        s = torch.empty(n, dtype=torch.int32, device="cuda")
        rt.eye_rays_insitu(cam, w, spp, block, stripe, rays, p, s)
        rt.sync()
        r = rays.cpu().numpy()
        assert r[:, 0:3].tobytes() == np.ascontiguousarray(org).tobytes()
        assert r[:, 4:7].tobytes() == np.ascontiguousarray(d).tobytes()
        assert (p.cpu().numpy() == pix).all() and (s.cpu().numpy() == sam).all()
        # the ids are the stripe's: its pixels of the image, its slots of the tile
        assert pix.min() == w * stripe[1] + stripe[0]
        assert pix.max() == w * (stripe[1] + stripe[3] - 1) + stripe[0] + stripe[2] - 1
        assert sam.max() < block[2] * block[3] * spp
    rt.close()


# ---- C: the image-parallel frame ----
def _image_rank_main(rank, world, port, out, spec, bands, envs):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        res = []
        for env in envs:  # SPRAY_IMAGE_CULL of each frame (None: unset)
            os.environ.pop("SPRAY_IMAGE_CULL", None)
            if env is not None:
                os.environ["SPRAY_IMAGE_CULL"] = env
            res.append(T._image_frame(rank, world, spec, "host", dist, bands))
        with open(os.path.join(out, "r%d.pkl" % rank), "wb") as fh:
            pickle.dump(res, fh)
    finally:
        dist.destroy_process_group()


def _image_frames(world, bands, spec, envs=(None,)):
    """[frame of envs[k]][rank] -> (records, totals, image, stats)."""
    if world == 1:
        per_rank = [[]]
        for env in envs:
            os.environ.pop("SPRAY_IMAGE_CULL", None)
            if env is not None:
                os.environ["SPRAY_IMAGE_CULL"] = env
            try:
                per_rank[0].append(T._image_frame(0, 1, spec, "rccl", None, bands))
            finally:
                os.environ.pop("SPRAY_IMAGE_CULL", None)
    else:
        assert world <= 4
        with tempfile.TemporaryDirectory() as out:
            torch.multiprocessing.spawn(_image_rank_main,
                                        args=(world, T._rendezvous_file(), out, spec, bands,
                                              tuple(envs)), nprocs=world)
            per_rank = []
            for r in range(world):
                with open(os.path.join(out, "r%d.pkl" % r), "rb") as fh:
                    per_rank.append(pickle.load(fh))
    return [[per_rank[r][k] for r in range(world)] for k in range(len(envs))]


def _check_image_frame(oracle, coverage, world, bands, spec, res, culled):
    """What every image frame must satisfy; culled: the frame launched U's
    eye rays only (else its bands whole)."""
    w, h = spec[3]
    spp = spec[4]
    U, hit = coverage[(w, h)]
    rows = [band_rows(h, world, bands, r) for r in range(world)]
    assert np.sum(rows, axis=0).tolist() == [1] * h  # the bands tile the rows
    for r in range(world):  # (CPU) every rank's rows hold some hit
        assert hit[rows[r]].any(), r
    if world > 1:
        log = T.same_collectives(res)
        assert [op for op, _, _ in log] == ["alltoallv_u8", "allreduce_sum_u64"], log
    ref, ref_img, ref_tot = reference(oracle, spec)
    merged = []
    for recs, tot, _, st in res:
        assert tot == ref_tot
        assert st["exchanges"] == 0 and st["host_count_reads"] == 0 and st["traces"] == 1
        merged += [(b, s) + v for (b, s), v in H.records_dict(recs).items()]
    assert len(merged) == len({(m[0], m[1]) for m in merged})  # shaded once
    H.compare_records(H.records_dict(merged), ref)
    # the gather is a copy: no tolerance
    im0 = res[0][2].reshape(h, w, 4).view(np.uint32)
    for r in range(1, world):
        im = res[r][2].reshape(h, w, 4).view(np.uint32)
        assert im[rows[r]].any(), r
        np.testing.assert_array_equal(im0[rows[r]], im[rows[r]])
        assert not im[~rows[r]].any(), r
    # the gather's bytes: the RGB of the rank's U pixels, or its rows whole
    recv = 0
    for r in range(1, world):
        want = int(U[rows[r]].sum()) * 12 if culled else int(rows[r].sum()) * w * 16
        assert res[r][3]["bytes_sent"] == want, (r, res[r][3]["bytes_sent"], want)
        assert res[r][3]["bytes_received"] == 0
        recv += want
    assert res[0][3]["bytes_sent"] == 0 and res[0][3]["bytes_received"] == recv
    assert (ref_img > 0).sum() > 500
    np.testing.assert_allclose(res[0][2], ref_img, rtol=1e-5, atol=1e-6)


_ONE = {}


def one_rank_frame(spec):
    """The one-rank all-local frame on the whole image's stored eye rays."""
    key = (spec[0], spec[2], spec[3], spec[4])
    if key not in _ONE:
        _ONE[key] = T._image_frame(0, 1, spec, "rccl", how="rays")[2]
    return _ONE[key]


IMAGE_CASES = [  # (world, bands, spec): the path the case is there for
    (1, 1, pt1(WIDE, 1)),    # 1: every lane its own run; cull on
    (1, 2, pt1(TALL, 64)),   # 2: a pixel fills a wave
    (1, 1, ao4(TALL, 3)),    # 3: whole bands without the environment override
    (2, 5, pt1(WIDE, 3)),    # 4: band pack + unpack, 10 bands of 5 rows
    (3, 5, pt1(TALL, 3)),    # 5: band unpack from ranks 1 and 2, 6-row bands
    (3, 1, pt1(WIDE, 3)),    # 6: direct gather, rows 16 / 17 / 17
    (4, 1, ao4(TALL, 3)),    # 7: direct gather, rows 22 / 23 / 22 / 23
    (2, 3, pt1(WIDE, 16)),   # 8: cull, interleaved bands of 8 / 9 rows
    (4, 2, pt1(TALL, 32)),   # 9: the same at world 4 (11 / 12 rows), w 50
]


def _case_id(p):
    world, bands, spec = p
    return "w%d-b%d-%s-%s-spp%d" % (world, bands, NAMES[spec[3]], spec[0], spec[4])


@pytest.mark.parametrize("world,bands,spec", IMAGE_CASES, ids=[_case_id(p) for p in IMAGE_CASES])
def test_image_frame_shapes(oracle, coverage, world, bands, spec):
    """spray_rt_insitu_trace_image at 90x50 / 50x90.  spp | 64: U's eye rays
    only, and rank 0's image bit-equal to the one-rank frame on stored eye
    rays.  Other spp: the bands traced whole (pixel runs cross wave edges at
    other places than in the one-rank frame, so no bit claim against it) --
    the gather moves whole rows, rows x w x 16 bytes per rank."""
    spp = spec[4]
    culled = 64 % spp == 0
    res = _image_frames(world, bands, spec)[0]
    _check_image_frame(oracle, coverage, world, bands, spec, res, culled)
    if culled:
        one = one_rank_frame(spec)
        assert (one > 0).sum() > 500
        np.testing.assert_array_equal(res[0][2].view(np.uint32), one.view(np.uint32))


def test_image_frame_whole_bands_equal_culled(oracle, coverage):
    """Case 10: world 2 x bands 3 at 50x90 (15-row bands), spp 4, the bands
    traced whole (SPRAY_IMAGE_CULL=0: the band pack / unpack) and culled (the
    RGB pack / unpack): image bits, records and totals equal on both ranks,
    and rank 0's equal to the one-rank frame's."""
    spec = pt1(TALL, 4)
    whole, culled = _image_frames(2, 3, spec, envs=("0", None))
    _check_image_frame(oracle, coverage, 2, 3, spec, whole, False)
    _check_image_frame(oracle, coverage, 2, 3, spec, culled, True)
    for r in range(2):
        assert whole[r][1] == culled[r][1]
        np.testing.assert_array_equal(whole[r][2].view(np.uint32), culled[r][2].view(np.uint32))
        assert H.records_dict(whole[r][0]) == H.records_dict(culled[r][0])
        assert len(whole[r][0]["samid"]) > 500
    one = one_rank_frame(spec)
    np.testing.assert_array_equal(whole[0][2].view(np.uint32), one.view(np.uint32))


# ---- E: unequal interleaved bands traced whole are refused up front ----
def _reject_rank_main(rank, world, port, out, spec, bands):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist
    import spray_amd
    from spray_amd import insitu
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        kind, bounces, samples, (w, h), spp, lights = spec
        c = H.BENCH_CAMERA
        cam = spray_amd.camera_init(c["pos"], c["lookat"], c["up"], c["fov"], w, h)
        rt = spray_amd.RtContext(0)
        nd = len(spray_amd.engine.host_parse_scene(WAVELETS64, SCENES)[0])
        insitu.setup_rank_context(rt, WAVELETS64, SCENES, np.full(nd, rank, np.int32), rank)
        rt.set_bsdfs(spray_amd.engine.host_scene_bsdfs(WAVELETS64))
        rt.set_stream(torch.cuda.current_stream())
        sh = spray_amd.frame.make_shader(kind, bounces, samples, lights=lights)
        eng = insitu.InsituEngine(rt, world, rank, dist=dist, transport="host")
        image = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
        eng.collective_log()
        code, msg = 0, ""
        try:
            eng.trace_image(sh, cam, w, h, spp, image, bands)
        except spray_amd.SprayRtError as e:
            code, msg = e.code, str(e)
        torch.cuda.synchronize()
        res = (code, msg, bool(image.any()), eng.collective_log(), eng.stats())
        eng.close()
        rt.close()
        with open(os.path.join(out, "r%d.pkl" % rank), "wb") as fh:
            pickle.dump(res, fh)
    finally:
        dist.destroy_process_group()


def test_image_frame_unequal_whole_bands_rejected_up_front():
    """World 2 x bands 3 over 50 rows at spp 3: the bands are traced whole
    and 6 does not divide 50, which the band copies cannot gather.  Both
    ranks refuse with ERR_ARG before anything is launched: the images still
    zero, no collective logged, nothing traced or sent.  (Under the cull the
    same split is accepted: test_image_frame_shapes, w2-b3 and w4-b2.)"""
    with tempfile.TemporaryDirectory() as out:
        torch.multiprocessing.spawn(_reject_rank_main,
                                    args=(2, T._rendezvous_file(), out, pt1(WIDE, 3), 3), nprocs=2)
        res = []
        for r in range(2):
            with open(os.path.join(out, "r%d.pkl" % r), "rb") as fh:
                res.append(pickle.load(fh))
    for code, msg, touched, log, st in res:
        assert code == ERR_ARG and "interleaved bands" in msg, (code, msg)
        assert not touched
        assert log == []
        assert st["traces"] == 0 and st["bytes_sent"] == 0, st


# ---- D: the camera frame (per-rank footprints) ----
def _camera_rank_main(rank, world, port, out, case, mode):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        res = [T._engine_rank(rank, world, case, "host", dist, False, rep, mode)
               for rep in ("camera", True)]
        with open(os.path.join(out, "r%d.pkl" % rank), "wb") as fh:
            pickle.dump(res, fh)
    finally:
        dist.destroy_process_group()


def _merged(results):
    out = []
    for r in results:
        out += [(b, s) + v for (b, s), v in H.records_dict(r[0]).items()]
    return H.records_dict(out)


@pytest.mark.parametrize("shape", [WIDE, TALL], ids=["wide", "tall"])
@pytest.mark.parametrize("world,mode,kind,samples", [(2, T.VIEW, "pt", 1), (3, 0, "pt", 1),
                                                     (2, T.VIEW, "ao", 4)])
def test_camera_frame_shapes(oracle, world, mode, kind, samples, shape):
    """spray_rt_insitu_trace_camera at 90x50 / 50x90, spp 2: records bit-exact
    and totals exact against the oracle, rank 0's image within the
    tolerance, and the records equal to spray_rt_insitu_trace_frame's on the
    same camera's stored eye rays."""
    case = (kind, 1, samples, shape, 2)
    with tempfile.TemporaryDirectory() as out:
        torch.multiprocessing.spawn(_camera_rank_main,
                                    args=(world, T._rendezvous_file(), out, case, mode),
                                    nprocs=world)
        res = []
        for r in range(world):
            with open(os.path.join(out, "r%d.pkl" % r), "rb") as fh:
                res.append(pickle.load(fh))
    cam = [r[0] for r in res]
    frm = [r[1] for r in res]
    T._check(oracle, case, cam)
    T._check(oracle, case, frm)
    assert _merged(cam) == _merged(frm)
    assert sum(len(r[0]["samid"]) > 50 for r in cam) >= 2
    for r in cam:
        assert r[3]["exchanges"] == 0 and r[3]["host_count_reads"] == 0
    assert all(not r[2].any() for r in cam[1:]) and cam[0][2].any()


@pytest.mark.parametrize("shape", [WIDE, TALL], ids=["wide", "tall"])
@pytest.mark.parametrize("kind,samples", [("pt", 1), ("ao", 4)])
def test_camera_steps_one_rank_rccl_shapes(oracle, kind, samples, shape, monkeypatch):
    """World 1 with the replicated steps forced through a one-rank RCCL
    communicator (SPRAY_INSITU_REPLICATED=1), as the multi-GPU run calls
    them."""
    case = (kind, 1, samples, shape, 2)
    monkeypatch.setenv("SPRAY_INSITU_REPLICATED", "1")
    cam = T._engine_rank(0, 1, case, "rccl", replicated="camera")
    frm = T._engine_rank(0, 1, case, "rccl", replicated=True)
    T._check(oracle, case, [cam])
    T._check(oracle, case, [frm])
    assert _merged([cam]) == _merged([frm])
    assert cam[3]["collectives"] >= 6 and cam[3]["exchanges"] == 0, cam[3]

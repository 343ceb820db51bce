"""The in-situ winner rule and the frame restatement on the hard ray classes of
ray_cases.py, on the CPU: before any kernel is judged by the rule "minimum
over the ranks of (t bits, list position, domain)", it is pinned here against
the whole-scene oracle on the nine-domain scene of touching boxes and
coincident triangles -- axis-parallel and signed-zero directions, rays in
lattice planes, origins on surfaces and edges, at the origin and at 1e4.

  * the keyed minimum over the two ranks of OWNER_CHECKER (every x and z pair
    of domains that shares coincident triangles is split) is the whole-scene
    oracle's hit record byte for byte, and the miss key exactly on misses;
  * the protocol and the replicated frames of oracle/insitu_ref.py over "gloo"
    at world 2, under both partitions, give the whole-scene reference frame's
    records, totals and image on the `mixed` class as eye rays.

The engine runs the same cases in test_gpu_insitu_ray_cases.py."""
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

import insitu_helpers as H
import ray_cases as RC
from test_insitu import _rendezvous_file

OFFSETS = pytest.mark.parametrize("offset", (0.0, RC.LARGE), ids=["origin", "large"])
PARTITIONS = {"checker": RC.OWNER_CHECKER, "one": RC.OWNER_ONE}
# (frame, shading case): the replicated frames are one bounce
FRAMES = (("trace", "pt1"), ("trace", "pt3"), ("trace", "ao4"),
          ("replicated", "pt1"), ("replicated", "ao4"))


def var_meshes(var):
    return (var["meshes"], var["boxes"], var["colors"], var["normals"])


@OFFSETS
def test_keyed_minimum_over_ranks_is_the_scene_hit(oracle, offset):
    var = RC.variant(oracle, offset)
    locs = [H.OracleLocal(oracle, RC.OWNER_CHECKER, r, meshes=var_meshes(var)) for r in (0, 1)]
    owner = np.asarray(RC.OWNER_CHECKER)
    ties = {}
    for name in RC.CLASSES + ("mixed", "nonfinite"):
        c = var["classes"][name]
        rays = H.rays_tensor(c["org"], c["dir"])  # the default extents
        ref, _ = var["osc"].intersect(c["org"], c["dir"])
        hk = [loc.intersect_keyed(rays) for loc in locs]
        keys = np.stack([k.numpy() for _, k in hk])
        hits = [np.ascontiguousarray(h.numpy()).view(oracle.HIT_DTYPE).reshape(-1) for h, _ in hk]
        best = keys.min(0)
        miss = ref["domain"] < 0
        assert ((best == H.MISS_KEY) == miss).all(), name
        win = keys.argmin(0)
        got = hits[0].copy()
        got[win == 1] = hits[1][win == 1]
        diff = got.view(np.uint8).reshape(len(got), -1) != ref.view(np.uint8).reshape(len(ref), -1)
        bad = np.flatnonzero(~miss & diff.any(1))
        assert len(bad) == 0, (name, len(bad), bad[:8])
        # the key restates the record: t bits, domain, and the winner's rank owns it
        assert ((best[~miss] >> 32) == ref["t"][~miss].view(np.uint32)).all(), name
        assert ((best[~miss] & 0xFFFF) == ref["domain"][~miss]).all(), name
        assert (owner[ref["domain"][~miss]] == win[~miss]).all(), name
        # a rank that misses leaves the miss record's domain
        for r in (0, 1):
            assert ((keys[r] == H.MISS_KEY) == (hits[r]["domain"] < 0)).all(), (name, r)
        both = (keys[0] != H.MISS_KEY) & (keys[1] != H.MISS_KEY)
        ties[name] = int((both & ((keys[0] >> 32) == (keys[1] >> 32))).sum())
        # routing masks: the owners of the domain query's lists
        ids, _, cnt, _ = oracle.domain_query(c["org"], c["dir"], var["boxes"], RC.NDOM)
        listed = np.arange(RC.NDOM)[None, :] < cnt[:, None]
        want = np.zeros(len(ids), np.int64)
        for r in (0, 1):
            want |= ((listed & (owner[np.maximum(ids, 0)] == r)).any(1).astype(np.int64)) << r
        for loc in locs:
            assert (loc.route(rays).numpy() == want).all(), name
        if name == "mixed":
            assert set(np.unique(want).tolist()) == {0, 1, 2, 3}
    # what keeps the comparison from being vacuous (measured: 110 / 95 ties)
    assert ties["mixed"] >= 50, ties
    assert ties["mixed"] == len(RC.cross_rank_ties(oracle, var, RC.OWNER_CHECKER,
                                                   var["classes"]["mixed"]["org"],
                                                   var["classes"]["mixed"]["dir"]))
    assert ties["axis_lattice"] > 0 and ties["surface"] > 0, ties
    d = var["classes"]["mixed"]["dir"]
    assert ((d == 0).any(1)).sum() >= 2000  # measured: 2048
    for name in ("axis_off", "axis_lattice"):
        assert (var["classes"][name]["dir"] == 0).any(1).all()


def _rank_main(rank, world, port, out, offset, owner):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    from oracle import insitu_ref, pyoracle as po
    dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world)
    try:
        var = RC.variant(po, offset)
        local = H.OracleLocal(po, owner, rank, meshes=var_meshes(var))
        fi = RC.frame_inputs(var, "mixed")
        n = len(fi["org"])
        comm = insitu_ref.Comm(dist)
        res = {}
        for frame, case in FRAMES:
            sh = RC.frame_shader(po.shader, offset, case)
            image = np.zeros(fi["w"] * fi["h"] * 4, np.float32)
            if frame == "trace":  # each rank its half of the eye rays (whole pixels)
                lo, hi = (0, n // 2) if rank == 0 else (n // 2, n)
                fn = insitu_ref.trace_frame
            else:
                lo, hi = 0, n
                fn = insitu_ref.trace_frame_replicated
            recs, tot = fn(po, local, comm, sh, list(RC.BSDFS), fi["org"][lo:hi], fi["dir"][lo:hi],
                           fi["pix"][lo:hi], fi["sam"][lo:hi], fi["spp"], image)
            res[(frame, case)] = (recs, tot, image)
        with open(os.path.join(out, "r%d.pkl" % rank), "wb") as fh:
            pickle.dump(res, fh)
    finally:
        dist.destroy_process_group()


@OFFSETS
@pytest.mark.parametrize("part", sorted(PARTITIONS))
def test_restated_frames_match_the_scene_frame(oracle, offset, part):
    """oracle/insitu_ref.py's trace_frame (PT 1 bounce, PT 3 bounces x 2
    samples, AO 4 samples), trace_frame_replicated (PT) and the replicated AO
    frame over "gloo" at world 2 on frame_inputs("mixed"): the whole-scene
    reference frame's records bit for bit, its totals, and its image within
    the film's summation order."""
    var = RC.variant(oracle, offset)
    owner = PARTITIONS[part]
    with tempfile.TemporaryDirectory() as out:
        torch.multiprocessing.spawn(_rank_main, args=(2, _rendezvous_file(), out, offset, owner),
                                    nprocs=2)
        res = []
        for r in range(2):
            with open(os.path.join(out, "r%d.pkl" % r), "rb") as fh:
                res.append(pickle.load(fh))
    for frame, case in FRAMES:
        ref, ref_img, ref_tot = RC.frame_reference(oracle, var, offset, "mixed", case)
        got = H.records_dict([x for r in res for x in r[(frame, case)][0]])
        H.compare_records(got, ref)
        for r in res:
            assert r[(frame, case)][1] == ref_tot, (frame, case)
        total = np.sum([r[(frame, case)][2] for r in res], axis=0)
        assert (ref_img > 0).sum() > 500
        np.testing.assert_allclose(total, ref_img, rtol=1e-5, atol=1e-6)
        if part == "one":  # rank 0 holds rays only: it wins (and records) nothing
            assert not res[0][(frame, case)][0] and len(res[1][(frame, case)][0]) == len(ref)
        else:
            assert all(len(r[(frame, case)][0]) > 1000 for r in res)
        if frame == "replicated":  # the whole film on rank 0
            assert not res[1][(frame, case)][2].any()
        # not vacuous: bounce 0 spawns and occludes, the later bounces stay populated
        hits, shadows, occluded = RC.bounce_counts(ref, 0)
        assert hits > 3000 and shadows > 3000 and occluded > 1500, (case, hits, shadows, occluded)
        if case == "pt3":
            assert RC.bounce_counts(ref, 2)[0] > 1000

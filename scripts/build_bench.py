#!/usr/bin/env python
"""Per-time-step geometry of new topology on wavelets64 (64 domains x 5,480
triangles): the device build against the uploads it replaces.

    python scripts/build_bench.py [--runs 20] [--warmup 3]

Timed, each a median of --runs runs after --warmup, by HIP events on the
context's stream and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_build of all 64 slots from device pointers;
  (b) 64 spray_rt_domain_upload calls of the same meshes from host arrays (a
      binned-SAH build on one host thread plus the copy, per domain);
  (c) the fused spray_rt_intersect_scene_shadow_pt launch of the bench camera
      (1024 x 1024 x 8 spp) on the device-built and on the uploaded trees, with
      the mean spray_rt_slot_sah of both sets of trees.
The hits, shadow flags and occlusion bytes of (c) must be identical on both
sets of trees, and (a) must be faster than (b).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SCENE = os.path.join(SCENES, "wavelets64.spray")
CAM = dict(pos=[90.172180, 84.141418, 82.480225], lookat=[30.0, 28.649426, 30.0],
           up=[0.0, 1.0, 0.0], fov=90.0)
W = H = 1024
SPP = 8
TILE_H = 128
SHADE = [0.0, 500.0, 1000.0, 1.0, 1.0, 1.0, 0.4, 0.4, 0.4, 10.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    runs = max(args.runs, 20)

    import torch
    import spray_amd
    from spray_amd.engine import host_domain_mesh, host_parse_scene

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    boxes, _ = host_parse_scene(SCENE, SCENES)
    nd = len(boxes)
    meshes = [host_domain_mesh(SCENE, SCENES, i) for i in range(nd)]
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
    slots = list(range(nd))

    def to_dev(x):  # uint32 arrays travel as their int32 bits
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)

    dcols = [[to_dev(m[k]) for m in meshes] for k in range(4)]
    dbounds = torch.empty((nd, 6), dtype=torch.float32, device=dev)

    def build_all():
        rt.build_domains(slots, *dcols, bounds=dbounds)

    def upload_all():
        for i, (v, f, c, n) in enumerate(meshes):
            rt.upload_domain(i, v, f, c, n)

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        rt.sync()
        wall = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), wall

    def median_of(fn):
        for _ in range(args.warmup):
            fn()
        t = [timed(fn) for _ in range(runs)]
        return (statistics.median(x[0] for x in t), statistics.median(x[1] for x in t))

    a_ev, a_wall = median_of(build_all)   # (a) one build of all slots, device pointers
    b_ev, b_wall = median_of(upload_all)  # (b) 64 uploads of the same meshes

    # ---- (c) the fused frame launch on device-built and on uploaded trees
    cam = spray_amd.camera_init(CAM["pos"], CAM["lookat"], CAM["up"], CAM["fov"], W, H)
    n = W * H * SPP
    per = W * TILE_H * SPP
    prim = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    hits = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    nsh = torch.zeros(1, dtype=torch.int32, device=dev)
    rt.set_coherence(rt.RAYS_COHERENT)

    def trace():
        rt.intersect_scene_shadow_pt(prim, hits, SHADE, occ, valid, nsh)

    def frame_on(prepare):
        prepare()
        rt.sync()
        rt.domain_bounds(dbounds.cpu().numpy())  # the build's exact boxes (same meshes in both)
        for i in slots:
            rt.map_domain(i, i)
        for k, y in enumerate(range(0, H, TILE_H)):
            rt.eye_rays_ooc(cam, W, SPP, (0, y, W, TILE_H), prim[k * per * 32:(k + 1) * per * 32])
        sah = statistics.mean(rt.slot_sah(i) for i in slots)
        nodes = sum(rt.slot_info(i)["nodes"] for i in slots)
        hits.zero_()
        occ.fill_(9)
        valid.fill_(7)
        ev, wall = median_of(trace)
        torch.cuda.synchronize()
        v = valid.cpu().numpy()
        res = (hits.cpu().numpy().tobytes(), v.tobytes(), occ.cpu().numpy()[v == 1].tobytes(),
               int(nsh.item()))
        return ev, wall, sah, res, nodes

    c_dev = frame_on(build_all)
    c_up = frame_on(upload_all)
    same = c_dev[3] == c_up[3]
    out = {
        "scene": "wavelets64", "domains": nd, "triangles": int(sum(len(m[1]) for m in meshes)),
        "runs": runs,
        "build_ms": {"events": round(a_ev, 4), "wall": round(a_wall, 4)},
        "upload64_ms": {"events": round(b_ev, 4), "wall": round(b_wall, 4)},
        "upload_over_build": {"events": round(b_ev / a_ev, 1), "wall": round(b_wall / a_wall, 1)},
        "trace_ms": {"device_built": round(c_dev[0], 4), "uploaded": round(c_up[0], 4),
                     "device_built_over_uploaded": round(c_dev[0] / c_up[0], 4)},
        "mean_slot_sah": {"device_built": round(c_dev[2], 4), "uploaded": round(c_up[2], 4)},
        "nodes": {"device_built": c_dev[4], "uploaded": c_up[4]},
        "shadow_rays": c_dev[3][3],
        "trace_results_identical": bool(same),
        "build_faster_than_uploads": bool(a_wall < b_wall and a_ev < b_ev),
    }
    print(json.dumps(out))
    rt.close()
    return 0 if same and out["build_faster_than_uploads"] else 1


if __name__ == "__main__":
    sys.exit(main())

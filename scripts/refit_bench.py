#!/usr/bin/env python
"""Per-time-step geometry update on wavelets64 (64 domains x 5,480 triangles):
the device refit against the rebuild it replaces.

    python scripts/refit_bench.py [--runs 20] [--warmup 3]

Every domain is deformed as v + 0.05 * extent * sin(k . v) (two phases, used
alternately so no run repeats the previous one's input).  Timed, each a
median of --runs runs after --warmup, by HIP events on the context's stream
and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_refit of all 64 slots from device pointers;
  (b) 64 spray_rt_domain_upload calls of the same deformed meshes from host
      arrays -- the only way to change a resident domain without the refit;
  (c) the fused spray_rt_intersect_scene_shadow_pt launch of the bench camera
      (1024 x 1024 x 8 spp) after (a) and after (b), with the mean
      spray_rt_slot_sah of both sets of trees.
The hits, shadow flags and occlusion bytes of (c) must be identical after (a)
and after (b).  Prints one JSON line.
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


def deform(v, phase):
    lo, hi = v.min(0), v.max(0)
    e = float((hi - lo).max())
    k = 2.0 * np.pi / e
    d = np.stack([np.sin(k * v[:, 1] + phase), np.sin(k * v[:, 2] + 1.0 + phase),
                  np.sin(k * v[:, 0] + 2.0 + phase)], 1)
    return (v + 0.05 * e * d).astype(np.float32)


def normals_of(v, f):
    """Area-weighted vertex normals (unnormalised), float32."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    fn = np.cross(b - a, c - a).astype(np.float32)
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    return n.astype(np.float32)


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
    # the deformed states: host arrays for (b), device tensors for (a)
    states = []
    for phase in (0.0, 1.5):
        vs = [deform(v, phase) for v, _, _, _ in meshes]
        ns = [normals_of(v1, m[1]) for v1, m in zip(vs, meshes)]
        states.append({"v": vs, "n": ns,
                       "dv": [torch.from_numpy(x).to(dev) for x in vs],
                       "dn": [torch.from_numpy(x).to(dev) for x in ns]})

    def upload_all(st):
        for i, (v, f, c, n) in enumerate(meshes):
            rt.upload_domain(i, v if st is None else st["v"][i], f, c,
                             n if st is None else st["n"][i])

    def set_bounds(b):
        rt.domain_bounds(b)
        for i in slots:
            rt.map_domain(i, i)

    upload_all(None)
    dbounds = torch.empty((nd, 6), dtype=torch.float32, device=dev)

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
        for k in range(args.warmup):
            fn(k)
        t = [timed(lambda: fn(k)) for k in range(runs)]
        return (statistics.median(x[0] for x in t), statistics.median(x[1] for x in t))

    # ---- (a) one refit of all slots, device pointers
    a_ev, a_wall = median_of(lambda k: rt.refit_domains(
        slots, states[k & 1]["dv"], states[k & 1]["dn"], bounds=dbounds))
    # ---- (b) 64 uploads of the same meshes
    b_ev, b_wall = median_of(lambda k: upload_all(states[k & 1]))

    # ---- (c) the fused frame launch on refitted and on rebuilt trees
    cam = spray_amd.camera_init(CAM["pos"], CAM["lookat"], CAM["up"], CAM["fov"], W, H)
    n = W * H * SPP
    per = W * TILE_H * SPP
    prim = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    hits = torch.empty(n * 48, dtype=torch.uint8, device=dev)
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    nsh = torch.zeros(1, dtype=torch.int32, device=dev)
    rt.set_coherence(rt.RAYS_COHERENT)
    st = states[0]

    def trace():
        rt.intersect_scene_shadow_pt(prim, hits, SHADE, occ, valid, nsh)

    def frame_on(prepare):
        prepare()
        rt.sync()
        b = dbounds.cpu().numpy()
        set_bounds(b)
        for k, y in enumerate(range(0, H, TILE_H)):
            rt.eye_rays_ooc(cam, W, SPP, (0, y, W, TILE_H), prim[k * per * 32:(k + 1) * per * 32])
        sah = statistics.mean(rt.slot_sah(i) for i in slots)
        hits.zero_()
        occ.fill_(9)
        valid.fill_(7)
        ev, wall = median_of(lambda k: trace())
        torch.cuda.synchronize()
        v = valid.cpu().numpy()
        res = (hits.cpu().numpy().tobytes(), v.tobytes(), occ.cpu().numpy()[v == 1].tobytes(),
               int(nsh.item()))
        return ev, wall, sah, res

    upload_all(None)  # the trees of the undeformed meshes, then refit them
    c_refit = frame_on(lambda: rt.refit_domains(slots, st["dv"], st["dn"], bounds=dbounds))
    c_build = frame_on(lambda: upload_all(st))  # bounds: the refit's (same vertices)
    same = c_refit[3] == c_build[3]
    out = {
        "scene": "wavelets64", "domains": nd, "triangles": int(sum(len(m[1]) for m in meshes)),
        "runs": runs,
        "refit_ms": {"events": round(a_ev, 4), "wall": round(a_wall, 4)},
        "upload64_ms": {"events": round(b_ev, 4), "wall": round(b_wall, 4)},
        "upload_over_refit": {"events": round(b_ev / a_ev, 1), "wall": round(b_wall / a_wall, 1)},
        "trace_ms": {"refitted": round(c_refit[0], 4), "rebuilt": round(c_build[0], 4),
                     "refitted_over_rebuilt": round(c_refit[0] / c_build[0], 4)},
        "mean_slot_sah": {"refitted": round(c_refit[2], 4), "rebuilt": round(c_build[2], 4)},
        "shadow_rays": c_refit[3][3],
        "trace_results_identical": bool(same),
        "refit_faster_than_uploads": bool(a_wall < b_wall and a_ev < b_ev),
    }
    print(json.dumps(out))
    rt.close()
    return 0 if same and out["refit_faster_than_uploads"] else 1


if __name__ == "__main__":
    sys.exit(main())

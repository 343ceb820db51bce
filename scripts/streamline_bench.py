#!/usr/bin/env python
"""Per-time-step streamlines of vector grids as tubes: 64 grids of 33^3 points,
each an ABC flow (A, B, C = 1, 0.8, 0.6, a phase per grid) sampled on the
lattice, 64 seeds per grid traced both ways for 10 steps of 0.125, drawn as
tubes of 6 sides with a constant colour into 64 resident slots: about a million
triangles, the scale of the other filters' benchmarks.

    python scripts/streamline_bench.py [--runs 20] [--warmup 3]

Timed, each a median of --runs runs after --warmup in the same process, by HIP
events on the context's stream and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_stream_tubes of all 64 slots from arrays in HBM, with
      its phases (spray_rt_stream_phase_times); the first phase (staging, check
      pass, count pass, scan, host read) holds the first of the two
      integrations with its overheads, so twice its time bounds the
      integrations' share of (a) from above;
  (b) spray_rt_stream_tubes_host per field, then ONE spray_rt_domains_build from
      the host arrays -- the path a caller without (a) has, given the arrays on
      the host already (no D2H is charged);
  (c) the polyline form alone with 4,096 seeds per grid, 50 steps both ways,
      into buffers allocated once, as RK4 steps (points beyond the seeds) per
      second; every step is computed twice, once by the count pass and once by
      the integrate pass.
The slots of (a) and (b) must hold the same bytes and (a) should be faster than
(b): the exit code follows the two.  Prints one JSON line.
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

N, GRIDS, SEEDS, STEPS, STEP, SIDES, RADIUS = 33, 64, 64, 10, 0.125, 6, 0.05
LINE_SEEDS, LINE_STEPS = 4096, 50
COLOR = 0x00C08040


def abc(n, phase):
    ax = 2.0 * np.pi * np.arange(n) / (n - 1) + phase
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return np.stack([np.sin(z) + 0.6 * np.cos(y), 0.8 * np.sin(x) + np.cos(z),
                     0.6 * np.sin(y) + 0.8 * np.cos(x)], -1).astype(np.float32)


def seeds(n, k):
    rng = np.random.default_rng(1000 + k)
    return rng.uniform(4.0, N - 5.0, (n, 3)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    runs = max(args.runs, 20)

    import torch
    import spray_amd

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    host_fields = [dict(vectors=abc(N, 0.37 * k), origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0),
                        seeds=seeds(SEEDS, k), step=STEP, max_steps=STEPS,
                        direction=spray_amd.STREAM_BOTH, min_speed=1e-6) for k in range(GRIDS)]
    put = lambda x: torch.from_numpy(x).to(dev)
    dev_fields = [dict(f, vectors=put(f["vectors"]), seeds=put(f["seeds"])) for f in host_fields]
    line_fields = [dict(f, seeds=put(seeds(LINE_SEEDS, 100 + k)), max_steps=LINE_STEPS)
                   for k, f in enumerate(dev_fields)]
    tube = dict(radius=RADIUS, nsides=SIDES, color=COLOR)
    slots = list(range(GRIDS))
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
    dbounds = torch.empty((GRIDS, 6), dtype=torch.float32, device=dev)

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

    def median_of(fn, after=None):
        for _ in range(args.warmup):
            fn()
        t, extra = [], []
        for _ in range(runs):
            t.append(timed(fn))
            if after:
                extra.append(after())
        out = {"events": round(statistics.median(x[0] for x in t), 4),
               "wall": round(statistics.median(x[1] for x in t), 4)}
        if after:
            out["phases"] = [round(statistics.median(x[k] for x in extra), 4)
                             for k in range(len(extra[0]))]
        return out

    def image():
        rt.sync()
        return [rt.slot_export(s, w).tobytes() for s in slots
                for w in (rt.SLOT_NODES, rt.SLOT_TRIS, rt.SLOT_QNODES4, rt.SLOT_NORMALS,
                          rt.SLOT_COLORS, rt.SLOT_FACES)]

    def device_all():   # (a)
        rt.stream_tubes_domains(slots, dev_fields, tube, normals=True, bounds=dbounds)

    def host_all():     # (b)
        m = [spray_amd.stream_tubes_host(f["vectors"], f["origin"], f["spacing"], f["seeds"], STEP,
                                         STEPS, RADIUS, SIDES, direction=f["direction"],
                                         min_speed=f["min_speed"], color=COLOR)
             for f in host_fields]
        rt.build_domains(slots, [x[0] for x in m], [x[3] for x in m], [x[2] for x in m],
                         [x[1] for x in m], bounds=dbounds)

    counts = rt.stream_tubes(dev_fields, tube, count_only=True)
    npts = rt.streamlines(dev_fields, count_only=True)
    a = median_of(device_all, after=rt.stream_phase_times)
    img_a = image()
    b = median_of(host_all)
    same = image() == img_a
    # (c) below the Python wrapper: its buffers are allocated once
    import ctypes as C
    from spray_amd import engine
    from spray_amd._native import lib
    lpts = rt.streamlines(line_fields, count_only=True)
    arr, _, _, keep = engine._stream_tables(line_fields)
    pts = [torch.empty((n, 3), dtype=torch.float32, device=dev) for n in lpts]
    off = [torch.empty(LINE_SEEDS + 1, dtype=torch.int32, device=dev) for _ in lpts]
    info = [torch.empty((LINE_SEEDS, 2), dtype=torch.int32, device=dev) for _ in lpts]
    ptrs = lambda xs: (C.c_void_p * GRIDS)(*[x.data_ptr() for x in xs])
    pp, po, pi, caps = ptrs(pts), ptrs(off), ptrs(info), (C.c_size_t * GRIDS)(*lpts)

    def lines_all():
        rc = lib().spray_rt_streamlines(rt.h, GRIDS, arr, pp, po, pi, caps, None)
        assert rc == 0, rc

    c = median_of(lines_all)
    steps = int(sum(lpts)) - GRIDS * LINE_SEEDS
    faster = a["wall"] < b["wall"]
    phases = a.pop("phases")
    out = {"workload": "%d vector grids of %d^3 points, %d seeds each, %d steps both ways, %d sides"
                       % (GRIDS, N, SEEDS, STEPS, SIDES),
           "runs": runs, "points": int(sum(npts)),
           "vertices": int(sum(x[0] for x in counts)), "triangles": int(sum(x[1] for x in counts)),
           "device_ms": a, "host_ms": b,
           "count_wall_ms": phases[0], "integrate_expand_enqueue_wall_ms": phases[1],
           "build_wall_ms": phases[2],
           "integrations_share_of_device_at_most": round(2 * phases[0] / a["wall"], 3),
           "lines_only": {"seeds": GRIDS * LINE_SEEDS, "rk4_steps": steps, "ms": c,
                          "rk4_steps_per_s": round(steps / (c["events"] * 1e-3), 1)},
           "host_over_device": {"events": round(b["events"] / a["events"], 1),
                                "wall": round(b["wall"] / a["wall"], 1)},
           "slots_identical": bool(same), "device_faster_than_host": bool(faster)}
    print(json.dumps(out))
    rt.close()
    return 0 if (same and faster) else 1


if __name__ == "__main__":
    sys.exit(main())

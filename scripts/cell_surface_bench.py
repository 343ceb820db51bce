#!/usr/bin/env python
"""Per-time-step boundary surfaces and thresholds of unstructured hexahedral
meshes: the workload of scripts/cell_isosurface_bench.py looked at instead of
contoured.  64 meshes, each the 32^3 hexahedra over a 33^3-point block of one
wavelet-like analytic field of 129^3 points, numbered x fastest, into 64
resident slots, with the negated gradient of the field as point normals and one
constant colour; once with every cell kept (SPRAY_RT_SELECT_ALL: the blocks'
outer surfaces) and once thresholded by points at the region field >= 0.3
(SPRAY_RT_SELECT_POINTS).

    python scripts/cell_surface_bench.py [--runs 20] [--warmup 3]

Timed per mode, each a median of --runs runs after --warmup in the same
process, by HIP events on the context's stream and by wall clock (the call,
then a stream sync):
  (a) ONE spray_rt_domains_cell_surface of all 64 slots from arrays in HBM, and
      the extraction's wall clock split at its two host reads with the sort's
      device time (spray_rt_cell_surface_phase_times), from runs of their own
      with the sort's events on;
  (b) spray_rt_cell_surface_host per mesh, then ONE spray_rt_domains_build from
      the host arrays -- the path a caller without (a) has, given the arrays on
      the host already (no D2H is charged).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cell_isosurface_bench import CELLS, COLOR, HEX, ISO, TILES, field, hexes  # noqa: E402

WIDE = 1e30   # a finite bound no sample reaches


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
    f = field()
    grad = np.stack(np.gradient(f.astype(np.float64))[::-1], -1)   # d/dx, d/dy, d/dz
    n1 = CELLS + 1
    conn = hexes(n1)
    ncells = len(conn) // 8
    types = np.full(ncells, HEX, np.uint8)
    offsets = (8 * np.arange(ncells + 1)).astype(np.uint32)
    ax = np.arange(n1, dtype=np.float32)
    host_meshes = []
    for kz in range(TILES):
        for ky in range(TILES):
            for kx in range(TILES):
                o = (kx * CELLS, ky * CELLS, kz * CELLS)
                cut = (slice(o[2], o[2] + n1), slice(o[1], o[1] + n1), slice(o[0], o[0] + n1))
                z, y, x = np.meshgrid(ax + o[2], ax + o[1], ax + o[0], indexing="ij")
                host_meshes.append(dict(
                    points=np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32),
                    types=types, offsets=offsets, conn=conn,
                    values=np.ascontiguousarray(f[cut]).reshape(-1),
                    normals=np.ascontiguousarray(-grad[cut]).reshape(-1, 3).astype(np.float32),
                    color=COLOR))
    nd = len(host_meshes)
    # one connectivity, 64 meshes
    shared = dict(types=torch.from_numpy(types).to(dev),
                  offsets=torch.from_numpy(offsets.view(np.int32)).to(dev),
                  conn=torch.from_numpy(conn.view(np.int32)).to(dev))
    dev_meshes = [dict(m, **shared, **{k: torch.from_numpy(m[k]).to(dev)
                                       for k in ("points", "values", "normals")})
                  for m in host_meshes]
    slots = list(range(nd))
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
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

    out = {"workload": "%d hex meshes of %d^3 points, %d hexahedra each" % (nd, n1, ncells),
           "runs": runs}
    ok = True
    for name, sel in (("all", None), ("threshold", dict(mode="points", lo=ISO, hi=WIDE))):
        sels = None if sel is None else [sel] * nd

        def device_all():   # (a)
            rt.cell_surface_domains(slots, dev_meshes, sels, normals=True, bounds=dbounds)

        def host_all():     # (b)
            m = [spray_amd.cell_surface_host(h["points"], h["types"], h["offsets"], h["conn"], sel,
                                             h["values"], h["normals"], color=COLOR)
                 for h in host_meshes]
            rt.build_domains(slots, [x[0] for x in m], [x[4] for x in m], [x[2] for x in m],
                             [x[1] for x in m], bounds=dbounds)

        counts = rt.cell_surface(dev_meshes, sels, count_only=True)
        a = median_of(device_all)
        img_a = image()
        rt.cell_surface_phase_times(on=True)
        phases = median_of(device_all, after=rt.cell_surface_phase_times)["phases"]
        rt.cell_surface_phase_times(on=False)
        b = median_of(host_all)
        same = image() == img_a
        faster = a["wall"] < b["wall"]
        ok = ok and same and faster
        out[name] = {
            "vertices": int(sum(c[0] for c in counts)), "triangles": int(sum(c[1] for c in counts)),
            "device_ms": a, "host_ms": b,
            "extract_wall_to_read1_ms": phases[0], "extract_wall_read1_to_read2_ms": phases[1],
            "extract_wall_after_read2_ms": phases[2], "sort_device_ms": phases[3],
            "host_over_device": {"events": round(b["events"] / a["events"], 1),
                                 "wall": round(b["wall"] / a["wall"], 1)},
            "slots_identical": bool(same), "device_faster_than_host": bool(faster),
        }
    print(json.dumps(out))
    rt.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

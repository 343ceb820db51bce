#!/usr/bin/env python
"""Per-time-step clips of unstructured hexahedral meshes: the workload of
scripts/cell_isosurface_bench.py cut open instead of contoured.  64 meshes, each
the 32^3 hexahedra over a 33^3-point block of one wavelet-like analytic field of
129^3 points, numbered x fastest, into 64 resident slots, with the negated
gradient of the field as point normals and one constant colour, clipped at that
benchmark's isovalue: the part with field >= 0.3, its cut face included.

    python scripts/cell_clip_bench.py [--runs 20] [--warmup 3]

Timed, each a median of --runs runs after --warmup in the same process, by HIP
events on the context's stream and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_cell_clip of all 64 slots from arrays in HBM, and the
      extraction's phases (spray_rt_cell_clip_phase_times), from runs of their
      own with the sorts' events on;
  (b) spray_rt_cell_clip_host per mesh, then ONE spray_rt_domains_build from the
      host arrays -- the path a caller without (a) has, given the arrays on the
      host already (no D2H is charged);
  (c) ONE spray_rt_domains_cell_isosurface plus ONE spray_rt_domains_cell_surface
      (SPRAY_RT_SELECT_ALL) of the same meshes, for scale: they do not make the
      clip.
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
                    values=np.ascontiguousarray(f[cut]).reshape(-1), iso=ISO,
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

    def device_all():   # (a)
        rt.cell_clip_domains(slots, dev_meshes, normals=True, bounds=dbounds)

    def host_all():     # (b)
        m = [spray_amd.cell_clip_host(h["points"], h["types"], h["offsets"], h["conn"], h["values"],
                                      ISO, False, h["normals"], color=COLOR)
             for h in host_meshes]
        rt.build_domains(slots, [x[0] for x in m], [x[5] for x in m], [x[2] for x in m],
                         [x[1] for x in m], bounds=dbounds)

    def parts_all():    # (c)
        rt.cell_isosurface_domains(slots, dev_meshes, normals=True, bounds=dbounds)
        rt.cell_surface_domains(slots, dev_meshes, None, normals=True, bounds=dbounds)

    counts = rt.cell_clip(dev_meshes, count_only=True)
    a = median_of(device_all)
    img_a = image()
    rt.cell_clip_phase_times(on=True)
    phases = median_of(device_all, after=rt.cell_clip_phase_times)["phases"]
    rt.cell_clip_phase_times(on=False)
    b = median_of(host_all)
    same = image() == img_a
    c = median_of(parts_all)
    faster = a["wall"] < b["wall"]
    out = {"workload": "%d hex meshes of %d^3 points, %d hexahedra each" % (nd, n1, ncells),
           "runs": runs,
           "vertices": int(sum(x[0] for x in counts)), "triangles": int(sum(x[1] for x in counts)),
           "cap_vertices": int(sum(x[2] for x in counts)),
           "cap_triangles": int(sum(x[3] for x in counts)),
           "device_ms": a, "host_ms": b, "isosurface_plus_surface_ms": c,
           "cell_pass_wall_ms": phases[0], "tet_count_wall_ms": phases[1],
           "weld_wall_ms": phases[2], "emit_wall_ms": phases[3], "sorts_device_ms": phases[4],
           "skin_passes_wall_ms": phases[5],
           "sorts_share_of_device": round(phases[4] / a["events"], 3),
           "host_over_device": {"events": round(b["events"] / a["events"], 1),
                                "wall": round(b["wall"] / a["wall"], 1)},
           "slots_identical": bool(same), "device_faster_than_host": bool(faster)}
    print(json.dumps(out))
    rt.close()
    return 0 if (same and faster) else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Per-time-step geometry from a scalar field: 64 grids of 33^3 points that
tile one wavelet-like analytic field (a Gaussian times a sum of sinusoids, 129^3
points; neighbouring grids share their boundary sample planes), contoured into
64 resident slots.

    python scripts/isosurface_bench.py [--runs 20] [--warmup 3]

Timed, each a median of --runs runs after --warmup in the same process, by HIP
events on the context's stream and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_isosurface of all 64 slots from fields in HBM, and
      its two parts on their own: spray_rt_isosurface into preallocated device
      buffers, and spray_rt_domains_build of those buffers;
  (b) spray_rt_isosurface_host per grid, then ONE spray_rt_domains_build from
      the host arrays -- the path a caller without (a) has, given the fields
      on the host already (no D2H of the fields is charged).
The slots of (a) and (b) must hold the same bytes, and (a) should be faster
than (b): the ratio is reported, the exit code follows it.  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILES, CELLS = 4, 32   # 4 x 4 x 4 grids of 33^3 points
ISO = 0.3
COLOR = 0x00C0A060


def field():
    n = TILES * CELLS + 1
    x = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(x, x, x, indexing="ij")
    c = (n - 1) / 2.0
    gauss = np.exp(-((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) / (2 * (0.3 * n) ** 2))
    waves = np.sin(0.19 * x) + np.sin(0.23 * y + 1.0) + np.cos(0.29 * z)
    return (gauss * waves).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    runs = max(args.runs, 20)

    import torch
    import spray_amd
    from spray_amd import _native, engine

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    f = field()
    host_grids = []
    for kz in range(TILES):
        for ky in range(TILES):
            for kx in range(TILES):
                o = (kx * CELLS, ky * CELLS, kz * CELLS)
                sub = f[o[2]:o[2] + CELLS + 1, o[1]:o[1] + CELLS + 1, o[0]:o[0] + CELLS + 1]
                host_grids.append((np.ascontiguousarray(sub), tuple(float(v) for v in o),
                                   (1.0, 1.0, 1.0), ISO, COLOR))
    nd = len(host_grids)
    dev_grids = [(torch.from_numpy(g[0]).to(dev),) + g[1:] for g in host_grids]
    slots = list(range(nd))
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
    dbounds = torch.empty((nd, 6), dtype=torch.float32, device=dev)

    def device_all():   # (a)
        rt.isosurface_domains(slots, dev_grids, normals=True, bounds=dbounds)

    def host_all():     # (b)
        m = [spray_amd.isosurface_host(*g[:4]) for g in host_grids]
        cols = [np.full(len(v), COLOR, np.uint32) for v, _, _ in m]
        rt.build_domains(slots, [x[0] for x in m], [x[2] for x in m], cols, [x[1] for x in m],
                         bounds=dbounds)

    # the parts of (a): exact-size device buffers, allocated once
    meshes = rt.isosurface(dev_grids, normals=True)
    ntris = int(sum(len(m[2]) for m in meshes))
    nverts = int(sum(len(m[0]) for m in meshes))
    colors = [torch.full((len(m[0]),), COLOR, dtype=torch.int32, device=dev) for m in meshes]
    arr, keep = engine._grid_table(dev_grids)
    ptrs = lambda xs: (C.c_void_p * nd)(*[x.data_ptr() for x in xs])
    pv, pn, pf = ptrs([m[0] for m in meshes]), ptrs([m[1] for m in meshes]), ptrs([m[2] for m in meshes])
    cv = (C.c_size_t * nd)(*[len(m[0]) for m in meshes])
    cf = (C.c_size_t * nd)(*[len(m[2]) for m in meshes])
    nv, nf = (C.c_size_t * nd)(), (C.c_size_t * nd)()

    def extract_only():
        rc = _native.lib().spray_rt_isosurface(rt.h, nd, arr, pv, pn, pf, cv, cf, nv, nf)
        assert rc == 0, rc

    def build_only():
        rt.build_domains(slots, [m[0] for m in meshes], [m[2] for m in meshes], colors,
                         [m[1] for m in meshes], bounds=dbounds)

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
        return {"events": round(statistics.median(x[0] for x in t), 4),
                "wall": round(statistics.median(x[1] for x in t), 4)}

    def image():
        rt.sync()
        return [rt.slot_export(s, w).tobytes() for s in slots
                for w in (rt.SLOT_NODES, rt.SLOT_TRIS, rt.SLOT_QNODES4, rt.SLOT_NORMALS)]

    a = median_of(device_all)
    img_a = image()
    a_extract = median_of(extract_only)
    a_build = median_of(build_only)
    b = median_of(host_all)
    same = image() == img_a
    out = {
        "workload": "%d grids of %d^3 points" % (nd, CELLS + 1), "isovalue": ISO,
        "triangles": ntris, "vertices": nverts, "runs": runs,
        "device_ms": a, "device_extract_ms": a_extract, "device_build_ms": a_build,
        "host_ms": b,
        "host_over_device": {"events": round(b["events"] / a["events"], 1),
                             "wall": round(b["wall"] / a["wall"], 1)},
        "slots_identical": bool(same),
        "device_faster_than_host": bool(a["wall"] < b["wall"]),
    }
    print(json.dumps(out))
    rt.close()
    return 0 if same and out["device_faster_than_host"] else 1


if __name__ == "__main__":
    sys.exit(main())

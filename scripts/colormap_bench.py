#!/usr/bin/env python
"""Isosurfaces coloured by a second field, and recolouring resident slots: the
workload of scripts/isosurface_bench.py (64 grids of 33^3 points that tile one
wavelet-like analytic field, contoured into 64 resident slots) with a second
analytic field (rings about one corner of the volume plus a slow ramp) mapped
through a 256-entry table.

    python scripts/colormap_bench.py [--runs 20] [--warmup 3]

Timed, each a median of --runs runs after --warmup in the same process, by HIP
events on the context's stream and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_isosurface_mapped of all 64 slots, and its
      extraction alone (spray_rt_isosurface_mapped into preallocated buffers);
  (b) ONE spray_rt_domains_isosurface of the same grids with a constant colour
      (the path without a colour map), and its extraction alone
      (spray_rt_isosurface);
  (c) recolouring the resident slots with another table: spray_rt_isosurface_mapped
      with colours alone into preallocated device buffers, then ONE
      spray_rt_domains_recolor;
  (d) what (c) replaces: (a) again with the other table.
(c) and (d) alternate between two tables, so every run changes the colours.
The slots after (c) must hold the bytes they hold after (d), and (c) must be
faster than (d): the exit code follows both.  (a) / (b) is reported only.
Prints one JSON line.
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
NTABLE = 256


def fields():
    n = TILES * CELLS + 1
    x = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(x, x, x, indexing="ij")
    c = (n - 1) / 2.0
    gauss = np.exp(-((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) / (2 * (0.3 * n) ** 2))
    waves = np.sin(0.19 * x) + np.sin(0.23 * y + 1.0) + np.cos(0.29 * z)
    r = np.sqrt(x * x + y * y + z * z)
    second = np.sin(0.11 * r) + 0.004 * r
    return (gauss * waves).astype(np.float32), second.astype(np.float32)


def ramp(seed):
    """A table between two colours."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
    t = np.linspace(0.0, 1.0, NTABLE)[:, None]
    rgb = np.rint(a + t * (b - a)).astype(np.uint32)
    return (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]


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
    f, g = fields()
    lo, hi = float(g.min()), float(g.max())
    tables = [ramp(1), ramp(2)]
    plain, coloured = [], [[], []]
    for kz in range(TILES):
        for ky in range(TILES):
            for kx in range(TILES):
                o = (kx * CELLS, ky * CELLS, kz * CELLS)
                cut = lambda a: torch.from_numpy(np.ascontiguousarray(
                    a[o[2]:o[2] + CELLS + 1, o[1]:o[1] + CELLS + 1, o[0]:o[0] + CELLS + 1])).to(dev)
                base = dict(values=cut(f), origin=tuple(float(v) for v in o),
                            spacing=(1.0, 1.0, 1.0), iso=ISO, color=COLOR)
                plain.append(base)
                cf = cut(g)
                for k in (0, 1):
                    coloured[k].append(dict(base, cfield=cf, cmap=(tables[k], lo, hi)))
    nd = len(plain)
    slots = list(range(nd))
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
    dbounds = torch.empty((nd, 6), dtype=torch.float32, device=dev)
    turn = [0]

    def mapped_all():    # (a), and (d) with alternating tables
        rt.isosurface_domains_mapped(slots, coloured[turn[0] & 1], normals=True, bounds=dbounds)

    def plain_all():     # (b)
        rt.isosurface_domains(slots, plain, normals=True, bounds=dbounds)

    # (c): exact-size colour buffers, allocated once
    mapped_all()
    counts = [len(m[2]) for m in rt.isosurface_mapped(coloured[0], colors_only=True)]
    nverts = int(sum(counts))
    ntris = int(sum(rt.slot_info(s)["tris"] for s in slots))
    cols = [torch.zeros(max(k, 1), dtype=torch.int32, device=dev) for k in counts]
    pc = (C.c_void_p * nd)(*[x.data_ptr() for x in cols])
    cv = (C.c_size_t * nd)(*counts)
    sl = (C.c_int * nd)(*slots)
    nv, nf = (C.c_size_t * nd)(), (C.c_size_t * nd)()
    L = _native.lib()

    def recolor_all():
        gs = coloured[turn[0] & 1]
        arr, keep = engine._grid_table(gs)
        carr, ckeep = engine._grid_color_table(gs)
        rc = L.spray_rt_isosurface_mapped(rt.h, nd, arr, carr, None, None, pc, None, cv, None,
                                          nv, nf)
        assert rc == 0, rc
        rc = L.spray_rt_domains_recolor(rt.h, nd, sl, pc, cv)
        assert rc == 0, rc

    # the extractions alone: exact-size buffers, allocated once
    meshes = rt.isosurface(plain, normals=True)
    ptrs = lambda xs: (C.c_void_p * nd)(*[x.data_ptr() for x in xs])
    pv, pn, pf = ptrs([m[0] for m in meshes]), ptrs([m[1] for m in meshes]), ptrs([m[2] for m in meshes])
    cfc = (C.c_size_t * nd)(*[len(m[2]) for m in meshes])
    parr, pkeep = engine._grid_table(plain)
    marr, mkeep = engine._grid_table(coloured[0])
    mcarr, mckeep = engine._grid_color_table(coloured[0])
    torch.cuda.synchronize()

    def extract_plain():
        rc = L.spray_rt_isosurface(rt.h, nd, parr, pv, pn, pf, cv, cfc, nv, nf)
        assert rc == 0, rc

    def extract_mapped():
        rc = L.spray_rt_isosurface_mapped(rt.h, nd, marr, mcarr, pv, pn, pc, pf, cv, cfc, nv, nf)
        assert rc == 0, rc

    def timed(fn):
        turn[0] += 1
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
            turn[0] += 1
            fn()
        t = [timed(fn) for _ in range(runs)]
        return {"events": round(statistics.median(x[0] for x in t), 4),
                "wall": round(statistics.median(x[1] for x in t), 4)}

    def image():
        rt.sync()
        return [rt.slot_export(s, w).tobytes() for s in slots
                for w in (rt.SLOT_NODES, rt.SLOT_TRIS, rt.SLOT_QNODES4, rt.SLOT_NORMALS,
                          rt.SLOT_COLORS, rt.SLOT_FACES)]

    a = median_of(mapped_all)
    b = median_of(plain_all)
    a_extract = median_of(extract_mapped)
    b_extract = median_of(extract_plain)
    d = median_of(mapped_all)
    img_d = (turn[0] & 1, image())
    c = median_of(recolor_all)
    if (turn[0] & 1) != img_d[0]:   # end on the table (d) ended on
        turn[0] += 1
        recolor_all()
    same = image() == img_d[1]
    out = {
        "workload": "%d grids of %d^3 points" % (nd, CELLS + 1), "isovalue": ISO,
        "table_entries": NTABLE, "triangles": ntris, "vertices": nverts, "runs": runs,
        "mapped_ms": a, "mapped_extract_ms": a_extract, "constant_ms": b,
        "constant_extract_ms": b_extract, "recolor_ms": c, "remap_by_extraction_ms": d,
        "mapped_over_constant": {"events": round(a["events"] / b["events"], 3),
                                 "wall": round(a["wall"] / b["wall"], 3)},
        "extraction_over_recolor": {"events": round(d["events"] / c["events"], 1),
                                    "wall": round(d["wall"] / c["wall"], 1)},
        "added_bytes": {"colour_fields": 4 * nd * (CELLS + 1) ** 3, "colours": 4 * nverts},
        "recolor_identical": bool(same),
        "recolor_faster": bool(c["wall"] < d["wall"] and c["events"] < d["events"]),
    }
    print(json.dumps(out))
    rt.close()
    return 0 if same and out["recolor_faster"] else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Per-time-step geometry from a scalar field on unstructured hexahedral
meshes: the workload of scripts/isosurface_bench.py and
scripts/tet_isosurface_bench.py as hex meshes.  64 meshes, each the 32^3
hexahedra over a 33^3-point block of one wavelet-like analytic field of 129^3
points, numbered x fastest, contoured at 0.3 into 64 resident slots, with the
negated gradient of the field as point normals and one constant colour.

    python scripts/cell_isosurface_bench.py [--runs 20] [--warmup 3]

Timed, each a median of --runs runs after --warmup in the same process, by HIP
events on the context's stream and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_cell_isosurface of all 64 slots from arrays in HBM;
      its extraction alone (spray_rt_cell_isosurface into preallocated device
      buffers) and the extraction's wall clock split at its three host reads
      (spray_rt_cell_phase_times): [0] is the time to host read 1, the cell
      pass;
  (b) spray_rt_cell_isosurface_host per mesh, then ONE spray_rt_domains_build
      from the host arrays -- the path a caller without (a) has, given the
      arrays on the host already (no D2H is charged);
  (c) reported only: spray_rt_domains_tet_isosurface on the same meshes split
      beforehand into Kuhn tets (section 14's call: the same surface, faces in
      another order), and spray_rt_domains_isosurface on the same field as 64
      structured grids (section 12's).
The slots of (a) and (b) must hold the same bytes, (a) should be faster than
(b) and the triangle count is section 12's: the exit code follows the three.
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
TILES, CELLS = 4, 32   # 4 x 4 x 4 blocks of 33^3 points
ISO = 0.3
COLOR = 0x00C0A060
TRIANGLES = 1029960    # of sections 12 and 14 on this field
HEX = 12
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def field():
    n = TILES * CELLS + 1
    x = np.arange(n, dtype=np.float64)
    z, y, x = np.meshgrid(x, x, x, indexing="ij")
    c = (n - 1) / 2.0
    gauss = np.exp(-((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) / (2 * (0.3 * n) ** 2))
    waves = np.sin(0.19 * x) + np.sin(0.23 * y + 1.0) + np.cos(0.29 * z)
    return (gauss * waves).astype(np.float32)


def cell_bases(n):
    k, j, i = np.meshgrid(*[np.arange(n - 1)] * 3, indexing="ij")
    return (i + n * (j + n * k)).reshape(-1)


def hexes(n):
    """uint32 [8 (n - 1)^3]: the hexahedra of an n^3-point lattice, x fastest, VTK order."""
    corner = np.array([0, 1, 1 + n, n])
    corner = np.concatenate([corner, corner + n * n])
    return (cell_bases(n)[:, None] + corner[None]).reshape(-1).astype(np.uint32)


def kuhn_tets(n):
    """uint32 [6 (n - 1)^3, 4]: the Kuhn split of the same lattice."""
    stride = (1, n, n * n)
    walks = [np.cumsum([0] + [stride[ax] for ax in perm]) for perm in PERMS]
    return (cell_bases(n)[:, None, None] + np.asarray(walks)[None]).reshape(-1, 4).astype(np.uint32)


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
    grad = np.stack(np.gradient(f.astype(np.float64))[::-1], -1)   # d/dx, d/dy, d/dz
    n1 = CELLS + 1
    conn = hexes(n1)
    ncells = len(conn) // 8
    types = np.full(ncells, HEX, np.uint8)
    offsets = (8 * np.arange(ncells + 1)).astype(np.uint32)
    tets = kuhn_tets(n1)
    ax = np.arange(n1, dtype=np.float32)
    host_meshes, host_grids = [], []
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
                    iso=ISO, color=COLOR))
                host_grids.append((np.ascontiguousarray(f[cut]), tuple(float(v) for v in o),
                                   (1.0, 1.0, 1.0), ISO, COLOR))
    nd = len(host_meshes)
    # one connectivity, 64 meshes
    shared = dict(types=torch.from_numpy(types).to(dev),
                  offsets=torch.from_numpy(offsets.view(np.int32)).to(dev),
                  conn=torch.from_numpy(conn.view(np.int32)).to(dev))
    d_tets = torch.from_numpy(tets.view(np.int32)).to(dev)
    dev_meshes = [dict(m, **shared, **{k: torch.from_numpy(m[k]).to(dev)
                                       for k in ("points", "values", "normals")})
                  for m in host_meshes]
    dev_tetmeshes = [dict(points=m["points"], values=m["values"], normals=m["normals"], tets=d_tets,
                          iso=ISO, color=COLOR) for m in dev_meshes]
    dev_grids = [(torch.from_numpy(g[0]).to(dev),) + g[1:] for g in host_grids]
    slots = list(range(nd))
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
    dbounds = torch.empty((nd, 6), dtype=torch.float32, device=dev)

    def device_all():   # (a)
        rt.cell_isosurface_domains(slots, dev_meshes, normals=True, bounds=dbounds)

    def host_all():     # (b)
        m = [spray_amd.cell_isosurface_host(h["points"], h["types"], h["offsets"], h["conn"],
                                            h["values"], ISO, h["normals"], color=COLOR)
             for h in host_meshes]
        rt.build_domains(slots, [x[0] for x in m], [x[3] for x in m], [x[2] for x in m],
                         [x[1] for x in m], bounds=dbounds)

    def tets_all():     # (c)
        rt.tet_isosurface_domains(slots, dev_tetmeshes, normals=True, bounds=dbounds)

    def grids_all():    # (c)
        rt.isosurface_domains(slots, dev_grids, normals=True, bounds=dbounds)

    # the extraction of (a) alone: exact-size device buffers, allocated once
    meshes = rt.cell_isosurface(dev_meshes, normals=True)
    ntris = int(sum(len(m[3]) for m in meshes))
    nverts = int(sum(len(m[0]) for m in meshes))
    arr, carr, keep = engine._cell_table(dev_meshes)
    ptrs = lambda xs: (C.c_void_p * nd)(*[x.data_ptr() for x in xs])
    pv, pn = ptrs([m[0] for m in meshes]), ptrs([m[1] for m in meshes])
    pc, pf = ptrs([m[2] for m in meshes]), ptrs([m[3] for m in meshes])
    cv = (C.c_size_t * nd)(*[len(m[0]) for m in meshes])
    cf = (C.c_size_t * nd)(*[len(m[3]) for m in meshes])
    nv, nf = (C.c_size_t * nd)(), (C.c_size_t * nd)()

    def extract_only():
        rc = _native.lib().spray_rt_cell_isosurface(rt.h, nd, arr, carr, pv, pn, pc, pf, cv, cf,
                                                    nv, nf)
        assert rc == 0, rc

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

    a = median_of(device_all)
    img_a = image()
    a_extract = median_of(extract_only, after=rt.cell_phase_times)
    phases = a_extract.pop("phases")
    b = median_of(host_all)
    same = image() == img_a
    c_tets = median_of(tets_all)
    c_grids = median_of(grids_all)
    out = {
        "workload": "%d hex meshes of %d^3 points, %d hexahedra each" % (nd, n1, ncells),
        "isovalue": ISO, "triangles": ntris, "vertices": nverts, "runs": runs,
        "device_ms": a, "device_extract_ms": a_extract,
        "extract_wall_to_read1_ms": phases[0], "extract_wall_read1_to_read2_ms": phases[1],
        "extract_wall_read2_to_read3_ms": phases[2], "extract_wall_after_read3_ms": phases[3],
        "host_ms": b, "tet_device_ms": c_tets, "grid_device_ms": c_grids,
        "host_over_device": {"events": round(b["events"] / a["events"], 1),
                             "wall": round(b["wall"] / a["wall"], 1)},
        "cell_over_tet": {"events": round(a["events"] / c_tets["events"], 3),
                          "wall": round(a["wall"] / c_tets["wall"], 3)},
        "slots_identical": bool(same),
        "device_faster_than_host": bool(a["wall"] < b["wall"]),
        "triangles_as_the_grids": bool(ntris == TRIANGLES),
    }
    print(json.dumps(out))
    rt.close()
    ok = same and out["device_faster_than_host"] and out["triangles_as_the_grids"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Per-time-step glyphs of particle sets: 64 point sets, 32 drawn as spheres
(404 points, every second one kept, icosphere level 1: 80 faces) and 32 as
arrows along their velocities (672 points, half kept by a select range, 8
sides: 48 faces, length scaled by the speed), coloured through a map, into 64
resident slots: 1,033,216 triangles, the scale of the other filters'
benchmarks.

    python scripts/glyph_bench.py [--runs 20] [--warmup 3] [--trace]

Timed, each a median of --runs runs after --warmup in the same process, by HIP
events on the context's stream and by wall clock (the call, then a stream sync):
  (a) ONE spray_rt_domains_glyphs of all 64 slots from arrays in HBM, with its
      phases (spray_rt_glyph_phase_times);
  (b) spray_rt_glyphs_host per set, then ONE spray_rt_domains_build from the
      host arrays -- the path a caller without (a) has, given the arrays on the
      host already (no D2H is charged);
  (c) the glyph form alone (no build) on one set of 1,048,576 points as spheres
      of level 0 into buffers allocated once, as glyphs per second and as bytes
      written per second against the HBM rate of a float4 copy (6.29 TB/s).
The slots of (a) and (b) must hold the same bytes and (a) should be faster than
(b): the exit code follows the two.  Prints one JSON line.  --trace runs (a)
and (c) five times each and nothing else, for a kernel trace.
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

SETS, NSPH, NARR, LEVEL, SIDES = 64, 404, 672, 1, 8
BIG = 1 << 20
HBM_COPY_BYTES_PER_S = 6.29e12


def particles(n, k):
    rng = np.random.default_rng(2000 + k)
    p = rng.uniform(-16.0, 16.0, (n, 3)).astype(np.float32)
    v = np.stack([-p[:, 1], p[:, 0], 2.0 + np.sin(p[:, 2])], 1).astype(np.float32) * np.float32(0.05)
    return p, v, rng.uniform(0.0, 1.0, n).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    runs = max(args.runs, 20)

    import torch
    import spray_amd
    from spray_amd import engine
    from spray_amd._native import lib

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    table = (np.arange(64, dtype=np.uint32) * 0x00040302) & 0x00FFFFFF
    host_sets, glyphs = [], []
    for k in range(SETS):
        arrows = k % 2 == 1
        p, v, a = particles(NARR if arrows else NSPH, k)
        S = dict(points=p, cfield=a, cmap=(table, 0.0, 1.0))
        if arrows:
            sel = np.tile(np.array([0.0, 1.0], np.float32), NARR // 2)
            S.update(vectors=v, select=sel, select_range=(0.5, 1.5))
            glyphs.append(dict(shape=spray_amd.GLYPH_ARROW, size=1.5, nsides=SIDES,
                               scale_by_vector=True))
        else:
            S.update(stride=2, scales=(0.5 + a).astype(np.float32))
            glyphs.append(dict(shape=spray_amd.GLYPH_SPHERE, size=0.3, level=LEVEL))
        host_sets.append(S)
    put = lambda x: torch.from_numpy(x).to(dev)
    keys = ("points", "vectors", "scales", "select", "cfield")
    dev_sets = [dict(S, **{k: put(S[k]) for k in keys if S.get(k) is not None}) for S in host_sets]
    slots = list(range(SETS))
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
    dbounds = torch.empty((SETS, 6), dtype=torch.float32, device=dev)

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
        rt.glyphs_domains(slots, dev_sets, glyphs, normals=True, bounds=dbounds)

    def host_all():     # (b)
        m = [spray_amd.glyphs_host(S, G, point_ids=False) for S, G in zip(host_sets, glyphs)]
        rt.build_domains(slots, [x[0] for x in m], [x[3] for x in m], [x[2] for x in m],
                         [x[1] for x in m], bounds=dbounds)

    # (c) below the Python wrapper: its buffers are allocated once
    p, v, a = particles(BIG, 999)
    big = [dict(points=put(p), scales=put((0.5 + a).astype(np.float32)), cfield=put(a),
                cmap=(table, 0.0, 1.0))]
    bigg = [dict(shape=spray_amd.GLYPH_SPHERE, size=0.01, level=0)]
    (nv, nf), = rt.glyphs(big, bigg, count_only=True)
    arr, garr, carr, keep = engine._glyph_tables(big, bigg)
    bv = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    bn = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    bc = torch.empty(nv, dtype=torch.int32, device=dev)
    bf = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    bi = torch.empty(nv // 12, dtype=torch.int32, device=dev)
    one = lambda x: (C.c_void_p * 1)(x.data_ptr())
    pv, pn, pc, pf, pi = one(bv), one(bn), one(bc), one(bf), one(bi)
    cv, cf = (C.c_size_t * 1)(nv), (C.c_size_t * 1)(nf)

    def big_all():
        rc = lib().spray_rt_glyphs(rt.h, 1, arr, garr, carr, pv, pn, pc, pf, pi, cv, cf, None, None)
        assert rc == 0, rc

    if args.trace:
        for _ in range(5):
            device_all()
        for _ in range(5):
            big_all()
        rt.sync()
        rt.close()
        return 0

    counts = rt.glyphs(dev_sets, glyphs, count_only=True)
    a_ms = median_of(device_all, after=rt.glyph_phase_times)
    img_a = image()
    b_ms = median_of(host_all)
    same = image() == img_a
    c_ms = median_of(big_all)
    nglyphs = nv // 12
    written = nv * 28 + nf * 12 + nglyphs * 4
    faster = a_ms["wall"] < b_ms["wall"]
    phases = a_ms.pop("phases")
    rate = written / (c_ms["events"] * 1e-3)
    out = {"workload": "%d point sets: %d of %d points as spheres of level %d (stride 2), %d of %d "
                       "points as arrows of %d sides (half selected)"
                       % (SETS, SETS // 2, NSPH, LEVEL, SETS // 2, NARR, SIDES),
           "runs": runs, "vertices": int(sum(x[0] for x in counts)),
           "triangles": int(sum(x[1] for x in counts)),
           "device_ms": a_ms, "host_ms": b_ms,
           "count_wall_ms": phases[0], "place_expand_enqueue_wall_ms": phases[1],
           "build_wall_ms": phases[2],
           "glyphs_only": {"points": BIG, "glyphs": nglyphs, "vertices": nv, "triangles": nf,
                           "ms": c_ms, "glyphs_per_s": round(nglyphs / (c_ms["events"] * 1e-3), 1),
                           "bytes_written": written, "bytes_written_per_s": round(rate, 1),
                           "share_of_hbm_copy_rate": round(rate / HBM_COPY_BYTES_PER_S, 3)},
           "host_over_device": {"events": round(b_ms["events"] / a_ms["events"], 1),
                                "wall": round(b_ms["wall"] / a_ms["wall"], 1)},
           "slots_identical": bool(same), "device_faster_than_host": bool(faster)}
    print(json.dumps(out))
    rt.close()
    return 0 if (same and faster) else 1


if __name__ == "__main__":
    sys.exit(main())

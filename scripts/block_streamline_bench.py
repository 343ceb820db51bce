#!/usr/bin/env python
"""Streamlines across the blocks of a decomposed vector field, as tubes into one
slot: an ABC flow on a 129^3 lattice at spacing 0.25, held as 64 blocks of 33^3
points (4 x 4 x 4, neighbours sharing a plane), 1,024 seeds traced both ways for
100 steps of 0.125, tubes of 6 sides with a constant colour.

    python scripts/block_streamline_bench.py [--runs 20] [--warmup 3]

Timed, each a median of --runs runs after --warmup in the same process, by wall
clock (the call, then a stream sync) and, for (a) and (b), by HIP events on the
context's stream:
  (a) ONE spray_rt_domains_block_stream_tubes of the 64 blocks in HBM, with its
      phases (spray_rt_block_stream_phase_times);
  (b) the same data as one unsplit grid through spray_rt_domains_stream_tubes:
      the floor; (a) - (b) is what the block lookup costs.  The splits share
      planes of a grid at origin 0 with a power-of-two spacing, so the two
      slots hold the same bytes unless a point falls exactly on a shared plane;
  (c) what a caller has without (a): spray_rt_streamlines over the blocks that
      hold live line ends (one batched call per generation), the lines and
      line_info read back, every line that ended at a block face re-seeded one
      extrapolated segment further in the neighbour, until no line continues,
      the pieces stitched on the host.  Its lines are not (a)'s: a stage point
      cannot be sampled across the face, so each crossing replaces an RK4 step
      by an extrapolation.  It stops at the polylines (the tubes and the slot
      would come on top), so spray_rt_block_streamlines of the same seeds is
      timed next to it.
Also the polyline forms alone with 16,384 seeds into buffers allocated once, as
RK4 steps (points beyond the seeds) per second, blocks against the unsplit grid.
Prints one JSON line, "slots_identical" saying whether the slots of (a) and (b)
agree.
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

NB, PARTS, H = 33, 4, 0.25
N = (NB - 1) * PARTS + 1
SEEDS, STEPS, STEP, SIDES, RADIUS = 1024, 100, 0.125, 6, 0.05
LINE_SEEDS = 16384
COLOR = 0x00C08040
GRID, STEPS_END = 0, 1


def abc(n):
    ax = 4.0 * np.pi * np.arange(n) / (n - 1)     # two periods across the lattice
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return np.stack([np.sin(z) + 0.6 * np.cos(y), 0.8 * np.sin(x) + np.cos(z),
                     0.6 * np.sin(y) + 0.8 * np.cos(x)], -1).astype(np.float32)


def seeds(n, k):
    rng = np.random.default_rng(1000 + k)
    return rng.uniform(1.0, (N - 1) * H - 1.0, (n, 3)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    runs = max(args.runs, 5)

    import torch
    import spray_amd
    from spray_amd import engine
    from spray_amd._native import lib

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    put = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    whole = abc(N)
    d_whole = put(whole)
    blocks = []
    for pz in range(PARTS):
        for py in range(PARTS):
            for px in range(PARTS):
                lo = [(NB - 1) * p for p in (px, py, pz)]
                sl = tuple(slice(l, l + NB) for l in lo[::-1])
                blocks.append(dict(vectors=put(whole[sl]), origin=tuple(H * l for l in lo),
                                   spacing=(H, H, H)))
    trace = dict(step=STEP, max_steps=STEPS, direction=spray_amd.STREAM_BOTH, min_speed=1e-6)
    d_seeds = put(seeds(SEEDS, 0))
    bset = dict(trace, blocks=blocks, seeds=d_seeds)
    field = dict(trace, vectors=d_whole, origin=(0.0, 0.0, 0.0), spacing=(H, H, H), seeds=d_seeds)
    tube = dict(radius=RADIUS, nsides=SIDES, color=COLOR)
    rt = spray_amd.RtContext(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rt.set_stream(stream)
    dbounds = torch.empty((1, 6), dtype=torch.float32, device=dev)

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

    def median_of(fn, after=None, n=runs):
        for _ in range(args.warmup):
            fn()
        t, extra = [], []
        for _ in range(n):
            t.append(timed(fn))
            if after:
                extra.append(after())
        out = {"events": round(statistics.median(x[0] for x in t), 4),
               "wall": round(statistics.median(x[1] for x in t), 4),
               "wall_min": round(min(x[1] for x in t), 4),
               "wall_max": round(max(x[1] for x in t), 4)}
        if after:
            out["phases"] = [round(statistics.median(x[k] for x in extra), 4)
                             for k in range(len(extra[0]))]
        return out

    def image(slot):
        rt.sync()
        return [rt.slot_export(slot, w).tobytes()
                for w in (rt.SLOT_NODES, rt.SLOT_TRIS, rt.SLOT_QNODES4, rt.SLOT_NORMALS,
                          rt.SLOT_COLORS, rt.SLOT_FACES)]

    def blocks_all():    # (a)
        rt.block_stream_tubes_domains([0], [bset], tube, normals=True, bounds=dbounds)

    def unsplit_all():   # (b)
        rt.stream_tubes_domains([1], [field], tube, normals=True, bounds=dbounds)

    h_seeds = seeds(SEEDS, 0)
    extent = np.float32((N - 1) * H)

    def caller_all():    # (c)
        """-> the stitched lines' points in all, the generations."""
        total, gens = 0, 0
        for direction in (spray_amd.STREAM_FORWARD, spray_amd.STREAM_BACKWARD):
            cur = h_seeds.copy()
            left = np.full(len(cur), STEPS)
            pieces = [[] for _ in cur]
            active = np.arange(len(cur))
            while len(active):
                gens += 1
                p = cur[active]
                ok = ((p >= 0) & (p <= extent)).all(1)
                active, p = active[ok], p[ok]
                cell = np.minimum((p / np.float32(H * (NB - 1))).astype(np.int64), PARTS - 1)
                blk = cell[:, 0] + PARTS * (cell[:, 1] + PARTS * cell[:, 2])
                used = np.unique(blk)
                groups = [active[blk == b] for b in used]
                fields = [dict(trace, vectors=blocks[b]["vectors"], origin=blocks[b]["origin"],
                               spacing=blocks[b]["spacing"], seeds=cur[g], direction=direction)
                          for b, g in zip(used, groups)]
                res = rt.streamlines(fields) if fields else []
                rt.sync()
                nxt = []
                for g, (pt, off, info) in zip(groups, res):
                    pt, off, info = pt.cpu().numpy(), off.cpu().numpy(), info.cpu().numpy()
                    for i, line in enumerate(g):
                        seg = pt[off[i]:off[i + 1]]
                        if direction == spray_amd.STREAM_BACKWARD:
                            seg = seg[::-1]           # the seed first
                        end = (info[i, 1] >> (0 if direction else 8)) & 255
                        take = min(len(seg) - 1, left[line])
                        pieces[line].append(seg[:take + 1])
                        left[line] -= take
                        if end == GRID and take == len(seg) - 1 and left[line] > 0 and take >= 1:
                            cur[line] = seg[take] + (seg[take] - seg[take - 1])
                            left[line] -= 1
                            nxt.append(line)
                active = np.array(nxt, np.int64)
            total += sum(len(np.concatenate(x)) if x else 0 for x in pieces)   # the stitching
        return total, gens

    counts = rt.block_stream_tubes([bset], tube, count_only=True)[0]
    npts = rt.block_streamlines([bset], count_only=True)[0]
    a = median_of(blocks_all, after=rt.block_stream_phase_times)
    b = median_of(unsplit_all, after=rt.stream_phase_times)
    same = image(0) == image(1)
    shape = {}

    def caller_timed():
        shape["points"], shape["generations"] = caller_all()

    c = median_of(caller_timed, n=max(3, runs // 4))
    # what (c) stops at, from (a)'s side: the polylines of the same seeds as GPU tensors
    al = median_of(lambda: rt.block_streamlines([bset]))

    # the polyline forms alone, below the Python wrapper: buffers allocated once
    l_seeds = put(seeds(LINE_SEEDS, 1))
    lset, lfield = dict(bset, seeds=l_seeds), dict(field, seeds=l_seeds)
    lpts = rt.block_streamlines([lset], count_only=True)[0]
    gpts = rt.streamlines([lfield], count_only=True)[0]
    barr, _, _, keep_b = engine._block_tables([lset])
    farr, _, _, keep_f = engine._stream_tables([lfield])
    pts = torch.empty((max(lpts, gpts), 3), dtype=torch.float32, device=dev)
    off = torch.empty(LINE_SEEDS + 1, dtype=torch.int32, device=dev)
    info = torch.empty((LINE_SEEDS, 2), dtype=torch.int32, device=dev)
    pblk = torch.empty(max(lpts, gpts), dtype=torch.int32, device=dev)
    one = lambda x: (C.c_void_p * 1)(x.data_ptr())
    caps = (C.c_size_t * 1)(max(lpts, gpts))

    def block_lines():
        rc = lib().spray_rt_block_streamlines(rt.h, 1, barr, one(pts), one(off), one(info),
                                              one(pblk), caps, None)
        assert rc == 0, rc

    def grid_lines():
        rc = lib().spray_rt_streamlines(rt.h, 1, farr, one(pts), one(off), one(info), caps, None)
        assert rc == 0, rc

    lb = median_of(block_lines)
    rt.sync()
    crossings = int((pblk[1:lpts] != pblk[:lpts - 1]).sum().item())   # line ends included: an upper bound
    lg = median_of(grid_lines)
    steps, gsteps = lpts - LINE_SEEDS, gpts - LINE_SEEDS
    pa, pb = a.pop("phases"), b.pop("phases")
    out = {"workload": "%d blocks of %d^3 points (%d^3 in all, spacing %g), %d seeds, %d steps of "
                       "%g both ways, %d sides" % (PARTS ** 3, NB, N, H, SEEDS, STEPS, STEP, SIDES),
           "runs": runs, "points": int(npts), "vertices": int(counts[0]),
           "triangles": int(counts[1]),
           "blocks_ms": a, "blocks_phases_wall_ms": pa,
           "unsplit_ms": b, "unsplit_phases_wall_ms": pb,
           "caller_ms": {k: c[k] for k in ("wall", "wall_min", "wall_max")},
           "blocks_polylines_ms": al,
           "caller_over_blocks_polylines_wall": round(c["wall"] / al["wall"], 1),
           "caller_generations": shape["generations"], "caller_points": int(shape["points"]),
           "blocks_over_unsplit_wall": round(a["wall"] / b["wall"], 3),
           "caller_over_blocks_wall": round(c["wall"] / a["wall"], 1),
           "lines_only": {"seeds": LINE_SEEDS, "rk4_steps": int(steps),
                          "block_changes_at_most": crossings,
                          "blocks_ms": lb, "unsplit_ms": lg,
                          "blocks_rk4_steps_per_s": round(steps / (lb["events"] * 1e-3), 1),
                          "unsplit_rk4_steps_per_s": round(gsteps / (lg["events"] * 1e-3), 1)},
           "slots_identical": bool(same)}
    print(json.dumps(out))
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The hard classes of the multi-block streamline tests
(test_block_stream_cases.py on the host, test_gpu_block_stream_cases.py on the
GPU), in block_stream_helpers' block_set(...) format, on top of its numpy
restatement and of stream_cases' fields.

Each class is a function returning {name: set}.  The paths a class is there for
stand next to its inputs and are asserted from the counters of Rule below by
test_block_stream_cases.py.

Scale classes sit on the kernels' own boundaries (block_stream_kernels.hip,
block_stream_common.h): 256 lanes per workgroup of the integration (LANES),
64 x 256 elements per trip of the check pass (TRIP), 65,535 blocks per set
(MAX_BLOCKS), 24-bit lane counts, 25-bit fields of the packed scan word.
"""
import collections
import functools

import numpy as np

import block_stream_helpers as bs
import color_helpers as ch
import stream_cases as sc
import stream_helpers as sh

F32 = np.float32
FORWARD, BACKWARD, BOTH = bs.FORWARD, bs.BACKWARD, bs.BOTH
GRID, STEPS, SPEED, SEED = bs.GRID, bs.STEPS, bs.SPEED, bs.SEED
LANES, TRIP = sc.LANES, sc.TRIP
MAX_BLOCKS = 65535   # kMaxBlocks of block_stream_common.h
STAGES = ("q2", "q3", "q4", "pn")


# ---- floats in their order ----

def fkey(x):
    """float_key of block_stream_common.h: floats as integers in their order, -0 below +0."""
    b = int(F32(x).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else b | 0x80000000


def kfloat(k):
    return np.uint32((k & 0x7FFFFFFF) if k & 0x80000000 else ~k & 0xFFFFFFFF).view(F32)


def shift(x, k):
    """The float k floats above x (below for k < 0); from +0 one down is -0."""
    return kfloat(fkey(x) + k)


# ---- the restatement with the counters of these classes ----

class LazyRules:
    """stream_helpers.Rule per block, made when first asked for."""

    def __init__(self, s):
        self.s, self.made = s, {}

    def __len__(self):
        return len(self.s["blocks"])

    def __getitem__(self, k):
        if k not in self.made:
            s, b = self.s, self.s["blocks"][k]
            self.made[k] = sh.Rule(dict(vectors=b["vectors"], origin=b["origin"],
                                        spacing=b["spacing"], step=s["step"],
                                        max_steps=s["max_steps"], min_speed=s["min_speed"],
                                        cfield=b.get("cfield")), F32, collections.Counter())
        return self.made[k]


class Rule(bs.BlockRule):
    """block_stream_helpers.BlockRule in float32 with the inside test of all
    blocks at once (the same subtraction and division per block and axis, as
    one numpy operation each) and further counters:

      miss, scanned       misses of the current block and the boxes the miss
                          path reads for them (up to and including the hit, all
                          of them without one); scan_max, full_scan, hit_last
      seed_scanned        the same for the seeds, which start in the miss path
      switch_q2 .. _pn    changes of the current block per stage
      grid_q2 .. _pn      exits per stage
      only_q2, _q3, _q4   a step whose one stage alone is sampled outside the
                          block of p, p' back in it; pn_back: p' in the block of
                          p after a stage outside it
      changes_2           a step in which the current block changes twice or more
      gap_q2 .. _pn       exits per stage into a gap: outside every block, inside
                          the bounding box of the set
      q2_gap_k1_inside    q2 in a gap while p + h k1 is inside a block
      near_seed, near_pn  (near="seed" / "all") a located seed / p' or a stage
                          point whose membership of some block changes within 2
                          floats along an axis
    """

    def __init__(self, s, stats=None, near=None):
        self.F = F32
        self.stats = collections.Counter() if stats is None else stats
        self.rules = LazyRules(s)
        r0 = self.rules[0]
        r0.stats = self.stats
        self.step, self.max_steps, self.r0 = r0.step, r0.max_steps, r0
        self.colored = s["blocks"][0].get("cfield") is not None
        self.near = near
        B = s["blocks"]
        self.O = np.array([b["origin"] for b in B], F32).reshape(-1, 3)
        self.S = np.array([b["spacing"] for b in B], F32).reshape(-1, 3)
        self.TOP = np.array([[n - 1 for n in b["vectors"].shape[2::-1]] for b in B],
                            F32).reshape(-1, 3)
        with np.errstate(all="ignore"):
            self.hull = self.O.min(0), (self.O + self.TOP * self.S).max(0)

    def inside_all(self, q):
        g = (np.asarray(q, F32)[None, :] - self.O) / self.S
        return ((g >= 0) & (g <= self.TOP)).all(1)

    def in_hull(self, q):
        """Whether q is within the bounding box of the set: outside every
        block there, it is in a gap."""
        return bool(((q >= self.hull[0]) & (q <= self.hull[1])).all())

    def near_bound(self, q):
        ins = self.inside_all(q)
        for a in range(3):
            for k in (-2, -1, 1, 2):
                r = np.array(q, F32)
                r[a] = shift(q[a], k)
                if (self.inside_all(r) != ins).any():
                    return True
        return False

    def locate(self, q, cur):
        st = self.stats
        ins = self.inside_all(q)
        n = len(ins)
        if cur is not None and ins[cur]:
            k = cur
            if ins[:cur].any():
                st["sticky_over_lower"] += 1
        else:
            k = int(np.argmax(ins)) if ins.any() else None
            scanned = n if k is None else k + 1
            if cur is None:
                st["seed_scanned"] += scanned
                st["seed_full_scan"] += k is None
            else:
                st["miss"] += 1
                st["scanned"] += scanned
                st["scan_max"] = max(st["scan_max"], scanned)
                st["full_scan"] += k is None
                st["hit_last"] += k == n - 1
        if k is None:
            return None
        ok, idx, fr = self.rules[k].locate(q)
        assert ok
        dims = self.rules[k].dims
        if ins.sum() > 1:
            st["in_several"] += 1
            if any((idx[a] == 0 and fr[a] == 0) or (idx[a] == dims[a] - 2 and fr[a] == 1)
                   for a in range(3)):
                st["on_shared_face"] += 1
        if cur is not None and k != cur:
            st["switch"] += 1
        return k, idx, fr

    def try_step(self, p, k1, h, steps, cur):
        F, st = self.F, self.stats
        ok, d = self.r0.usable(k1)
        if not ok:
            st["speed_overflow" if not d < np.inf else "speed_low"] += 1
            return None, None, SPEED
        hh, h6 = F(0.5) * h, h / F(6.0)
        seen, ks = [cur], [k1]
        for name in STAGES:
            if name == "q2":
                q = p + hh * k1
            elif name == "q3":
                q = p + hh * ks[1]
            elif name == "q4":
                q = p + h * ks[2]
            else:
                q = p + h6 * (((k1 + F(2) * ks[1]) + F(2) * ks[2]) + ks[3])
            got = self.locate(q, seen[-1])
            if got is None:
                st["grid_" + name] += 1
                if self.in_hull(q):
                    st["gap_" + name] += 1
                    if name == "q2" and self.inside_all(p + h * k1).any():
                        st["q2_gap_k1_inside"] += 1
                return None, None, GRID
            if self.near == "all" and self.near_bound(q):
                st["near_" + name] += 1
            k, idx, fr = got
            if k != seen[-1]:
                st["switch_" + name] += 1
            seen.append(k)
            if name != "pn":
                ks.append(self.rules[k].sample(self.rules[k].v, idx, fr))
        pn = q
        a = seen[0]
        for j, name in enumerate(STAGES[:3]):
            if seen[j + 1] != a and all(seen[i] == a for i in range(5) if i != j + 1):
                st["only_" + name] += 1
        if seen[4] == a and any(b != a for b in seen[1:4]):
            st["pn_back"] += 1
        if sum(seen[i] != seen[i + 1] for i in range(4)) >= 2:
            st["changes_2"] += 1
        if len({seen[1], seen[3], seen[4]}) == 3:
            st["three_blocks_in_step"] += 1
        if pn.tobytes() == p.tobytes():
            st["no_motion"] += 1
            return None, None, SPEED
        if steps >= self.max_steps:
            return None, None, STEPS
        return pn, got, None

    def lines(self, seeds, direction):
        if self.near:
            with np.errstate(all="ignore"):
                for s in np.asarray(seeds, F32):
                    if self.inside_all(s).any() and self.near_bound(s):
                        self.stats["near_seed"] += 1
        return super().lines(seeds, direction)


def lines_numpy(s, stats=None, near=None):
    return Rule(s, stats, near).lines(s["seeds"], s["direction"])


def restate(s, near=None):
    """(lines dict, counters) of a set."""
    st = collections.Counter()
    return lines_numpy(s, st, near), st


def nlanes(s):
    return len(s["seeds"]) * (2 if s["direction"] == BOTH else 1)


def mirrored(s):
    """The set whose BACKWARD lines are s's FORWARD ones: the negated fields."""
    return dict(s, direction=BACKWARD,
                blocks=[dict(b, vectors=-b["vectors"]) for b in s["blocks"]])


# ---- hard boxes ----

HB_SPACINGS = (("tenth", (0.1, 0.1, 0.1)), ("third", (1 / 3, 1 / 3, 1 / 3)),
               ("seventh", (0.7, 0.7, 0.7)), ("fine", (3e-5, 3e-5, 3e-5)),
               ("sub", (1e-38, 1e-38, 1e-38)), ("huge", (3e37, 3e37, 3e37)),
               ("mixed", (0.1, 1 / 3, 0.7)), ("wild", (3e-5, 0.7, 1e-38)))
HB_ORIGINS = (0.0, -0.0, 1e6, -123456.7, 1e-30)
HB_JOINTS = ("coincide", "overlap", "gap")   # the neighbour's origin: the face, a float below, above
HB_OFFSETS = (0, -1, 1, -2, 2, -3, 3)        # seeds in floats from a face


def far_face(o, n, s):
    """origin + (n - 1) * spacing in float."""
    return F32(F32(o) + F32(n - 1) * F32(s))


def hard_box(i):
    """Set i of the class: two or three blocks in a row along one axis,
    spacing, origin, joint, axis and size by i; a uniform field across the
    joint, other per block; seeds on, and one, two and three floats either side
    of every face of every axis; a step of eight floats of the first joint."""
    name, sp = HB_SPACINGS[i % len(HB_SPACINGS)]
    o = HB_ORIGINS[(i // len(HB_SPACINGS)) % len(HB_ORIGINS)]
    joint = i % 3
    ax = (i // 3) % 3
    n = 2 + i % 4
    nb = 3 if i % 5 == 0 else 2
    if max(sp) > 1e30:
        n = min(n, 3)          # the far face of the row stays finite
    origins, faces = [], []
    at = F32(o)
    for j in range(nb):
        org = [F32(o)] * 3
        org[ax] = at
        origins.append(org)
        face = far_face(at, n, sp[ax])
        faces.append(face)
        at = shift(face, (0, -1, 1)[joint])
    blocks = []
    for j, org in enumerate(origins):
        v = [0.0625 * j, 0.0625 * j, 0.0625 * j]
        v[ax] = 1.0
        blocks.append(bs.block(sh.uniform(n, n, n, v), [float(x) for x in org],
                               [float(F32(x)) for x in sp]))
    mid = [F32(F32(o) + F32(0.5 * (n - 1)) * F32(sp[a])) for a in range(3)]
    mid[ax] = F32(origins[i % nb][ax] + F32(0.5 * (n - 1)) * F32(sp[ax]))
    seeds = []
    for a in range(3):
        walls = [F32(o), far_face(o, n, sp[a])] if a != ax else [F32(o)] + faces
        for w in walls:
            for k in HB_OFFSETS:
                s = list(mid)
                s[a] = shift(w, k)
                seeds.append(s)
    step = float(F32(8.0) * np.spacing(np.abs(faces[0])))
    s = bs.block_set(blocks, seeds, step, i % 4, BOTH)
    s["hb"] = dict(spacing=name, origin=o, joint=HB_JOINTS[joint], axis=ax, n=n,
                   faces=faces, starts=[org[ax] for org in origins])
    return s


HB_COUNT = 40


@functools.lru_cache(maxsize=None)
def hard_boxes():
    return {"hb_%02d" % i: hard_box(i) for i in range(HB_COUNT)}


LANDING_ORIGINS = (0.0, 1e6, -123456.7)
LANDING_SPACINGS = (0.1, 1 / 3, 0.7)
LANDING_TRIES = (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6)


@functools.lru_cache(maxsize=None)
def landings():
    """One step from the middle of block 0 that puts p' within a few floats of
    the joint, from inside: the steps h, 13 adjacent floats about (face - p),
    for which the restatement's p' has a block membership that changes within 2
    floats, the first three of each pair kept."""
    out = {}
    for oi, o in enumerate(LANDING_ORIGINS):
        for si, sp in enumerate(LANDING_SPACINGS):
            ax, joint = (oi + si) % 3, (oi + 2 * si) % 3
            n = 3 + (oi + si) % 3
            o0 = F32(o)
            face = far_face(o0, n, sp)
            org1 = [float(o0)] * 3
            org1[ax] = float(shift(face, (0, -1, 1)[joint]))
            v0, v1 = [0.0, 0.0, 0.0], [0.125, 0.125, 0.125]
            v0[ax] = v1[ax] = 1.0
            blocks = [bs.block(sh.uniform(n, n, n, v0), [float(o0)] * 3, [float(F32(sp))] * 3),
                      bs.block(sh.uniform(n, n, n, v1), org1, [float(F32(sp))] * 3)]
            p0 = [F32(o0 + F32(0.5 * (n - 1)) * F32(sp))] * 3
            kept = 0
            for k in LANDING_TRIES:
                h = shift(F32(face - p0[ax]), k)
                s = bs.block_set(blocks, [p0], float(h), 2, FORWARD)
                L, st = restate(s, near="all")
                if h > 0 and st["near_pn"] and kept < 3:
                    out["land_%d%d_%+d" % (oi, si, k)] = s
                    kept += 1
    return out


# ---- many blocks ----

ROW_DISTINCT = 16


@functools.lru_cache(maxsize=None)
def row_arrays():
    """16 arrays of 2 x 2 x 2 points: (1 + k / 16, ((k % 4) - 1.5) / 4096, 0):
    600 steps of 0.75 drift by less than 0.2 in y."""
    return tuple(sh.uniform(2, 2, 2, (1.0 + k / 16.0, ((k % 4) - 1.5) / 4096.0, 0.0))
                 for k in range(ROW_DISTINCT))


def row_blocks(n):
    """block_stream_helpers.hop_blocks' row: n unit blocks of 2^3 points along
    x sharing planes; block k holds array k % 16, by reference."""
    arr = row_arrays()
    return [dict(vectors=arr[k % ROW_DISTINCT], origin=(float(k), 0.0, 0.0),
                 spacing=(1.0, 1.0, 1.0), cfield=None) for k in range(n)]


def row_seeds(n):
    """Inside the first, the middle, the last but one and the last block, on
    the plane of the last two, and outside every block."""
    return [[0.25, 0.5, 0.5], [n // 2 + 0.375, 0.25, 0.75], [n - 1.75, 0.5, 0.25],
            [n - 0.5, 0.5, 0.5], [n - 1.0, 0.75, 0.5], [n + 0.5, 0.5, 0.5], [-1.0, 0.5, 0.5]]


ROW_SIZES = (255, 256, 257, 4097, MAX_BLOCKS)


def many_blocks():
    out = {}
    for n in ROW_SIZES:
        out["row_%d" % n] = bs.block_set(row_blocks(n), row_seeds(n), 0.75, 12, BOTH)
    # one line through several hundred blocks, both ways
    out["row_4097_long"] = bs.block_set(row_blocks(4097), [[1500.5, 0.5, 0.5]], 0.75, 600, BOTH)
    out["row_257_reversed"] = bs.block_set(row_blocks(257)[::-1], row_seeds(257)
                                           + [[k + 0.0, 0.5, 0.5] for k in (1, 128, 256)],
                                           0.75, 12, BOTH)
    stack = [bs.block(sh.uniform(3, 3, 3, (1.0, (k - 20) / 64.0, 0.0))) for k in range(64)]
    seeds = [[0.25, 1.0, 1.0], [1.0, 1.0, 1.0], [1.5, 0.5, 1.75], [0.0, 0.0, 0.0], [2.0, 2.0, 2.0]]
    out["stack64"] = bs.block_set(stack, seeds, 0.25, 6, BOTH)
    out["stack64_reversed"] = bs.block_set(stack[::-1], seeds, 0.25, 6, BOTH)
    return out


# ---- the check pass ----

PROBE_N = 33
PROBE_SEEDS = 6000
PROBE_VALUES = (np.nan, np.inf, -np.inf)


@functools.lru_cache(maxsize=None)
def probe33():
    """One block of 33^3 points with a colour field: 107,811 vector floats
    (seven trips of the check pass), 35,937 colour samples (three), 6,000 seeds
    (18,000 floats, two)."""
    n = PROBE_N
    b = bs.block(sc.box_flow(n, n, n), cfield=sh.scalar_field((n, n, n), 6))
    s = bs.block_set([b], sh.random_seeds(PROBE_SEEDS, (n, n, n), 5), 0.125, 2, FORWARD,
                     cmap=(ch.table(29, 6), -0.5, 0.625))
    return s


def probe_positions(size):
    """An element in every trip of a loop over `size` elements (the first, the
    last of its trip, the first of its trip, then a third of the way in), and
    the last element."""
    trips = (size + TRIP - 1) // TRIP
    pos = []
    for t in range(trips):
        at = (0, TRIP - 1, 0, TRIP // 3)[min(t, 3)] if t < trips - 1 else (size - t * TRIP) // 2
        pos.append(t * TRIP + at)
    return pos + [size - 1]


PROBE_KINDS = (("vectors", "block 0"), ("cfield", "colour"), ("seeds", "seed"))


def probed(s, key, pos, value):
    """probe33 with one element of the block's vectors or colour field, or of
    the seeds, replaced."""
    if key == "seeds":
        a = s["seeds"].copy()
        a.reshape(-1)[pos] = value
        return dict(s, seeds=a)
    b = dict(s["blocks"][0])
    a = np.array(b[key], F32)
    a.reshape(-1)[pos] = value
    b[key] = a
    return dict(s, blocks=[b])


ROW300_BAD = (((299,), ()), ((17, 299), ()), ((299, 17, 250), ()), ((9,), (3,)))


@functools.lru_cache(maxsize=None)
def row300():
    """300 blocks of the row with colour fields, a few seeds."""
    blocks = [dict(b, cfield=sh.scalar_field((2, 2, 2), 40 + k % 5))
              for k, b in enumerate(row_blocks(300))]
    return bs.block_set(blocks, row_seeds(300)[:4], 0.75, 6, BOTH,
                        cmap=(ch.table(11, 3), -0.5, 0.625))


def row300_bad(bad_vectors, bad_colours):
    """row300 with a non-finite vector sample in blocks bad_vectors and a
    non-finite colour sample in blocks bad_colours, set in the order given."""
    s = row300()
    blocks = list(s["blocks"])
    for j, k in enumerate(bad_vectors):
        v = blocks[k]["vectors"].copy()
        v.reshape(-1)[(5 * j + 7) % v.size] = PROBE_VALUES[j % 3]
        blocks[k] = dict(blocks[k], vectors=v)
    for j, k in enumerate(bad_colours):
        g = blocks[k]["cfield"].copy()
        g.reshape(-1)[(3 * j + 1) % g.size] = PROBE_VALUES[(j + 1) % 3]
        blocks[k] = dict(blocks[k], cfield=g)
    return dict(s, blocks=blocks)


# ---- lanes and lengths ----

ORBIT_STEPS = 4100    # 128 x 4,101 + 128 x 4,100 points a workgroup: above 2^20


@functools.lru_cache(maxsize=None)
def orbits():
    """The rigid rotation on 17^3 points split 2 x 2 x 2, 513 seeds BOTH (1,026
    lanes, five workgroups) at radii 1.5 to 7 about the axis: RK4 contracts a
    circle by 1 - (h omega)^6 / 144 a step, so every half takes all its steps:
    513 lines of 2 x 4,100 + 1 points, 20 revolutions each."""
    rng = np.random.default_rng(17)
    r, a = rng.uniform(1.5, 7.0, 513), rng.uniform(0.0, 2 * np.pi, 513)
    seeds = np.stack([8.0 + r * np.cos(a), 8.0 + r * np.sin(a), rng.uniform(0.5, 15.5, 513)], -1)
    return bs.block_set(bs.split(sh.rotation(17, 0.125), (1.0, 1.0, 1.0)), seeds, 0.25,
                        ORBIT_STEPS, BOTH)


def two_blocks(f):
    """A field of stream_helpers at origin 0 as a set of two blocks, split
    across its longest axis (the lowest of equals)."""
    dims = f["vectors"].shape[2::-1]
    ax = int(np.argmax(dims))
    parts = [1, 1, 1]
    parts[ax] = 2
    assert tuple(f["origin"]) == (0.0, 0.0, 0.0)
    s = bs.block_set(bs.split(f["vectors"], f["spacing"], parts, f.get("cfield")), f["seeds"],
                     f["step"], f["max_steps"], f["direction"], f["min_speed"], f.get("cmap"))
    if f.get("tube"):
        s["tube"] = f["tube"]
    return s


def conveyor_blocks(length, planes=False):
    """stream_cases.conveyor(length) (planes) or the uniform field (1, 0, 0) as
    two blocks of 2^3 points that share the plane x = length / 2."""
    v = sc.conveyor(length) if planes else sh.uniform(2, 2, 2, (1, 0, 0))
    half = length / 2.0
    return [bs.block(v, (0.0, 0.0, 0.0), (half, 1.0, 1.0)),
            bs.block(v, (half, 0.0, 0.0), (half, 1.0, 1.0))]


def fullblock():
    """stream_cases.fullblock over two blocks: 257 lanes of 65,535 steps of 1.0
    from x = 0; points[65536 l + k] = (k, y_l, z_l), in block 0 up to x = 32768
    (its upper face holds the line) and in block 1 beyond; workgroup 0 sums to
    exactly 2^24 in both fields of the scan word."""
    f = sc.fullblock()["fullblock"]
    s = bs.block_set(conveyor_blocks(65536.0), f["seeds"], 1.0, sc.MAX_STEPS, FORWARD)
    s["tube"] = f["tube"]
    return s


def longest():
    """stream_cases.longest over two blocks that share x = 65536: the long
    line's backward half runs down block 0, its forward half crosses at once."""
    f = sc.longest()["longest"]
    s = bs.block_set(conveyor_blocks(131072.0, planes=True), f["seeds"], 1.0, sc.MAX_STEPS, BOTH)
    s["tube"] = f["tube"]
    return s


GAP_PICK = ("gaps_base_3", "gaps_first_4", "gaps_onlyN_7")


def gaps():
    g = sc.gaps()
    return {k: two_blocks(g[k]) for k in GAP_PICK}


# ---- mid-step block changes ----

MID_LAYOUTS = ("abut", "overlap", "gap", "three")


def mid_set(layout, seed):
    """Two or three blocks of 3^3 points in a row along x (abutting at x = 2,
    overlapping over [1.5, 2], with a gap (2, 2.25), or three abutting), the x
    component of each random per lattice point in [-2.5, 3], y and z constant
    and small; 24 random seeds within a cell of the joints, one step of 1.0
    at a time."""
    rng = np.random.default_rng(1000 * MID_LAYOUTS.index(layout) + seed)
    starts = dict(abut=(0.0, 2.0), overlap=(0.0, 1.5), gap=(0.0, 2.25), three=(0.0, 2.0, 4.0))[layout]
    blocks = []
    for x0 in starts:
        v = np.zeros((3, 3, 3, 3), F32)
        v[..., 0] = rng.uniform(-2.5, 3.0, (3, 3, 3))
        v[..., 1] = rng.uniform(-0.25, 0.25)
        v[..., 2] = rng.uniform(-0.25, 0.25)
        blocks.append(bs.block(v, (x0, 0.0, 0.0)))
    seeds = np.stack([rng.uniform(0.75, starts[-1] + 1.25, 24), rng.uniform(0.5, 1.5, 24),
                      rng.uniform(0.5, 1.5, 24)], -1)
    return bs.block_set(blocks, seeds, 1.0, 3, FORWARD)


# of the seeds 0 .. 29 of each layout, searched with the restatement: those whose
# counters show the most of MID_CLASSES (test_block_stream_cases.py asserts them)
MID_SEEDS = {"abut": (0, 18, 24), "overlap": (0, 3, 26), "gap": (7, 13, 21), "three": (4, 5, 29)}
MID_CLASSES = ("only_q2", "only_q3", "only_q4", "pn_back", "q2_gap_k1_inside", "gap_pn",
               "changes_2")


def mid_steps():
    """The searched sets and, of each, the mirror that runs BACKWARD."""
    out = {}
    for layout in MID_LAYOUTS:
        for seed in MID_SEEDS[layout]:
            s = mid_set(layout, seed)
            out["mid_%s_%d_fwd" % (layout, seed)] = s
            out["mid_%s_%d_back" % (layout, seed)] = mirrored(s)
    return out


def carried():
    """The small-field classes of stream_cases that bear on the block rk4 and
    advance, each field split in two across its longest axis."""
    fields = {}
    for cls in (sc.subnormal, sc.zeros_and_ties, sc.stall, sc.fast):
        fields.update(cls())
    th = sc.threshold()
    for k in ("turn_59.75", "turn_60.25", "turn_pair_repick", "turn_pair_carried"):
        fields[k] = th[k]
    return {"split_" + k: two_blocks(f) for k, f in fields.items()}


# ---- all of them ----

@functools.lru_cache(maxsize=None)
def small():
    """{name: set} of every class small enough for the numpy restatement."""
    out = {}
    out.update(hard_boxes())
    out.update(landings())
    out.update(many_blocks())
    out.update(gaps())
    out.update(mid_steps())
    out.update(carried())
    return out


def tube_of(s, i=0):
    return s.get("tube") or bs.tube_of(i)


def with_colors(s, seed):
    """s with a colour field per block and a map, unless it has them."""
    if s["blocks"][0].get("cfield") is not None or len(s["blocks"]) > 300:
        return s
    return bs.colored(s, seed)

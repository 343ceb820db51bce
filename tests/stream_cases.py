"""The hard classes of the streamline tests (test_stream_cases.py on the host,
test_gpu_stream_cases.py on the GPU), in stream_helpers' field(...) format.

Each class is a function returning {name: field}; a field may carry a "tube"
(radius, nsides, color) where the tube matters, else tube_of() picks one.  The
paths a class is there for stand next to its inputs and are asserted from the
numpy restatement by test_stream_cases.py.

Scale classes sit on the kernels' own boundaries (stream_kernels.hip,
stream_common.h): 256 lanes per block of the integration (LANES), 256 blocks per
chunk of the scan, 64 x 256 elements per trip of the check pass (TRIP), 25-bit
fields of the packed scan word, 24-bit lane counts.
"""
import collections
import functools

import numpy as np

import color_helpers as ch
import stream_helpers as sh

F32 = np.float32
FORWARD, BACKWARD, BOTH = sh.FORWARD, sh.BACKWARD, sh.BOTH
LANES = 256          # kBlock of stream_common.h: lanes per block
CHUNK = 256          # kScanBlock of stream_kernels.hip: blocks per chunk of the scan
TRIP = 64 * 256      # kCheckBlocks x kCheckBlock: elements per trip of the check loops
MAX_STEPS = 65535
FLT_MIN = F32(1.17549435e-38)
FLT_MAX = np.finfo(F32).max
# the smallest min_speed the API accepts: its float square is a normal float
MIN_SPEED = F32(np.sqrt(np.float64(FLT_MIN)))
while MIN_SPEED * MIN_SPEED < FLT_MIN:
    MIN_SPEED = np.nextafter(MIN_SPEED, F32(1))


def nlanes(f):
    return len(f["seeds"]) * (2 if f["direction"] == BOTH else 1)


def nblocks(f):
    return (nlanes(f) + LANES - 1) // LANES


def tube_of(f, i=0):
    """The field's tube, else one that varies with i."""
    return f.get("tube") or dict(radius=0.03125 * (1 + i % 3), nsides=3 + (5 * i) % 14,
                                 color=None if i % 3 == 1 else 0x00203040 + i)


def box_flow(nx, ny, nz, A=1.0, B=0.8, C=0.6):
    """The ABC flow on the lattice of [0, 2 pi]^3 with nx x ny x nz points."""
    x, y, z = sh.lattice(nx, ny, nz)
    x, y, z = 2 * np.pi * x / (nx - 1), 2 * np.pi * y / (ny - 1), 2 * np.pi * z / (nz - 1)
    return np.stack([A * np.sin(z) + C * np.cos(y), B * np.sin(x) + A * np.cos(z),
                     C * np.sin(y) + B * np.cos(x)], -1).astype(F32)


# ---- scale ----

PERIOD = 509   # prime: a tiling of 509 seeds never aligns with a block of 256 lanes
CHUNK_FIELDS = (("chunks256", 65536, FORWARD), ("chunks257", 32769, BOTH),
                ("chunks513", 131073, BACKWARD))


def chunk_flow():
    """abc(9) with the eight corners of cell (0, 0, 0) zeroed: a stagnant cell."""
    v = sh.abc(9)
    v[:2, :2, :2] = 0
    return v


def chunk_seeds():
    """The 509 distinct seeds: random in the 9^3 grid, three outside it, one in
    the stagnant cell."""
    s = sh.random_seeds(PERIOD, (9, 9, 9), 77)
    s[7] += F32(9.0)
    s[100, 1] = F32(-0.125)
    s[508, 2] = F32(8.5)
    s[300] = (0.5, 0.25, 0.75)
    return s


def chunks(distinct=False):
    """Fields of exactly 256, 257 and 513 blocks (one, two and three chunks of
    the scan; 65,536, 65,538 and 131,073 lanes), two steps of 0.0625 per half:
    at most 393,219 points.  distinct: the same fields over the 509 seeds."""
    flow, seeds = chunk_flow(), chunk_seeds()
    out = {}
    for name, n, d in CHUNK_FIELDS:
        s = seeds if distinct else seeds[np.arange(n) % PERIOD]
        out[name] = sh.field(flow, s, 0.0625, 2, d)
        out[name]["tube"] = dict(radius=0.03125, nsides=3 + n % 3, color=0x00405060)
    return out


def conveyor(length):
    """2 x 2 x 2, spacing (length, 1, 1): (1, 0, 0) on the z = 0 plane, so a
    step of 1.0 from (x, y, 0) is exactly (x + 1, y, 0) (h / 6.0f times 6
    rounds to 1.0f, integers below 2^24 are exact, a lerp at fraction 0 returns
    its first end); (0, 0.75, 0) on the z = 1 plane."""
    v = np.zeros((2, 2, 2, 3), F32)
    v[0, :, :, 0] = 1.0
    v[1, :, :, 1] = 0.75
    return v


def fullblock():
    """The uniform field (1, 0, 0) on 2 x 2 x 2 with spacing (65536, 1, 1): 257
    seeds FORWARD at x = 0 with distinct dyadic (y, z), 65,535 steps of 1.0
    each.  Block 0 sums to exactly 2^24 points and 2^24 tube points, lane 256
    starts at bbase 2^24.  points[65536 l + k] = (k, y_l, z_l), info {0, STEPS |
    STEPS << 8}."""
    l = np.arange(257)
    seeds = np.zeros((257, 3), F32)
    seeds[:, 1] = (l % 16) / 16.0
    seeds[:, 2] = (l // 16 % 16) / 16.0
    seeds[256, 1:] = 1.0 / 32.0
    f = sh.field(sh.uniform(2, 2, 2, (1, 0, 0)), seeds, 1.0, MAX_STEPS, FORWARD,
                 spacing=(65536.0, 1.0, 1.0))
    f["tube"] = dict(radius=0.125, nsides=3, color=0x00112233)
    return {"fullblock": f}


def longest():
    """One seed BOTH in the middle of a conveyor of 131,072: both halves take
    65,535 steps, one line of 131,071 points (k, 0, 0) with nback = 65535; at 16
    sides 2,097,138 vertices and 4,194,272 faces.  Then a seed on the z = 1
    plane, where the flow is (0, 0.75, 0): from y = 1 one step backward to
    y = 0.25, none forward: a line of two points after the long one."""
    seeds = [[65535.0, 0.0, 0.0], [1000.0, 1.0, 1.0]]
    f = sh.field(conveyor(131072), seeds, 1.0, MAX_STEPS, BOTH, spacing=(131072.0, 1.0, 1.0))
    f["tube"] = dict(radius=0.25, nsides=16, color=None)
    return {"longest": f}


GAP_OUT, GAP_STILL = "out", "still"


def gap_field(runs, nsides):
    """A 41 x 4 x 2 field: (1, 0, 0) on the rows y = 0, 1 and zero on the rows
    y = 2, 3.  runs: (kind, count) with kind "out" (a seed outside: an empty
    line), "still" (a seed in the stagnant rows: one point) or a number of
    points m (a seed at x = 40.5 - m, y in [0, 1]: m points at step 1)."""
    v = np.zeros((2, 4, 41, 3), F32)
    v[:, :2, :, 0] = 1.0
    seeds, want = [], []
    for kind, count in runs:
        for k in range(count):
            t = (len(seeds) % 17) / 16.0
            if kind == GAP_OUT:
                seeds.append((41.0 + t, 0.5, 0.5))
                want.append(0)
            elif kind == GAP_STILL:
                seeds.append((10.0 + t, 2.0 + t * 0.5, 0.5))
                want.append(1)
            else:
                seeds.append((40.5 - kind, t, 1.0 - t))
                want.append(kind)
    f = sh.field(v, seeds, 1.0, 100, FORWARD)
    f["tube"] = dict(radius=0.125, nsides=nsides, color=0x00010203 * nsides)
    f["want"] = np.array(want, np.int64)
    return f


def gaps():
    """About 1,500 seeds FORWARD per field, line lengths in runs: empty runs of
    300 (longer than a block, each across a block boundary) at the start, in the
    middle and at the end, 300 one-point lines, tubes of 2, 3 and 40 points.
    Variants: a tube on the first line, on the last line, the only tube at index
    0 and at index nseeds - 1.  Every nsides from 3 to 16 goes to one field."""
    O, S = GAP_OUT, GAP_STILL
    mid = [(40, 1), (S, 300), (2, 1), (3, 1), (40, 1), (O, 300), (2, 2), (S, 290)]
    layouts = {
        "base": [(O, 300)] + mid + [(O, 300)],
        "first": [(40, 1), (O, 300)] + mid + [(O, 299)],
        "last": [(O, 300)] + mid + [(O, 299), (3, 1)],
        "only0": [(2, 1), (O, 300), (S, 600), (O, 300), (S, 299)],
        "onlyN": [(O, 300), (S, 600), (O, 300), (S, 299), (40, 1)],
    }
    out = {}
    for k, ns in enumerate(range(3, 17)):
        name = list(layouts)[k % len(layouts)]
        out["gaps_%s_%d" % (name, ns)] = gap_field(layouts[name], ns)
    return out


# ---- the check pass ----

PROBE_DIMS = (33, 25, 21)
PROBE_SEEDS = 6000


def probe():
    """33 x 25 x 21: 51,975 vector floats (four trips of the check loop), 17,325
    colour samples (two trips), 6,000 seeds (18,000 floats, two trips)."""
    nx, ny, nz = PROBE_DIMS
    f = sh.field(box_flow(nx, ny, nz), sh.random_seeds(PROBE_SEEDS, PROBE_DIMS, 5), 0.125, 3,
                 FORWARD)
    f["cfield"] = sh.scalar_field((nz, ny, nx), 6)
    f["cmap"] = (ch.table(29, 6), -0.5, 0.625)
    f["tube"] = dict(radius=0.0625, nsides=4, color=None)
    return f


def probe_positions(n):
    """Element 0, the last of the first trip, the first of the second, one in
    between (in the last but one trip, or the middle of the second where there
    are only two) and the last element of an array of n floats."""
    trips = (n + TRIP - 1) // TRIP
    between = (trips - 2) * TRIP + TRIP // 3 if trips > 2 else TRIP + (n - TRIP) // 2
    return [0, TRIP - 1, TRIP, between, n - 1]


PROBE_KINDS = (("vectors", "vector"), ("seeds", "seed"), ("cfield", "colour"))
PROBE_VALUES = (np.nan, np.inf, -np.inf)


def probed(f, key, pos, value):
    """f with one element of its array `key` replaced."""
    a = np.array(f[key], F32)
    a.reshape(-1)[pos] = value
    return dict(f, **{key: a})


def probe_control(f):
    """f with values of FLT_MAX's scale and subnormals at the probe positions:
    finite, so accepted."""
    g = dict(f)
    vals = (FLT_MAX, F32(1e-42), -FLT_MAX, F32(-1.1e-38), F32(3e38))
    for key, _ in PROBE_KINDS:
        a = np.array(f[key], F32)
        for p, v in zip(probe_positions(a.size), vals):
            a.reshape(-1)[p] = v
        g[key] = a
    return g


# ---- arithmetic ----

def uniform_case(v, seeds=((1.5, 1.25, 1.0), (1.0, 1.0, 1.0)), step=0.25, max_steps=3, **kw):
    return sh.field(sh.uniform(3, 3, 3, v), seeds, step, max_steps, BOTH, **kw)


def subnormal():
    """Subnormal components beside normal ones: T_a = v_a / |v| is subnormal and
    decides the axis (a flushed one would tie with a zero and lose to the lower
    axis); d just above and just below msq at the smallest min_speed; squares
    that underflow; a colour field of subnormal samples over a subnormal range.
      sub_z0      (1, 1e-40, -0.0): axis 2, by |-0| < 1e-40
      sub_zy      (1, 2e-40, 1e-40): axis 2, by 1e-40 < 2e-40
      sub_x       (3e-39, 1, 0.5) and sub_y (0.5, 1e-45, 1): a subnormal T_a times T
      slowest*    |v| one float either side of MIN_SPEED, step 1e18
      tiny        (2e-19, 3e-23, -1e-42), min_speed 1.1e-19, step 1e18: real steps"""
    out = {}
    out["sub_z0"] = uniform_case((1.0, 1e-40, -0.0))
    out["sub_zy"] = uniform_case((1.0, 2e-40, 1e-40))
    out["sub_x"] = uniform_case((3e-39, 1.0, 0.5))
    out["sub_y"] = uniform_case((0.5, 1e-45, 1.0))
    ms = float(MIN_SPEED)
    up, dn = float(np.nextafter(MIN_SPEED, F32(1))), float(np.nextafter(MIN_SPEED, F32(0)))
    out["slowest_at"] = uniform_case((ms, 0.0, 0.0), step=1e18, min_speed=ms)
    out["slowest_up"] = uniform_case((0.0, -up, 1e-30), step=1e18, min_speed=ms)
    out["slowest_dn"] = uniform_case((0.0, 0.0, dn), step=1e18, min_speed=ms)
    out["tiny"] = uniform_case((2e-19, 3e-23, -1e-42), step=1e18, min_speed=1.1e-19)
    # a rotation of subnormal-scale speeds cannot be traced (msq is normal); its
    # samples are interpolated all the same before the speed test
    f = sh.field(sh.rotation(5) * F32(1e-39), sh.random_seeds(6, (5, 5, 5), 8), 0.5, 3, BOTH)
    out["sub_rotation"] = f
    g = sh.field(sh.abc(5), sh.random_seeds(6, (5, 5, 5), 9), 0.125, 6, BOTH)
    rng = np.random.default_rng(10)
    g["cfield"] = (rng.uniform(-1.0, 1.0, (5, 5, 5)) * 1e-38).astype(F32)
    g["cmap"] = (ch.table(4, 10), -1e-38, 1e-38)   # scale 4 / 2e-38 = 2e38: finite
    out["sub_colour"] = g
    return out


def zeros_and_ties():
    """+-0 in the two small components in every sign pattern, |T_x| == |T_y|
    with equal and opposite signs, all three equal, T along each axis in both
    directions: every one an exact tie of the axis rule, the lowest axis of the
    tie wins."""
    out = {}
    for a, sa in enumerate((0.0, -0.0)):
        for b, sb in enumerate((0.0, -0.0)):
            out["zero_%d%d" % (a, b)] = uniform_case((1.0, sa, sb))
    out["tie_xy_same"] = uniform_case((1.0, 1.0, 2.0))
    out["tie_xy_opp"] = uniform_case((1.0, -1.0, 2.0))
    out["tie_yz_same"] = uniform_case((2.0, -1.0, -1.0))
    out["tie_yz_opp"] = uniform_case((-2.0, 1.0, -1.0))
    out["tie_xz"] = uniform_case((0.3, 0.7, -0.3))
    out["tie_all"] = uniform_case((1.0, 1.0, 1.0))
    out["tie_all_signs"] = uniform_case((-0.7, 0.7, -0.7))
    for a in range(3):
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[a] = s
            out["axis_%d%s" % (a, "+" if s > 0 else "-")] = uniform_case(v)
    return out


def turn_field(c, s):
    """stream_helpers.corner_turn() with the flow (c, s, 0) from x = 2 on: one
    step of 1.5 from x = 1 lands past x = 2, where the tangent is (c, s, 0)
    normalised.  The seed's normal is (0, 1, 0) (T = (1, 0, 0): a tie of y and
    z), so |w|^2 = 1 - s^2 = c^2 against 0.25: carried up to 60 degrees."""
    v = np.zeros((2, 4, 4, 3), F32)
    v[:, :, :2, 0] = 1.0
    v[:, :, 2:, 0] = c
    v[:, :, 2:, 1] = s
    return sh.field(v, [[1.0, 0.25, 0.5]], 1.5, 2, FORWARD)


def repicks(f):
    st = collections.Counter()
    sh.lines_numpy(f, stats=st)
    assert st["repick"] + st["carried"] == 2, st
    return st["repick"] > 0


@functools.lru_cache(None)
def threshold_pair():
    """Adjacent float32 values (c_repick, c_carried) of the turned flow's x
    component, at s = float32(sin 60), between which the restatement's second
    point changes from the axis rule to the carried normal."""
    s = F32(np.sin(np.radians(60.0)))
    lo, hi = F32(np.cos(np.radians(60.25))), F32(np.cos(np.radians(59.75)))
    assert repicks(turn_field(lo, s)) and not repicks(turn_field(hi, s))
    lo, hi = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if repicks(turn_field(np.uint32(mid).view(F32), s)):
            lo = mid
        else:
            hi = mid
    return np.uint32(lo).view(F32), np.uint32(hi).view(F32), s


def threshold():
    """Turns of 56 to 64 degrees in steps of 0.25, then the adjacent pair of
    threshold_pair(): the frame is carried on one side and picked again on the
    other."""
    out = {}
    for q in range(56 * 4, 64 * 4 + 1):
        a = np.radians(q / 4.0)
        out["turn_%05.2f" % (q / 4.0)] = turn_field(F32(np.cos(a)), F32(np.sin(a)))
    lo, hi, s = threshold_pair()
    out["turn_pair_repick"] = turn_field(lo, s)
    out["turn_pair_carried"] = turn_field(hi, s)
    return out


EXIT_SEEDS = 49


def exit_field(axis, upper, direction):
    """The accelerating field (0.5, 1, 2, 4) along `axis` of a grid with 4
    points on that axis and 2 on the others; upper: the flow leaves through the
    upper face, else the mirror image leaves through the lower one.  BACKWARD
    integrates the negated field: the same points.  49 seeds 1/32 apart over
    the last cell and a half before the face, at step 1.0: from the face inward
    the step leaves at q2 (a cell deep), q3 (0.4 more), q4 (0.5 more) and p'
    (a band of 0.04, where the RK4 mean exceeds k3: one seed)."""
    speed = np.array([0.5, 1.0, 2.0, 4.0])
    if not upper:
        speed = -speed[::-1]
    if direction == BACKWARD:
        speed = -speed
    dims = [2, 2, 2]
    dims[axis] = 4
    v = np.zeros((dims[2], dims[1], dims[0], 3), F32)
    shape = [1, 1, 1]
    shape[2 - axis] = 4
    v[..., axis] = speed.reshape(shape)
    t = np.arange(EXIT_SEEDS) / float(EXIT_SEEDS - 1)
    seeds = np.zeros((EXIT_SEEDS, 3), F32)
    seeds[:, (axis + 1) % 3] = 0.25
    seeds[:, (axis + 2) % 3] = 0.625
    seeds[:, axis] = 1.0 + 1.5 * t if upper else 2.0 - 1.5 * t
    return sh.field(v, seeds, 1.0, 4, direction)


def exits():
    """Every stage at which a step leaves the grid (q2, q3, q4, p'), each at a
    lower and an upper face of each axis, forward and backward."""
    out = {}
    for axis in range(3):
        for upper in (True, False):
            for d in (FORWARD, BACKWARD):
                out["exit_%s%s_%s" % ("xyz"[axis], "+" if upper else "-",
                                      "fwd" if d == FORWARD else "back")] = exit_field(axis, upper, d)
    # Outside the grid a stage samples cell 0 of that axis, extrapolated.  With
    # the first two samples (3, 0) that value is about -6 past the upper face,
    # so the stages after a q3 or a q4 outside come back inside: only the test
    # of that one stage ends the line (a rule without it would take the step).
    f = exit_field(0, True, FORWARD)
    f["vectors"][..., 0] = np.array([3.0, 0.0, 2.0, 4.0], F32)
    f["seeds"][:, 0] = 2.0 + np.arange(EXIT_SEEDS, dtype=F32) / F32(EXIT_SEEDS - 1)
    out["exit_bent"] = dict(f, step=0.25)
    return out


def offlattice():
    """The ABC flow on 40 x 7 x 5 and its two cyclic transposes, origin (1e6,
    -0.1, 1/3) and spacing (0.1, 0.3, 1e-3) permuted with the axes: nothing is
    dyadic, and at 1e6 a float is 0.0625 apart.  Seeds from index space through
    float64, then the float on, below and above every face in world
    coordinates."""
    out = {}
    dims0, org0, sp0 = (40, 7, 5), (1e6, -0.1, 1.0 / 3.0), (0.1, 0.3, 1e-3)
    for r in range(3):
        perm = [(a + r) % 3 for a in range(3)]
        dims = [dims0[p] for p in perm]
        org = np.array([org0[p] for p in perm], F32)
        sp = np.array([sp0[p] for p in perm], F32)
        idx = sh.random_seeds(12, dims, 30 + r).astype(np.float64)
        world = org.astype(np.float64) + idx * sp.astype(np.float64)
        seeds = [w for w in world.astype(F32)]
        mid = (org.astype(np.float64) + 0.5 * (np.array(dims) - 1) * sp.astype(np.float64)).astype(F32)
        for a in range(3):
            hi = F32(np.float64(org[a]) + (dims[a] - 1) * np.float64(sp[a]))
            for face in (org[a], hi):
                for w in (np.nextafter(face, F32(-np.inf)), face, np.nextafter(face, F32(np.inf))):
                    s = mid.copy()
                    s[a] = w
                    seeds.append(s)
        f = sh.field(box_flow(*dims), seeds, 2.0 ** -11, 6, BOTH, origin=tuple(float(x) for x in org),
                     spacing=tuple(float(x) for x in sp))
        f["tube"] = dict(radius=2.0 ** -12, nsides=5 + r, color=0x00304050)
        out["off_%d" % r] = f
    return out


def stall():
    """The sink v = (1 - x, 0, 0) with the smallest min_speed: a line runs into
    x = 1 until a step moves nothing: SPEED by no motion after steps, the last
    point's tangent still that of a usable speed.  A seed on x = 1 has no speed."""
    seeds = [[0.25, 0.5, 0.5], [1.9, 0.25, 0.75], [0.3, 0.1, 0.2], [1.7, 0.9, 0.1],
             [0.999, 0.5, 0.5], [1.0, 0.5, 0.5]]
    return {"stall": sh.field(sh.sink(), seeds, 0.5, 120, BOTH, min_speed=float(MIN_SPEED))}


def fast():
    """d just below overflow (1.3e19 squared is 1.7e38) and just above it,
    steps of 1e-20 that still move by a tenth of a cell."""
    out = {}
    out["fast_x"] = uniform_case((1.3e19, 0.0, 0.0), step=1e-20, max_steps=5)
    out["fast_xyz"] = uniform_case((1.0e19, -1.0e19, 0.6e19), step=1e-20, max_steps=5)
    out["fast_over"] = uniform_case((1.1e19, 1.1e19, 1.1e19), step=1e-20, max_steps=5)
    out["fast_rotation"] = sh.field(sh.rotation(5) * F32(4e18), sh.random_seeds(6, (5, 5, 5), 12),
                                    2e-20, 6, BOTH)
    out["fast_rotation"]["tube"] = dict(radius=0.125, nsides=6, color=0x00607080)
    return out


ARITHMETIC = (subnormal, zeros_and_ties, threshold, exits, offlattice, stall, fast)


def arithmetic():
    """{name: field} of every arithmetic class."""
    out = {}
    for cls in ARITHMETIC:
        out.update(cls())
    return out

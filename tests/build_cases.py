"""The scale, key and batch classes of the device-build and refit tests
(test_build_cases.py on the host, test_gpu_build_cases.py on the GPU).

Each case is a Case(name, klass, verts, faces) made from numpy alone with fixed
seeds.  There is no restatement of the build here: the references are
spray_rt_bvh_build_device_host, the numpy forms of build_helpers /
refit_helpers and the oracle's brute force.  What a case is there for stands
in its docstring and is asserted from the host image by test_build_cases.py.

Scale classes sit on the kernels' own boundaries (build_kernels.hip,
refit_kernels.hip): 512 threads per workgroup of build_topology and
build_collapse (TREE_BLOCK: one chunk of a BFS level), 64 blocks of 256
triangles per slot of build_check (CHECK_TRIP), 4,096 blocks of 256 items of
build_keys and the refit kernels (GRID_TRIP).
"""
import collections
import functools

import numpy as np

import build_helpers as bh
import refit_helpers as rh

F32 = np.float32
TREE_BLOCK = 512             # kTreeBlock
CHECK_TRIP = 64 * 256        # kBuildParts x kCodeBlock
GRID_TRIP = 4096 * 256       # kMaxGridX x kRefitBlock, build_keys' 4,096 x kCodeBlock
ERR_ARG, ERR_LIMIT = -1, -5

Case = collections.namedtuple("Case", "name klass verts faces")


def case(name, klass, v, f):
    return Case(name, klass, np.ascontiguousarray(v, F32).reshape(-1, 3),
                np.ascontiguousarray(f, np.uint32).reshape(-1, 3))


# ---- triangles in chosen Morton cells ----

def cell_of(code):
    """(cx, cy, cz) of a 30-bit Morton code, x in the highest bit of a triple."""
    c = [0, 0, 0]
    for b in range(10):
        for a in range(3):
            c[a] |= ((code >> (3 * b + 2 - a)) & 1) << b
    return c


def cluster(centers, counts, half=(1.0 / 16, 1.0 / 16, 1.0 / 16)):
    """counts[i] different triangles whose box is centers[i] -+ half (exactly:
    the box centroid is the centre), up to 4,096 a centre: triangle k of a
    centre moves two coordinates that lie strictly inside its box by k % 64
    and k // 64 steps of half / 64."""
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    counts = np.asarray(counts, np.int64).reshape(-1)
    assert counts.max() <= 4096
    c = np.repeat(centers, counts, axis=0)
    k = np.concatenate([np.arange(n) for n in counts])
    h = np.broadcast_to(np.asarray(half, np.float64), c.shape)
    off = np.array([[-1.0, -1.0, -1.0], [1.0, -1.0, 0.0], [0.0, 1.0, 1.0]])
    tri = c[:, None, :] + off[None] * h[:, None, :]
    tri[:, 1, 2] += (k % 64) / 64.0 * h[:, 2]
    tri[:, 2, 0] -= (k // 64) / 64.0 * h[:, 0]
    v = tri.reshape(-1, 3).astype(F32)
    assert np.array_equal(v.astype(np.float64), tri.reshape(-1, 3))  # every coordinate is a float
    return v, np.arange(3 * len(c), dtype=np.uint32).reshape(-1, 3)


def unit_cells(codes, counts):
    """Triangles in the Morton cells `codes` of centroid bounds [0, 1024]^3 (one
    unit a cell, as build_helpers.stairs): centre = cell + 1/2; the callers add
    a triangle at 0 and one at 1024 on every axis, which pin the bounds."""
    return [[x + 0.5 for x in cell_of(c)] for c in codes], list(counts)


CORNERS = ([[0.0, 0.0, 0.0], [1024.0, 1024.0, 1024.0]], [1, 1])  # codes 0 and 2^30 - 1


def dups(n):
    """build_helpers.dups with n triangles: one centroid, one code, every split
    the median of the face order, so level k of the tree holds 2^k ranges."""
    return cluster([[1.0, 2.0, 3.0]], [n])


# ---- scale classes ----

LEVEL512_N = 2561   # the smallest of 2,561 .. 4,105, which all give 512


@functools.lru_cache(maxsize=None)
def level512():
    """dups(2,561): levels of 1, 2, 4 .. 512 nodes, the 512 ranges of level 9
    hold 5 or 6 triangles (inner) and their halves 2 or 3 (leaves).  The widest
    BFS level is exactly one chunk of build_topology."""
    return case("level512", "scale", *dups(LEVEL512_N))


LEVEL513_CLUSTER = 4100


def _level513(overlap):
    codes = [1 << 29] + [(1 << 29) + (1 << k) for k in range(9)]
    if overlap:
        cen, cnt = unit_cells(codes, [5] + [1] * 9)
        cen = [[0.5, 0.5, 0.5], [0.25, 0.25, 0.25]] + cen
        cnt = [2050, LEVEL513_CLUSTER - 1 - 2050] + cnt
        return cluster(cen + CORNERS[0], cnt + CORNERS[1])
    rng = np.random.default_rng(109)
    site = rng.choice(32 ** 3, LEVEL513_CLUSTER - 1, replace=False)
    cen = [(np.stack([site % 32, (site // 32) % 32, site // 1024], 1) + 0.5) / 32.0]
    cen.append(np.array(cell_of(codes[0]), np.float64) + [[.25, .25, .25], [.5, .25, .25],
                                                          [.25, .5, .25], [.25, .25, .5],
                                                          [.5, .5, .5]])
    cen.append(np.array([cell_of(c) for c in codes[1:]], np.float64) + 0.5)
    cen.append(np.array(CORNERS[0]))
    return bh._tiny_tris(np.concatenate(cen), 1.0 / 128)


@functools.lru_cache(maxsize=None)
def level513():
    """A construction (no search): 4,099 triangles 1/64 wide at different
    places of Morton cell 0 (the unit cube at the origin) beside the corner
    triangle at 0: 4,100 of code 0; on the other side of the root (code bit 29)
    a chain as build_helpers.stairs: five triangles of code 2^29, one each of
    2^29 + 2^k, k = 0..8, and the corner at 1024.  The root splits at bit 29.
    The code-0 side is a median tree whose level k (depth k + 1) holds 2^k
    nodes, 512 at depth 10: ranges of 8 and four of 9, whose upper halves of 5
    are the four inner nodes it has at depth 11.  The chain peels one triangle a
    level and has one inner node at every depth 1..11.  Depth 10 holds 513
    nodes, the chain's last: the first level of two chunks, the second chunk
    one node whose inner child is numbered after the four of the first (the
    carry)."""
    return case("level513", "scale", *_level513(False))


@functools.lru_cache(maxsize=None)
def level513_overlap():
    """The same tree over 4,099 triangles about two centres (as
    build_helpers.dups: they share a vertex and overlap): images only."""
    return case("level513_overlap", "scale", *_level513(True))


@functools.lru_cache(maxsize=None)
def levels3():
    """refit_helpers._grid(100): 20,000 triangles (build_check strides, all 64
    partials live), widest node level 1,200 and widest QNode4 level 1,347: three
    chunks each of build_topology and build_collapse."""
    return case("levels3", "scale", *rh._grid(100))


QLEVEL512_GRID = 60


@functools.lru_cache(maxsize=None)
def qlevel512():
    """refit_helpers._grid(60): the widest QNode4 level is exactly 512."""
    return case("qlevel512", "scale", *rh._grid(QLEVEL512_GRID))


QLEVEL513 = (66, 8147)  # (grid, faces kept): what find_qlevel(513) returns


def find_qlevel(want, grids=range(60, 70), step=5):
    """The search behind qlevel513 (40 s; not run by the tests, which assert
    its result): over the grids whose widest QNode4 level is at least `want`,
    the longest truncation of the face list, `step` faces at a time, whose
    widest QNode4 level is `want` with a live carry (build_helpers.carry_live)
    -> (grid, faces kept).  _grid(60) .. (63) give 512, 500, 502, 503; the first
    7,682 faces of _grid(64) give 513 too, but the one QNode4 of the second
    chunk has no inner child there."""
    def widest(v, f):
        q = bh.build_device_host(v, f)["qnodes4"]["child"]
        return max(bh.level_widths(q)), bh.carry_live(q, TREE_BLOCK)

    for g in grids:
        v, f = rh._grid(g)
        if widest(v, f)[0] < want:
            continue
        for n in range(len(f), len(f) - 1500, -step):
            if widest(v, f[:n]) == (want, True):
                return g, n
    return None


@functools.lru_cache(maxsize=None)
def qlevel513():
    """A search over truncations of a grid's face list (find_qlevel): the first
    8,147 of the 8,712 faces of _grid(66); the widest QNode4 level is exactly
    513, and the numbering of the last one's children needs the carry."""
    g, n = QLEVEL513
    v, f = rh._grid(g)
    return case("qlevel513", "scale", v, f[:n])


@functools.lru_cache(maxsize=None)
def check_edge():
    """The first 16,384 and 16,385 faces of _grid(91) (16,562): the last size
    build_check covers without a stride and the first with one."""
    v, f = rh._grid(91)
    return {"check_%d" % n: case("check_%d" % n, "scale", v, f[:n])
            for n in (CHECK_TRIP, CHECK_TRIP + 1)}


MILLION_GRID = 725


@functools.lru_cache(maxsize=None)
def million():
    """_grid(725): 1,051,250 triangles (> 4,096 x 256: build_keys and
    refit_tris stride), 527,076 vertices (1,581,228 normal floats: refit_commit
    strides), depth 24 by the depth rule (nmedian 112,114).  Its 166,531
    QNode4s are 666,124 children: refit_quant still covers them in one trip."""
    return case("million", "scale", *rh._grid(MILLION_GRID))


def scale_cases():
    """{name: Case} of the scale classes but `million`."""
    out = {c.name: c for c in (level512(), level513(), level513_overlap(), levels3(),
                               qlevel512(), qlevel513())}
    out.update(check_edge())
    return out


# ---- key classes ----

def _lattice(rng, n, hi=(64, 64, 64)):
    """n centres on multiples of 1/4 in [0, hi)."""
    return np.stack([rng.integers(0, 4 * h, n) / 4.0 if h else np.zeros(n) for h in hi], 1)


def flat():
    """Centroids without extent on one axis (z), and on two (y and z)."""
    r1, r2 = np.random.default_rng(101), np.random.default_rng(102)
    c1 = _lattice(r1, 300, (64, 64, 0)) + [0.0, 0.0, 2.0]
    c2 = _lattice(r2, 300, (64, 0, 0)) + [0.0, -3.0, 2.0]
    return [case("flat1", "key", *bh._tiny_tris(c1)), case("flat2", "key", *bh._tiny_tris(c2))]


def tiny_extent():
    """_grid(12) with z scaled to a centroid extent of about 2e-38 (x and y
    stay): 1024 / ext is inf on z, every z cell is 0 or 1023 (the centroid at
    the lower bound gives 0 * inf = NaN: cell 0), the differences x - lo are
    subnormal.  The triangles keep their area in x and y, so rays hit them."""
    v, f = rh._grid(12)
    v = v.copy()
    v[:, 2] = (v[:, 2].astype(np.float64) * (2e-38 / 1.5)).astype(F32)
    return case("tiny_extent", "key", v, f)


def tiny_all():
    """_grid(12) scaled to an extent of 2e-38 on every axis: every cell is 0 or
    1023.  No ray hits it (every Ng underflows to 0): images only."""
    v, f = rh._grid(12)
    return case("tiny_all", "key", (v.astype(np.float64) * (2e-38 / 6.0)).astype(F32), f)


def subnormal():
    """_grid(12) scaled to 1e-42: every coordinate subnormal.  Refused with
    ERR_LIMIT (no quantization grid)."""
    v, f = rh._grid(12)
    return case("subnormal", "key", (v.astype(np.float64) * (1e-42 / 6.0)).astype(F32), f)


def huge():
    """_grid(12) scaled to +-1.2e38 (hi - lo is finite, 1024 / ext is subnormal
    times 2^k: about 4e-36) beside _grid(12) itself: the triangles at 1e37 have
    an Ng that overflows and are never hit, the unit ones are all in one cell
    of the keys and of the quantization grid, and rays are built around them."""
    v, f = rh._grid(12)
    big = (v.astype(np.float64) * (1.2e38 / 3.0)).astype(F32)
    return case("huge", "key", np.concatenate([big, v]), np.concatenate([f, f + len(v)]))


def huge_ray_verts():
    """The vertices check_queries builds the rays of `huge` around: its unit
    half (the far half's own box overflows the ray generators)."""
    c = huge()
    v = c.verts.copy()
    n = len(v) // 2
    v[:n] = v[n:]
    return v


def overflow():
    """Two groups of triangles a few floats wide at -3e38 and +3e38: vertices
    and edges are finite, hi - lo of the centroids is inf, the scale 0, and
    (x - lo) * 0 is NaN for the upper group (inf * 0).  Every cell is 0."""
    rng = np.random.default_rng(103)
    base = F32(3e38)
    step = float(np.spacing(base))
    k = rng.integers(0, 64, (200, 3, 3)).astype(np.float64)
    sign = np.where(np.arange(200) % 2 == 0, 1.0, -1.0)[:, None, None]
    v = (sign * (float(base) - k * step)).reshape(-1, 3).astype(F32)
    return case("overflow", "key", v, np.arange(600, dtype=np.uint32).reshape(-1, 3))


def ulps():
    """300 triangles whose centroids are 1e6 + k * 0.0625 (k = 0..5, 0..3,
    0..6 per axis: single floats apart, 168 places): many equal codes, and a
    scale 1024 / (5 * 0.0625) that is not a float."""
    rng = np.random.default_rng(104)
    k = np.stack([rng.integers(0, 6, 300), rng.integers(0, 4, 300), rng.integers(0, 7, 300)], 1)
    k[:3] = [[0, 0, 0], [5, 3, 6], [5, 0, 6]]
    return case("ulps", "key", *cluster(1e6 + k * 0.0625, np.ones(300, int), (1.0, 1.0, 1.0)))


def at_hi():
    """300 triangles, a third of them with the centroid exactly at the upper
    bound of x, a third at that of y (some both) and 40 at that of z: t = 1024
    there, clamped to cell 1023."""
    rng = np.random.default_rng(105)
    c = _lattice(rng, 300, (24, 24, 24))
    c[0:100, 0] = 24.0
    c[60:160, 1] = 24.0
    c[200:240, 2] = 24.0
    return case("at_hi", "key", *bh._tiny_tris(c))


TWO_CELLS_N = 20000


def two_cells():
    """20,000 triangles at different places of [0, 8)^3 and one at 16384: two
    codes, a run of 20,000 equal ones split at medians all the way down."""
    rng = np.random.default_rng(106)
    pick = rng.choice(32 ** 3, TWO_CELLS_N, replace=False)
    c = np.stack([pick % 32, (pick // 32) % 32, pick // 1024], 1) / 4.0
    c = np.concatenate([c, [[16384.0, 16384.0, 16384.0]]])
    return case("two_cells", "key", *bh._tiny_tris(c))


DEEP_CHAIN = 10
DEEP_CLUSTER = 16384


def deep_stack():
    """A chain along x whose every level adds three entries to the walk stack.
    Centroids differ in x alone (cells of one unit, the bounds pinned at 0 and
    1024), so triangles may be as large in y and z as wanted.  Level d = 0..9
    of the chain splits cells [0, 2^(10-d)) at x bit 9 - d: the upper half S_d
    holds two triangles in cell 2^(9-d) and six in cell 3 * 2^(8-d) (one code:
    a median split into two leaves), all 2^(11-d) wide in y and z, twice as
    wide as anything in the lower half.  The collapse of the chain node expands
    S_d and its six-triangle half first (the largest boxes) and keeps the
    lower half as one child: four children for one level of depth.  Cell 0 ends
    the chain with 16,384 small triangles of one code, a median tree 12 levels
    high, in which the stack rule then refuses expansions: stack_bound is
    kQ4Stack = 40 exactly, and 2,047 QNode4s keep an inner child unexpanded
    with room for it among their four (test_build_cases.py asserts both)."""
    cen, cnt, half = [], [], []
    for d in range(DEEP_CHAIN):
        w = 2.0 ** (10 - d)
        lo, up = 2 ** (9 - d), 3 * 2 ** (8 - d) if d < 9 else 1
        groups = [(lo, 2), (up, 6)] if d < 9 else [(1, 7)]
        if d == 0:
            groups = [(lo, 2), (up, 4), (1024, 1)]
        for cell, n in groups:
            cen.append([float(cell), 0.0, 0.0])
            cnt.append(n)
            half.append([1.0 / 16, w, w])
    v, f = [], []
    for c, n, h in zip(cen, cnt, half):
        vv, ff = cluster([c], [n], h)
        f.append(ff + sum(len(x) for x in v))
        v.append(vv)
    per = DEEP_CLUSTER // 4
    for k in range(4):
        vv, ff = cluster([[0.0, 0.0, 0.0]], [per], (1.0 / 16, 0.25 + k / 16.0, 0.25 + k / 16.0))
        f.append(ff + sum(len(x) for x in v))
        v.append(vv)
    return case("deep_stack", "key", np.concatenate(v), np.concatenate(f))


def degenerate():
    """_grid(14) with zero-area faces scattered through the list: (a, a, b),
    (a, b, a), (a, a, a), three different vertices at one point, and three
    collinear ones, 16 of each."""
    v, f = rh._grid(14)
    rng = np.random.default_rng(107)
    nv = len(v)
    a, b = rng.integers(0, nv, 16), rng.integers(0, nv, 16)
    extra, faces = [], [np.stack([a, a, b], 1), np.stack([a, b, a], 1), np.stack([b, b, b], 1)]
    for i in range(16):   # coincident: three new vertices at one point
        extra += [v[a[i]]] * 3
    faces.append(nv + np.arange(48).reshape(16, 3))
    for i in range(16):   # collinear: p, p + d, p + 2 d, exactly
        p = np.round(v[b[i]].astype(np.float64) * 64) / 64
        d = np.array([0.25, -0.125, 0.0625])
        extra += [p, p + d, p + 2 * d]
    faces.append(nv + 48 + np.arange(48).reshape(16, 3))
    allf = np.concatenate([f] + [x.astype(np.uint32) for x in faces])
    order = rng.permutation(len(allf))
    return case("degenerate", "key", np.concatenate([v, np.array(extra, F32)]), allf[order])


def twins():
    """_grid(12) with 60 of its faces listed twice, 60 again as (b, c, a), 60 as
    (a, c, b) (the other winding), and 30 over copies of their vertices, in a
    shuffled list: equal centroids and codes, ties of (t, primID)."""
    v, f = rh._grid(12)
    rng = np.random.default_rng(108)
    pick = rng.choice(len(f), 210, replace=False)
    again, rot, flip, copy = pick[:60], pick[60:120], pick[120:180], pick[180:]
    cv = v[f[copy]].reshape(-1, 3)
    cf = (len(v) + np.arange(90)).reshape(30, 3).astype(np.uint32)
    allf = np.concatenate([f, f[again], f[rot][:, [1, 2, 0]], f[flip][:, [0, 2, 1]], cf])
    return case("twins", "key", np.concatenate([v, cv]), allf[rng.permutation(len(allf))])


def stairs_wide():
    """build_helpers.stairs with 100 triangles in each of its 30 cells 2^k (and
    5 at cell 0): 3,007 triangles; the bit splits alone would be 30 + 5 levels
    deep, the depth rule cuts in."""
    codes = [0] + [1 << k for k in range(30)]
    cen, cnt = unit_cells(codes, [5] + [100] * 30)
    return case("stairs_wide", "key", *cluster(cen + CORNERS[0], cnt + CORNERS[1]))


@functools.lru_cache(maxsize=None)
def key_cases():
    cs = flat() + [tiny_extent(), tiny_all(), subnormal(), huge(), overflow(), ulps(), at_hi(),
                   two_cells(), deep_stack(), degenerate(), twins(), stairs_wide()]
    return {c.name: c for c in cs}


# what spray_rt_bvh_build_device_host answers for a key case: 0 or the error
OUTCOME = {"subnormal": ERR_LIMIT, "overflow": ERR_LIMIT}

QUERIED = ("level513", "levels3", "two_cells", "degenerate", "twins", "tiny_extent", "huge",
           "deep_stack", "stairs_wide")


def ray_verts(name):
    """The vertices check_queries builds rays around, None: the case's own.

    level513, two_cells: the dense cluster alone (every other vertex moved to
    the cluster's first).  Around the whole mesh the rays start 2,000 and more
    from triangles 1/8 wide; at grazing incidence the rounding error of t (0.4
    at t = 2,485) then exceeds the leaf boxes, a triangle's t falls outside its
    own box's interval, and a walk that culls by the best t so far can differ
    from brute force whatever the tree (3 of 3,063 rays did, around the whole
    of the mesh that is now level513_overlap).
    tiny_extent: _grid(12) itself.  Rays in the plane of triangles thinner
    than 1e-20 are out: the slab test clamps a zero direction component to
    1e-20, so it gives such a box an interval of t of about 1e-18 and misses
    what brute force hits (139 of 3,063 rays did, all along x or y)."""
    if name == "huge":
        return huge_ray_verts()
    if name == "tiny_extent":
        return rh._grid(12)[0]
    if name in ("level513", "two_cells"):
        c = small()[name]
        n = 3 * (LEVEL513_CLUSTER - 1 if name == "level513" else TWO_CELLS_N)
        v = c.verts.copy()
        v[n:] = v[0]
        return v
    return None


@functools.lru_cache(maxsize=None)
def small():
    """{name: Case} of every scale and key case but `million`."""
    out = dict(scale_cases())
    out.update(key_cases())
    return out


# ---- batch classes ----

def named(name, oracle=None):
    """The meshes of build_helpers by name, as cases."""
    if name == "empty":
        v, f = rh._fan(1)
        return case("empty", "batch", v[:0], f[:0])
    if name == "dups":
        return case("dups", "batch", *bh.dups())
    return case(name, "batch", *bh.mesh(name, oracle))


def mixed():
    """One call whose grid is sized by its largest mesh: most blocks see none
    of a small slot's triangles."""
    return [levels3(), named("empty"), named("tri1"), named("dups"), level513(), named("tri5")]


def mixed_orders():
    m = mixed()
    return {"as_listed": m, "reversed": m[::-1], "rotated": m[2:] + m[:2]}


# rocPRIM's segmented_radix_sort configuration for 8-byte integer keys without
# values on gfx950 (rocprim/device/detail/config/device_segmented_radix_sort.hpp
# has no entry for this architecture, so default_segmented_radix_sort_config_base<6>
# of device_config_helper.hpp holds): 6 radix bits, blocks of 128 threads x 17
# keys, WarpSortConfig<32, 4, 256, 3000, 32, 4, 256>.
SORT_PARTITION = 3000   # segments: from here the call partitions them by size
SORT_SMALL = 32 * 4     # keys: up to here a segment is sorted by one logical warp
SORT_MEDIUM = 32 * 4    # the medium bound equals the small one: two-way partitioning
SORT_BLOCK = 128 * 17   # keys: up to here by one block in registers, above it radix passes
MANY_SIZES = (0, 1, 4, 5, 40, SORT_SMALL - 1, SORT_SMALL, SORT_SMALL + 1, 288, 1030,
              SORT_BLOCK, SORT_BLOCK + 1)


@functools.lru_cache(maxsize=None)
def many_meshes():
    """Twelve meshes of MANY_SIZES triangles: the sizes either side of the
    warp-sort bound (128) and of the one-block bound (2,176), zero, and the
    halvings of the one-block sort (the block sort tries 17, 8, 4, 2, 1 keys a
    thread: 2,176, 1,024, 512, 256, 128)."""
    v91, f91 = rh._grid(40)
    out = []
    for i, n in enumerate(MANY_SIZES):
        if n == 40:
            c = case("many_40", "batch", *bh.dups())
        elif n == 288:
            c = case("many_288", "batch", *rh._grid(12))
        elif n <= 5:
            v, f = rh._fan(max(n, 1))
            c = case("many_%d" % n, "batch", v if n else v[:0], f[:n])
        else:
            c = case("many_%d" % n, "batch", v91, np.roll(f91, -37 * i, axis=0)[:n])
        assert len(c.faces) == n
        out.append(c)
    return tuple(out)


def many(nslots):
    """nslots slots cycling through many_meshes(), the cycle started at 5."""
    m = many_meshes()
    return [m[(5 + k) % len(m)] for k in range(nslots)]


MANY_CALLS = (SORT_PARTITION, SORT_PARTITION - 1)


def poison_positions():
    """Triangles of levels3 at the block and the stride boundary of build_check."""
    n = len(levels3().faces)
    return (0, 255, 256, CHECK_TRIP - 1, CHECK_TRIP, n - 1)


def poisoned(kind, tri):
    """levels3 with triangle `tri` made bad: kind "face": an index out of range;
    "nan": a NaN in a vertex only that triangle refers to."""
    c = levels3()
    v, f = c.verts, c.faces.copy()
    if kind == "face":
        f[tri, tri % 3] = len(v) + tri % 2
        return case("bad_face_%d" % tri, "batch", v, f)
    v = np.concatenate([v, [[np.nan, 0.0, 0.0]]]).astype(F32)
    f[tri, (tri + 1) % 3] = len(v) - 1
    return case("bad_nan_%d" % tri, "batch", v, f)

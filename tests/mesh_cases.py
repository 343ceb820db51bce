"""Hard meshes, fields and batches for the five mesh extractions (DESIGN.md
sections 12 and 14 to 17), shared by test_mesh_cases.py (host restatements
against numpy, and that every class reaches the path it exists for) and
test_gpu_mesh_cases.py (kernels against the host restatements).

Every case is a mesh dict of the existing helpers (cell_helpers.mesh,
tet_helpers.mesh, iso_helpers.grid) with two more keys, "klass" and "name".
There is no restatement here: references are the helpers'.

Topology classes (cell meshes; those of tets only also serve the tet call):
fan, duplicates, nonmanifold, nonconforming, collapsed, flat.  Field classes
(a renumbered hex lattice of 6x5x4 points, its Kuhn tet mesh, structured
grids): onlevel, zeros, subnormal, huge, ulps, constant.  Structured grids
only: pencils.
"""
import numpy as np

import cell_helpers as ch
import iso_helpers as ih
import surface_helpers as sh
import tet_helpers as th

F32 = np.float32
NFAN = 640
FMAX = float(np.finfo(F32).max)
TYPES = (ch.TET, ch.HEX, ch.WEDGE, ch.PYRAMID)
TYPE_NAME = {ch.TET: "tet", ch.HEX: "hex", ch.WEDGE: "wedge", ch.PYRAMID: "pyramid"}
LATTICE = (6, 5, 4)


def decoration(k):
    """Keywords of cell_helpers.mesh by a counter: normals on odd counts; no
    colour, a constant colour, tables of 1, 16 and 4096 entries in turn."""
    kw = dict(normals=bool(k & 1))
    which = k % 5
    if which == 1:
        kw["color"] = 0x00102030 + k
    elif which > 1:
        kw.update(cmap_seed=20 + k, ntable=(1, 16, 4096)[which - 2], clamp=0.5)
    return kw


def case(klass, name, geometry, f, iso, k):
    m = ch.mesh(geometry, f, iso, **decoration(k))
    m.update(klass=klass, name=name)
    return m


def with_normals(m):
    """m with seeded point normals where it has none."""
    if m.get("normals") is not None:
        return m
    rng = np.random.default_rng(len(m["points"]) + 1)
    return dict(m, normals=rng.normal(size=np.shape(m["points"])).astype(F32))


def by_position(conn, values):
    """A field that gives the point at listed position k values[k]."""
    conn = np.asarray(conn)

    def f(p):
        out = np.zeros(len(p))
        out[conn] = np.asarray(values, np.float64)[:len(conn)]
        return out
    return f


# ---- fans ----
def fan_geometry(ctype, half, place, n=NFAN):
    """n tets (a, b, r_k, r_k+1) or wedges (a, r_k, r_k+1, b, s_k, s_k+1) round
    the edge a = (0, 0, 0), b = (0, 0, 1), over a full turn or half of one, with
    a and b at the two lowest, two highest or two middle point indices
    -> (geometry, a, b)."""
    nr = n + 1 if half else n
    ang = (np.pi if half else 2 * np.pi) * np.arange(nr) / n
    x, y = np.cos(ang), np.sin(ang)
    if ctype == ch.TET:
        ring = np.stack([x, y, 0.5 + 0.1 * np.sin(3 * ang)], 1)
    else:
        ring = np.concatenate([np.stack([x, y, 0 * x], 1), np.stack([x, y, 0 * x + 1], 1)])
    at = {"lowest": 0, "middle": len(ring) // 2, "highest": len(ring)}[place]
    pts = np.concatenate([ring[:at], [[0, 0, 0], [0, 0, 1]], ring[at:]]).astype(F32)
    a, b = at, at + 1
    idx = lambda r: r if r < at else r + 2     # ring position -> point index
    lists = []
    for k in range(n):
        k1 = (k + 1) % nr
        if ctype == ch.TET:
            lists.append([a, b, idx(k), idx(k1)])
        else:
            lists.append([a, idx(k), idx(k1), b, idx(nr + k), idx(nr + k1)])
    return (pts,) + ch.cells([ctype] * n, lists), a, b


def fan_f(ctype, crossing):
    """A field that separates a from b in every cell, or one that leaves both
    outside and cuts the ring."""
    if not crossing:
        return lambda p: p[:, 0].astype(np.float64) - 0.2 + 0.1 * p[:, 2]
    if ctype == ch.TET:     # b alone inside: three crossing edges per tet
        return lambda p: p[:, 2].astype(np.float64) - 0.8
    return lambda p: p[:, 2].astype(np.float64) - 0.5 + 0.05 * p[:, 0]


def fans():
    """Twelve fans whose field crosses (a, b) and one control whose field does not."""
    out, k = [], 0
    for ctype in (ch.TET, ch.WEDGE):
        for half in (False, True):
            for place in ("lowest", "highest", "middle"):
                geom, a, b = fan_geometry(ctype, half, place)
                name = "fan-%s-%s-%s" % (TYPE_NAME[ctype], "half" if half else "full", place)
                m = case("fan", name, geom, fan_f(ctype, True), 0.0, k)
                m.update(ab=(a, b), half=half, place=place, crossing=True)
                out.append(m)
                k += 1
    geom, a, b = fan_geometry(ch.WEDGE, True, "middle")
    m = case("fan", "fan-wedge-half-control", geom, fan_f(ch.WEDGE, False), 0.0, k)
    m.update(ab=(a, b), half=True, place="middle", crossing=False)
    return out + [m]


# ---- duplicates ----
def repeated(geometry, which, count):
    """The geometry with cell `which` listed count times in a row."""
    p, types, offsets, conn = geometry
    lists = [conn[offsets[i]:offsets[i + 1]].tolist() for i in range(len(types))]
    order = list(range(which)) + [which] * count + list(range(which + 1, len(types)))
    return (p,) + ch.cells([int(types[i]) for i in order], [lists[i] for i in order])


def duplicates():
    """The middle hex of three in a row, and a tet of a Kuhn mesh, listed 2, 3
    and 300 times; the host tests' three-hex and two-hex meshes."""
    out, k = [], 0
    f = lambda q: th.wave_f(q) - 1.9
    # cuts the cells at x in [1, 2]
    g = lambda q: q[:, 0].astype(np.float64) - 1.4 + 0.1 * q[:, 1] + 0.05 * q[:, 2]
    row = ch.hex_lattice((4, 2, 2), seed=4)
    kp, kt = th.kuhn_mesh((3, 3, 2))
    kp, kl = ch.renumbered(kp, kt.tolist(), 6)
    kuhn = (kp,) + ch.cells([ch.TET] * len(kl), kl)
    for count in (2, 3, 300):
        out.append(case("duplicates", "hex-x%d" % count, repeated(row, 1, count), g, 0.0, k))
        out.append(case("duplicates", "tet-x%d" % count, repeated(kuhn, 7, count), g, 0.0, k + 1))
        k += 2
    p, types, offsets, conn = ch.hex_lattice((3, 2, 2), seed=4)
    two = conn.reshape(2, 8)
    three = (p,) + ch.cells([ch.HEX] * 3, [two[0], two[0], two[1]])
    out.append(case("duplicates", "three-hex", three, f, 0.0, k))
    out.append(case("duplicates", "two-hex", (p,) + ch.cells([ch.HEX] * 2, [two[0], two[0]]),
                    f, 0.0, k + 1))
    return out


# ---- non-manifold and non-conforming meshes ----
def nonmanifold():
    """Two regions of a lattice touching along an edge (a cells select), and a
    face shared by three cells: three tets on a triangle, three pyramids on a quad."""
    m = case("nonmanifold", "edge", ch.hex_lattice((3, 3, 2), seed=2), th.wave_f, 1.6, 1)
    m["cells_select"] = sh.select("cells", 1.0, 1.0, np.array([1, 0, 0, 1], F32))
    pts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0.2, 0.2, 1), (0.3, 0.3, -1), (0.25, 0.3, 2)]
    p, lists = ch.renumbered(pts, [[0, 1, 2, 3], [0, 2, 1, 4], [1, 2, 0, 5]], 3)
    t = case("nonmanifold", "three-tets", (p,) + ch.cells([ch.TET] * 3, lists),
             lambda q: q[:, 2].astype(np.float64) - 0.4 + 0.2 * q[:, 0], 0.0, 2)
    pts = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0.5, 0.5, 1), (0.4, 0.5, -1), (0.5, 0.6, 2)]
    p, lists = ch.renumbered(pts, [[0, 1, 2, 3, 4], [1, 2, 3, 0, 5], [3, 2, 1, 0, 6]], 5)
    q = case("nonmanifold", "three-pyramids", (p,) + ch.cells([ch.PYRAMID] * 3, lists),
             lambda q: q[:, 2].astype(np.float64) - 0.4 + 0.2 * q[:, 0], 0.0, 3)
    return [m, t, q]


def nonconforming():
    """A hex over two tets through both diagonals of the shared quad, and the
    mixed mesh whose pyramid is cut into tets, over seeds."""
    out, k = [], 0
    for through_min in (True, False):
        for seed in (None, 1, 2, 3, 5):
            name = "cut-%s-%s" % ("min" if through_min else "other", seed)
            out.append(case("nonconforming", name, sh.cut_quad_mesh(through_min, seed),
                            ch.sphere((0.4, 0.6, 0.1), 0.9), 0.0, k))
            k += 1
    for seed in (3, 11):
        out.append(case("nonconforming", "mixed-%d" % seed, ch.mixed_mesh(seed),
                        ch.sphere((1.0, 0.7, 0.8), 1.7), 0.0, k))
        k += 1
    return out


# ---- collapsed cells ----
PATTERNS = (0x01, 0x02, 0x0C, 0x10, 0x35, 0x5A, 0xE8, 0x7F)   # bit k: position k is inside


def collapsed():
    """Every single-position collapse conn[i] = conn[j], i != j, of one cell of
    each type under eight sign patterns by listed position (944 one-cell
    meshes), with a mesh without cells or one the level misses after every
    eighth: the many-segment batch."""
    out, k = [], 0
    for ctype in TYPES:
        n = ch.NPOINTS[ctype]
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                for s, bits in enumerate(PATTERNS):
                    p, types, offsets, conn = ch.one_cell(ctype, k % 7)
                    vals = [(1 if (bits >> q) & 1 else -1) * (0.5 + 0.1 * q) for q in range(n)]
                    f = by_position(conn, vals)
                    conn = conn.copy()
                    conn[i] = conn[j]
                    m = case("collapsed", "%s-%d=%d-%02x" % (TYPE_NAME[ctype], i, j, bits),
                             (p, types, offsets, conn), f, 0.0, k)
                    out.append(m)
                    k += 1
                    if k % 16 == 8:
                        e = dict(m, name="no-cells-%d" % k, types=types[:0], offsets=offsets[:1],
                                 conn=conn[:0])
                        out.append(e)
                    elif k % 16 == 0:
                        out.append(dict(m, name="missed-%d" % k, iso=5.0))
    return out


# ---- flat cells and slivers ----
def flat():
    """One cell of each type with its points exactly coplanar (small integer
    coordinates, so every float32 product is exact and every determinant 0;
    hexes and wedges in a tilted plane), and slivers: the same footprint at
    coordinates float32 rounds, with heights of a few 1e-7 of either sign, so
    the determinants of the split's tets lie within 1e-6 of the product of their
    edge lengths on both sides of 0.  Then the same moved by 1e6, where the
    float32 spacing is 1/16 and the slivers' heights are -1, 0 or 1 of it."""
    out, k = [], 0
    rng = np.random.default_rng(17)
    for far in (False, True):
        for ctype in TYPES:
            U = np.rint(ch.UNIT[ctype].astype(np.float64) * 4)
            n = len(U)
            X, Y = U[:, 0] + 3 * U[:, 2], U[:, 1] + U[:, 2]    # distinct points of the plane
            for kind in ("flat", "sliver-a", "sliver-b", "sliver-c"):
                if kind == "flat":
                    Z = X + 2 * Y if ctype in (ch.HEX, ch.WEDGE) else 0 * X
                    q = np.stack([X, Y, Z], 1) + (1e6 if far else 0)
                elif far:
                    q = np.stack([X, Y, rng.integers(-1, 2, n) / 16.0], 1) + 1e6
                else:
                    h = rng.choice([-3e-7, -2e-7, -1e-7, 1e-7, 2e-7, 3e-7], n)
                    q = np.stack([0.07 * X + 0.1, 0.13 * Y + 0.1, h], 1)
                geom = ch.one_cell(ctype, k % 5, points=q.astype(F32))
                vals = np.sin(1.7 * np.arange(n) + k)
                out.append(case("flat", "%s-%s%s" % (TYPE_NAME[ctype], kind, "-far" if far else ""),
                                geom, by_position(geom[3], vals), 0.0, k))
                k += 1
    return out


# ---- fields ----
def _point_number(p):
    """The lattice number of the points of LATTICE at unit spacing."""
    q = np.rint(np.asarray(p, np.float64)).astype(np.int64)
    return q[..., 0] + LATTICE[0] * (q[..., 1] + LATTICE[1] * q[..., 2])


def _table_field(table):
    return lambda p: np.asarray(table, np.float64)[_point_number(p)]


def _wave_centred(p):
    w = th.wave_f(np.asarray(p, np.float64))
    return w - np.median(w)


def _wave_wide(p):
    """The uncentred wave over a wider stretch (the lattice at spacing 2 from
    (3, 2, 1), as the existing batches place it), where it crosses 0.3."""
    return th.wave_f(2.0 * np.asarray(p, np.float64) + np.array([3.0, 2.0, 1.0]))


def fields():
    """[(name, f(points) -> float64 exactly representable in float32 where it
    matters, isovalue)] on the points of LATTICE."""
    npts = int(np.prod(LATTICE))
    rng = np.random.default_rng(23)
    zeros = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), npts)
    steps = rng.integers(-2, 3, npts)
    near = np.full(npts, 0.75, F32)
    for _ in range(2):   # up to two steps of one ulp either way
        near = np.where(steps > 0, np.nextafter(near, F32(2)),
                        np.where(steps < 0, np.nextafter(near, F32(0)), near))
        steps = steps - np.sign(steps)
    tiny = 2.0 ** -140

    def huge(p):   # at spacing 7 the wave swings far enough within one cell
        w = _wave_centred(7.0 * np.asarray(p, np.float64))
        return w * (3e38 / np.abs(w).max())

    return [("onlevel", lambda p: np.rint(np.asarray(p, np.float64)[..., 0]) - 2.0, 0.0),
            ("zeros+0", _table_field(zeros), 0.0),
            ("zeros-0", _table_field(zeros), -0.0),
            ("subnormal", lambda p: _wave_centred(p) * tiny, 0.0),
            ("subnormal-iso", lambda p: _wave_wide(p) * tiny, 0.3 * tiny),
            ("huge", huge, 0.0),
            ("ulps", _table_field(near.astype(np.float64)), 0.75),
            ("constant", lambda p: np.full(np.shape(p)[:-1], 0.3), float(F32(0.3)))]


def klass_of(name):
    return name.split("+")[0].split("-")[0]


def field_cells():
    """The field classes on the renumbered hex lattice."""
    geom = ch.hex_lattice(LATTICE, seed=8)
    return [case(klass_of(name), "cells-" + name, geom, f, iso, k)
            for k, (name, f, iso) in enumerate(fields())]


def field_tets():
    """The field classes on the Kuhn tet mesh of the lattice, renumbered; cell
    mesh dicts of tets (tets_of gives the tet call's)."""
    p, t = th.kuhn_mesh(LATTICE)
    p, lists = ch.renumbered(p, t.tolist(), 9)
    geom = (p,) + ch.cells([ch.TET] * len(lists), lists)
    return [case(klass_of(name), "kuhn-" + name, geom, f, iso, k + 3)
            for k, (name, f, iso) in enumerate(fields())]


def field_grids():
    """The field classes as structured grids, one with a spacing and an origin."""
    out = []
    for k, (name, f, iso) in enumerate(fields()):
        g = ih.grid(f(ih.lattice(LATTICE)), iso=iso, color=None if k & 1 else 0x00405060 + k)
        g.update(klass=klass_of(name), name="grid-" + name)
        out.append(g)
    return out


def _pencil(ax, seed):
    dims = [2, 2, 2]
    dims[ax] = 257
    rng = np.random.default_rng(seed)
    p = ih.lattice(tuple(dims))
    f = p @ (0.003 * rng.normal(size=3)) + rng.normal(size=p.shape[:-1]) * 0.7
    return ih.grid(f - np.median(f), iso=0.1)


def pencils():
    """257 points along each axis in turn, 2 along the others: one point past a
    block of 256.  A shallow ramp plus noise, so the level is crossed all
    along; the seed is the first from 40 on for which the long axis' last edge
    and first edge are both crossed."""
    out = []
    for ax in range(3):
        for seed in range(40, 80):
            g = _pencil(ax, seed)
            ins = np.moveaxis(g["values"] >= F32(g["iso"]), 2 - ax, 0)
            if (ins[256] != ins[255]).any() and (ins[1] != ins[0]).any():
                break
        g.update(klass="pencil", name="pencil-%d" % ax, color=0x00A0B0C0 if ax == 1 else None)
        out.append(g)
    return out


# ---- batches ----
def is_tets(m):
    return len(m["types"]) > 0 and (np.asarray(m["types"]) == ch.TET).all()


def tets_of(m):
    """The tet mesh dict of a cell mesh dict of tets only."""
    t = dict(m, tets=np.ascontiguousarray(m["conn"]).reshape(-1, 4))
    for k in ("types", "offsets", "conn"):
        t.pop(k)
    return t


def split_of(m):
    """The tet mesh dict of the split of any cell mesh dict (cell_helpers.split_numpy)."""
    t = ch.as_tets(m)
    t["tets"] = np.ascontiguousarray(t["tets"], np.uint32).reshape(-1, 4)
    return t


def with_twins(cases, names):
    """The list with the named cases placed twice in a row."""
    out = []
    for m in cases:
        out.append(m)
        if m["name"] in names:
            out.append(dict(m, name=m["name"] + "-twin", twin_of=m["name"]))
    assert sum("twin_of" in m for m in out) == len(names)
    return out


CELL_TWINS = ("fan-wedge-half-middle", "hex-x3")
TET_TWINS = ("fan-tet-full-highest", "tet-x300")
GRID_TWINS = ("grid-zeros-0", "pencil-1")


def topology_cases():
    """Every topology class but the whole collapsed family: of that, every 23rd."""
    return fans() + duplicates() + nonmanifold() + nonconforming() + collapsed()[::23] + flat()


def cell_batch():
    """All classes as cell meshes in one list, two of them twice in a row."""
    return with_twins(topology_cases() + field_cells() + field_tets()[:2], CELL_TWINS)


def tet_batch():
    """All classes that are tets only, as tet mesh dicts, two of them twice in a row."""
    cases = [m for m in topology_cases() if is_tets(m)] + field_tets()
    return with_twins([tets_of(m) for m in cases], TET_TWINS)


def grid_batch():
    return with_twins(field_grids() + pencils(), GRID_TWINS)


def selects(m):
    """The three selects of the surface call for a case: all, the points at or
    above the case's level, and cells by a value per cell (the case's own
    select where it has one; else two cells of every three, the first among
    them, which lays inner faces bare)."""
    if m.get("cells_select") is not None:
        by_cell = m["cells_select"]
    else:
        cv = (np.arange(len(m["types"])) % 3 != 1).astype(F32)
        by_cell = sh.select("cells", 1.0, 1.0, cv)
    return [None, sh.select("points", m["iso"], FMAX), by_cell]


# ---- facts about the inputs, from the numpy side ----
def crossing_keys(m):
    """The sorted pair keys (lo << 32 | hi) of the crossing (tet, walk edge)
    instances of the split of a cell mesh dict."""
    T = ch.split_numpy(m).astype(np.int64)
    ins = np.asarray(m["values"], F32) >= F32(m["iso"])
    keys = []
    for u, w in th.WALK_EDGES:
        c = ins[T[:, u]] != ins[T[:, w]]
        keys.append((np.minimum(T[c, u], T[c, w]) << 32) | np.maximum(T[c, u], T[c, w]))
    return np.sort(np.concatenate(keys))


def runs(sorted_keys):
    """(starts, lengths) of the runs of equal neighbours."""
    k = np.asarray(sorted_keys)
    if len(k) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    starts = np.nonzero(np.concatenate([[True], k[1:] != k[:-1]]))[0]
    return starts, np.diff(np.concatenate([starts, [len(k)]]))


def face_key_runs(m, sel=None):
    """The lengths of the runs of equal face keys of the kept cells."""
    keys = sorted(key for key, _, _ in sh.cell_faces(m, sh.kept_cells(m, sel)))
    return runs(_rank(keys))[1]


def _rank(keys):
    """Sorted tuples -> equal integers for equal tuples, ascending."""
    out, last, n = [], None, -1
    for k in keys:
        if k != last:
            n, last = n + 1, k
        out.append(n)
    return np.asarray(out, np.int64)


def crossing_pairs(m):
    """The distinct crossing point pairs (a, b), a < b, of a cell mesh dict."""
    k = np.unique(crossing_keys(m))
    return k >> 32, k & 0xFFFFFFFF


def grid_crossing_pairs(g):
    """(fa, fb) float32 of the crossing edges of a structured grid."""
    f = np.ascontiguousarray(g["values"], F32)
    ins = f >= F32(g["iso"])
    nz, ny, nx = f.shape
    fa, fb = [], []
    for dx, dy, dz in ih.EDGE:
        A = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        B = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        c = ins[A] != ins[B]
        fa.append(f[A][c])
        fb.append(f[B][c])
    return np.concatenate(fa), np.concatenate(fb)


def triangle_areas(verts, faces):
    t = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)

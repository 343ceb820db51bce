"""A numpy restatement of the glyph rule and the point sets shared by the
glyph tests (test_glyphs_host.py, test_gpu_glyphs.py).

Written from the rule in include/spray_rt.h ("glyphs of point sets"), not from
the C code: keep, order, sphere, arrow.  Every operation is one numpy
operation on arrays of one dtype (float32 for the byte comparisons, float64
for the error estimates), so nothing is contracted and division and square
root are correctly rounded.  The sphere and ring tables are the library's
(spray_amd.glyph_sphere, spray_amd.tube_ring).  `stats` counts the paths a
case reaches.
"""
import collections
import math

import numpy as np

import color_helpers as ch
import stream_cases as sc

F32 = np.float32
SPHERE, ARROW = 0, 1
TINY = F32(1.17549435e-38)   # the smallest normal float


def pset(points, vectors=None, scales=None, select=None, select_range=(0.0, 0.0), stride=1,
         cfield=None, cmap=None):
    f = lambda x, w: None if x is None else np.ascontiguousarray(x, F32).reshape((-1,) + w)
    return dict(points=f(points, (3,)), vectors=f(vectors, (3,)), scales=f(scales, ()),
                select=f(select, ()), select_range=select_range, stride=stride, cfield=f(cfield, ()),
                cmap=cmap)


def sphere(size, level=0, color=None):
    return dict(shape=SPHERE, size=size, level=level, color=color)


def arrow(size, nsides=5, scale_by_vector=False, min_speed=1e-6, color=None):
    return dict(shape=ARROW, size=size, nsides=nsides, scale_by_vector=scale_by_vector,
                min_speed=min_speed, color=color)


def per_glyph(G):
    """(V, F) of a glyph."""
    if G["shape"] == SPHERE:
        return 10 * 4 ** G["level"] + 2, 20 * 4 ** G["level"]
    return 4 * G["nsides"] + 1, 6 * G["nsides"]


# ---- the rule ----

def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def keep_numpy(S, G, F=F32, stats=None):
    """(kept mask, s, d) over the points of S."""
    st = collections.Counter() if stats is None else stats
    n = len(S["points"])
    idx = np.arange(n)
    cand = idx % int(S["stride"]) == 0
    st["off_stride"] += int((~cand).sum())
    if S["select"] is not None:
        lo, hi = (F32(x) for x in S["select_range"])
        v = S["select"]
        inside = (lo <= v) & (v <= hi)
        st["select_on_lo"] += int((cand & (v == lo)).sum())
        st["select_on_hi"] += int((cand & (v == hi)).sum())
        st["select_out"] += int((cand & ~inside).sum())
        cand = cand & inside
    size = F(F32(G["size"]))
    with np.errstate(all="ignore"):
        s = np.full(n, size, F) if S["scales"] is None else size * S["scales"].astype(F)
        d = np.zeros(n, F)
        fast = np.ones(n, bool)
        if G["shape"] == ARROW:
            v = S["vectors"].astype(F)
            d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            ms = F(F32(G["min_speed"]))
            fast = (ms * ms <= d) & (d < np.inf)
            st["speed_low"] += int((cand & ~(ms * ms <= d)).sum())
            st["speed_overflow"] += int((cand & ~(d < np.inf)).sum())
            st["square_underflow"] += int((cand & fast & ((v * v == 0) & (v != 0)).any(1)).sum())
            if G["scale_by_vector"]:
                s = s * np.sqrt(d)
    kept = cand & (0 < s) & (s < np.inf) & fast
    st["s_zero"] += int((cand & (s == 0)).sum())
    st["s_overflow"] += int((cand & fast & ~(s < np.inf)).sum())
    st["s_subnormal"] += int((kept & (s < F(TINY))).sum())
    st["kept"] += int(kept.sum())
    return kept, s, d


def axis_normal(T, F, st):
    """The streamlines' axis rule on the rows of T."""
    a = np.abs(T)
    n = len(T)
    rows = np.arange(n)
    e = np.where(a[:, 1] < a[:, 0], 1, 0)
    e = np.where(a[:, 2] < a[rows, e], 2, e)
    st["axis_tie"] += int(((a == a[rows, e][:, None]).sum(1) > 1).sum())
    for k in range(3):
        st["axis_%d" % k] += int((e == k).sum())
    E = np.zeros((n, 3), F)
    E[rows, e] = 1
    w = E - T[rows, e][:, None] * T
    return w / np.sqrt(dot(w, w))[:, None]


def arrow_faces(ns):
    """The arrow's face table as the header lists it."""
    at = lambda j, k: j * ns + k % ns
    f = []
    for j in (0, 1):   # the shaft, then the annulus
        for k in range(ns):
            f += [(at(j, k), at(j + 1, k), at(j, k + 1)), (at(j, k + 1), at(j + 1, k), at(j + 1, k + 1))]
    f += [(at(2, k), at(3, k), at(2, k + 1)) for k in range(ns)]
    f += [(4 * ns, at(0, k), at(0, k + 1)) for k in range(ns)]
    return np.array(f, np.uint32)


def cone_constants():
    h = math.hypot(0.35, 0.1)
    return F32(0.35 / h), F32(0.1 / h)


def glyphs_numpy(S, G, spray, F=F32, stats=None, kept=None):
    """(verts, normals, colors, faces, point_ids) of set S under glyph G; kept
    overrides the keep decisions (the float64 estimates take float32's)."""
    st = collections.Counter() if stats is None else stats
    k0, s, d = keep_numpy(S, G, F, st)
    kept = k0 if kept is None else kept
    ids = np.nonzero(kept)[0].astype(np.uint32)
    ng = len(ids)
    V, nF = per_glyph(G)
    p = S["points"].astype(F)[ids]
    s = s[ids]
    with np.errstate(all="ignore"):
        if G["shape"] == SPHERE:
            u, tf = spray.glyph_sphere(G["level"])
            u = u.astype(F)
            verts = p[:, None, :] + s[:, None, None] * u[None, :, :]
            normals = np.broadcast_to(u[None, :, :], (ng, V, 3))
        else:
            ns = G["nsides"]
            v = S["vectors"].astype(F)[ids]
            T = v / np.sqrt(d[ids])[:, None]
            N = axis_normal(T, F, st)
            B = np.stack([T[:, 1] * N[:, 2] - T[:, 2] * N[:, 1], T[:, 2] * N[:, 0] - T[:, 0] * N[:, 2],
                          T[:, 0] * N[:, 1] - T[:, 1] * N[:, 0]], 1)
            ring = spray.tube_ring(ns).astype(F)
            cn, ct = (F(x) for x in cone_constants())
            L = s[:, None, None]
            rs, rh, hl = F(F32(0.03)) * L, F(F32(0.1)) * L, F(F32(0.35)) * L
            ls = L - hl
            off = ring[None, :, 0, None] * N[:, None, :] + ring[None, :, 1, None] * B[:, None, :]
            cone = cn * off + ct * T[:, None, :]
            P, Tk = p[:, None, :], T[:, None, :]
            end = P + ls * Tk
            tip = np.broadcast_to(P + L * Tk, (ng, ns, 3))
            verts = np.concatenate([P + rs * off, end + rs * off, end + rh * off, tip, P], 1)
            normals = np.concatenate([off, off, cone, cone, -Tk], 1)
            tf = arrow_faces(ns)
    if S["cfield"] is not None:
        col = ch.colormap_numpy(S["cfield"][ids], *S["cmap"])
    else:
        col = np.full(ng, G["color"] or 0, np.uint32)
    faces = tf[None, :, :].astype(np.uint32) + (np.arange(ng, dtype=np.uint32) * np.uint32(V))[:, None, None]
    return (np.ascontiguousarray(verts, F).reshape(-1, 3), np.ascontiguousarray(normals, F).reshape(-1, 3),
            np.repeat(col, V).astype(np.uint32), faces.reshape(-1, 3).astype(np.uint32), ids)


# ---- mesh properties ----

def geometric_normals(v, f):
    """Ng = (v0 - v1) x (v2 - v0) per face, in float64."""
    v = v.astype(np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return np.cross(a - b, c - a)


def closed_oriented(f, nv):
    """Whether every directed edge of the faces has its opposite exactly once
    (a closed oriented 2-manifold) and the Euler characteristic over the
    vertices the faces use."""
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * nv + e[:, 1]
    rev = e[:, 1] * nv + e[:, 0]
    ok = len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))
    chi = len(np.unique(f)) - len(key) // 2 + len(f)
    return ok, chi


# ---- point sets ----

def cloud(n, seed, extent=4.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-extent, extent, (n, 3)).astype(F32)


def swirl(p, seed=0):
    """A velocity per point without zeros."""
    rng = np.random.default_rng(seed)
    v = np.stack([-p[:, 1], p[:, 0], 0.5 + 0.25 * np.sin(p[:, 2])], 1)
    return (v + 0.05 * rng.normal(size=v.shape)).astype(F32)


def with_color(S, seed, ntable=37):
    """S with a colour field and a map that clamps at both ends."""
    rng = np.random.default_rng(seed)
    T = dict(S)
    T["cfield"] = rng.uniform(-1.0, 1.0, len(S["points"])).astype(F32)
    T["cmap"] = (ch.table(ntable, seed), -0.5, 0.625)
    return T


def tie_vectors():
    """The vectors of stream_cases.zeros_and_ties: every sign pattern of +-0,
    ties of two and of three components, T along each axis both ways."""
    cases = sc.zeros_and_ties()
    return np.array([cases[k]["vectors"][0, 0, 0] for k in sorted(cases)], F32)


def min_speed_floor():
    """The smallest min_speed whose float32 square is a normal float."""
    m = F32(np.sqrt(np.float64(TINY)))
    while F32(m * m) < TINY:
        m = np.nextafter(m, F32(1))
    while F32(np.nextafter(m, F32(0)) * np.nextafter(m, F32(0))) >= TINY:
        m = np.nextafter(m, F32(0))
    return m


def small_cases():
    """The small sets of the host test, as {name: (set, glyph)}."""
    up, dn = (lambda x: np.nextafter(F32(x), F32(np.inf))), (lambda x: np.nextafter(F32(x), F32(-np.inf)))
    c = {}
    p7 = cloud(7, 1)
    c["n0"] = (pset(np.zeros((0, 3))), sphere(0.5))
    c["n0_arrow"] = (pset(np.zeros((0, 3)), vectors=np.zeros((0, 3))), arrow(0.5))
    c["n1"] = (pset([[1, 2, 3]]), sphere(0.25, 1, 0x00AA5500))
    c["n1_arrow"] = (pset([[1, 2, 3]], vectors=[[0.5, -2, 1]]), arrow(0.75, 3))
    c["all_dropped"] = (pset(p7, scales=np.zeros(7)), sphere(0.5))
    sel = np.arange(7, dtype=F32)
    c["first_only"] = (pset(p7, select=sel, select_range=(-1.0, 0.5)), sphere(0.5))
    c["last_only"] = (pset(p7, select=sel, select_range=(5.5, 99.0)), sphere(0.5))
    for st in (1, 2, 3, 8):
        c["stride%d" % st] = (pset(p7, stride=st), sphere(0.125 * st, st % 2))
        c["stride%d_arrow" % st] = (pset(p7, vectors=swirl(p7), stride=st), arrow(0.5, 3 + st))
    lo, hi = F32(0.25), F32(0.75)
    edge = [dn(lo), lo, up(lo), 0.5, dn(hi), hi, up(hi)]
    c["select_edges"] = (pset(p7, select=edge, select_range=(lo, hi)), sphere(0.5))
    c["select_point"] = (pset(p7, select=[dn(lo), lo, up(lo), lo, 0, 1, lo], select_range=(lo, lo)),
                         sphere(0.5))
    tiny = F32(1e-45)
    c["select_zero"] = (pset(p7, select=[-0.0, 0.0, tiny, -tiny, 1, -1, -0.0],
                             select_range=(0.0, 0.0)), sphere(0.5))
    c["select_negzero"] = (pset(p7, select=[-0.0, 0.0, tiny, -tiny, 1, -1, -0.0],
                                select_range=(-0.0, -0.0)), sphere(0.5))
    c["scales"] = (pset(p7, scales=[0.0, 1e-45, 3e-39, 1.0, 3e38, -0.0, 2.5]), sphere(2.0, 1))
    c["scales_arrow"] = (pset(p7, vectors=swirl(p7), scales=[0.0, 1e-45, 3e-39, 1.0, 3e38, -0.0, 2.5]),
                         arrow(2.0, 4))
    # arrows: the speed either side of the smallest min_speed, d overflowing,
    # squares that underflow, with the length scaled by the speed and not
    m = min_speed_floor()
    vec = [[dn(m), 0, 0], [m, 0, 0], [up(m), 0, 0], [0, dn(m), 0], [0, 0, up(m)],
           [2e19, 2e19, 0], [1.5e19, 0, 1e19], [3e-19, 1e-30, -1e-25], [1e-23, 2e-19, 1e-24],
           [1.0, 1e-30, 1e-25], [0, 0, 0]]
    pv = cloud(len(vec), 2)
    for sbv in (False, True):
        c["speeds_%d" % sbv] = (pset(pv, vectors=vec), arrow(3.0 if sbv else 0.5, 4, sbv, float(m)))
    # a length that overflows through the speed, and one that underflows to zero
    c["length_range"] = (pset(cloud(4, 3), vectors=[[1e19, 0, 0], [2e-19, 0, 0], [3, 4, 0], [0, 1e10, 0]],
                              scales=[1e30, 1e-30, 1.0, 1e-30]), arrow(1e-3, 3, True, float(m)))
    tv = tie_vectors()
    for sbv in (False, True):
        c["ties_%d" % sbv] = (pset(cloud(len(tv), 4), vectors=tv), arrow(0.5, 6, sbv))
    p3 = cloud(3, 5)
    for ns in range(3, 17):
        c["nsides%d" % ns] = (pset(p3, vectors=swirl(p3, ns)), arrow(0.25 * ns, ns, ns % 2 == 0))
    for lv in range(4):
        c["level%d" % lv] = (pset(p3, scales=[1.0, 0.5, 2.0]), sphere(0.5, lv, 0x00010203 * lv))
    return c


def runs_case(n, runs, seed, arrows=False):
    """n points of which the index ranges `runs` are kept (by select)."""
    p = cloud(n, seed, 16.0)
    sel = np.zeros(n, F32)
    for a, b in runs:
        sel[a:b] = 1.0
    S = pset(p, vectors=swirl(p, seed) if arrows else None, select=sel, select_range=(0.5, 1.5))
    return S, (arrow(0.5, 3 + seed % 5) if arrows else sphere(0.25, seed % 2))


def tiled_case(n, prime, seed, stride=1):
    """n points tiled from `prime` distinct ones, spheres at level 0."""
    base = cloud(prime, seed, 64.0)
    reps = -(-n // prime)
    p = np.tile(base, (reps, 1))[:n]
    scales = np.tile(np.linspace(0.5, 1.5, prime).astype(F32), reps)[:n]
    return pset(p, scales=scales, stride=stride), sphere(0.25, 0, 0x00203040)

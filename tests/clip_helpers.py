"""Meshes and a numpy restatement of the clip of cell meshes by a level of
their scalar field, shared by test_cell_clip_host.py and test_gpu_cell_clip.py.

The restatement is written from the text of include/spray_rt.h, not from the C
code.  Point p is kept when values[p] >= isovalue, with invert when it is not.
The first vertices and faces are the cell isosurface's (cell_helpers), the
faces with corners 1 and 2 swapped under invert; vert_pairs is the vertex's
point pair (a, b), a < b, vert_t = (iso - f[a]) / (f[b] - f[a]).  A cell takes
part when one of its listed points is kept.  The skin's source is the boundary
triangles (surface_helpers: faces, keys, once-only, diagonal, outward turn) of
the cells that take part; a triangle (v0, v1, v2) gives, by its kept corners,

    3         (P0, P1, P2)
    0         nothing
    only k    (Pk, X(k,k+1), X(k,k+2))
    all but k (Pk+1, Pk+2, X(k+2,k)) then (Pk+1, X(k+2,k), X(k,k+1))

with X(i,j) the cap vertex of the pair of corners i and j.  The skin's vertices
are the kept points its pieces use, ascending, behind the cap's: the point's own
bytes, vert_pairs (p, p), vert_t 0.
"""
from collections import Counter

import numpy as np

import cell_helpers as ch
import color_helpers as colh
import surface_helpers as sh
import tet_helpers as th

F32 = np.float32


def skin_triangles(m, part):
    """The boundary triangles, turned outward, of the cells part marks: int64 [n, 3]."""
    p = np.ascontiguousarray(m["points"], F32).reshape(-1, 3)
    faces = sh.cell_faces(m, part)
    count = Counter(key for key, _, _ in faces)
    tris = []
    for key, c, pref in faces:
        if count[key] != 1:
            continue
        if len(c) == 3:
            mine = [c]
        else:
            j = c.index(min(c))
            r = [c[(j + d) % 4] for d in range(4)]
            mine = [[r[0], r[1], r[2]], [r[0], r[2], r[3]]]
        odd = bool(th.orientation_odd(p, np.array([mine[0] + [pref]], np.int64))[0])
        tris += [[t[0], t[2], t[1]] if odd else t for t in mine]
    return np.asarray(tris, np.int64).reshape(-1, 3)


def pieces(tri, kept):
    """The pieces of one triangle as corner pairs (i, j) of point indices; i == j
    is the kept point itself."""
    k3 = [bool(kept[v]) for v in tri]
    P = lambda i: (tri[i % 3], tri[i % 3])
    X = lambda i, j: (tri[i % 3], tri[j % 3])
    n = sum(k3)
    if n == 3:
        return [[P(0), P(1), P(2)]]
    if n == 0:
        return []
    if n == 1:
        k = k3.index(True)
        return [[P(k), X(k, k + 1), X(k, k + 2)]]
    k = k3.index(False)
    return [[P(k + 1), P(k + 2), X(k + 2, k)], [P(k + 1), X(k + 2, k), X(k, k + 1)]]


def clip_numpy(m, invert=False):
    """-> verts float32 [nv, 3], normals float32 [nv, 3] or None, colors uint32
    [nv], vert_pairs uint32 [nv, 2], vert_t float32 [nv], faces uint32 [nf, 3],
    ncap_verts, ncap_faces of a mesh dict."""
    p = np.ascontiguousarray(m["points"], F32).reshape(-1, 3)
    f = np.ascontiguousarray(m["values"], F32)
    iso = F32(m["iso"])
    inside = f >= iso
    kept = inside != bool(invert)
    # the cap
    cv, cn, cc, cf = ch.cell_isosurface_numpy(m)
    T = ch.split_numpy(m).astype(np.int64)
    lo = np.stack([np.minimum(T[:, u], T[:, w]) for u, w in th.WALK_EDGES], 1)
    hi = np.stack([np.maximum(T[:, u], T[:, w]) for u, w in th.WALK_EDGES], 1)
    cross = np.stack([inside[T[:, u]] != inside[T[:, w]] for u, w in th.WALK_EDGES], 1)
    ukeys = np.unique(((lo << 32) | hi)[cross])
    a, b = ukeys >> 32, ukeys & 0xFFFFFFFF
    assert len(ukeys) == len(cv)
    with np.errstate(all="ignore"):
        ct = ((iso - f[a]) / (f[b] - f[a])).astype(F32)
    if invert:
        cf = cf[:, [0, 2, 1]]
    # the skin
    conn, off = np.asarray(m["conn"]), np.asarray(m["offsets"]).astype(np.int64)
    part = np.array([kept[conn[off[i]:off[i + 1]]].any() for i in range(len(off) - 1)], bool)
    corners = [c for tri in skin_triangles(m, part).tolist() for pc in pieces(tri, kept)
               for c in pc]
    corners = np.asarray(corners, np.int64).reshape(-1, 2)
    own = corners[:, 0] == corners[:, 1]
    ids = np.unique(corners[own, 0])
    key = (np.minimum(corners[:, 0], corners[:, 1]) << 32) | np.maximum(corners[:, 0], corners[:, 1])
    at = np.searchsorted(ukeys, key)
    found = np.zeros(len(key), bool)
    if len(ukeys):
        found = ukeys[np.minimum(at, len(ukeys) - 1)] == key
    assert (own | found).all()     # every cut edge is a crossing edge of the tet split
    sf = np.where(own, len(cv) + np.searchsorted(ids, corners[:, 0]), at).reshape(-1, 3)
    verts = np.concatenate([cv, p[ids]])
    normals = None
    if m.get("normals") is not None:
        normals = np.concatenate([cn, np.ascontiguousarray(m["normals"], F32).reshape(-1, 3)[ids]])
    if m.get("cfield") is not None:
        table, clo, chi = m["cmap"]
        sc = colh.colormap_numpy(np.ascontiguousarray(m["cfield"], F32)[ids], table, clo, chi)
    else:
        sc = np.full(len(ids), m.get("color") or 0, np.uint32)
    colors = np.concatenate([cc.astype(np.uint32), sc.astype(np.uint32)])
    pairs = np.concatenate([np.stack([a, b], 1), np.stack([ids, ids], 1)]).astype(np.uint32)
    vt = np.concatenate([ct, np.zeros(len(ids), F32)])
    faces = np.concatenate([cf.astype(np.uint32).reshape(-1, 3), sf.astype(np.uint32)])
    return (verts.astype(F32), normals, colors, pairs.reshape(-1, 2), vt.astype(F32),
            faces.reshape(-1, 3), len(cv), len(cf))


def host_clip(spray, m, invert=False, normals=True):
    """The same eight results from the host restatement of the engine."""
    return spray.cell_clip_host(m["points"], m["types"], m["offsets"], m["conn"], m["values"],
                                m["iso"], invert, m.get("normals") if normals else None,
                                m.get("cfield"), m.get("cmap"), m.get("color"))


def assert_same(got, want, what=""):
    """Byte equality of two clip results."""
    names = ("verts", "normals", "colors", "vert_pairs", "vert_t", "faces")
    for name, g, w in zip(names, got, want):
        if w is None or g is None:
            assert g is None and w is None, (what, name)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)
    assert tuple(got[6:]) == tuple(want[6:]), (what, got[6:], want[6:])


def components(faces):
    """The number of edge-connected components of a triangle list."""
    f = np.asarray(faces, np.int64)
    parent = {int(v): int(v) for v in np.unique(f)}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f.tolist():
        parent[find(a)] = find(b)
        parent[find(b)] = find(c)
    return len({find(v) for v in parent})


def plane_numpy(points, origin, normal):
    """values[p] = ((px - ox) * nx + (py - oy) * ny) + (pz - oz) * nz, step by
    step in float32."""
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    o, n = np.asarray(origin, F32), np.asarray(normal, F32)
    tx = ((p[:, 0] - o[0]).astype(F32) * n[0]).astype(F32)
    ty = ((p[:, 1] - o[1]).astype(F32) * n[1]).astype(F32)
    tz = ((p[:, 2] - o[2]).astype(F32) * n[2]).astype(F32)
    return ((tx + ty).astype(F32) + tz).astype(F32)


def x_minus(c):
    return lambda p: p[..., 0].astype(np.float64) - c


def lattice_4(seed=5):
    """The renumbered lattice of 4^3 points with values x - 1.5."""
    return ch.mesh(ch.hex_lattice((4, 4, 4), seed=seed), x_minus(1.5), 0.0)


def sphere_9(seed=None):
    """9^3 points, R^2 - |p - c|^2 with the sphere strictly inside."""
    c, R = np.array([4.1, 3.9, 4.2]), 2.7
    f = lambda p: R * R - ((p.astype(np.float64) - c) ** 2).sum(-1)
    return ch.mesh(ch.hex_lattice((9, 9, 9), seed=seed), f, 0.0)


# ---- the GPU batch ----
(ONE_TET, ONE_HEX, ONE_WEDGE, ONE_PYRAMID, HEX_TETS, MIXED, SMALL, FULL, PARTIAL, OUTSIDE, NOCELLS,
 INSIDE, LARGE) = range(13)


def gpu_batch():
    """(meshes, invert flags) of the GPU batch: one cell of each type, a hex
    over two tets, the conforming mixed mesh, a renumbered lattice of 5^3
    points, 9x9x5 points (256 hexes: one full block), 17x9x6 (640: a partial
    last block), a mesh wholly outside, one without cells in the middle, one
    wholly inside, 53^3 points (140,608 hexes in 550 blocks, 582 blocks of
    points: past one stride of the 512-wide scan in both) with a busy field that
    cuts about half the cells.  Tables of 1 and 4096 entries, one constant
    colour, one colourless; some with normals; mixed invert flags."""
    inner = ch.sphere((0.3, 0.2, 0.1), 0.8)
    ms = [ch.mesh(ch.one_cell(ch.TET, 1), ch.sphere((0.1, 0.2, 0.1), 1.0), 0.0),
          ch.mesh(ch.one_cell(ch.HEX, 2), inner, 0.0, normals=True, color=0x00123456),
          ch.mesh(ch.one_cell(ch.WEDGE, 3), inner, 0.0, cmap_seed=15, ntable=8),
          ch.mesh(ch.one_cell(ch.PYRAMID, 4), inner, 0.0, normals=True),
          ch.mesh(sh.cut_quad_mesh(True, 5), ch.sphere((0.4, 0.6, 0.1), 0.9), 0.0, normals=True,
                  cmap_seed=18, ntable=32),
          ch.mesh(sh.conforming_mesh(), x_minus(0.9), 0.0, normals=True, cmap_seed=16, ntable=64),
          ch.mesh(ch.hex_lattice((5, 5, 5), (3, 2, 1), (2, 2, 2), seed=7), th.wave_f, 0.3,
                  cmap_seed=11, ntable=1),
          ch.mesh(ch.hex_lattice((9, 9, 5), (-1, 2, 0.5), (0.5, 0.75, 1.25)), th.wave_f, 0.3,
                  normals=True, cmap_seed=12, ntable=4096, clamp=0.3),
          ch.mesh(ch.hex_lattice((17, 9, 6)), th.wave_f, 0.3, normals=True, color=0x00ABCDEF),
          ch.mesh(ch.hex_lattice((4, 3, 3)), th.wave_f, 100.0, normals=True, cmap_seed=13,
                  ntable=16),
          ch.mesh(ch.hex_lattice((4, 3, 3)), th.wave_f, 0.3, normals=True, color=0x00333333),
          ch.mesh(ch.hex_lattice((4, 3, 3)), th.wave_f, -100.0, normals=True, cmap_seed=17,
                  ntable=16),
          ch.mesh(ch.hex_lattice((53, 53, 53), (0, 0, 0), (0.6, 0.6, 0.6)), th.busy_f, 0.1,
                  normals=True, cmap_seed=14, ntable=256)]
    e = ms[NOCELLS]
    e.update(types=e["types"][:0], offsets=e["offsets"][:1], conn=e["conn"][:0])
    inv = [False, True, False, True, True, False, True, False, True, False, True, False, False]
    return ms, inv

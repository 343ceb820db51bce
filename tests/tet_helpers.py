"""Meshes, fields and a numpy restatement of the isosurface extraction from
tetrahedral meshes, shared by test_tet_isosurface_host.py and
test_gpu_tet_isosurface.py.

The restatement is written from DESIGN.md section 14, not from the C code, in
float32 arithmetic: a point is inside when f >= iso; one vertex per distinct
point pair (a, b), a < b, that is an edge of some tet and changes sign, at
t = (iso - f[a]) / (f[b] - f[a]); vertices ascending by (a, b); faces per tet
in input order from the marching-tetrahedra cases of section 12
(iso_helpers.tet_triangles) with the tet's listed points as the walk and the
parity from the sign of det = dot(cross(p1 - p0, p2 - p0), p3 - p0).
"""
import numpy as np

import color_helpers as ch
import iso_helpers as ih

F32 = np.float32
WALK_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
EVEN, ODD = (0, 1, 2), (0, 2, 1)   # axis orders of either parity for ih.tet_triangles


def orientation_odd(p, T):
    """det < 0 per tet, every product and sum rounded to float32, left to right."""
    p0, p1, p2, p3 = (p[T[:, v]] for v in range(4))
    a, b, c = p1 - p0, p2 - p0, p3 - p0
    x = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    y = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    z = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    det = (x * c[:, 0] + y * c[:, 1]) + z * c[:, 2]
    assert det.dtype == F32
    return det < 0


def _case_table():
    """[odd][signs] -> up to two triangles, each three walk edges as indices
    into WALK_EDGES (-1: no triangle)."""
    tab = np.full((2, 16, 2, 3), -1, np.int64)
    for odd, perm in ((0, EVEN), (1, ODD)):
        for s in range(16):
            tris = ih.tet_triangles(perm, [bool((s >> v) & 1) for v in range(4)])
            for n, tri in enumerate(tris):
                tab[odd, s, n] = [WALK_EDGES.index(e) for e in tri]
    return tab


CASES = _case_table()


def tet_isosurface_numpy(m):
    """-> verts float32 [nv, 3], normals float32 [nv, 3] or None, colors uint32
    [nv], faces uint32 [nf, 3] of a mesh dict."""
    p = np.ascontiguousarray(m["points"], F32).reshape(-1, 3)
    T = np.ascontiguousarray(m["tets"]).reshape(-1, 4).astype(np.int64)
    f = np.ascontiguousarray(m["values"], F32)
    iso = F32(m["iso"])
    ins = (f >= iso)[T]                                    # [nt, 4]
    lo = np.stack([np.minimum(T[:, u], T[:, w]) for u, w in WALK_EDGES], 1)
    hi = np.stack([np.maximum(T[:, u], T[:, w]) for u, w in WALK_EDGES], 1)
    cross = np.stack([ins[:, u] != ins[:, w] for u, w in WALK_EDGES], 1)
    key = (lo << 32) | hi                                  # [nt, 6]
    ukeys = np.unique(key[cross])
    a, b = ukeys >> 32, ukeys & 0xFFFFFFFF
    with np.errstate(all="ignore"):
        t = ((iso - f[a]) / (f[b] - f[a])).astype(F32)
        lerp = lambda x: (x[a] + (t.reshape((-1,) + (1,) * (x.ndim - 1)) * (x[b] - x[a]))).astype(F32)
        verts = lerp(p)
        normals = None
        if m.get("normals") is not None:
            normals = lerp(np.ascontiguousarray(m["normals"], F32).reshape(-1, 3))
        if m.get("cfield") is not None:
            table, clo, chi = m["cmap"]
            colors = ch.colormap_numpy(lerp(np.ascontiguousarray(m["cfield"], F32)), table, clo, chi)
        else:
            colors = np.full(len(ukeys), m.get("color") or 0, np.uint32)
    signs = (ins * (1 << np.arange(4))).sum(1)
    odd = orientation_odd(p, T).astype(np.int64) if len(T) else np.zeros(0, np.int64)
    tri = CASES[odd, signs]                                # [nt, 2, 3] walk edge or -1
    live = tri[:, :, 0] >= 0
    rows = np.arange(len(T))[:, None, None]
    ids = np.searchsorted(ukeys, key[rows, np.maximum(tri, 0)])
    faces = ids[live].astype(np.uint32).reshape(-1, 3)
    return verts.reshape(-1, 3), normals, colors, faces


# ---- mesh makers ----
def kuhn_mesh(dims, origin=(0, 0, 0), spacing=(1, 1, 1)):
    """(points float32 [np, 3], tets uint32 [nt, 4]): the Kuhn split of the
    lattice, tets in (cell, x fastest; tetrahedron 0..5) order with the walk's
    corners as vertices 0..3."""
    nx, ny, nz = dims
    points = ih.lattice(dims, origin, spacing).astype(F32).reshape(-1, 3)
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    base = (i + nx * (j + ny * k)).reshape(-1)
    stride = (1, nx, nx * ny)
    walks = []
    for perm in ih.PERMS:
        off = [0]
        for ax in perm:
            off.append(off[-1] + stride[ax])
        walks.append(off)
    tets = base[:, None, None] + np.asarray(walks)[None]
    return points, tets.reshape(-1, 4).astype(np.uint32)


def five_tet_cube():
    """The five-tet split of the unit cube (corner c: bit 0 +x, bit 1 +y, bit 2
    +z): four corner tets and the central one, orientations as they come."""
    points = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)], F32)
    tets = np.array([[0, 1, 2, 4], [3, 1, 2, 7], [5, 1, 4, 7], [6, 2, 4, 7], [1, 2, 4, 7]], np.uint32)
    return points, tets


def single_tet():
    points = np.array([[0, 0, 0], [1.5, 0.25, 0], [0.25, 1.25, 0.5], [0.5, 0.5, 2]], F32)
    return points, np.array([[0, 1, 2, 3]], np.uint32)


def reoriented(m, seed):
    """A copy of mesh dict m with the tet order permuted and two vertices
    swapped in a seeded half of the tets."""
    rng = np.random.default_rng(seed)
    T = np.array(m["tets"], np.uint32).reshape(-1, 4)[rng.permutation(len(m["tets"]))]
    flip = rng.random(len(T)) < 0.5
    u = rng.integers(0, 4, len(T))
    w = (u + rng.integers(1, 4, len(T))) % 4
    rows = np.nonzero(flip)[0]
    T[rows, u[rows]], T[rows, w[rows]] = T[rows, w[rows]].copy(), T[rows, u[rows]].copy()
    return dict(m, tets=np.ascontiguousarray(T))


# ---- fields ----
def wave_f(p):
    p = p.astype(np.float64)
    return (np.sin(0.31 * p[..., 0]) + np.sin(0.23 * p[..., 1] + 1.0) + np.cos(0.41 * p[..., 2])
            + 0.05 * p[..., 0] - 0.03 * p[..., 2])


def busy_f(p):
    """A field that changes sign within a few cells: about half of the tets cross."""
    p = p.astype(np.float64)
    return np.sin(1.3 * p[..., 0] + 0.2) * np.sin(1.1 * p[..., 1] + 0.4) * np.cos(0.9 * p[..., 2])


def mesh(points, tets, f, iso, normals=False, color=None, cmap_seed=None, ntable=0, clamp=1.0):
    """A mesh dict with values f(points), optionally seeded pseudo-normals and
    a colour field mapped through a seeded table (color_helpers)."""
    m = dict(points=points, tets=tets, values=f(points).astype(F32), iso=float(iso), color=color)
    if normals:
        rng = np.random.default_rng(len(points))
        m["normals"] = rng.normal(size=points.shape).astype(F32)
    if cmap_seed is not None:
        rng = np.random.default_rng(cmap_seed)
        cf = (points.astype(np.float64) @ rng.normal(size=3) * 0.2
              + np.sin(0.37 * points[:, 0] + 0.5) + 0.1 * rng.normal(size=len(points))).astype(F32)
        mid = 0.5 * (float(cf.max()) + float(cf.min()))
        half = max(0.5 * (float(cf.max()) - float(cf.min())), 0.25) * clamp
        m.update(cfield=cf, cmap=(ch.table(ntable, cmap_seed + 100), mid - half, mid + half))
    return m


SINGLE, CUBE, SMALL, FULL, PARTIAL, EMPTY, LARGE, REORIENTED = range(8)


def gpu_meshes():
    """The meshes of the GPU batch: a single tet, the five-tet cube, Kuhn
    meshes of 5^3 points, of 17x9x6 (15 full blocks of 256 tets), of 10x9x8 (a
    partial last block), an empty surface in the middle (a zero-length sort
    segment), 29^3 points (515 blocks of tets and, the field being busy, 675 of
    instances: more than one stride of either 512-wide scan), and a re-oriented
    copy.  Mapped with tables of 1 and 4096 entries,
    one constant colour, one colourless; some with normals."""
    sphere = lambda c, r: (lambda p: r - np.linalg.norm(p.astype(np.float64) - c, axis=-1))
    ms = [mesh(*single_tet(), sphere(np.array([0.1, 0.2, 0.1]), 1.0), 0.0),
          mesh(*five_tet_cube(), sphere(np.array([0.2, 0.1, 0.3]), 0.9), 0.0, normals=True,
               color=0x00123456),
          mesh(*kuhn_mesh((5, 5, 5), (3, 2, 1), (2, 2, 2)), wave_f, 0.3, cmap_seed=11, ntable=1),
          mesh(*kuhn_mesh((17, 9, 6), (-1, 2, 0.5), (0.5, 0.75, 1.25)), wave_f, 0.3, normals=True,
               cmap_seed=12, ntable=4096, clamp=0.3),
          mesh(*kuhn_mesh((10, 9, 8)), wave_f, 0.3, normals=True, color=0x00ABCDEF),
          mesh(*kuhn_mesh((4, 3, 3)), wave_f, 100.0, normals=True, cmap_seed=13, ntable=16),
          mesh(*kuhn_mesh((29, 29, 29), (0, 0, 0), (0.6, 0.6, 0.6)), busy_f, 0.1, normals=True,
               cmap_seed=14, ntable=256)]
    ms.append(reoriented(ms[FULL], 5))
    return ms


def on_device(meshes):
    import torch
    out = []
    for m in meshes:
        m = dict(m)
        for k in ("points", "values", "normals", "cfield"):
            if m.get(k) is not None:
                m[k] = torch.from_numpy(np.ascontiguousarray(m[k])).cuda()
        m["tets"] = torch.from_numpy(np.ascontiguousarray(m["tets"]).view(np.int32)).cuda()
        out.append(m)
    return out


def host_mesh(spray, m, normals=True):
    """(verts, normals, colors, faces) of a mesh dict from the host restatement."""
    return spray.tet_isosurface_host(m["points"], m["tets"], m["values"], m["iso"],
                                     m.get("normals") if normals else None, m.get("cfield"),
                                     m.get("cmap"), m.get("color"))


def instances(m):
    """Crossing (tet, walk edge) instances of a mesh dict: 3 per tet with one or
    three points inside, 4 with two."""
    T = np.ascontiguousarray(m["tets"]).reshape(-1, 4).astype(np.int64)
    nin = (np.ascontiguousarray(m["values"], F32) >= F32(m["iso"]))[T].sum(1)
    return int(3 * ((nin == 1) | (nin == 3)).sum() + 4 * (nin == 2).sum())


def patches(m, faces):
    """The oriented patch of every tet that has one, as a sorted list of vertex
    id cycles rotated to start at their smallest id: the triangle of a tet with
    one or three points inside, the quad (q0, x, y, z) of the two triangles
    (q0, x, y), (q0, y, z) of a tet with two.  Which diagonal splits a quad
    follows the listed order of the tet's points (the fixed rule calls
    iso::tet_triangles with the listed points as the walk), so two listings of
    one tet share the quad, not always its two triangles."""
    T = np.ascontiguousarray(m["tets"]).reshape(-1, 4).astype(np.int64)
    nin = (np.ascontiguousarray(m["values"], F32) >= F32(m["iso"]))[T].sum(1)
    ntri = np.where(nin == 2, 2, np.where((nin == 1) | (nin == 3), 1, 0))
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert ntri.sum() == len(f)
    out, at = [], 0
    for n in ntri[ntri > 0]:
        if n == 1:
            cyc = list(f[at])
        else:
            g, h = (f[at], f[at + 1]) if f[at, 2] == f[at + 1, 1] else (f[at + 1], f[at])
            assert g[0] == h[0] and g[2] == h[1]   # (q0, x, y) then (q0, y, z)
            cyc = [g[0], g[1], g[2], h[2]]
        at += n
        k = int(np.argmin(cyc))
        out.append(tuple(int(x) for x in cyc[k:] + cyc[:k]))
    return sorted(out)


def canonical_faces(faces):
    """Rows rotated so the smallest id comes first (orientation kept), sorted."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = np.argmin(f, axis=1)
    rot = np.stack([f[np.arange(len(f)), (k + d) % 3] for d in range(3)], 1)
    return rot[np.lexsort(rot.T[::-1])]

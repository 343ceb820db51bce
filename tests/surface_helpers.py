"""Meshes, selects and a numpy restatement of the boundary-surface and
threshold extraction from cell meshes, shared by test_cell_surface_host.py and
test_gpu_cell_surface.py.

The restatement is written from the text of include/spray_rt.h, not from the C
code.  A select keeps cells: all; those whose listed points all have lo <=
values[p] <= hi; those with lo <= cell_values[i] <= hi.  A kept cell has the
faces of its type's table in table order (cell_helpers.FACES; a tet (0,1,2)
(0,1,3) (1,2,3) (2,0,3)).  With c the point indices of a face and j the
position of the smallest (lowest on ties), the face's key is its corner count
with (c[j], min(a, b), max(a, b)), a and b the corners on either side of c[j]:
a triangle never matches a quad.  A face whose key occurs exactly once in its
mesh is on the surface.  Vertices are the points such faces
use, ascending; a triangle face is (c0, c1, c2), a quad (r0, r1, r2) then (r0,
r2, r3) with r_d = c[(j + d) % 4]; with pref the cell's point at the lowest
local position not on the face, det = dot(cross(p1 - p0, p2 - p0), pref - p0) <
0 in float32 on the first triangle swaps the last two corners of the face's
triangles.
"""
from collections import Counter

import numpy as np

import cell_helpers as ch
import color_helpers as colh
import tet_helpers as th

F32 = np.float32
FACES = dict(ch.FACES)
FACES[ch.TET] = ((0, 1, 2), (0, 1, 3), (1, 2, 3), (2, 0, 3))
ALL, POINTS, CELLS = 0, 1, 2
WIDE = 1e30   # a finite bound no value reaches


def select(mode="all", lo=0.0, hi=0.0, cell_values=None):
    return dict(mode=mode, lo=lo, hi=hi, cell_values=cell_values)


def kept_cells(m, sel):
    """bool [ncells]."""
    off = np.asarray(m["offsets"]).astype(np.int64)
    nc = len(off) - 1
    mode = "all" if sel is None else sel["mode"]
    if mode == "all":
        return np.ones(nc, bool)
    lo, hi = F32(sel["lo"]), F32(sel["hi"])
    if mode == "cells":
        cv = np.asarray(sel["cell_values"], F32)
        return (lo <= cv) & (cv <= hi)
    v = np.asarray(m["values"], F32)
    ok = (lo <= v) & (v <= hi)
    conn = np.asarray(m["conn"])
    return np.array([ok[conn[off[i]:off[i + 1]]].all() for i in range(nc)], bool)


def cell_faces(m, kept):
    """[(key, corners as listed, pref)] of the kept cells' faces, by cell then face."""
    off, conn, types = np.asarray(m["offsets"]), np.asarray(m["conn"]), np.asarray(m["types"])
    out = []
    for i in np.nonzero(kept)[0]:
        P = [int(x) for x in conn[off[i]:off[i + 1]]]
        for q in FACES[int(types[i])]:
            c = [P[x] for x in q]
            n = len(c)
            j = c.index(min(c))
            a, b = c[(j + 1) % n], c[(j + n - 1) % n]
            pref = P[min(set(range(len(P))) - set(q))]
            out.append(((n, c[j], min(a, b), max(a, b)), c, pref))
    return out


def surface_numpy(m, sel=None):
    """-> verts float32 [nv, 3], normals float32 [nv, 3] or None, colors uint32
    [nv], point_ids uint32 [nv], faces uint32 [nf, 3] of a mesh dict."""
    p = np.ascontiguousarray(m["points"], F32).reshape(-1, 3)
    faces = cell_faces(m, kept_cells(m, sel))
    count = Counter(key for key, _, _ in faces)
    tris, refs = [], []
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
        refs += [pref] * len(mine)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    ids = np.unique(tris)
    verts = p[ids]
    normals = None
    if m.get("normals") is not None:
        normals = np.ascontiguousarray(m["normals"], F32).reshape(-1, 3)[ids]
    if m.get("cfield") is not None:
        table, clo, chi = m["cmap"]
        colors = colh.colormap_numpy(np.ascontiguousarray(m["cfield"], F32)[ids], table, clo, chi)
    else:
        colors = np.full(len(ids), m.get("color") or 0, np.uint32)
    return (verts, normals, colors.astype(np.uint32), ids.astype(np.uint32),
            np.searchsorted(ids, tris).astype(np.uint32).reshape(-1, 3))


def host_surface(spray, m, sel=None, normals=True):
    """The same five arrays from the host restatement of the engine."""
    return spray.cell_surface_host(m["points"], m["types"], m["offsets"], m["conn"], sel,
                                   m.get("values"), m.get("normals") if normals else None,
                                   m.get("cfield"), m.get("cmap"), m.get("color"))


# ---- mesh makers ----
def mesh(geometry, f=None, normals=False, color=None, cmap_seed=None, ntable=0, clamp=1.0):
    """A cell mesh dict as cell_helpers.mesh, its values f(points) (None: none)."""
    m = ch.mesh(geometry, f or (lambda p: np.zeros(len(p))), 0.0, normals, color, cmap_seed, ntable,
                clamp)
    m.pop("iso")
    if f is None:
        m.pop("values")
    return m


def conforming_mesh(seed=3):
    """Hexes, wedges and pyramids sharing whole faces only: the cube [0, 2]^3
    as six pyramids around its centre, a hex glued on each face of the cube; the
    hex on +x is cut into two wedges whose triangles lie on the free boundary;
    indices permuted.  32 units of volume."""
    pts = [(x, y, z) for z in (0, 2) for y in (0, 2) for x in (0, 2)] + [(1, 1, 1)]
    cid = lambda x, y, z: (x // 2) + 2 * (y // 2) + 4 * (z // 2)
    centre = 8
    types, lists = [], []
    for ax, sign in ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)):
        u, v = [a for a in range(3) if a != ax]
        B, O = [], []
        for du, dv in ((0, 0), (2, 0), (2, 2), (0, 2)):
            c = [0, 0, 0]
            c[ax], c[u], c[v] = (2 if sign > 0 else 0), du, dv
            B.append(cid(*c))
            c[ax] += sign
            O.append(len(pts))
            pts.append(tuple(c))
        types.append(ch.PYRAMID)
        lists.append(B + [centre])
        if (ax, sign) == (0, 1):
            types += [ch.WEDGE, ch.WEDGE]
            lists += [[B[0], B[1], O[1], B[3], B[2], O[2]], [B[0], O[1], O[0], B[3], O[2], O[3]]]
        else:
            types.append(ch.HEX)
            lists.append(B + O)
    points, lists = ch.renumbered(pts, lists, seed)
    return (points,) + ch.cells(types, lists)


def cut_quad_mesh(through_min, seed=None):
    """A unit hex and two tets under its face (0,1,2,3), which together cover
    that quad: cut through the quad's smallest point index, as the hex's own
    triangles are, or along the other diagonal; indices permuted by a seed."""
    pts = list(map(tuple, ch.UNIT[ch.HEX].tolist())) + [(0.5, 0.5, -1.0)]
    points, (H, A) = ch.renumbered(pts, [list(range(8)), [8]], seed)
    B = H[:4]
    j = B.index(min(B))
    r = [B[(j + d) % 4] for d in range(4)]
    tets = ([[r[0], r[1], r[2], A[0]], [r[0], r[2], r[3], A[0]]] if through_min else
            [[r[0], r[1], r[3], A[0]], [r[1], r[2], r[3], A[0]]])
    return (points,) + ch.cells([ch.HEX, ch.TET, ch.TET], [H] + tets)


def cell_centres(m):
    p = np.asarray(m["points"], np.float64)
    off = np.asarray(m["offsets"]).astype(np.int64)
    return np.array([p[m["conn"][off[i]:off[i + 1]]].mean(0) for i in range(len(off) - 1)])


def signed_volume(verts, faces):
    """The volume a closed surface encloses by the divergence theorem, positive
    where Ng = (v0 - v1) x (v2 - v0) points outward; exact in float64 on small
    integer coordinates."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(a - b, c - a)).sum()) / 6.0


def assert_closed_oriented(faces):
    """Every directed edge as often as its reverse: closed and consistently
    oriented, manifold or not."""
    f = np.asarray(faces, np.int64)
    fwd = Counter(map(tuple, np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist()))
    assert len(f) > 0 and all(fwd[(b, a)] == n for (a, b), n in fwd.items())


def euler(faces):
    f = np.asarray(faces, np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [0, 2]]]), axis=1), axis=0)
    return len(np.unique(f)) - len(e) + len(f)


# ---- the GPU batch ----
(ONE_TET, ONE_HEX, ONE_WEDGE, ONE_PYRAMID, MIXED, SMALL, FULL, PARTIAL, EMPTY, NOCELLS,
 LARGE, CUT) = range(12)


def gpu_batch():
    """(meshes, selects) of the GPU batch: one cell of each type, the
    conforming mixed mesh, a renumbered lattice of 5^3 points, 9x9x5 points (256
    hexes: one full block), 17x9x6 (640: a partial last block), a mesh whose
    threshold keeps nothing and one without cells in the middle, 53^3 points
    (140,608 hexes in 550 blocks, 582 blocks of points: past one stride of the
    512-wide scan in both) with a busy threshold field that keeps about half
    the cells; a hex whose quad faces the two triangles of tets cut along the
    diagonal that misses the quad's smallest index.  All three modes; tables of
    1 and 4096 entries, one constant colour, one colourless; some with normals."""
    ms = [mesh(ch.one_cell(ch.TET, 1)),
          mesh(ch.one_cell(ch.HEX, 2), normals=True, color=0x00123456),
          mesh(ch.one_cell(ch.WEDGE, 3), th.wave_f, cmap_seed=15, ntable=8),
          mesh(ch.one_cell(ch.PYRAMID, 4), normals=True),
          mesh(conforming_mesh(), normals=True, cmap_seed=16, ntable=64),
          mesh(ch.hex_lattice((5, 5, 5), (3, 2, 1), (2, 2, 2), seed=7), th.wave_f, cmap_seed=11,
               ntable=1),
          mesh(ch.hex_lattice((9, 9, 5), (-1, 2, 0.5), (0.5, 0.75, 1.25)), normals=True,
               cmap_seed=12, ntable=4096, clamp=0.3),
          mesh(ch.hex_lattice((17, 9, 6)), normals=True, color=0x00ABCDEF),
          mesh(ch.hex_lattice((4, 3, 3)), th.wave_f, normals=True, cmap_seed=13, ntable=16),
          mesh(ch.hex_lattice((4, 3, 3)), th.wave_f, normals=True, color=0x00333333),
          mesh(ch.hex_lattice((53, 53, 53), (0, 0, 0), (0.6, 0.6, 0.6)), th.busy_f, normals=True,
               cmap_seed=14, ntable=256),
          mesh(cut_quad_mesh(False, 5), normals=True, cmap_seed=18, ntable=32)]
    e = ms[NOCELLS]
    e.update(types=e["types"][:0], offsets=e["offsets"][:1], conn=e["conn"][:0])
    sels = [None,
            select("all"),
            select("points", -WIDE, WIDE),
            select("cells", 0.0, 2.0, np.ones(1, F32)),
            None,
            select("points", 0.3, WIDE),
            None,
            select("cells", 0.3, WIDE, th.wave_f(cell_centres(ms[PARTIAL])).astype(F32)),
            select("points", 100.0, 200.0),
            select("points", 0.3, WIDE),
            select("points", -0.2, WIDE),
            None]
    return ms, sels


def on_device(meshes, sels):
    import torch
    out = []
    for m in meshes:
        m = dict(m)
        for k in ("points", "values", "normals", "cfield", "types"):
            if m.get(k) is not None:
                m[k] = torch.from_numpy(np.ascontiguousarray(m[k])).cuda()
        for k in ("offsets", "conn"):
            m[k] = torch.from_numpy(np.ascontiguousarray(m[k]).view(np.int32)).cuda()
        out.append(m)
    dsels = []
    for s in sels:
        if s is not None and s.get("cell_values") is not None:
            s = dict(s, cell_values=torch.from_numpy(np.ascontiguousarray(s["cell_values"])).cuda())
        dsels.append(s)
    return out, dsels

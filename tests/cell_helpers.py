"""Meshes of hexahedra, wedges, pyramids and tets, and a numpy restatement of
the rule that splits them into tets, shared by test_cell_isosurface_host.py and
test_gpu_cell_isosurface.py.

The restatement is written from DESIGN.md section 15, not from the C code.  A
tet is its four listed points.  Any other cell is the cone from its apex, the
local position m of its smallest point index (lowest position on ties), over
the faces of its table that do not contain m, in table order: a triangle
(q0, q1, q2) gives (P[m], P[q0], P[q1], P[q2]); a quad, with j the position
within the face of its smallest point index (lowest j on ties) and
r_d = q[(j + d) mod 4], gives (P[m], P[r0], P[r1], P[r2]) then
(P[m], P[r0], P[r2], P[r3]).  The surface is section 14's of that tet list
(tet_helpers.tet_isosurface_numpy).
"""
import numpy as np

import tet_helpers as th
from tet_helpers import canonical_faces, patches, tet_isosurface_numpy  # noqa: F401

F32 = np.float32
TET, HEX, WEDGE, PYRAMID = 10, 12, 13, 14
NPOINTS = {TET: 4, HEX: 8, WEDGE: 6, PYRAMID: 5}
NTETS = {TET: 1, HEX: 6, WEDGE: 3, PYRAMID: 2}
FACES = {
    HEX: ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)),
    WEDGE: ((0, 1, 2), (3, 4, 5), (0, 1, 4, 3), (1, 2, 5, 4), (2, 0, 3, 5)),
    PYRAMID: ((0, 1, 2, 3), (0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)),
}


def split_cell(ctype, P):
    """-> (tets of one cell as lists of point indices, the apex position m,
    [(face index, j)] of the far quads)."""
    P = [int(x) for x in P]
    if ctype == TET:
        return [P], None, []
    m = P.index(min(P))
    tets, quads = [], []
    for fi, q in enumerate(FACES[ctype]):
        if m in q:
            continue
        if len(q) == 3:
            tets.append([P[m], P[q[0]], P[q[1]], P[q[2]]])
            continue
        ids = [P[x] for x in q]
        j = ids.index(min(ids))
        r = [ids[(j + d) % 4] for d in range(4)]
        tets.append([P[m], r[0], r[1], r[2]])
        tets.append([P[m], r[0], r[2], r[3]])
        quads.append((fi, j))
    return tets, m, quads


def split_numpy(m):
    """The full tet list of a mesh dict, uint32 [ntets, 4]."""
    conn, off = np.asarray(m["conn"]), np.asarray(m["offsets"])
    out = []
    for i, t in enumerate(np.asarray(m["types"])):
        out += split_cell(int(t), conn[off[i]:off[i + 1]])[0]
    return np.asarray(out, np.uint32).reshape(-1, 4)


def as_tets(m, tets=None):
    """The tet mesh dict (tet_helpers) of a cell mesh dict."""
    t = dict(m, tets=split_numpy(m) if tets is None else tets)
    for k in ("types", "offsets", "conn"):
        t.pop(k)
    return t


def cell_isosurface_numpy(m):
    return tet_isosurface_numpy(as_tets(m))


# ---- mesh makers ----
def cells(types, lists):
    """(types uint8, offsets uint32, conn uint32) of per-cell index lists."""
    sizes = [len(x) for x in lists]
    assert sizes == [NPOINTS[t] for t in types]
    return (np.asarray(types, np.uint8), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32),
            np.asarray([i for x in lists for i in x], np.uint32))


def renumbered(points, lists, seed):
    """Points and cells with the point indices permuted by a seed (None: as they are)."""
    points = np.asarray(points, F32)
    if seed is None:
        return points, [list(x) for x in lists]
    perm = np.random.default_rng(seed).permutation(len(points))
    out = np.empty_like(points)
    out[perm] = points
    return out, [[int(perm[i]) for i in x] for x in lists]


UNIT = {
    TET: th.single_tet()[0],
    HEX: np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0],
                   [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], F32),
    WEDGE: np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], F32),
    PYRAMID: np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1]], F32),
}


def one_cell(ctype, seed=None, points=None):
    """(points, types, offsets, conn) of one cell of a type (points: its
    corners by local position), renumbered by a seed."""
    p, lists = renumbered(UNIT[ctype] if points is None else points,
                          [list(range(NPOINTS[ctype]))], seed)
    return (p,) + cells([ctype], lists)


def hex_lattice(dims, origin=(0, 0, 0), spacing=(1, 1, 1), seed=None):
    """The hex mesh of a lattice of dims points, cells x fastest, numbered x
    fastest (seed None) or renumbered."""
    nx, ny, nz = dims
    points = th.ih.lattice(dims, origin, spacing).astype(F32).reshape(-1, 3)
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    base = (i + nx * (j + ny * k)).reshape(-1)
    corner = np.array([0, 1, 1 + nx, nx])
    corner = np.concatenate([corner, corner + nx * ny])
    lists = base[:, None] + corner[None]
    if seed is not None:
        perm = np.random.default_rng(seed).permutation(len(points))
        out = np.empty_like(points)
        out[perm] = points
        points, lists = out, perm[lists]
    n = len(lists)
    return (points, np.full(n, HEX, np.uint8), (8 * np.arange(n + 1)).astype(np.uint32),
            lists.reshape(-1).astype(np.uint32))


def mixed_mesh(seed=3):
    """All four types sharing faces: the cube [0, 2]^3 as six pyramids around
    its centre, a hex glued on each face of the cube; the hex on +x is cut into
    two wedges whose triangles lie on the free boundary, the pyramid on -x into
    two tets along the min-index diagonal of its base; indices permuted."""
    pts = [(x, y, z) for z in (0, 2) for y in (0, 2) for x in (0, 2)] + [(1, 1, 1)]
    cid = lambda x, y, z: (x // 2) + 2 * (y // 2) + 4 * (z // 2)
    centre = 8
    bases = []   # the cube's faces, cyclic, with their outward axis and sign
    for ax, sign in ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)):
        u, v = [a for a in range(3) if a != ax]
        quad = []
        for du, dv in ((0, 0), (2, 0), (2, 2), (0, 2)):
            c = [0, 0, 0]
            c[ax], c[u], c[v] = (2 if sign > 0 else 0), du, dv
            quad.append(tuple(c))
        bases.append((ax, sign, quad))
    outer = {}
    for ax, sign, quad in bases:
        for c in quad:
            o = list(c)
            o[ax] += sign
            outer[(ax, sign, c)] = len(pts)
            pts.append(tuple(o))
    perm = np.random.default_rng(seed).permutation(len(pts))
    N = lambda i: int(perm[i])
    types, lists = [], []
    for ax, sign, quad in bases:
        B = [N(cid(*c)) for c in quad]
        O = [N(outer[(ax, sign, c)]) for c in quad]
        if (ax, sign) == (0, -1):   # two tets, cut like the hex cuts the base
            j = B.index(min(B))
            r = [B[(j + d) % 4] for d in range(4)]
            types += [TET, TET]
            lists += [[r[0], r[1], r[2], N(centre)], [r[0], r[2], r[3], N(centre)]]
        else:
            types.append(PYRAMID)
            lists.append(B + [N(centre)])
        if (ax, sign) == (0, 1):    # two wedges: the sides B0 B1 O1 O0 and B3 B2 O2 O3 are cut
            types += [WEDGE, WEDGE]
            lists += [[B[0], B[1], O[1], B[3], B[2], O[2]], [B[0], O[1], O[0], B[3], O[2], O[3]]]
        else:
            types.append(HEX)
            lists.append(B + O)
    points = np.empty((len(pts), 3), F32)
    points[perm] = np.asarray(pts, F32)
    return (points,) + cells(types, lists)


def tets_only(tm):
    """The cell mesh dict of a tet_helpers mesh dict."""
    T = np.ascontiguousarray(tm["tets"]).reshape(-1, 4)
    m = dict(tm, types=np.full(len(T), TET, np.uint8),
             offsets=(4 * np.arange(len(T) + 1)).astype(np.uint32),
             conn=T.reshape(-1).astype(np.uint32))
    m.pop("tets")
    return m


def mesh(geometry, f, iso, normals=False, color=None, cmap_seed=None, ntable=0, clamp=1.0):
    """A cell mesh dict of (points, types, offsets, conn) with tet_helpers.mesh's fields."""
    points, types, offsets, conn = geometry
    m = th.mesh(points, None, f, iso, normals, color, cmap_seed, ntable, clamp)
    m.pop("tets")
    m.update(types=types, offsets=offsets, conn=conn)
    return m


def sphere(c, r):
    return lambda p: r - np.linalg.norm(p.astype(np.float64) - np.asarray(c), axis=-1)


ONE_TET, ONE_HEX, ONE_WEDGE, ONE_PYRAMID, MIXED, SMALL, FULL, PARTIAL, EMPTY, NOCELLS, LARGE = range(11)


def gpu_meshes():
    """The meshes of the GPU batch: one cell of each type, the mixed mesh, a
    renumbered lattice of 5^3 points, 9x9x5 points (256 hexes: one full block),
    17x9x6 (640: a partial last block), a mesh no cell crosses and one without
    cells in the middle, 53^3 points with a busy field (140,608 hexes in 550
    blocks: past one stride of the 512-wide scan).  Tables of 1 and 4096
    entries, one constant colour, one colourless; some with normals."""
    inner = sphere((0.3, 0.2, 0.1), 0.8)
    ms = [mesh(one_cell(TET, 1), sphere((0.1, 0.2, 0.1), 1.0), 0.0),
          mesh(one_cell(HEX, 2), inner, 0.0, normals=True, color=0x00123456),
          mesh(one_cell(WEDGE, 3), inner, 0.0, cmap_seed=15, ntable=8),
          mesh(one_cell(PYRAMID, 4), inner, 0.0, normals=True),
          mesh(mixed_mesh(), sphere((1.0, 0.7, 0.8), 1.7), 0.0, normals=True, cmap_seed=16,
               ntable=64),
          mesh(hex_lattice((5, 5, 5), (3, 2, 1), (2, 2, 2), seed=7), th.wave_f, 0.3, cmap_seed=11,
               ntable=1),
          mesh(hex_lattice((9, 9, 5), (-1, 2, 0.5), (0.5, 0.75, 1.25)), th.wave_f, 0.3, normals=True,
               cmap_seed=12, ntable=4096, clamp=0.3),
          mesh(hex_lattice((17, 9, 6)), th.wave_f, 0.3, normals=True, color=0x00ABCDEF),
          mesh(hex_lattice((4, 3, 3)), th.wave_f, 100.0, normals=True, cmap_seed=13, ntable=16),
          mesh(hex_lattice((4, 3, 3)), th.wave_f, 0.3, normals=True, color=0x00333333),
          mesh(hex_lattice((53, 53, 53), (0, 0, 0), (0.6, 0.6, 0.6)), th.busy_f, 0.1, normals=True,
               cmap_seed=14, ntable=256)]
    e = ms[NOCELLS]
    e.update(types=e["types"][:0], offsets=e["offsets"][:1], conn=e["conn"][:0])
    return ms


def on_device(meshes):
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
    return out


def host_mesh(spray, m, normals=True):
    """(verts, normals, colors, faces) of a cell mesh dict from the host restatement."""
    return spray.cell_isosurface_host(m["points"], m["types"], m["offsets"], m["conn"], m["values"],
                                      m["iso"], m.get("normals") if normals else None,
                                      m.get("cfield"), m.get("cmap"), m.get("color"))


def host_tets(spray, m):
    return spray.cell_split_host(m["types"], m["offsets"], m["conn"], len(m["points"]))


def tet_face_counts(tets):
    """(distinct tet-face triangles as sorted index triples, their counts)."""
    T = np.asarray(tets, np.int64).reshape(-1, 4)
    tri = np.concatenate([T[:, [a, b, c]] for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))])
    return np.unique(np.sort(tri, axis=1), axis=0, return_counts=True)


def assert_closed_manifold(tris):
    """Undirected: every edge in exactly two triangles, one connected piece per
    vertex fan is not asked for -- the boundary of a solid."""
    t = np.asarray(tris, np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    assert len(t) > 0 and (cnt == 2).all()


def det6(p, T):
    """Six times the signed volume of tets T of integer points p, exact in float64."""
    p = np.asarray(p, np.float64)
    a, b, c = (p[T[:, v]] - p[T[:, 0]] for v in (1, 2, 3))
    return (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1])
            - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0])
            + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]))

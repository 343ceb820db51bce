"""Fields, a numpy restatement of the isosurface extraction and mesh checks
shared by the isosurface tests (test_isosurface_host.py, test_gpu_isosurface.py).

The restatement is written from DESIGN.md section 12, not from the C code:
marching tetrahedra over the Kuhn split, vertices ordered by (point, edge
type), faces by (cell, tetrahedron, triangle), all arithmetic in float32.
"""
import itertools

import numpy as np

F32 = np.float32
# edge type -> (dx, dy, dz) of the partner: +x +y +z +xy +xz +yz +xyz
EDGE = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: xyz xzy yxz yzx zxy zyx


def _parity(seq):
    """Inversions of a sequence, mod 2."""
    return sum(a > b for a, b in itertools.combinations(seq, 2)) & 1


def tet_triangles(perm, s):
    """Triangles of one tetrahedron: perm its axis order, s[v] whether vertex v
    of the walk (0,0,0) -> (1,1,1) is inside.  Each triangle is three edges
    (u, v), u < v, of walk vertices.  Ng = (p0 - p1) x (p2 - p0) must leave the
    inside region."""
    ins = [v for v in range(4) if s[v]]
    out = [v for v in range(4) if not s[v]]
    if not ins or not out:
        return []
    odd = _parity(perm)
    e = lambda u, v: (min(u, v), max(u, v))
    if len(ins) != 2:
        a = ins[0] if len(ins) == 1 else out[0]
        b, c, d = [v for v in range(4) if v != a]
        # (a, b, c, d) is an even or odd arrangement of the walk; the walk of an
        # even permutation is positively oriented
        positive = (_parity((a, b, c, d)) ^ odd) == 0
        # positive: the right-handed normal of (ab, ac, ad) points away from a,
        # so Ng (its negative) points at a -- right when a is outside
        keep = positive == (len(ins) == 3)
        t = [e(a, b), e(a, c), e(a, d)]
        return [t if keep else [t[0], t[2], t[1]]]
    a, b = ins
    c, d = out
    q = [e(a, c), e(a, d), e(b, d), e(b, c)]
    positive = (_parity((a, b, c, d)) ^ odd) == 0
    if positive:
        return [[q[0], q[2], q[1]], [q[0], q[3], q[2]]]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


def neg_gradient(f, spacing):
    """[nz, ny, nx, 3]: -(central difference * 0.5, one-sided on the boundary) / spacing."""
    g = np.zeros(f.shape + (3,), F32)
    for ax_np, ax in ((2, 0), (1, 1), (0, 2)):
        m = np.moveaxis(f, ax_np, -1)
        d = np.empty_like(m)
        d[..., 1:-1] = (m[..., 2:] - m[..., :-2]) * F32(0.5)
        d[..., 0] = m[..., 1] - m[..., 0]
        d[..., -1] = m[..., -1] - m[..., -2]
        g[..., ax] = -(np.moveaxis(d, -1, ax_np) / F32(spacing[ax]))
    return g


def isosurface_numpy(values, origin, spacing, iso, normals=True):
    """-> verts float32 [nv, 3], normals float32 [nv, 3] (or None), faces uint32 [nf, 3]."""
    f = np.ascontiguousarray(values, F32)
    nz, ny, nx = f.shape
    origin = np.asarray(origin, F32)
    spacing = np.asarray(spacing, F32)
    iso = F32(iso)
    ins = f >= iso
    g = neg_gradient(f, spacing) if normals else None
    keys, pos, nrm = [], [], []
    with np.errstate(all="ignore"):
        for t, (dx, dy, dz) in enumerate(EDGE):
            A = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
            B = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
            k, j, i = np.nonzero(ins[A] != ins[B])
            fa, fb = f[A][k, j, i], f[B][k, j, i]
            w = ((iso - fa) / (fb - fa)).astype(F32)
            p = np.empty((len(w), 3), F32)
            for ax, (idx, step) in enumerate(((i, dx), (j, dy), (k, dz))):
                pa = origin[ax] + idx.astype(F32) * spacing[ax]
                pb = origin[ax] + (idx + step).astype(F32) * spacing[ax]
                p[:, ax] = pa + w * (pb - pa)
            keys.append((i + nx * (j + ny * k)) * 7 + t)
            pos.append(p)
            if normals:
                na, nb = g[A][k, j, i], g[B][k, j, i]
                nrm.append((na + w[:, None] * (nb - na)).astype(F32))
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    verts = np.concatenate(pos)[order]
    vn = np.concatenate(nrm)[order] if normals else None
    vid = {int(k): n for n, k in enumerate(keys[order])}
    faces = []
    type_of = {d: t for t, d in enumerate(EDGE)}
    for k, j, i in itertools.product(range(nz - 1), range(ny - 1), range(nx - 1)):
        cell = ins[k:k + 2, j:j + 2, i:i + 2]
        if cell.all() or not cell.any():
            continue
        for perm in PERMS:
            walk = [(0, 0, 0)]
            for ax in perm:
                w = list(walk[-1])
                w[ax] = 1
                walk.append(tuple(w))
            s = [bool(cell[z, y, x]) for x, y, z in walk]
            for tri in tet_triangles(perm, s):
                ids = []
                for u, v in tri:
                    (ax, ay, az), (bx, by, bz) = walk[u], walk[v]
                    t = type_of[(bx - ax, by - ay, bz - az)]
                    ids.append(vid[((i + ax) + nx * ((j + ay) + ny * (k + az))) * 7 + t])
                faces.append(ids)
    return verts, vn, np.asarray(faces, np.uint32).reshape(-1, 3)


# ---- fields ----
def lattice(dims, origin=(0, 0, 0), spacing=(1, 1, 1)):
    """Float64 coordinates [nz, ny, nx, 3] of the float32 lattice points."""
    nx, ny, nz = dims
    o, s = np.asarray(origin, F32), np.asarray(spacing, F32)
    ax = [(o[a] + np.arange(n).astype(F32) * s[a]).astype(np.float64)
          for a, n in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1)


def sphere_f(p):
    return 2.3 - np.linalg.norm(p - np.array([4.2, 3.4, 3.1]), axis=-1)


def sphere_grad(p):
    d = p - np.array([4.2, 3.4, 3.1])
    return -d / np.linalg.norm(d, axis=-1, keepdims=True)


TORUS_C, TORUS_R, TORUS_r = np.array([8.0, 8.0, 8.0]), 4.6, 1.7


def torus_f(p):
    d = p - TORUS_C
    q = np.hypot(d[..., 0], d[..., 1]) - TORUS_R
    return TORUS_r - np.hypot(q, d[..., 2])


def torus_grad(p):
    d = p - TORUS_C
    rho = np.hypot(d[..., 0], d[..., 1])
    q = rho - TORUS_R
    h = np.hypot(q, d[..., 2])
    return -np.stack([q / h * d[..., 0] / rho, q / h * d[..., 1] / rho, d[..., 2] / h], -1)


def wavelet_f(p, centre=(32.0, 32.0, 16.0), sigma=18.0):
    """A Gaussian times a sum of sinusoids (the shape of the wavelet source)."""
    d = p - np.asarray(centre)
    gauss = np.exp(-(d ** 2).sum(-1) / (2 * sigma * sigma))
    return gauss * (np.sin(0.31 * p[..., 0]) + np.sin(0.23 * p[..., 1] + 1.0)
                    + np.cos(0.41 * p[..., 2]))


def grid(values, origin=(0, 0, 0), spacing=(1, 1, 1), iso=0.0, color=None):
    return dict(values=np.ascontiguousarray(values, F32), origin=tuple(origin),
                spacing=tuple(spacing), iso=float(iso), color=color)


def sphere_grid():
    return grid(sphere_f(lattice((9, 8, 7))))


def torus_grid():
    return grid(torus_f(lattice((17, 17, 17))))


def ramp_grid(dims, iso, seed):
    """A generic field without symmetry: a random linear ramp plus noise."""
    rng = np.random.default_rng(seed)
    p = lattice(dims)
    f = p @ rng.normal(size=3) + rng.normal(size=p.shape[:-1]) * 0.7
    return grid(f - np.median(f), iso=iso)


def gpu_grids():
    """The grids of the GPU batch (ISSUE table), an empty surface last."""
    w = wavelet_f(lattice((65, 65, 33)))
    return [ramp_grid((2, 2, 2), 0.0, 1), ramp_grid((5, 4, 3), 0.1, 2),
            dict(sphere_grid(), color=0x00123456), dict(torus_grid(), color=0x00ABCDEF),
            ramp_grid((33, 17, 9), 0.2, 3), grid(w, iso=0.35, color=0x00C08040),
            grid(sphere_f(lattice((6, 5, 4))), iso=100.0)]


# ---- mesh checks ----
def directed_edges(faces):
    f = faces.astype(np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def assert_closed_oriented(faces, nverts, euler):
    e = directed_edges(faces)
    key = e[:, 0] * nverts + e[:, 1]
    rev = e[:, 1] * nverts + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    assert cnt.max() == 1                       # every directed edge once
    assert np.array_equal(uniq, np.unique(rev))  # and its reverse once
    assert nverts - len(uniq) // 2 + len(faces) == euler


def geometric_normals(verts, faces):
    """The project's Ng = (v0 - v1) x (v2 - v0), float64."""
    v = verts.astype(np.float64)[faces]
    return np.cross(v[:, 0] - v[:, 1], v[:, 2] - v[:, 0])

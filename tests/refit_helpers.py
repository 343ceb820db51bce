"""Meshes, deformations and numpy restatements shared by the refit tests
(test_refit_host.py, test_gpu_refit.py)."""
import ctypes as C
import os

import numpy as np

from conftest import SCENES, axis_rays, edge_rays, random_rays

F32 = np.float32
KNOCHILD = -(1 << 31)
NODE_DTYPE = np.dtype([("l_lo", "<f4", 3), ("l_hi", "<f4", 3), ("r_lo", "<f4", 3),
                       ("r_hi", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("pad", "<i4", 2)])
QNODE4_DTYPE = np.dtype([("q", "<u2", (4, 6)), ("child", "<i4", 4)])
assert NODE_DTYPE.itemsize == 64 and QNODE4_DTYPE.itemsize == 64


# ---- meshes: the smallest that reach each code path ----
def _fan(n):
    """n triangles around the origin, no two coplanar."""
    a = np.linspace(0.0, 1.7 * np.pi, n + 1)  # open: no two rim points share x, y
    rim = np.stack([np.cos(a) * 2.0, np.sin(a) * 2.0, 0.3 * np.cos(3.0 * a) + 0.1 * a], 1)
    v = np.concatenate([[[0.1, -0.2, 1.0]], rim]).astype(F32)
    f = np.array([[0, i + 1, i + 2] for i in range(n)], np.uint32)
    return v, f


def _grid(n):
    """n x n quads, z = a bump."""
    g = np.linspace(-3.0, 3.0, n + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 1.5 * np.exp(-(x * x + y * y) / 4.0) + 0.05 * x
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3),
                        np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.uint32)
    return v, f


MESHES = ("tri1", "tri4", "tri5", "grid12", "wavelet0")


def mesh(name, oracle):
    """(verts float32 [nv, 3], faces uint32 [nf, 3])."""
    if name == "tri1":
        return _fan(1)   # the root is itself a leaf, with an empty right child
    if name == "tri4":
        return _fan(4)
    if name == "tri5":
        return _fan(5)   # the first split
    if name == "grid12":
        return _grid(12)  # 288 triangles: several levels in both trees
    v, f, _ = oracle.load_ply(os.path.join(SCENES, name + ".ply"))
    return np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.uint32)


# ---- deformations, each float32 in, float32 out ----
def _extent(v):
    return float((v.max(0) - v.min(0)).max())


def deform(name, v):
    v = np.asarray(v, F32)
    if name == "identity":
        return v.copy()
    if name == "translate":  # moves the grid base
        return (v + np.array([1000.0, -500.0, 250.0], F32)).astype(F32)
    if name == "scale":
        return (v * np.array([3.0, 1.0, 0.25], F32)).astype(F32)
    if name == "flatten":  # the zero-extent branch of make_qgrid
        o = v.copy()
        o[:, 2] = F32(2.0)
        return o
    if name == "sin":  # smooth per-vertex displacement, 10 % of the extent
        e = _extent(v)
        k = 2.0 * np.pi / max(e, 1e-6)
        d = np.stack([np.sin(k * v[:, 1]), np.sin(k * v[:, 2] + 1.0), np.sin(k * v[:, 0] + 2.0)], 1)
        return (v + 0.1 * e * d).astype(F32)
    if name == "shear":  # 4 x the extent along x: a bad tree, large overlaps
        e = _extent(v)
        ylo, ey = float(v[:, 1].min()), float(v[:, 1].max() - v[:, 1].min())
        s = (v[:, 1] - ylo) / ey if ey > 0 else np.zeros(len(v))
        o = v.copy()
        o[:, 0] = (v[:, 0] + 4.0 * e * s).astype(F32)
        return o
    raise KeyError(name)


DEFORMS = ("identity", "translate", "scale", "flatten", "sin", "shear")


def vertex_normals(oracle, v, f):
    n = np.zeros_like(v)
    oracle.lib().or_compute_normals(oracle._p(v), len(v), oracle._p(f), len(f), oracle._p(n))
    return n


def vertex_colors(nv):
    return ((np.arange(nv, dtype=np.uint64) * 2654435761) & 0xFFFFFF).astype(np.uint32)


# ---- the canonical build through the host ABI ----
def build_host(v, f):
    """dict(nodes NODE_DTYPE[], tris [nt, 12], prims, grid [6], qnodes4 QNODE4_DTYPE[])."""
    from spray_amd._native import lib
    L = lib()
    nn, nq = C.c_size_t(), C.c_size_t()
    depth, bound = C.c_int(), C.c_int()
    assert L.spray_rt_bvh_build_host(v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(nn),
                                     C.byref(depth), None, None, None) == 0
    nodes = np.zeros(nn.value, NODE_DTYPE)
    tris = np.zeros((len(f), 12), F32)
    prims = np.zeros(len(f), np.uint32)
    assert L.spray_rt_bvh_build_host(v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(nn),
                                     C.byref(depth), nodes.ctypes.data, tris.ctypes.data,
                                     prims.ctypes.data) == 0
    assert L.spray_rt_qnodes4_host(v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(nq),
                                   C.byref(bound), None, None) == 0
    grid = np.zeros(6, F32)
    q4 = np.zeros(nq.value, QNODE4_DTYPE)
    assert L.spray_rt_qnodes4_host(v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(nq),
                                   C.byref(bound), grid.ctypes.data, q4.ctypes.data) == 0
    return {"nodes": nodes, "tris": tris, "prims": prims, "grid": grid, "qnodes4": q4}


def refit_host(v0, v1, f):
    """spray_rt_bvh_refit_host with the records typed as build_host's."""
    import spray_amd
    r = spray_amd.bvh_refit_host(v0, v1, f)
    return {"nodes": r["nodes"].reshape(-1).view(NODE_DTYPE), "tris": r["tris"],
            "grid": r["grid"], "qnodes4": r["qnodes4"].reshape(-1).view(QNODE4_DTYPE)}


# ---- numpy restatements ----
def _empty(lo):
    return lo[0] == np.inf


def _leaf(ref):
    u = (~int(ref)) & 0xFFFFFFFF
    return u >> 2, (u & 3) + 1


def pad_np(lo, hi):
    """The builder's pad, float32, in its operation order."""
    lo, hi = lo.astype(F32), hi.astype(F32)
    e = hi - lo
    m = np.maximum(np.maximum(np.abs(lo), np.abs(hi)), e)
    p = m * F32(1e-6)
    return lo - p, hi + p


def expected_boxes(nodes, prims, f, v):
    """Per (node, side): pad(exact min/max of the subtree's vertices); the
    never-hit box of a root that is a leaf stays.  -> (lo, hi) [nn, 2, 3], and
    the leaf-order triangle range [first, end) of every (node, side)."""
    nn = len(nodes)
    lo = np.zeros((nn, 2, 3), F32)
    hi = np.zeros((nn, 2, 3), F32)
    rng = np.zeros((nn, 2, 2), np.int64)
    for i in range(nn - 1, -1, -1):  # children have larger indices
        for side, (kl, kh, kr) in enumerate((("l_lo", "l_hi", "left"), ("r_lo", "r_hi", "right"))):
            if _empty(nodes[kl][i]):
                lo[i, side], hi[i, side] = nodes[kl][i], nodes[kh][i]
                rng[i, side] = (-1, -1)
                continue
            ref = int(nodes[kr][i])
            if ref < 0:
                first, cnt = _leaf(ref)
                rng[i, side] = (first, first + cnt)
            else:
                rng[i, side] = (rng[ref, 0, 0], rng[ref, 1, 1] if rng[ref, 1, 1] >= 0
                                else rng[ref, 0, 1])
            first, end = rng[i, side]
            pts = v[f[prims[first:end]].reshape(-1)]
            lo[i, side], hi[i, side] = pts.min(0), pts.max(0)
    plo, phi = pad_np(lo, hi)
    for i in range(nn):
        for side, kl in enumerate(("l_lo", "r_lo")):
            if _empty(nodes[kl][i]):
                plo[i, side], phi[i, side] = lo[i, side], hi[i, side]
    return plo, phi, rng


def expected_tris(prims, f, v):
    """The twelve floats of every leaf-order record: v0, e1 = v0 - v1, e2 = v2 -
    v0, Ng = e1 x e2 with one fused multiply-add per component."""
    ff = f[prims]
    a, b, c = v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]]
    e1, e2 = (a - b).astype(F32), (c - a).astype(F32)
    out = np.zeros((len(ff), 12), F32)
    out[:, 0:3], out[:, 3:6], out[:, 6:9] = a, e1, e2
    out[:, 9] = fma_neg(e1[:, 1], e2[:, 2], e1[:, 2], e2[:, 1])
    out[:, 10] = fma_neg(e1[:, 2], e2[:, 0], e1[:, 0], e2[:, 2])
    out[:, 11] = fma_neg(e1[:, 0], e2[:, 1], e1[:, 1], e2[:, 0])
    return out


def fma_neg(x, y, z, w):
    """fmaf(x, y, -(z * w)) per element, bit exact.  z * w is rounded to
    float32 first; x * y is exact in float64 (48 bits); where the float64 sum
    of the two is exact too (TwoSum's error term is zero) its rounding to
    float32 is the fused result, elsewhere the sum is formed with fractions."""
    from fractions import Fraction
    zw = (z.astype(F32) * w.astype(F32)).astype(F32)
    a = x.astype(np.float64) * y.astype(np.float64)
    b = -zw.astype(np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    out = s.astype(F32)
    for i in np.nonzero(err != 0)[0]:
        out[i] = _round_f32(Fraction(float(a[i])) + Fraction(float(b[i])))
    return out


def _round_f32(fr):
    """Fraction -> nearest float32, ties to even (normal range)."""
    from fractions import Fraction
    near = F32(float(fr))  # within one float32 step of the answer
    cand = {float(near), float(np.nextafter(near, F32(np.inf))),
            float(np.nextafter(near, F32(-np.inf)))}
    return F32(min(cand, key=lambda c: (abs(Fraction(c) - fr),
                                        int(F32(c).view(np.uint32)) & 1)))


def decode_q(grid, q):
    """fmaf(float(q), scale, base) per axis for q [..., 3] -> float64 [..., 3]
    (q * scale is exact in float64; the sum is rounded to float64, then to
    float32 as the kernels' folded slab holds it)."""
    base, scale = grid[:3].astype(np.float64), grid[3:].astype(np.float64)
    return (q.astype(np.float64) * scale + base).astype(F32).astype(np.float64)


def q4_child_ranges(q4):
    """Leaf-order triangle range of every QNode4 child ((-1, -1): empty)."""
    nq = len(q4)
    rng = np.full((nq, 4, 2), -1, np.int64)
    for i in range(nq - 1, -1, -1):  # children after parents
        for c in range(4):
            ref = int(q4["child"][i, c])
            if ref == KNOCHILD:
                continue
            if ref < 0:
                first, cnt = _leaf(ref)
                rng[i, c] = (first, first + cnt)
            else:
                sub = rng[ref][rng[ref][:, 0] >= 0]
                rng[i, c] = (sub[:, 0].min(), sub[:, 1].max())
    return rng


def refit_rays(rng, v, f, n=1500):
    """About 3,000 rays of conftest's three generators around mesh (v, f)."""
    lo, hi = v.min(0), v.max(0)
    c = (lo + hi) / 2
    r = float(np.linalg.norm(hi - lo))
    o1, d1 = random_rays(rng, n, c, max(r, 1e-3) * 0.75)
    o2, d2 = edge_rays(rng, v, f, n - 300)
    o3, d3 = axis_rays(v, 100)
    return (np.concatenate([o1, o2, o3]).astype(F32), np.concatenate([d1, d2, d3]).astype(F32))

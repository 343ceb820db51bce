"""A numpy restatement of the colour map rule and the fields, tables and grids
shared by the colour map tests (test_colormap_host.py, test_gpu_colormap.py).

Written from DESIGN.md section 13, not from the C code, in float32 arithmetic:
scale = float(n) / (hi - lo); x = (g - lo) * scale; the bin is 0 where
!(x >= 0), n - 1 where x >= n, else trunc(x); the vertex on lattice edge
(a, b) at the extraction's t gets the bin of ga + t * (gb - ga).  The
(point, type, t) enumeration is iso_helpers.isosurface_numpy's.
"""
import numpy as np

import iso_helpers as ih

F32 = np.float32


def map_scale(n, lo, hi):
    with np.errstate(all="ignore"):
        return F32(n) / (F32(hi) - F32(lo))


def colormap_numpy(g, table, lo, hi):
    """table[bin(g)] for finite float32 g of any shape."""
    table = np.asarray(table, np.uint32)
    n = len(table)
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        x = ((g - F32(lo)).astype(F32) * map_scale(n, lo, hi)).astype(F32)
    inside = (x >= 0) & (x < F32(n))
    idx = np.where(inside, x, 0).astype(np.int64)   # trunc toward zero of 0 <= x < n
    idx = np.where(x >= F32(n), n - 1, idx)         # !(x >= 0) stays 0
    return table[idx]


def edge_scalars(values, iso, cfield):
    """The interpolated colour scalar of every mesh vertex, in vertex order
    (point, x fastest; edge type)."""
    f = np.ascontiguousarray(values, F32)
    g = np.ascontiguousarray(cfield, F32)
    nz, ny, nx = f.shape
    iso = F32(iso)
    ins = f >= iso
    keys, out = [], []
    with np.errstate(all="ignore"):
        for t, (dx, dy, dz) in enumerate(ih.EDGE):
            A = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
            B = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
            k, j, i = np.nonzero(ins[A] != ins[B])
            fa, fb = f[A][k, j, i], f[B][k, j, i]
            w = ((iso - fa) / (fb - fa)).astype(F32)
            ga, gb = g[A][k, j, i], g[B][k, j, i]
            out.append((ga + (w * (gb - ga)).astype(F32)).astype(F32))
            keys.append((i + nx * (j + ny * k)) * 7 + t)
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(out)[order]


def vertex_colors_numpy(g):
    """The colours of a grid dict: mapped, constant, or 0 without either."""
    if g.get("cfield") is None:
        nv = len(edge_scalars(g["values"], g["iso"], g["values"]))
        return np.full(nv, g.get("color") or 0, np.uint32)
    table, lo, hi = g["cmap"]
    return colormap_numpy(edge_scalars(g["values"], g["iso"], g["cfield"]), table, lo, hi)


# ---- tables, fields, grids ----
def table(n, seed):
    return (np.random.default_rng(seed).integers(0, 1 << 24, n)).astype(np.uint32)


def color_field(g, seed):
    """A second field on g's lattice without the first one's symmetry."""
    nz, ny, nx = g["values"].shape
    p = ih.lattice((nx, ny, nz), g["origin"], g["spacing"])
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    return (p @ w * 0.2 + np.sin(0.37 * p[..., 0] + 0.5) * np.cos(0.21 * p[..., 2])
            + 0.1 * rng.normal(size=p.shape[:-1])).astype(F32)


def mapped(g, seed, ntable, clamp=1.0):
    """g coloured by color_field(g, seed) through a table of ntable entries over
    clamp times the field's range about its middle (clamp < 1: both ends clamp)."""
    cf = color_field(g, seed)
    mid, half = 0.5 * (float(cf.max()) + float(cf.min())), 0.5 * (float(cf.max()) - float(cf.min()))
    half = max(half, 0.25) * clamp
    return dict(g, cfield=cf, cmap=(table(ntable, seed + 100), mid - half, mid + half))


MAPPED = (0, 3, 4, 5, 6)    # of gpu_grids(): mapped; 2 keeps its constant colour, 1 none


def gpu_grids():
    """iso_helpers.gpu_grids() with five grids mapped: one cell, a grid that had
    a constant colour, several blocks, more blocks than one scan stride, and the
    empty surface; tables of 1, 7, 256 and 4096 entries, ranges that clamp."""
    gs = ih.gpu_grids()
    for k, (nt, clamp) in zip(MAPPED, ((7, 1.0), (256, 0.25), (1, 1.0), (4096, 0.3), (16, 1.0))):
        gs[k] = mapped(gs[k], 10 + k, nt, clamp)
    return gs


def on_device(grids):
    import torch
    out = []
    for g in grids:
        g = dict(g, values=torch.from_numpy(g["values"]).cuda())
        if g.get("cfield") is not None:
            g["cfield"] = torch.from_numpy(g["cfield"]).cuda()
        out.append(g)
    return out


def host_mesh(spray, g, normals=True):
    """(verts, normals, colors, faces) of a grid dict from the host restatement."""
    return spray.isosurface_mapped_host(g["values"], g["origin"], g["spacing"], g["iso"],
                                        g.get("cfield"), g.get("cmap"), normals, g.get("color"))

"""Python front-end of the engine: RtContext (spray_rt.h) and Scene
(spray_scene.h).

Buffers may be numpy arrays (host: the call is synchronous, like Embree's)
or torch tensors on the GPU (device: enqueued on the context's stream; call
``sync()``).  The method names follow the reference's scene surface
(src/render/scene.h:153-205): load, intersect, occluded, intersectDomains.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._native import (HIT_DTYPE, INVALID_ID, RAY_DTYPE, RTC_ISECT_DTYPE, BsdfRec,
                      SprayRtError, CellMesh, CellSelect, TetMesh, lib)

__all__ = ["RtContext", "Scene", "OocCache", "ooc_scene", "camera_init", "make_rays",
           "bvh_refit_host", "bvh_build_device_host", "isosurface_host",
           "isosurface_mapped_host", "colormap_host", "tet_isosurface_host",
           "cell_isosurface_host", "cell_split_host", "cell_surface_host", "cell_clip_host",
           "plane_values_host", "streamlines_host", "stream_tubes_host", "tube_ring",
           "block_streamlines_host", "block_stream_tubes_host",
           "STREAM_FORWARD", "STREAM_BACKWARD", "STREAM_BOTH", "LINE_END_GRID", "LINE_END_STEPS",
           "LINE_END_SPEED", "LINE_END_SEED", "glyphs_host", "glyph_sphere", "GLYPH_SPHERE",
           "GLYPH_ARROW", "SLOT_COLORS",
           "SLOT_FACES",
           "host_parse_scene", "host_scene_bsdfs",
           "host_domain_mesh", "RAY_DTYPE",
           "HIT_DTYPE", "RTC_ISECT_DTYPE", "INVALID_ID", "SprayRtError"]


def _addr(x):
    """(address, keepalive) of a numpy array / torch tensor / int / None."""
    if x is None:
        return None, None
    if isinstance(x, int):
        return x, None
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("arrays must be C-contiguous")
        return x.ctypes.data, x
    if hasattr(x, "data_ptr"):
        if hasattr(x, "is_contiguous") and not x.is_contiguous():
            raise ValueError("tensors must be contiguous")
        return x.data_ptr(), x
    raise TypeError("unsupported buffer type %r" % type(x))


def _nbytes(x):
    if isinstance(x, np.ndarray):
        return x.nbytes
    return x.numel() * x.element_size()


def _lv_pixels(lv, nsamples):
    """Pixels the (pixel, sample) table lv holds (float4 per entry): the
    engine's bound on the pixel ids of an AO pairs spawn."""
    return _nbytes(lv) // (16 * int(nsamples))


def camera_init(pos, lookat, up, vfov, w, h):
    """Camera::init (src/render/camera.h:128-166) -> float32[14]."""
    cam = np.zeros(14, np.float32)
    p = np.asarray(pos, np.float32)
    la = np.asarray(lookat, np.float32)
    u = np.asarray(up, np.float32)
    lib().spray_camera_init(p.ctypes.data, la.ctypes.data, u.ctypes.data,
                            float(vfov), int(w), int(h), cam.ctypes.data)
    return cam


def make_rays(org, dir, tnear=0.001, tfar=np.inf):
    """Packs org/dir [n,3] into the 32-B ray records of the scene path."""
    org = np.asarray(org, np.float32).reshape(-1, 3)
    r = np.zeros(len(org), RAY_DTYPE)
    r["org"] = org
    r["dir"] = np.asarray(dir, np.float32).reshape(-1, 3)
    r["tnear"] = tnear
    r["tfar"] = tfar
    return r


def bvh_refit_host(verts0, new_verts, faces):
    """spray_rt_bvh_refit_host (no GPU): the image a refit of the canonical
    build of (verts0, faces) to new_verts produces -> dict of nodes (uint8
    [nnodes, 64]), tris (float32 [ntris, 12]), grid (float32 [6]), qnodes4
    (uint8 [nq, 64])."""
    v0 = np.ascontiguousarray(verts0, np.float32).reshape(-1, 3)
    v1 = np.ascontiguousarray(new_verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    if v0.shape != v1.shape:
        raise ValueError("new_verts must have the shape of verts0")
    L = lib()
    nn, nq = C.c_size_t(), C.c_size_t()
    if L.spray_rt_bvh_build_host(v0.ctypes.data, len(v0), f.ctypes.data, len(f), C.byref(nn),
                                 None, None, None, None) != 0:
        raise SprayRtError("bvh_refit_host: invalid mesh")
    rc = L.spray_rt_qnodes4_host(v0.ctypes.data, len(v0), f.ctypes.data, len(f), C.byref(nq),
                                 None, None, None)
    if rc != 0:
        e = SprayRtError("bvh_refit_host: the built mesh cannot be quantized (%d)" % rc)
        e.code = rc
        raise e
    out = {"nodes": np.zeros((nn.value, 64), np.uint8), "tris": np.zeros((len(f), 12), np.float32),
           "grid": np.zeros(6, np.float32), "qnodes4": np.zeros((nq.value, 64), np.uint8)}
    rc = L.spray_rt_bvh_refit_host(v0.ctypes.data, v1.ctypes.data, len(v0), f.ctypes.data, len(f),
                                   out["nodes"].ctypes.data, out["tris"].ctypes.data,
                                   out["grid"].ctypes.data, out["qnodes4"].ctypes.data)
    if rc != 0:
        e = SprayRtError("bvh_refit_host failed (%d)" % rc)
        e.code = rc
        raise e
    return out


def bvh_build_device_host(verts, faces):
    """spray_rt_bvh_build_device_host (no GPU): the image RtContext.build_domains
    leaves in a slot -> dict of nodes (uint8 [nnodes, 64]), tris (float32
    [ntris, 12]), prims (uint32 [ntris]), grid (float32 [6]), qnodes4 (uint8
    [nq, 64]), depth, stack_bound, nmedian."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    L = lib()
    nn, nq = C.c_size_t(), C.c_size_t()
    depth, bound, nmed = C.c_int(), C.c_int(), C.c_int()

    def call(*outs):
        rc = L.spray_rt_bvh_build_device_host(v.ctypes.data, len(v), f.ctypes.data, len(f),
                                              C.byref(nn), C.byref(nq), C.byref(depth),
                                              C.byref(bound), C.byref(nmed), *outs)
        if rc != 0:
            e = SprayRtError("bvh_build_device_host failed (%d)" % rc)
            e.code = rc
            raise e

    call(None, None, None, None, None)
    out = {"nodes": np.zeros((nn.value, 64), np.uint8), "tris": np.zeros((len(f), 12), np.float32),
           "prims": np.zeros(len(f), np.uint32), "grid": np.zeros(6, np.float32),
           "qnodes4": np.zeros((nq.value, 64), np.uint8)}
    call(*[out[k].ctypes.data for k in ("nodes", "tris", "prims", "grid", "qnodes4")])
    out.update(depth=depth.value, stack_bound=bound.value, nmedian=nmed.value)
    return out


class _Grid(C.Structure):
    """spray_rt_grid."""
    _fields_ = [("values", C.c_void_p), ("dims", C.c_int32 * 3), ("origin", C.c_float * 3),
                ("spacing", C.c_float * 3), ("isovalue", C.c_float), ("color_rgb", C.c_uint32),
                ("has_color", C.c_int32)]


assert C.sizeof(_Grid) == 56


def _grid_table(grids):
    """[(values, origin, spacing, iso[, color])] or dicts with those keys ->
    (spray_rt_grid array, keepalive).  values: float32 [nz, ny, nx], a numpy
    array or a torch tensor on the GPU."""
    arr = (_Grid * max(len(grids), 1))()
    keep = []
    for g, rec in zip(grids, arr):
        if isinstance(g, dict):
            g = (g["values"], g["origin"], g["spacing"], g["iso"], g.get("color"))
        values, origin, spacing, iso = g[:4]
        color = g[4] if len(g) > 4 else None
        if hasattr(values, "data_ptr"):
            if values.element_size() != 4 or not values.is_floating_point():
                raise TypeError("isosurface: fields are float32")
        else:
            values = np.ascontiguousarray(values, np.float32)
        if len(values.shape) != 3:
            raise ValueError("isosurface: a field is a [nz, ny, nx] array")
        a, k = _addr(values)
        keep.append(k)
        rec.values = a
        nz, ny, nx = (int(d) for d in values.shape)
        rec.dims = (C.c_int32 * 3)(nx, ny, nz)
        rec.origin = (C.c_float * 3)(*[float(x) for x in origin])
        rec.spacing = (C.c_float * 3)(*[float(x) for x in spacing])
        rec.isovalue = float(iso)
        rec.has_color = 0 if color is None else 1
        rec.color_rgb = 0 if color is None else int(color)
    return arr, keep


def isosurface_host(values, origin, spacing, iso, normals=True):
    """spray_rt_isosurface_host (no GPU): the mesh RtContext.isosurface extracts
    from a float32 [nz, ny, nx] field -> (verts float32 [nv, 3], normals float32
    [nv, 3] or None, faces uint32 [nf, 3])."""
    arr, keep = _grid_table([(np.ascontiguousarray(values, np.float32), origin, spacing, iso)])
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_isosurface_host(C.addressof(arr), C.byref(nv), C.byref(nf), *outs)
        if rc != 0:
            e = SprayRtError("isosurface_host failed (%d)" % rc)
            e.code = rc
            raise e

    call(None, None, None)
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals else None
    f = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, f.ctypes.data)
    return v, n, f


class _GridColor(C.Structure):
    """spray_rt_grid_color."""
    _fields_ = [("field", C.c_void_p), ("table_rgb", C.c_void_p), ("ntable", C.c_int32),
                ("lo", C.c_float), ("hi", C.c_float)]


assert C.sizeof(_GridColor) == 32

# spray_rt_slot_export's arrays beyond RtContext.SLOT_NORMALS
SLOT_COLORS, SLOT_FACES = 6, 7


def _cmap_args(cmap):
    """(table uint32[n], lo, hi) -> (table array, its address, n, lo, hi)."""
    table, lo, hi = cmap
    t = np.ascontiguousarray(table, np.uint32).reshape(-1)
    return t, (t.ctypes.data if t.size else None), int(t.size), float(lo), float(hi)


def _fills_done():
    """Tensors created just now are zero-filled on torch's current stream; the
    context's stream is not ordered after it, so the fills complete first."""
    import torch
    torch.cuda.current_stream().synchronize()


def _grid_color_table(grids):
    """The spray_rt_grid_color array parallel to _grid_table(grids): dicts may
    carry "cfield" (float32 [nz, ny, nx], numpy or a torch tensor on the GPU)
    and "cmap" = (table uint32[n], lo, hi); other grids keep their constant
    colour -> (array, keepalive)."""
    arr = (_GridColor * max(len(grids), 1))()
    keep = []
    for g, rec in zip(grids, arr):
        cf = g.get("cfield") if isinstance(g, dict) else None
        if cf is None:
            continue
        values = g["values"]
        if hasattr(cf, "data_ptr"):
            if cf.element_size() != 4 or not cf.is_floating_point():
                raise TypeError("isosurface: fields are float32")
        else:
            cf = np.ascontiguousarray(cf, np.float32)
        if tuple(cf.shape) != tuple(values.shape):
            raise ValueError("isosurface: a colour field has its grid's shape")
        a, k = _addr(cf)
        keep.append(k)
        rec.field = a
        if g.get("cmap") is not None:
            t, rec.table_rgb, rec.ntable, rec.lo, rec.hi = _cmap_args(g["cmap"])
            keep.append(t)
    return arr, keep


def isosurface_mapped_host(values, origin, spacing, iso, cfield=None, cmap=None, normals=True,
                           color=None):
    """spray_rt_isosurface_mapped_host (no GPU): isosurface_host plus the
    per-vertex colours, mapped from cfield through cmap = (table, lo, hi) or the
    constant color -> (verts, normals or None, colors uint32 [nv], faces)."""
    g = dict(values=np.ascontiguousarray(values, np.float32), origin=origin, spacing=spacing,
             iso=iso, color=color, cfield=cfield, cmap=cmap)
    arr, keep = _grid_table([g])
    carr, ckeep = _grid_color_table([g])
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_isosurface_mapped_host(C.addressof(arr), C.addressof(carr), C.byref(nv),
                                               C.byref(nf), *outs)
        if rc != 0:
            e = SprayRtError("isosurface_mapped_host failed (%d)" % rc)
            e.code = rc
            raise e

    call(None, None, None, None)
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals else None
    c = np.zeros(nv.value, np.uint32)
    f = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, f.ctypes.data)
    return v, n, c, f


def colormap_host(scalars, table, lo, hi):
    """spray_rt_colormap_host (no GPU): table[bin] of every scalar -> uint32
    array of scalars' shape."""
    x = np.ascontiguousarray(scalars, np.float32)
    t, ta, nt, lo, hi = _cmap_args((table, lo, hi))
    out = np.zeros(x.shape, np.uint32)
    rc = lib().spray_rt_colormap_host(x.ctypes.data, x.size, ta, nt, lo, hi, out.ctypes.data)
    if rc != 0:
        e = SprayRtError("colormap_host failed (%d)" % rc)
        e.code = rc
        raise e
    return out


def _tet_array(x, dtype, cols, what):
    """x as the [n, cols] (cols 0: [n]) 32-bit array the engine reads: a numpy
    array of dtype or a torch tensor on the GPU -> (array, rows)."""
    if hasattr(x, "data_ptr"):
        if x.element_size() != 4 or x.is_floating_point() != (dtype == np.float32):
            raise TypeError("tet_isosurface: %s are %s" % (what, np.dtype(dtype).name))
        size = x.numel()
    else:
        x = np.ascontiguousarray(x, dtype)
        size = x.size
    if cols and size % cols:
        raise ValueError("tet_isosurface: %s are a [n, %d] array" % (what, cols))
    return x, size // max(cols, 1)


def _tet_table(meshes):
    """Dicts with "points" (float32 [np, 3]), "tets" (uint32 or int32 [nt, 4]),
    "values" (float32 [np]), "iso" and optionally "normals" (float32 [np, 3]),
    "color", "cfield" (float32 [np]) with "cmap" = (table uint32[n], lo, hi) ->
    (spray_rt_tetmesh array, spray_rt_grid_color array, keepalive).  Arrays are
    numpy arrays or torch tensors on the GPU."""
    arr = (TetMesh * max(len(meshes), 1))()
    carr = (_GridColor * max(len(meshes), 1))()
    keep = []

    def put(x):
        a, k = _addr(x)
        keep.append(k)
        return a

    for m, rec, crec in zip(meshes, arr, carr):
        tets = m["tets"]
        if not hasattr(tets, "data_ptr"):
            tets = np.asarray(tets)
            tets = tets.view(np.uint32) if tets.dtype == np.int32 else tets
        points, npts = _tet_array(m["points"], np.float32, 3, "points")
        tets, ntets = _tet_array(tets, np.uint32, 4, "tets")
        values, nval = _tet_array(m["values"], np.float32, 0, "values")
        if nval != npts:
            raise ValueError("tet_isosurface: one value per point")
        rec.points, rec.tets, rec.values = put(points), put(tets), put(values)
        rec.npoints, rec.ntets = npts, ntets
        if m.get("normals") is not None:
            nrm, nn = _tet_array(m["normals"], np.float32, 3, "normals")
            if nn != npts:
                raise ValueError("tet_isosurface: one normal per point")
            rec.point_normals = put(nrm)
        rec.isovalue = float(m["iso"])
        color = m.get("color")
        rec.has_color = 0 if color is None else 1
        rec.color_rgb = 0 if color is None else int(color)
        if m.get("cfield") is not None:
            cf, nc = _tet_array(m["cfield"], np.float32, 0, "colour samples")
            if nc != npts:
                raise ValueError("tet_isosurface: one colour sample per point")
            crec.field = put(cf)
            if m.get("cmap") is not None:
                t, crec.table_rgb, crec.ntable, crec.lo, crec.hi = _cmap_args(m["cmap"])
                keep.append(t)
    return arr, carr, keep


def tet_isosurface_host(points, tets, values, iso, normals=None, cfield=None, cmap=None,
                        color=None):
    """spray_rt_tet_isosurface_host (no GPU): the mesh RtContext.tet_isosurface
    extracts from a tetrahedral mesh (see _tet_table; numpy arrays) -> (verts
    float32 [nv, 3], normals float32 [nv, 3] or None without point normals,
    colors uint32 [nv], faces uint32 [nf, 3])."""
    m = dict(points=points, tets=tets, values=values, iso=iso, normals=normals, cfield=cfield,
             cmap=cmap, color=color)
    arr, carr, keep = _tet_table([m])
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_tet_isosurface_host(C.addressof(arr), C.addressof(carr), C.byref(nv),
                                            C.byref(nf), *outs)
        if rc != 0:
            e = SprayRtError("tet_isosurface_host failed (%d)" % rc)
            e.code = rc
            raise e

    call(None, None, None, None)
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals is not None else None
    c = np.zeros(nv.value, np.uint32)
    f = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, f.ctypes.data)
    return v, n, c, f


def _cell_list(x, dtype, what):
    """x as the flat array of dtype (uint8 or uint32; int32 bits pass as uint32)
    the engine reads: numpy or a torch tensor on the GPU -> (array, count)."""
    size = np.dtype(dtype).itemsize
    if hasattr(x, "data_ptr"):
        if x.element_size() != size or x.is_floating_point():
            raise TypeError("cell_isosurface: %s are %s" % (what, np.dtype(dtype).name))
        return x, x.numel()
    x = np.asarray(x)
    if x.dtype.kind == "i" and x.dtype.itemsize == size:
        x = x.view(dtype)
    x = np.ascontiguousarray(x, dtype)
    return x, x.size


def _cell_table(meshes, contoured=True):
    """Dicts with "points" (float32 [np, 3]), "types" (uint8 [nc], the
    SPRAY_RT_CELL_* = VTK codes), "offsets" (uint32 [nc + 1]), "conn" (uint32
    [nconn]), "values" (float32 [np]), "iso" and optionally "normals", "color",
    "cfield" with "cmap" as in _tet_table -> (spray_rt_cellmesh array,
    spray_rt_grid_color array, keepalive).  Arrays are numpy arrays or torch
    tensors on the GPU.  contoured False: "values" and "iso" are optional (a
    NULL pointer, isovalue 0)."""
    arr = (CellMesh * max(len(meshes), 1))()
    carr = (_GridColor * max(len(meshes), 1))()
    keep = []

    def put(x):
        a, k = _addr(x)
        keep.append(k)
        return a

    for m, rec, crec in zip(meshes, arr, carr):
        points, npts = _tet_array(m["points"], np.float32, 3, "points")
        values = None
        if contoured or m.get("values") is not None:
            values, nval = _tet_array(m["values"], np.float32, 0, "values")
            if nval != npts:
                raise ValueError("cell_isosurface: one value per point")
        types, ncells = _cell_list(m["types"], np.uint8, "types")
        offsets, noff = _cell_list(m["offsets"], np.uint32, "offsets")
        conn, nconn = _cell_list(m["conn"], np.uint32, "conn")
        if noff != ncells + 1:
            raise ValueError("cell_isosurface: one offset per cell and one more")
        rec.points, rec.values = put(points), put(values)
        rec.types, rec.offsets, rec.conn = put(types), put(offsets), put(conn)
        rec.npoints, rec.ncells, rec.nconn = npts, ncells, nconn
        if m.get("normals") is not None:
            nrm, nn = _tet_array(m["normals"], np.float32, 3, "normals")
            if nn != npts:
                raise ValueError("cell_isosurface: one normal per point")
            rec.point_normals = put(nrm)
        rec.isovalue = float(m["iso"] if contoured else m.get("iso", 0.0))
        color = m.get("color")
        rec.has_color = 0 if color is None else 1
        rec.color_rgb = 0 if color is None else int(color)
        if m.get("cfield") is not None:
            cf, nc = _tet_array(m["cfield"], np.float32, 0, "colour samples")
            if nc != npts:
                raise ValueError("cell_isosurface: one colour sample per point")
            crec.field = put(cf)
            if m.get("cmap") is not None:
                t, crec.table_rgb, crec.ntable, crec.lo, crec.hi = _cmap_args(m["cmap"])
                keep.append(t)
    return arr, carr, keep


def _cell_fail(what, rc):
    e = SprayRtError("%s failed (%d)" % (what, rc))
    e.code = rc
    raise e


def cell_split_host(types, offsets, conn, npoints):
    """spray_rt_cell_split_host (no GPU): the full tet list of the split rule
     of a mesh's cells -> uint32 [ntets, 4]."""
    types, ncells = _cell_list(types, np.uint8, "types")
    offsets, noff = _cell_list(offsets, np.uint32, "offsets")
    conn, nconn = _cell_list(conn, np.uint32, "conn")
    if noff != ncells + 1:
        raise ValueError("cell_split_host: one offset per cell and one more")
    rec = CellMesh()
    rec.types, rec.offsets, rec.conn = types.ctypes.data, offsets.ctypes.data, conn.ctypes.data
    rec.npoints, rec.ncells, rec.nconn = int(npoints), ncells, nconn
    L = lib()
    nt = C.c_size_t()
    rc = L.spray_rt_cell_split_host(C.byref(rec), C.byref(nt), None)
    if rc != 0:
        _cell_fail("cell_split_host", rc)
    tets = np.zeros((nt.value, 4), np.uint32)
    rc = L.spray_rt_cell_split_host(C.byref(rec), C.byref(nt), tets.ctypes.data)
    if rc != 0:
        _cell_fail("cell_split_host", rc)
    return tets


def cell_isosurface_host(points, types, offsets, conn, values, iso, normals=None, cfield=None,
                         cmap=None, color=None):
    """spray_rt_cell_isosurface_host (no GPU): the mesh RtContext.cell_isosurface
    extracts from a mesh of mixed cells (see _cell_table; numpy arrays), with
    tet_isosurface_host's results."""
    m = dict(points=points, types=types, offsets=offsets, conn=conn, values=values, iso=iso,
             normals=normals, cfield=cfield, cmap=cmap, color=color)
    arr, carr, keep = _cell_table([m])
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_cell_isosurface_host(C.addressof(arr), C.addressof(carr), C.byref(nv),
                                             C.byref(nf), *outs)
        if rc != 0:
            _cell_fail("cell_isosurface_host", rc)

    call(None, None, None, None)
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals is not None else None
    c = np.zeros(nv.value, np.uint32)
    f = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, f.ctypes.data)
    return v, n, c, f


SELECT_MODES = {"all": 0, "points": 1, "cells": 2}


def _surf_table(meshes, selects):
    """Mesh dicts as in _cell_table, where "values" and "iso" are optional
    ("values" is needed by a "points" select only), with selects parallel to
    them (None: every cell of every mesh): None for every cell, or a dict with
    "mode" ("all", "points", "cells" or the SPRAY_RT_SELECT_* number), "lo",
    "hi" and, for "cells", "cell_values" (float32 [ncells], numpy or a torch
    tensor on the GPU) -> (spray_rt_cellmesh array, spray_rt_cell_select array,
    spray_rt_grid_color array, keepalive)."""
    if selects is not None and len(selects) != len(meshes):
        raise ValueError("cell_surface: one select per mesh")
    sarr = (CellSelect * max(len(meshes), 1))()
    arr, carr, keep = _cell_table(meshes, contoured=False)
    for i in range(len(meshes)):
        sel = selects[i] if selects is not None else None
        if sel is None:
            continue
        mode = sel.get("mode", "all")
        sarr[i].mode = SELECT_MODES[mode] if isinstance(mode, str) else int(mode)
        sarr[i].lo, sarr[i].hi = float(sel.get("lo", 0.0)), float(sel.get("hi", 0.0))
        if sel.get("cell_values") is not None:
            cv, ncv = _tet_array(sel["cell_values"], np.float32, 0, "cell values")
            if ncv != arr[i].ncells:
                raise ValueError("cell_surface: one cell value per cell")
            a, k = _addr(cv)
            keep.append(k)
            sarr[i].cell_values = a
    return arr, sarr, carr, keep


def cell_surface_host(points, types, offsets, conn, select=None, values=None, normals=None,
                      cfield=None, cmap=None, color=None):
    """spray_rt_cell_surface_host (no GPU): the boundary surface of the cells
    a select keeps (see _surf_table; numpy arrays) -> (verts float32 [nv, 3],
    normals float32 [nv, 3] or None without point normals, colors uint32 [nv],
    point_ids uint32 [nv], faces uint32 [nf, 3])."""
    m = dict(points=points, types=types, offsets=offsets, conn=conn, values=values,
             normals=normals, cfield=cfield, cmap=cmap, color=color)
    arr, sarr, carr, keep = _surf_table([m], [select])
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_cell_surface_host(C.addressof(arr), C.addressof(sarr), C.addressof(carr),
                                          C.byref(nv), C.byref(nf), *outs)
        if rc != 0:
            _cell_fail("cell_surface_host", rc)

    call(None, None, None, None, None)
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals is not None else None
    c = np.zeros(nv.value, np.uint32)
    ids = np.zeros(nv.value, np.uint32)
    f = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, ids.ctypes.data,
         f.ctypes.data)
    return v, n, c, ids, f


def _invert_arg(invert, n):
    """invert (None, one flag, or one per mesh) -> int32 array of n or None."""
    if invert is None:
        return None
    flags = [invert] * n if isinstance(invert, (bool, int)) else list(invert)
    if len(flags) != n:
        raise ValueError("cell_clip: one invert flag per mesh")
    return (C.c_int32 * max(n, 1))(*[1 if f else 0 for f in flags])


def cell_clip_host(points, types, offsets, conn, values, iso, invert=False, normals=None,
                   cfield=None, cmap=None, color=None):
    """spray_rt_cell_clip_host (no GPU): the surface of the part of a mesh of
    mixed cells (see _cell_table; numpy arrays) with values >= iso (invert: the
    other part) -> (verts float32 [nv, 3], normals float32 [nv, 3] or None
    without point normals, colors uint32 [nv], vert_pairs uint32 [nv, 2], vert_t
    float32 [nv], faces uint32 [nf, 3], ncap_verts, ncap_faces): the cap's
    vertices and faces come first."""
    m = dict(points=points, types=types, offsets=offsets, conn=conn, values=values, iso=iso,
             normals=normals, cfield=cfield, cmap=cmap, color=color)
    arr, carr, keep = _cell_table([m])
    L = lib()
    nv, nf, ncv, ncf = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_cell_clip_host(C.addressof(arr), 1 if invert else 0, C.addressof(carr),
                                       C.byref(nv), C.byref(nf), C.byref(ncv), C.byref(ncf), *outs)
        if rc != 0:
            _cell_fail("cell_clip_host", rc)

    call(None, None, None, None, None, None)
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals is not None else None
    c = np.zeros(nv.value, np.uint32)
    pairs = np.zeros((nv.value, 2), np.uint32)
    t = np.zeros(nv.value, np.float32)
    f = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, pairs.ctypes.data,
         t.ctypes.data, f.ctypes.data)
    return v, n, c, pairs, t, f, ncv.value, ncf.value


def _plane_args(origin, normal):
    o = np.ascontiguousarray(origin, np.float32).reshape(-1)
    d = np.ascontiguousarray(normal, np.float32).reshape(-1)
    if o.size != 3 or d.size != 3:
        raise ValueError("plane_values: origin and normal have three components")
    return o, d


def plane_values_host(points, origin, normal):
    """spray_rt_plane_values_host (no GPU): ((p - origin) . normal) of every
    point, term by term in float32 -> float32 [npoints]."""
    pts = np.ascontiguousarray(points, np.float32)
    if pts.size % 3:
        raise ValueError("plane_values: points are a [n, 3] array")
    o, d = _plane_args(origin, normal)
    out = np.zeros(pts.size // 3, np.float32)
    rc = lib().spray_rt_plane_values_host(pts.ctypes.data, pts.size // 3, o.ctypes.data,
                                          d.ctypes.data, out.ctypes.data)
    if rc != 0:
        _cell_fail("plane_values_host", rc)
    return out


STREAM_FORWARD, STREAM_BACKWARD, STREAM_BOTH = 0, 1, 2
LINE_END_GRID, LINE_END_STEPS, LINE_END_SPEED, LINE_END_SEED = 0, 1, 2, 3


def _float_array(x, what, tail):
    """A float32 numpy array or GPU tensor whose shape ends in tail."""
    if hasattr(x, "data_ptr"):
        if x.element_size() != 4 or not x.is_floating_point():
            raise TypeError("streamlines: %s are float32" % what)
    else:
        x = np.ascontiguousarray(x, np.float32)
    if tuple(x.shape[len(x.shape) - len(tail):]) != tuple(tail):
        raise ValueError("streamlines: %s are a [..., %s] array"
                         % (what, ", ".join(str(t) for t in tail)))
    return x


def _stream_tables(fields, tubes=None):
    """Dicts with the keys vectors (float32 [nz, ny, nx, 3]), origin, spacing,
    seeds (float32 [nseeds, 3]), step, max_steps and optionally direction
    (STREAM_FORWARD), min_speed (1e-6), cfield (float32 [nz, ny, nx]) and cmap =
    (table uint32[n], lo, hi); arrays are numpy arrays or torch tensors on the
    GPU.  tubes: dicts with radius, nsides and optionally color, one per field
    or one for all -> (spray_rt_vecfield array, spray_rt_tube array or None,
    spray_rt_grid_color array, keepalive)."""
    from ._native import Tube, VecField
    m = max(len(fields), 1)
    arr, carr = (VecField * m)(), (_GridColor * m)()
    keep = []
    for f, rec, crec in zip(fields, arr, carr):
        vec = _float_array(f["vectors"], "vectors", (3,))
        if len(vec.shape) != 4:
            raise ValueError("streamlines: vectors are a [nz, ny, nx, 3] array")
        seeds = _float_array(f["seeds"], "seeds", (3,))
        nseeds = int(np.prod(seeds.shape[:-1])) if len(seeds.shape) > 1 else 1
        keep += [vec, seeds]
        rec.vectors = _addr(vec)[0]
        nz, ny, nx = (int(d) for d in vec.shape[:3])
        rec.dims = (C.c_int32 * 3)(nx, ny, nz)
        rec.origin = (C.c_float * 3)(*[float(x) for x in f["origin"]])
        rec.spacing = (C.c_float * 3)(*[float(x) for x in f["spacing"]])
        rec.seeds = _addr(seeds)[0] if nseeds else None
        rec.nseeds = nseeds
        rec.step = float(f["step"])
        rec.max_steps = int(f["max_steps"])
        rec.direction = int(f.get("direction", STREAM_FORWARD))
        rec.min_speed = float(f.get("min_speed", 1e-6))
        cf = f.get("cfield")
        if cf is not None:
            cf = _float_array(cf, "colour fields", ())
            if tuple(cf.shape) != tuple(vec.shape[:3]):
                raise ValueError("streamlines: a colour field has its grid's shape")
            keep.append(cf)
            crec.field = _addr(cf)[0]
            if f.get("cmap") is not None:
                t, crec.table_rgb, crec.ntable, crec.lo, crec.hi = _cmap_args(f["cmap"])
                keep.append(t)
    tarr = None
    if tubes is not None:
        if isinstance(tubes, dict):
            tubes = [tubes] * len(fields)
        if len(tubes) != len(fields):
            raise ValueError("stream_tubes: one tube per field")
        tarr = (Tube * m)()
        for t, rec in zip(tubes, tarr):
            rec.radius = float(t["radius"])
            rec.nsides = int(t["nsides"])
            color = t.get("color")
            rec.has_color = 0 if color is None else 1
            rec.color_rgb = 0 if color is None else int(color)
    return arr, tarr, carr, keep


def _stream_field(vectors, origin, spacing, seeds, step, max_steps, direction, min_speed,
                  cfield=None, cmap=None):
    return dict(vectors=np.ascontiguousarray(vectors, np.float32), origin=origin, spacing=spacing,
                seeds=np.ascontiguousarray(seeds, np.float32).reshape(-1, 3), step=step,
                max_steps=max_steps, direction=direction, min_speed=min_speed, cfield=cfield,
                cmap=cmap)


def streamlines_host(vectors, origin, spacing, seeds, step, max_steps,
                     direction=STREAM_FORWARD, min_speed=1e-6):
    """spray_rt_streamlines_host (no GPU): the polylines RtContext.streamlines
    traces -> (points float32 [np, 3], line_offsets uint32 [nseeds + 1],
    line_info uint32 [nseeds, 2])."""
    f = _stream_field(vectors, origin, spacing, seeds, step, max_steps, direction, min_speed)
    arr, _, _, keep = _stream_tables([f])
    L = lib()
    npts = C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_streamlines_host(C.addressof(arr), C.byref(npts), *outs)
        if rc != 0:
            e = SprayRtError("streamlines_host failed (%d)" % rc)
            e.code = rc
            e.counts = npts.value
            raise e

    call(None, None, None)
    ns = int(arr[0].nseeds)
    p = np.zeros((npts.value, 3), np.float32)
    off = np.zeros(ns + 1, np.uint32)
    info = np.zeros((ns, 2), np.uint32)
    call(p.ctypes.data, off.ctypes.data, info.ctypes.data)
    return p, off, info


def stream_tubes_host(vectors, origin, spacing, seeds, step, max_steps, radius, nsides,
                      direction=STREAM_FORWARD, min_speed=1e-6, color=None, cfield=None, cmap=None,
                      normals=True, count_only=False):
    """spray_rt_stream_tubes_host (no GPU): the tube mesh RtContext.stream_tubes
    builds -> (verts float32 [nv, 3], normals float32 [nv, 3] or None, colors
    uint32 [nv], faces uint32 [nf, 3]); count_only: (nv, nf)."""
    f = _stream_field(vectors, origin, spacing, seeds, step, max_steps, direction, min_speed,
                      cfield, cmap)
    arr, tarr, carr, keep = _stream_tables([f], dict(radius=radius, nsides=nsides, color=color))
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_stream_tubes_host(C.addressof(arr), C.addressof(tarr), C.addressof(carr),
                                          C.byref(nv), C.byref(nf), *outs)
        if rc != 0:
            e = SprayRtError("stream_tubes_host failed (%d)" % rc)
            e.code = rc
            e.counts = (nv.value, nf.value)
            raise e

    call(None, None, None, None)
    if count_only:
        return nv.value, nf.value
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals else None
    c = np.zeros(nv.value, np.uint32)
    fc = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, fc.ctypes.data)
    return v, n, c, fc


def tube_ring(nsides):
    """spray_rt_tube_ring_host: the tubes' cross-section table -> float32
    [nsides, 2] of (cos, sin)."""
    out = np.zeros((max(int(nsides), 0), 2), np.float32)
    rc = lib().spray_rt_tube_ring_host(int(nsides), out.ctypes.data)
    if rc != 0:
        e = SprayRtError("tube_ring failed (%d)" % rc)
        e.code = rc
        raise e
    return out


def _block_tables(sets, tubes=None):
    """Dicts with the keys blocks (a list of dicts with vectors float32 [nz, ny,
    nx, 3], origin, spacing and optionally cfield float32 [nz, ny, nx]), seeds
    (float32 [nseeds, 3]), step, max_steps and optionally direction
    (STREAM_FORWARD), min_speed (1e-6) and cmap = (table uint32[n], lo, hi) for
    sets whose blocks have a cfield; arrays are numpy arrays or torch tensors on
    the GPU.  tubes as in _stream_tables -> (spray_rt_blockfield array,
    spray_rt_tube array or None, spray_rt_block_color array, keepalive)."""
    from ._native import BlockColor, BlockField, Tube, VecBlock
    m = max(len(sets), 1)
    arr, carr = (BlockField * m)(), (BlockColor * m)()
    keep = []
    for f, rec, crec in zip(sets, arr, carr):
        blocks = list(f["blocks"])
        barr = (VecBlock * max(len(blocks), 1))()
        keep.append(barr)
        for b, brec in zip(blocks, barr):
            vec = _float_array(b["vectors"], "vectors", (3,))
            if len(vec.shape) != 4:
                raise ValueError("streamlines: vectors are a [nz, ny, nx, 3] array")
            keep.append(vec)
            brec.vectors = _addr(vec)[0]
            nz, ny, nx = (int(d) for d in vec.shape[:3])
            brec.dims = (C.c_int32 * 3)(nx, ny, nz)
            brec.origin = (C.c_float * 3)(*[float(x) for x in b["origin"]])
            brec.spacing = (C.c_float * 3)(*[float(x) for x in b["spacing"]])
            cf = b.get("cfield")
            if cf is not None:
                cf = _float_array(cf, "colour fields", ())
                if tuple(cf.shape) != tuple(vec.shape[:3]):
                    raise ValueError("streamlines: a colour field has its grid's shape")
                keep.append(cf)
                brec.color_field = _addr(cf)[0]
        seeds = _float_array(f["seeds"], "seeds", (3,))
        nseeds = int(np.prod(seeds.shape[:-1])) if len(seeds.shape) > 1 else 1
        keep.append(seeds)
        rec.blocks = C.addressof(barr) if blocks else None
        rec.nblocks = len(blocks)
        rec.seeds = _addr(seeds)[0] if nseeds else None
        rec.nseeds = nseeds
        rec.step = float(f["step"])
        rec.max_steps = int(f["max_steps"])
        rec.direction = int(f.get("direction", STREAM_FORWARD))
        rec.min_speed = float(f.get("min_speed", 1e-6))
        if f.get("cmap") is not None:
            t, crec.table_rgb, crec.ntable, crec.lo, crec.hi = _cmap_args(f["cmap"])
            keep.append(t)
    tarr = None
    if tubes is not None:
        if isinstance(tubes, dict):
            tubes = [tubes] * len(sets)
        if len(tubes) != len(sets):
            raise ValueError("block_stream_tubes: one tube per set")
        tarr = (Tube * m)()
        for t, rec in zip(tubes, tarr):
            rec.radius = float(t["radius"])
            rec.nsides = int(t["nsides"])
            color = t.get("color")
            rec.has_color = 0 if color is None else 1
            rec.color_rgb = 0 if color is None else int(color)
    return arr, tarr, carr, keep


def _block_set(blocks, seeds, step, max_steps, direction, min_speed, cmap=None):
    bl = [dict(b, vectors=np.ascontiguousarray(b["vectors"], np.float32)) for b in blocks]
    return dict(blocks=bl, seeds=np.ascontiguousarray(seeds, np.float32).reshape(-1, 3),
                step=step, max_steps=max_steps, direction=direction, min_speed=min_speed,
                cmap=cmap)


def block_streamlines_host(blocks, seeds, step, max_steps, direction=STREAM_FORWARD,
                           min_speed=1e-6):
    """spray_rt_block_streamlines_host (no GPU): the polylines
    RtContext.block_streamlines traces through a set of blocks (see
    _block_tables) -> (points float32 [np, 3], line_offsets uint32 [nseeds + 1],
    line_info uint32 [nseeds, 2], point_blocks uint32 [np])."""
    f = _block_set(blocks, seeds, step, max_steps, direction, min_speed)
    arr, _, _, keep = _block_tables([f])
    L = lib()
    npts = C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_block_streamlines_host(C.addressof(arr), C.byref(npts), *outs)
        if rc != 0:
            e = SprayRtError("block_streamlines_host failed (%d)" % rc)
            e.code = rc
            e.counts = npts.value
            raise e

    call(None, None, None, None)
    ns = int(arr[0].nseeds)
    p = np.zeros((npts.value, 3), np.float32)
    off = np.zeros(ns + 1, np.uint32)
    info = np.zeros((ns, 2), np.uint32)
    blk = np.zeros(npts.value, np.uint32)
    call(p.ctypes.data, off.ctypes.data, info.ctypes.data, blk.ctypes.data)
    return p, off, info, blk


def block_stream_tubes_host(blocks, seeds, step, max_steps, radius, nsides,
                            direction=STREAM_FORWARD, min_speed=1e-6, color=None, cmap=None,
                            normals=True, count_only=False):
    """spray_rt_block_stream_tubes_host (no GPU): the tube mesh
    RtContext.block_stream_tubes builds, as stream_tubes_host."""
    f = _block_set(blocks, seeds, step, max_steps, direction, min_speed, cmap)
    arr, tarr, carr, keep = _block_tables([f], dict(radius=radius, nsides=nsides, color=color))
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_block_stream_tubes_host(C.addressof(arr), C.addressof(tarr),
                                                C.addressof(carr), C.byref(nv), C.byref(nf),
                                                *outs)
        if rc != 0:
            e = SprayRtError("block_stream_tubes_host failed (%d)" % rc)
            e.code = rc
            e.counts = (nv.value, nf.value)
            raise e

    call(None, None, None, None)
    if count_only:
        return nv.value, nf.value
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals else None
    c = np.zeros(nv.value, np.uint32)
    fc = np.zeros((nf.value, 3), np.uint32)
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, fc.ctypes.data)
    return v, n, c, fc


GLYPH_SPHERE, GLYPH_ARROW = 0, 1


def _glyph_array(x, what, tail, n=None):
    """A float32 numpy array or GPU tensor of shape [n, *tail]."""
    if hasattr(x, "data_ptr"):
        if x.element_size() != 4 or not x.is_floating_point():
            raise TypeError("glyphs: %s are float32" % what)
    else:
        x = np.ascontiguousarray(x, np.float32)
    shape = tuple(int(d) for d in x.shape)
    if len(shape) != 1 + len(tail) or shape[1:] != tuple(tail) or (n is not None and shape[0] != n):
        raise ValueError("glyphs: %s are a [npoints%s] array"
                         % (what, "".join(", %d" % t for t in tail)))
    return x


def _glyph_tables(sets, glyphs):
    """sets: dicts with the key points (float32 [npoints, 3]) and optionally
    vectors (float32 [npoints, 3]), scales, select (float32 [npoints]),
    select_range = (lo, hi), stride (1), cfield (float32 [npoints]) and cmap =
    (table uint32[n], lo, hi); arrays are numpy arrays or torch tensors on the
    GPU.  glyphs: dicts with shape (GLYPH_SPHERE / GLYPH_ARROW), size and
    optionally level (1), nsides (8), scale_by_vector (False), min_speed (1e-6),
    color, one per set or one for all -> (spray_rt_pointset array,
    spray_rt_glyph array, spray_rt_grid_color array, keepalive)."""
    from ._native import Glyph, PointSet
    if isinstance(glyphs, dict):
        glyphs = [glyphs] * len(sets)
    if len(glyphs) != len(sets):
        raise ValueError("glyphs: one glyph per set")
    m = max(len(sets), 1)
    arr, garr, carr = (PointSet * m)(), (Glyph * m)(), (_GridColor * m)()
    keep = []
    for S, rec, crec in zip(sets, arr, carr):
        pts = _glyph_array(S["points"], "points", (3,))
        n = int(pts.shape[0])
        keep.append(pts)
        rec.points = _addr(pts)[0] if n else None
        rec.npoints = n
        for key, tail in (("vectors", (3,)), ("scales", ()), ("select", ())):
            x = S.get(key)
            if x is not None:
                x = _glyph_array(x, key, tail, n)
                keep.append(x)
                setattr(rec, key, _addr(x)[0] if n else None)
        lo, hi = S.get("select_range", (0.0, 0.0))
        rec.select_lo, rec.select_hi = float(lo), float(hi)
        rec.stride = int(S.get("stride", 1))
        cf = S.get("cfield")
        if cf is not None:
            cf = _glyph_array(cf, "colour fields", (), n)
            keep.append(cf)
            crec.field = _addr(cf)[0] if n else None
            if n and S.get("cmap") is not None:
                t, crec.table_rgb, crec.ntable, crec.lo, crec.hi = _cmap_args(S["cmap"])
                keep.append(t)
    for G, rec in zip(glyphs, garr):
        rec.shape = int(G["shape"])
        rec.size = float(G["size"])
        rec.level = int(G.get("level", 1))
        rec.nsides = int(G.get("nsides", 8))
        rec.scale_by_vector = 1 if G.get("scale_by_vector") else 0
        rec.min_speed = float(G.get("min_speed", 1e-6))
        color = G.get("color")
        rec.has_color = 0 if color is None else 1
        rec.color_rgb = 0 if color is None else int(color)
    return arr, garr, carr, keep


def _glyph_counts(arr, garr, i, nv):
    """Glyphs of set i from its vertex count."""
    g = garr[i]
    V = 10 * 4 ** g.level + 2 if g.shape == GLYPH_SPHERE else 4 * g.nsides + 1
    return nv // V


def glyphs_host(pointset, glyph, normals=True, count_only=False, point_ids=True):
    """spray_rt_glyphs_host (no GPU): the glyph mesh RtContext.glyphs builds of
    one set (see _glyph_tables) -> (verts float32 [nv, 3], normals float32
    [nv, 3] or None, colors uint32 [nv], faces uint32 [nf, 3], point_ids uint32
    [nglyphs] or None); count_only: (nv, nf)."""
    arr, garr, carr, keep = _glyph_tables([pointset], [glyph])
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()

    def call(*outs):
        rc = L.spray_rt_glyphs_host(C.addressof(arr), C.addressof(garr), C.addressof(carr),
                                    C.byref(nv), C.byref(nf), *outs)
        if rc != 0:
            e = SprayRtError("glyphs_host failed (%d)" % rc)
            e.code = rc
            e.counts = (nv.value, nf.value)
            raise e

    call(None, None, None, None, None)
    if count_only:
        return nv.value, nf.value
    v = np.zeros((nv.value, 3), np.float32)
    n = np.zeros((nv.value, 3), np.float32) if normals else None
    c = np.zeros(nv.value, np.uint32)
    fc = np.zeros((nf.value, 3), np.uint32)
    ids = np.zeros(_glyph_counts(arr, garr, 0, nv.value), np.uint32) if point_ids else None
    call(v.ctypes.data, None if n is None else n.ctypes.data, c.ctypes.data, fc.ctypes.data,
         None if ids is None else ids.ctypes.data)
    return v, n, c, fc, ids


def glyph_sphere(level):
    """spray_rt_glyph_sphere_host: the unit icosphere table of the sphere
    glyphs -> (verts float32 [V, 3], faces uint32 [F, 3])."""
    L = lib()
    nv, nf = C.c_size_t(), C.c_size_t()
    rc = L.spray_rt_glyph_sphere_host(int(level), C.byref(nv), C.byref(nf), None, None)
    if rc == 0:
        v = np.zeros((nv.value, 3), np.float32)
        f = np.zeros((nf.value, 3), np.uint32)
        rc = L.spray_rt_glyph_sphere_host(int(level), None, None, v.ctypes.data, f.ctypes.data)
    if rc != 0:
        e = SprayRtError("glyph_sphere failed (%d)" % rc)
        e.code = rc
        raise e
    return v, f


def host_parse_scene(desc, ply_path=""):
    """Scene file -> (boxes [n,6], lights [nl,7]) without touching the GPU
    (spray_host_parse_scene)."""
    nd, nl = C.c_int(), C.c_int()
    err = C.create_string_buffer(1024)
    if lib().spray_host_parse_scene(desc.encode(), (ply_path or "").encode(), C.byref(nd),
                                    C.byref(nl), None, None, None, err, 1024) != 0:
        raise SprayRtError("parse %s: %s" % (desc, err.value.decode()))
    boxes = np.zeros((nd.value, 6), np.float32)
    xf = np.zeros((nd.value, 16), np.float32)
    lights = np.zeros((nl.value, 7), np.float32)
    if lib().spray_host_parse_scene(desc.encode(), (ply_path or "").encode(), C.byref(nd),
                                    C.byref(nl), boxes.ctypes.data, xf.ctypes.data,
                                    lights.ctypes.data, err, 1024) != 0:
        raise SprayRtError("parse %s: %s" % (desc, err.value.decode()))
    return boxes, lights


def host_scene_bsdfs(desc):
    """Scene file -> [(type, p0, p1, p2)] per domain (SceneLoader::parseMaterial)."""
    nd = C.c_int()
    err = C.create_string_buffer(1024)
    L = lib()
    if L.spray_host_scene_bsdfs(desc.encode(), C.byref(nd), None, err, 1024) != 0:
        raise SprayRtError("parse %s: %s" % (desc, err.value.decode()))
    arr = (BsdfRec * max(nd.value, 1))()
    if L.spray_host_scene_bsdfs(desc.encode(), C.byref(nd), C.addressof(arr), err, 1024) != 0:
        raise SprayRtError("materials of %s: %s" % (desc, err.value.decode()))
    return [(arr[i].type, arr[i].p[0], arr[i].p[1], arr[i].p[2]) for i in range(nd.value)]


def host_domain_mesh(desc, ply_path, domain_id):
    """TriMeshBuffer::load of one domain on the host -> (verts, faces,
    colors, normals)."""
    nv, nf = C.c_size_t(), C.c_size_t()
    L = lib()
    if L.spray_host_domain_mesh(desc.encode(), (ply_path or "").encode(), int(domain_id),
                                C.byref(nv), C.byref(nf), None, None, None, None) != 0:
        raise SprayRtError("domain %d of %s failed to load" % (domain_id, desc))
    v = np.zeros((nv.value, 3), np.float32)
    f = np.zeros((nf.value, 3), np.uint32)
    c = np.zeros(nv.value, np.uint32)
    n = np.zeros((nv.value, 3), np.float32)
    if L.spray_host_domain_mesh(desc.encode(), (ply_path or "").encode(), int(domain_id),
                                C.byref(nv), C.byref(nf), v.ctypes.data, f.ctypes.data,
                                c.ctypes.data, n.ctypes.data) != 0:
        raise SprayRtError("domain %d of %s failed to load" % (domain_id, desc))
    return v, f, c, n


class RtContext:
    """One engine context (one GPU).  ``owner=False`` wraps a context owned
    by a Scene."""

    def __init__(self, device=0, handle=None):
        self._own = handle is None
        if handle is None:
            h = C.c_void_p()
            rc = lib().spray_rt_create(int(device), C.byref(h))
            if rc != 0:
                raise SprayRtError("spray_rt_create(%d) failed: %d" % (device, rc))
            handle = h.value
        self.h = handle
        self._device = int(device)
        self._nverts = {}  # slot -> vertices of its last upload_domain (refit argument checks)
        self._children = []  # engines / caches created on this context: closed before it

    def _adopt(self, child):
        """Objects whose native handle points into this context (InsituEngine,
        OocCache) register here: the context must outlive them, also when the
        garbage collector finalizes an unreachable group in any order -- their
        destroy calls read the context (its device, its stream)."""
        self._children.append(child)

    def _release(self, child):
        kids = getattr(self, "_children", None)
        if kids and child in kids:
            kids.remove(child)

    def close(self):
        for child in list(getattr(self, "_children", ())):
            child.close()
        if getattr(self, "h", None) and self._own:
            lib().spray_rt_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().spray_rt_last_error(self.h)
            e = SprayRtError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))
            e.code = rc
            raise e

    # ---- context ----
    def set_stream(self, stream):
        """stream: torch.cuda.Stream, raw hipStream_t int, or None."""
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        self._check(lib().spray_rt_set_stream(self.h, stream), "set_stream")

    def sync(self):
        self._check(lib().spray_rt_sync(self.h), "sync")

    RAYS_ADAPTIVE, RAYS_COHERENT, RAYS_INCOHERENT = 0, 1, 2

    def set_coherence(self, mode):
        """Traversal form of the any-hit launches (results are identical)."""
        self._check(lib().spray_rt_set_coherence(self.h, int(mode)), "set_coherence")

    def scene_launch_info(self):
        """What the launcher decided for the last scene launch of the process
        (not of this context; not thread-safe; for tests): dict(persist, grid,
        chunk, W, STK, TRAV, ANY, EPI) -- spray_rt_scene_launch_info."""
        out = (C.c_int * 8)()
        self._check(lib().spray_rt_scene_launch_info(self.h, out), "scene_launch_info")
        return dict(zip(("persist", "grid", "chunk", "W", "STK", "TRAV", "ANY", "EPI"),
                        (int(x) for x in out)))

    # ---- domains ----
    def upload_domain(self, slot, verts, faces, colors=None, normals=None, async_=False):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        c = None if colors is None else np.ascontiguousarray(colors, np.uint32)
        n = None if normals is None else np.ascontiguousarray(normals, np.float32)
        self._check(lib().spray_rt_domain_upload(
            self.h, int(slot), v.ctypes.data, len(v), f.ctypes.data, len(f),
            None if c is None else c.ctypes.data, None if n is None else n.ctypes.data,
            1 if async_ else 0), "domain_upload")
        self._nverts[int(slot)] = len(v)

    def release_domain(self, slot):
        self._check(lib().spray_rt_domain_release(self.h, int(slot)), "domain_release")
        self._nverts.pop(int(slot), None)

    # ---- moving geometry ----
    SLOT_NODES, SLOT_TRIS, SLOT_PRIMS, SLOT_QNODES4, SLOT_QGRID, SLOT_NORMALS = range(6)
    SLOT_COLORS, SLOT_FACES = SLOT_COLORS, SLOT_FACES
    _SLOT_DTYPES = (np.uint8, np.float32, np.uint32, np.uint8, np.float32, np.float32,
                    np.uint32, np.uint32)

    def _bounds_out(self, bounds, n):
        """Where a batched slot call writes its [n, 6] boxes: a new GPU tensor
        (bounds True), the caller's tensor, or nowhere."""
        if bounds is True:
            import torch
            return torch.empty((max(n, 1), 6), dtype=torch.float32,
                               device="cuda:%d" % self._device)
        return None if bounds is False else bounds

    def refit_domains(self, slots, verts, normals=None, bounds=False):
        """spray_rt_domains_refit: new vertex positions (and normals, for
        slots uploaded with them) for resident slots of unchanged topology.
        verts[i] / normals[i]: float32 [nverts, 3] numpy arrays (staged; the
        call is synchronous) or torch tensors on the GPU (enqueued).  bounds:
        True returns the slots' new exact boxes as a numpy [n, 6] array
        (synchronises); a float32 [n, 6] GPU tensor is filled in place."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(verts) != n or (normals is not None and len(normals) != n):
            e = SprayRtError("refit_domains: %d slots, %d vertex arrays, %s normal arrays"
                             % (n, len(verts), "no" if normals is None else len(normals)))
            e.code = -1
            raise e
        keep = []

        def pointer(x, slot, what):
            if x is None:
                return None
            if not hasattr(x, "data_ptr"):
                x = np.ascontiguousarray(x, np.float32)
            want = self._nverts.get(slot)
            if want is not None and _nbytes(x) != 12 * want:
                e = SprayRtError("refit_domains: %s of slot %d hold %d bytes, its %d vertices "
                                 "need %d" % (what, slot, _nbytes(x), want, 12 * want))
                e.code = -1
                raise e
            a, k = _addr(x)
            keep.append(k)
            return a

        vp = (C.c_void_p * max(n, 1))(*[pointer(v, s, "vertices") for v, s in zip(verts, slots)])
        npp = None
        if normals is not None:
            npp = (C.c_void_p * max(n, 1))(*[pointer(x, s, "normals")
                                             for x, s in zip(normals, slots)])
        sl = (C.c_int * max(n, 1))(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        self._check(lib().spray_rt_domains_refit(self.h, n, sl, vp, npp, b), "domains_refit")
        if bounds is True:
            self.sync()
            return out[:n].cpu().numpy()
        return out

    def build_domains(self, slots, verts, faces, colors=None, normals=None, bounds=None):
        """spray_rt_domains_build: new triangle lists into slots (empty or
        loaded), the trees built on the device in one batched call.  verts[i]
        float32 [nv, 3], faces[i] uint32 [nf, 3], colors[i] uint32 [nv],
        normals[i] float32 [nv, 3] (the lists, or single entries, may be None):
        numpy arrays (staged; the call is synchronous) or torch tensors on the
        GPU (enqueued).  bounds as in refit_domains."""
        slots = [int(s) for s in slots]
        n = len(slots)
        for name, arr in (("vertex", verts), ("face", faces), ("color", colors),
                          ("normal", normals)):
            if (arr is None and name in ("vertex", "face")) or (arr is not None and len(arr) != n):
                e = SprayRtError("build_domains: %d slots, %s %s arrays"
                                 % (n, "no" if arr is None else len(arr), name))
                e.code = -1
                raise e
        keep = []

        def pointer(x, dtype):
            if x is None:
                return None
            if not hasattr(x, "data_ptr"):
                x = np.ascontiguousarray(x, dtype)
            elif x.element_size() != 4:
                raise TypeError("build_domains: tensors hold 32-bit elements")
            a, k = _addr(x)
            keep.append(k)
            return a

        def count(x, per):
            if hasattr(x, "data_ptr"):
                return x.numel() // per
            return np.asarray(x).size // per

        nv = [count(v, 3) for v in verts]
        nf = [count(f, 3) for f in faces]
        for i in range(n):
            for name, arr, per in (("colors", colors, 1), ("normals", normals, 3)):
                if arr is not None and arr[i] is not None and count(arr[i], per) != nv[i]:
                    e = SprayRtError("build_domains: %s of slot %d do not match its %d vertices"
                                     % (name, slots[i], nv[i]))
                    e.code = -1
                    raise e
        m = max(n, 1)
        vp = (C.c_void_p * m)(*[pointer(x, np.float32) for x in verts])
        fp = (C.c_void_p * m)(*[pointer(x, np.uint32) for x in faces])
        cp = None if colors is None else (C.c_void_p * m)(*[pointer(x, np.uint32) for x in colors])
        npp = None if normals is None else (C.c_void_p * m)(*[pointer(x, np.float32)
                                                               for x in normals])
        sl = (C.c_int * m)(*slots)
        nvp, nfp = (C.c_size_t * m)(*nv), (C.c_size_t * m)(*nf)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        self._check(lib().spray_rt_domains_build(self.h, n, sl, vp, nvp, fp, nfp, cp, npp, b),
                    "domains_build")
        for s, k in zip(slots, nv):
            self._nverts[s] = k
        if bounds is True:
            self.sync()
            return out[:n].cpu().numpy()
        return out

    # ---- isosurfaces ----
    def isosurface(self, grids, normals=True, capacity=None):
        """spray_rt_isosurface: the isosurfaces of grids (see _grid_table) in one
        batched call -> [(verts float32 [nv, 3], normals float32 [nv, 3] or
        None, faces int32 [nf, 3] holding the uint32 bits)] as GPU tensors of
        the exact sizes (a counting call first).  capacity=(nverts, nfaces)
        skips the counting call and extracts into buffers of that size per
        grid (SPRAY_RT_ERR_LIMIT if one is too small)."""
        import torch
        n = len(grids)
        arr, keep = _grid_table(grids)
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        if capacity is None:
            self._check(lib().spray_rt_isosurface(self.h, n, arr, None, None, None, None, None,
                                                  nv, nf), "isosurface")
            caps = [(nv[i], nf[i]) for i in range(n)]
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        v = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) for cv, _ in caps]
        nr = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) if normals else None
              for cv, _ in caps]
        f = [torch.zeros((max(cf, 1), 3), dtype=torch.int32, device=dev) for _, cf in caps]
        ptrs = lambda xs: (C.c_void_p * m)(*[None if x is None else x.data_ptr() for x in xs])
        try:
            self._check(lib().spray_rt_isosurface(
                self.h, n, arr, ptrs(v), ptrs(nr) if normals else None, ptrs(f),
                (C.c_size_t * m)(*[c[0] for c in caps]), (C.c_size_t * m)(*[c[1] for c in caps]),
                nv, nf), "isosurface")
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i]) for i in range(n)]
            e.buffers = (v, nr, f)
            raise
        return [(v[i][:nv[i]], nr[i][:nv[i]] if normals else None, f[i][:nf[i]])
                for i in range(n)]

    def isosurface_domains(self, slots, grids, normals=True, bounds=None):
        """spray_rt_domains_isosurface: the isosurfaces of grids (see
        _grid_table; a grid's optional colour is every vertex's) into slots
        (empty or loaded), extracted and built on the device.  bounds as in
        refit_domains; slot_info(slot)["tris"] has the triangle counts."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(grids) != n:
            e = SprayRtError("isosurface_domains: %d slots, %d grids" % (n, len(grids)))
            e.code = -1
            raise e
        arr, keep = _grid_table(grids)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(lib().spray_rt_domains_isosurface(self.h, n, sl, arr, 1 if normals else 0, b,
                                                      nf), "domains_isosurface")
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the extraction's
        if bounds is True:
            self.sync()
            return out[:n].cpu().numpy()
        return out

    # ---- colour maps ----
    def isosurface_mapped(self, grids, normals=True, capacity=None, colors_only=False):
        """spray_rt_isosurface_mapped: isosurface() with per-vertex colours,
        mapped from a grid's "cfield" through its "cmap" (see
        _grid_color_table) or its constant colour -> [(verts, normals or None,
        colors int32 [nv] holding the 0x00RRGGBB bits, faces)] as GPU tensors.
        colors_only: the colours alone (the other entries are None), without
        the position, normal and face work -- what recolor_domains takes.
        Enqueued on the context's stream: sync() before reading the tensors on
        another stream."""
        import torch
        n = len(grids)
        arr, keep = _grid_table(grids)
        carr, ckeep = _grid_color_table(grids)
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        L = lib()
        if capacity is None:
            self._check(L.spray_rt_isosurface_mapped(self.h, n, arr, carr, None, None, None, None,
                                                     None, None, nv, nf), "isosurface_mapped")
            caps = [(nv[i], nf[i]) for i in range(n)]
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        full = not colors_only
        # zeroed, one element at least: a buffer a failed call must not touch
        v = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) if full else None
             for cv, _ in caps]
        nr = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev)
              if full and normals else None for cv, _ in caps]
        col = [torch.zeros(max(cv, 1), dtype=torch.int32, device=dev) for cv, _ in caps]
        f = [torch.zeros((max(cf, 1), 3), dtype=torch.int32, device=dev) if full else None
             for _, cf in caps]

        def ptrs(xs):
            if all(x is None for x in xs):
                return None
            return (C.c_void_p * m)(*[None if x is None else x.data_ptr() for x in xs])

        _fills_done()
        try:
            self._check(L.spray_rt_isosurface_mapped(
                self.h, n, arr, carr, ptrs(v), ptrs(nr), ptrs(col), ptrs(f),
                (C.c_size_t * m)(*[c[0] for c in caps]),
                (C.c_size_t * m)(*[c[1] for c in caps]) if full else None, nv, nf),
                "isosurface_mapped")
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i]) for i in range(n)]
            e.buffers = tuple(b for b in (v, nr, col, f) if b[0] is not None) if n else ()
            raise
        cut = lambda x, k: None if x is None else x[:k]
        return [(cut(v[i], nv[i]), cut(nr[i], nv[i]), col[i][:nv[i]], cut(f[i], nf[i]))
                for i in range(n)]

    def isosurface_domains_mapped(self, slots, grids, normals=True, bounds=None):
        """spray_rt_domains_isosurface_mapped: isosurface_domains() with the
        colours of isosurface_mapped()."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(grids) != n:
            e = SprayRtError("isosurface_domains_mapped: %d slots, %d grids" % (n, len(grids)))
            e.code = -1
            raise e
        arr, keep = _grid_table(grids)
        carr, ckeep = _grid_color_table(grids)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(lib().spray_rt_domains_isosurface_mapped(
            self.h, n, sl, arr, carr, 1 if normals else 0, b, nf), "domains_isosurface_mapped")
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the extraction's
        if bounds is True:
            self.sync()
            return out[:n].cpu().numpy()
        return out

    def recolor_domains(self, slots, colors):
        """spray_rt_domains_recolor: new per-vertex colours for resident slots
        that carry colours.  colors[i]: uint32 [nverts] numpy arrays (staged; the
        call is synchronous) or 32-bit torch tensors on the GPU (enqueued)."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(colors) != n:
            e = SprayRtError("recolor_domains: %d slots, %d colour arrays" % (n, len(colors)))
            e.code = -1
            raise e
        keep, ptr, cnt = [], [], []
        for x in colors:
            if x is None:
                ptr.append(None)
                cnt.append(0)
                continue
            if not hasattr(x, "data_ptr"):
                x = np.ascontiguousarray(x, np.uint32)
                cnt.append(x.size)
            elif x.element_size() != 4:
                raise TypeError("recolor_domains: tensors hold 32-bit elements")
            else:
                cnt.append(x.numel())
            a, k = _addr(x)
            keep.append(k)
            ptr.append(a)
        m = max(n, 1)
        self._check(lib().spray_rt_domains_recolor(self.h, n, (C.c_int * m)(*slots),
                                                   (C.c_void_p * m)(*ptr), (C.c_size_t * m)(*cnt)),
                    "domains_recolor")

    def colormap_apply(self, scalars, cmap, out=None):
        """spray_rt_colormap_apply: cmap = (table uint32[n], lo, hi) over
        scalars (float32, numpy or a GPU tensor) -> int32 GPU tensor holding the
        0x00RRGGBB bits (out, if given: a 32-bit GPU tensor of that many
        elements).  Synchronises."""
        import torch
        if hasattr(scalars, "data_ptr"):
            if scalars.element_size() != 4 or not scalars.is_floating_point():
                raise TypeError("colormap_apply: scalars are float32")
            count = scalars.numel()
        else:
            scalars = np.ascontiguousarray(scalars, np.float32)
            count = scalars.size
        if out is None:
            out = torch.zeros(count, dtype=torch.int32, device="cuda:%d" % self._device)
            _fills_done()
        elif out.numel() != count or out.element_size() != 4:
            raise ValueError("colormap_apply: out holds one 32-bit element per scalar")
        t, ta, nt, lo, hi = _cmap_args(cmap)
        a, k = _addr(scalars)
        o, ko = _addr(out)
        self._check(lib().spray_rt_colormap_apply(self.h, a, count, ta, nt, lo, hi, o),
                    "colormap_apply")
        return out

    # ---- isosurfaces of tetrahedral meshes ----
    def tet_isosurface(self, meshes, normals=True, capacity=None, count_only=False):
        """spray_rt_tet_isosurface: the isosurfaces of tetrahedral meshes (see
        _tet_table) in one batched call -> [(verts float32 [nv, 3], normals
        float32 [nv, 3] or None (normals False, or a mesh without them), colors
        int32 [nv] holding the 0x00RRGGBB bits, faces int32 [nf, 3] holding the
        uint32 bits)] as GPU tensors of the exact sizes (a counting call
        first).  capacity=(nverts, nfaces) skips the counting call and extracts
        into buffers of that size per mesh (SPRAY_RT_ERR_LIMIT if one is too
        small).  count_only: [(nverts, nfaces)] alone.  Enqueued on the
        context's stream: sync() before reading the tensors on another stream."""
        return self._mesh_isosurface(lib().spray_rt_tet_isosurface, "tet_isosurface",
                                     _tet_table(meshes), meshes, normals, capacity, count_only)

    def _mesh_isosurface(self, fn, what, table, meshes, normals, capacity, count_only):
        """The body of tet_isosurface / cell_isosurface: fn the C entry point,
        table the (mesh array, colour array, keepalive) of meshes."""
        import torch
        n = len(meshes)
        arr, carr, keep = table
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, carr, None, None, None, None, None, None, nv, nf),
                        what)
            caps = [(nv[i], nf[i]) for i in range(n)]
            if count_only:
                return caps
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        v = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) for cv, _ in caps]
        nr = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev)
              if normals and meshes[i].get("normals") is not None else None
              for i, (cv, _) in enumerate(caps)]
        col = [torch.zeros(max(cv, 1), dtype=torch.int32, device=dev) for cv, _ in caps]
        f = [torch.zeros((max(cf, 1), 3), dtype=torch.int32, device=dev) for _, cf in caps]

        def ptrs(xs):
            if all(x is None for x in xs):
                return None
            return (C.c_void_p * m)(*[None if x is None else x.data_ptr() for x in xs])

        _fills_done()
        try:
            self._check(fn(
                self.h, n, arr, carr, ptrs(v), ptrs(nr), ptrs(col), ptrs(f),
                (C.c_size_t * m)(*[c[0] for c in caps]), (C.c_size_t * m)(*[c[1] for c in caps]),
                nv, nf), what)
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i]) for i in range(n)]
            e.buffers = (v, [x for x in nr if x is not None], col, f)
            raise
        cut = lambda x, k: None if x is None else x[:k]
        return [(v[i][:nv[i]], cut(nr[i], nv[i]), col[i][:nv[i]], f[i][:nf[i]])
                for i in range(n)]

    def tet_isosurface_domains(self, slots, meshes, normals=True, bounds=None):
        """spray_rt_domains_tet_isosurface: the isosurfaces of tetrahedral meshes
        (see _tet_table) into slots (empty or loaded), extracted and built on
        the device; a slot carries normals where normals and its mesh has them,
        colours where its mesh is mapped or has a colour.  bounds as in
        refit_domains; slot_info(slot)["tris"] has the triangle counts."""
        return self._mesh_isosurface_domains(lib().spray_rt_domains_tet_isosurface,
                                             "tet_isosurface_domains", "domains_tet_isosurface",
                                             _tet_table, slots, meshes, normals, bounds)

    def _mesh_isosurface_domains(self, fn, name, what, table_of, slots, meshes, normals, bounds):
        """The body of tet_isosurface_domains / cell_isosurface_domains."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(meshes) != n:
            e = SprayRtError("%s: %d slots, %d meshes" % (name, n, len(meshes)))
            e.code = -1
            raise e
        arr, carr, keep = table_of(meshes)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(fn(self.h, n, sl, arr, carr, 1 if normals else 0, b, nf), what)
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the extraction's
        if bounds is True:
            self.sync()
            return out[:n].cpu().numpy()
        return out

    def tet_phase_times(self, on=None):
        """spray_rt_tet_phase_times of the last tet extraction -> [ms to host
        read 1, to host read 2, to the end of the enqueue, the sort's device
        time]; on (True / False) first switches the sort's timing."""
        if on is not None:
            self._check(lib().spray_rt_tet_set_timing(self.h, 1 if on else 0), "tet_set_timing")
        out = (C.c_double * 4)()
        self._check(lib().spray_rt_tet_phase_times(self.h, out), "tet_phase_times")
        return list(out)

    # ---- isosurfaces of hexahedral, wedge, pyramid and tet cells ----
    def cell_isosurface(self, meshes, normals=True, capacity=None, count_only=False):
        """spray_rt_cell_isosurface: tet_isosurface for meshes of mixed cells
        (see _cell_table), with its arguments and results."""
        return self._mesh_isosurface(lib().spray_rt_cell_isosurface, "cell_isosurface",
                                     _cell_table(meshes), meshes, normals, capacity, count_only)

    def cell_isosurface_domains(self, slots, meshes, normals=True, bounds=None):
        """spray_rt_domains_cell_isosurface: tet_isosurface_domains for meshes of
        mixed cells (see _cell_table)."""
        return self._mesh_isosurface_domains(lib().spray_rt_domains_cell_isosurface,
                                             "cell_isosurface_domains", "domains_cell_isosurface",
                                             _cell_table, slots, meshes, normals, bounds)

    def cell_phase_times(self):
        """spray_rt_cell_phase_times of the last cell extraction -> [ms to the
        cell pass's host read, then tet_phase_times' four from there on]."""
        out = (C.c_double * 5)()
        self._check(lib().spray_rt_cell_phase_times(self.h, out), "cell_phase_times")
        return list(out)

    # ---- boundary surfaces and thresholds of cell meshes ----
    def cell_surface(self, meshes, selects=None, normals=True, capacity=None, count_only=False):
        """spray_rt_cell_surface: the boundary surfaces of the cells the selects
        keep (see _surf_table) in one batched call -> [(verts float32 [nv, 3],
        normals float32 [nv, 3] or None (normals False, or a mesh without them),
        colors int32 [nv] holding the 0x00RRGGBB bits, point_ids int32 [nv],
        faces int32 [nf, 3] holding the uint32 bits)] as GPU tensors of the
        exact sizes (a counting call first).  capacity and count_only as in
        tet_isosurface.  Enqueued on the context's stream."""
        import torch
        fn = lib().spray_rt_cell_surface
        n = len(meshes)
        arr, sarr, carr, keep = _surf_table(meshes, selects)
        sel = None if selects is None else sarr
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, sel, carr, None, None, None, None, None, None, None,
                           nv, nf), "cell_surface")
            caps = [(nv[i], nf[i]) for i in range(n)]
            if count_only:
                return caps
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        v = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) for cv, _ in caps]
        nr = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev)
              if normals and meshes[i].get("normals") is not None else None
              for i, (cv, _) in enumerate(caps)]
        col = [torch.zeros(max(cv, 1), dtype=torch.int32, device=dev) for cv, _ in caps]
        ids = [torch.zeros(max(cv, 1), dtype=torch.int32, device=dev) for cv, _ in caps]
        f = [torch.zeros((max(cf, 1), 3), dtype=torch.int32, device=dev) for _, cf in caps]

        def ptrs(xs):
            if all(x is None for x in xs):
                return None
            return (C.c_void_p * m)(*[None if x is None else x.data_ptr() for x in xs])

        _fills_done()
        try:
            self._check(fn(
                self.h, n, arr, sel, carr, ptrs(v), ptrs(nr), ptrs(col), ptrs(ids), ptrs(f),
                (C.c_size_t * m)(*[c[0] for c in caps]), (C.c_size_t * m)(*[c[1] for c in caps]),
                nv, nf), "cell_surface")
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i]) for i in range(n)]
            e.buffers = (v, [x for x in nr if x is not None], col, ids, f)
            raise
        cut = lambda x, k: None if x is None else x[:k]
        return [(v[i][:nv[i]], cut(nr[i], nv[i]), col[i][:nv[i]], ids[i][:nv[i]], f[i][:nf[i]])
                for i in range(n)]

    def cell_surface_domains(self, slots, meshes, selects=None, normals=True, bounds=None):
        """spray_rt_domains_cell_surface: the boundary surfaces of the cells the
        selects keep (see _surf_table) into slots (empty or loaded), extracted
        and built on the device; normals, colours and bounds as in
        tet_isosurface_domains."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(meshes) != n:
            e = SprayRtError("cell_surface_domains: %d slots, %d meshes" % (n, len(meshes)))
            e.code = -1
            raise e
        arr, sarr, carr, keep = _surf_table(meshes, selects)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(lib().spray_rt_domains_cell_surface(
            self.h, n, sl, arr, None if selects is None else sarr, carr, 1 if normals else 0, b,
            nf), "domains_cell_surface")
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the extraction's
        if bounds is True:
            self.sync()
            return out[:n].cpu().numpy()
        return out

    def cell_surface_phase_times(self, on=None):
        """spray_rt_cell_surface_phase_times of the last surface extraction, as
        tet_phase_times (on switches the same sort timing)."""
        if on is not None:
            self._check(lib().spray_rt_tet_set_timing(self.h, 1 if on else 0), "tet_set_timing")
        out = (C.c_double * 4)()
        self._check(lib().spray_rt_cell_surface_phase_times(self.h, out),
                    "cell_surface_phase_times")
        return list(out)

    # ---- clips of cell meshes ----
    def cell_clip(self, meshes, invert=None, normals=True, capacity=None, count_only=False):
        """spray_rt_cell_clip: the surfaces of the parts of meshes of mixed cells
        (see _cell_table) with values >= iso (invert, one flag or one per mesh:
        the other part) in one batched call -> [(verts float32 [nv, 3], normals
        float32 [nv, 3] or None (normals False, or a mesh without them), colors
        int32 [nv] holding the 0x00RRGGBB bits, vert_pairs int32 [nv, 2],
        vert_t float32 [nv], faces int32 [nf, 3] holding the uint32 bits,
        ncap_verts, ncap_faces)] as GPU tensors of the exact sizes (a counting
        call first); the cap's vertices and faces come first.  capacity=(nverts,
        nfaces) and count_only ([(nverts, nfaces, ncap_verts, ncap_faces)]) as
        in tet_isosurface.  Enqueued on the context's stream."""
        import torch
        fn = lib().spray_rt_cell_clip
        n = len(meshes)
        arr, carr, keep = _cell_table(meshes)
        inv = _invert_arg(invert, n)
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        ncv, ncf = (C.c_size_t * m)(), (C.c_size_t * m)()
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, inv, carr, None, None, None, None, None, None, None,
                           None, nv, nf, ncv, ncf), "cell_clip")
            caps = [(nv[i], nf[i]) for i in range(n)]
            if count_only:
                return [(nv[i], nf[i], ncv[i], ncf[i]) for i in range(n)]
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        v = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) for cv, _ in caps]
        nr = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev)
              if normals and meshes[i].get("normals") is not None else None
              for i, (cv, _) in enumerate(caps)]
        col = [torch.zeros(max(cv, 1), dtype=torch.int32, device=dev) for cv, _ in caps]
        pairs = [torch.zeros((max(cv, 1), 2), dtype=torch.int32, device=dev) for cv, _ in caps]
        vt = [torch.zeros(max(cv, 1), dtype=torch.float32, device=dev) for cv, _ in caps]
        f = [torch.zeros((max(cf, 1), 3), dtype=torch.int32, device=dev) for _, cf in caps]

        def ptrs(xs):
            if all(x is None for x in xs):
                return None
            return (C.c_void_p * m)(*[None if x is None else x.data_ptr() for x in xs])

        _fills_done()
        try:
            self._check(fn(
                self.h, n, arr, inv, carr, ptrs(v), ptrs(nr), ptrs(col), ptrs(pairs), ptrs(vt),
                ptrs(f), (C.c_size_t * m)(*[c[0] for c in caps]),
                (C.c_size_t * m)(*[c[1] for c in caps]), nv, nf, ncv, ncf), "cell_clip")
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i], ncv[i], ncf[i]) for i in range(n)]
            e.buffers = (v, [x for x in nr if x is not None], col, pairs, vt, f)
            raise
        cut = lambda x, k: None if x is None else x[:k]
        return [(v[i][:nv[i]], cut(nr[i], nv[i]), col[i][:nv[i]], pairs[i][:nv[i]],
                 vt[i][:nv[i]], f[i][:nf[i]], ncv[i], ncf[i]) for i in range(n)]

    def cell_clip_domains(self, slots, meshes, invert=None, normals=True, bounds=None):
        """spray_rt_domains_cell_clip: the clipped meshes (see cell_clip) into
        slots (empty or loaded), extracted and built on the device; normals,
        colours and bounds as in tet_isosurface_domains."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(meshes) != n:
            e = SprayRtError("cell_clip_domains: %d slots, %d meshes" % (n, len(meshes)))
            e.code = -1
            raise e
        arr, carr, keep = _cell_table(meshes)
        inv = _invert_arg(invert, n)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(lib().spray_rt_domains_cell_clip(
            self.h, n, sl, arr, inv, carr, 1 if normals else 0, b, nf), "domains_cell_clip")
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the extraction's
        if bounds is True:
            self.sync()
            return out[:n].cpu().numpy()
        return out

    def cell_clip_phase_times(self, on=None):
        """spray_rt_cell_clip_phase_times of the last clip -> cell_phase_times'
        five for the cap ([3] the emit of cap and skin, [4] both sorts), then
        the wall clock of the skin passes; on switches the sorts' timing."""
        if on is not None:
            self._check(lib().spray_rt_tet_set_timing(self.h, 1 if on else 0), "tet_set_timing")
        out = (C.c_double * 6)()
        self._check(lib().spray_rt_cell_clip_phase_times(self.h, out), "cell_clip_phase_times")
        return list(out)

    def plane_values(self, points, origin, normal, out=None):
        """spray_rt_plane_values: ((p - origin) . normal) of every point (float32
        [n, 3], numpy or a GPU tensor) -> float32 GPU tensor [n] (out, if given:
        a float32 GPU tensor of that many elements), the values of a plane clip
        or slice at isovalue 0.  Enqueued on the context's stream."""
        import torch
        pts, npts = _tet_array(points, np.float32, 3, "points")
        o, d = _plane_args(origin, normal)
        if out is None:
            out = torch.zeros(npts, dtype=torch.float32, device="cuda:%d" % self._device)
            _fills_done()
        elif out.numel() != npts or out.dtype != torch.float32:
            raise ValueError("plane_values: out holds one float32 per point")
        a, k = _addr(pts)
        self._check(lib().spray_rt_plane_values(self.h, a, npts, o.ctypes.data, d.ctypes.data,
                                                out.data_ptr()), "plane_values")
        return out

    # ---- streamlines ----
    def streamlines(self, fields, capacity=None, count_only=False):
        """spray_rt_streamlines: the streamlines of vector grids (see
        _stream_tables) in one batched call -> [(points float32 [np, 3],
        line_offsets int32 [nseeds + 1], line_info int32 [nseeds, 2], holding
        the uint32 bits)] as GPU tensors of the exact sizes (a counting call
        first).  capacity skips the counting call and traces into buffers of
        that many points per field (SPRAY_RT_ERR_LIMIT if one is too small);
        count_only: the point counts alone."""
        import torch
        n = len(fields)
        arr, _, _, keep = _stream_tables(fields)
        m = max(n, 1)
        npts = (C.c_size_t * m)()
        fn = lib().spray_rt_streamlines
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, None, None, None, None, npts), "streamlines")
            if count_only:
                return [npts[i] for i in range(n)]
            caps = [npts[i] for i in range(n)]
        else:
            caps = [int(capacity)] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        p = [torch.zeros((max(c, 1), 3), dtype=torch.float32, device=dev) for c in caps]
        off = [torch.zeros(int(arr[i].nseeds) + 1, dtype=torch.int32, device=dev)
               for i in range(n)]
        info = [torch.zeros((max(int(arr[i].nseeds), 1), 2), dtype=torch.int32, device=dev)
                for i in range(n)]
        ptrs = lambda xs: (C.c_void_p * m)(*[x.data_ptr() for x in xs])
        _fills_done()
        try:
            self._check(fn(self.h, n, arr, ptrs(p), ptrs(off), ptrs(info),
                           (C.c_size_t * m)(*caps), npts), "streamlines")
        except SprayRtError as e:
            e.counts = [npts[i] for i in range(n)]
            e.buffers = (p, off, info)
            raise
        return [(p[i][:npts[i]], off[i], info[i][:int(arr[i].nseeds)]) for i in range(n)]

    def stream_tubes(self, fields, tubes, normals=True, capacity=None, count_only=False):
        """spray_rt_stream_tubes: the streamlines of fields as tubes (see
        _stream_tables) -> [(verts float32 [nv, 3], normals float32 [nv, 3] or
        None, colors int32 [nv] holding the 0x00RRGGBB bits, faces int32 [nf, 3]
        holding the uint32 bits)] as GPU tensors.  capacity=(nverts, nfaces) and
        count_only as in streamlines (count_only: [(nv, nf)])."""
        import torch
        n = len(fields)
        arr, tarr, carr, keep = _stream_tables(fields, tubes)
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        fn = lib().spray_rt_stream_tubes
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, tarr, carr, None, None, None, None, None, None, nv, nf),
                        "stream_tubes")
            if count_only:
                return [(nv[i], nf[i]) for i in range(n)]
            caps = [(nv[i], nf[i]) for i in range(n)]
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        v = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) for cv, _ in caps]
        nr = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) if normals else None
              for cv, _ in caps]
        col = [torch.zeros(max(cv, 1), dtype=torch.int32, device=dev) for cv, _ in caps]
        f = [torch.zeros((max(cf, 1), 3), dtype=torch.int32, device=dev) for _, cf in caps]
        ptrs = lambda xs: (C.c_void_p * m)(*[None if x is None else x.data_ptr() for x in xs])
        _fills_done()
        try:
            self._check(fn(self.h, n, arr, tarr, carr, ptrs(v), ptrs(nr) if normals else None,
                           ptrs(col), ptrs(f), (C.c_size_t * m)(*[c[0] for c in caps]),
                           (C.c_size_t * m)(*[c[1] for c in caps]), nv, nf), "stream_tubes")
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i]) for i in range(n)]
            e.buffers = tuple(b for b in (v, nr, col, f) if n and b[0] is not None)
            raise
        return [(v[i][:nv[i]], nr[i][:nv[i]] if normals else None, col[i][:nv[i]], f[i][:nf[i]])
                for i in range(n)]

    def stream_tubes_domains(self, slots, fields, tubes, normals=True, bounds=None):
        """spray_rt_domains_stream_tubes: the tubes of stream_tubes() into slots
        (empty or loaded), traced, expanded and built on the device; a slot
        carries colours when its field has a cfield or its tube a color.
        bounds as in refit_domains -> (bounds result, triangle counts)."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(fields) != n:
            e = SprayRtError("stream_tubes_domains: %d slots, %d fields" % (n, len(fields)))
            e.code = -1
            raise e
        arr, tarr, carr, keep = _stream_tables(fields, tubes)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(lib().spray_rt_domains_stream_tubes(
            self.h, n, sl, arr, tarr, carr, 1 if normals else 0, b, nf), "domains_stream_tubes")
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the expansion's
        if bounds is True:
            self.sync()
            out = out[:n].cpu().numpy()
        return out, [nf[i] for i in range(n)]

    def stream_phase_times(self):
        """spray_rt_stream_phase_times of the last streamline call -> [ms to the
        end of the host read, ms of the second integration and the expansion,
        ms of the device build]."""
        out = (C.c_double * 3)()
        self._check(lib().spray_rt_stream_phase_times(self.h, out), "stream_phase_times")
        return list(out)

    # ---- streamlines across blocks ----
    def block_streamlines(self, sets, capacity=None, count_only=False):
        """spray_rt_block_streamlines: the streamlines through sets of vector
        blocks (see _block_tables) in one batched call -> [(points, line_offsets,
        line_info, point_blocks int32 [np] holding the uint32 bits)], the first
        three and capacity / count_only as in streamlines."""
        import torch
        n = len(sets)
        arr, _, _, keep = _block_tables(sets)
        m = max(n, 1)
        npts = (C.c_size_t * m)()
        fn = lib().spray_rt_block_streamlines
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, None, None, None, None, None, npts),
                        "block_streamlines")
            if count_only:
                return [npts[i] for i in range(n)]
            caps = [npts[i] for i in range(n)]
        else:
            caps = [int(capacity)] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        p = [torch.zeros((max(c, 1), 3), dtype=torch.float32, device=dev) for c in caps]
        off = [torch.zeros(int(arr[i].nseeds) + 1, dtype=torch.int32, device=dev)
               for i in range(n)]
        info = [torch.zeros((max(int(arr[i].nseeds), 1), 2), dtype=torch.int32, device=dev)
                for i in range(n)]
        blk = [torch.zeros(max(c, 1), dtype=torch.int32, device=dev) for c in caps]
        ptrs = lambda xs: (C.c_void_p * m)(*[x.data_ptr() for x in xs])
        _fills_done()
        try:
            self._check(fn(self.h, n, arr, ptrs(p), ptrs(off), ptrs(info), ptrs(blk),
                           (C.c_size_t * m)(*caps), npts), "block_streamlines")
        except SprayRtError as e:
            e.counts = [npts[i] for i in range(n)]
            e.buffers = (p, off, info, blk)
            raise
        return [(p[i][:npts[i]], off[i], info[i][:int(arr[i].nseeds)], blk[i][:npts[i]])
                for i in range(n)]

    def block_stream_tubes(self, sets, tubes, normals=True, capacity=None, count_only=False):
        """spray_rt_block_stream_tubes: the streamlines through sets of blocks as
        tubes (see _block_tables); results, capacity and count_only as in
        stream_tubes."""
        import torch
        n = len(sets)
        arr, tarr, carr, keep = _block_tables(sets, tubes)
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        fn = lib().spray_rt_block_stream_tubes
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, tarr, carr, None, None, None, None, None, None, nv, nf),
                        "block_stream_tubes")
            if count_only:
                return [(nv[i], nf[i]) for i in range(n)]
            caps = [(nv[i], nf[i]) for i in range(n)]
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        # zeroed, one element at least: a buffer a failed call must not touch
        v = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) for cv, _ in caps]
        nr = [torch.zeros((max(cv, 1), 3), dtype=torch.float32, device=dev) if normals else None
              for cv, _ in caps]
        col = [torch.zeros(max(cv, 1), dtype=torch.int32, device=dev) for cv, _ in caps]
        f = [torch.zeros((max(cf, 1), 3), dtype=torch.int32, device=dev) for _, cf in caps]
        ptrs = lambda xs: (C.c_void_p * m)(*[None if x is None else x.data_ptr() for x in xs])
        _fills_done()
        try:
            self._check(fn(self.h, n, arr, tarr, carr, ptrs(v), ptrs(nr) if normals else None,
                           ptrs(col), ptrs(f), (C.c_size_t * m)(*[c[0] for c in caps]),
                           (C.c_size_t * m)(*[c[1] for c in caps]), nv, nf),
                        "block_stream_tubes")
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i]) for i in range(n)]
            e.buffers = tuple(b for b in (v, nr, col, f) if n and b[0] is not None)
            raise
        return [(v[i][:nv[i]], nr[i][:nv[i]] if normals else None, col[i][:nv[i]], f[i][:nf[i]])
                for i in range(n)]

    def block_stream_tubes_domains(self, slots, sets, tubes, normals=True, bounds=None):
        """spray_rt_domains_block_stream_tubes: the tubes of block_stream_tubes()
        into slots, a whole set's tubes into one slot; a slot carries colours
        when its set's blocks have a cfield or its tube a color.  bounds as in
        refit_domains -> (bounds result, triangle counts)."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(sets) != n:
            e = SprayRtError("block_stream_tubes_domains: %d slots, %d sets" % (n, len(sets)))
            e.code = -1
            raise e
        arr, tarr, carr, keep = _block_tables(sets, tubes)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(lib().spray_rt_domains_block_stream_tubes(
            self.h, n, sl, arr, tarr, carr, 1 if normals else 0, b, nf),
            "domains_block_stream_tubes")
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the expansion's
        if bounds is True:
            self.sync()
            out = out[:n].cpu().numpy()
        return out, [nf[i] for i in range(n)]

    def block_stream_phase_times(self):
        """spray_rt_block_stream_phase_times of the last block streamline call,
        as stream_phase_times."""
        out = (C.c_double * 3)()
        self._check(lib().spray_rt_block_stream_phase_times(self.h, out),
                    "block_stream_phase_times")
        return list(out)

    # ---- glyphs ----
    def glyphs(self, sets, glyphs, normals=True, capacity=None, count_only=False, arrays=None):
        """spray_rt_glyphs: the kept points of sets as spheres or arrows (see
        _glyph_tables) in one batched call -> [(verts float32 [nv, 3], normals
        float32 [nv, 3] or None, colors int32 [nv] holding the 0x00RRGGBB bits,
        faces int32 [nf, 3] and point_ids int32 [nglyphs] holding the uint32
        bits)] as GPU tensors.  capacity=(nverts, nfaces) and count_only as in
        stream_tubes (count_only: [(nv, nf)]).  arrays: the subset of ("verts",
        "normals", "colors", "faces", "point_ids") to extract, the others None
        (verts and normals alone feed refit_domains, colors alone
        recolor_domains)."""
        import torch
        n = len(sets)
        arr, garr, carr, keep = _glyph_tables(sets, glyphs)
        m = max(n, 1)
        nv, nf = (C.c_size_t * m)(), (C.c_size_t * m)()
        fn = lib().spray_rt_glyphs
        if capacity is None or count_only:
            self._check(fn(self.h, n, arr, garr, carr, None, None, None, None, None, None, None,
                           nv, nf), "glyphs")
            if count_only:
                return [(nv[i], nf[i]) for i in range(n)]
            caps = [(nv[i], nf[i]) for i in range(n)]
        else:
            caps = [(int(capacity[0]), int(capacity[1]))] * n
        dev = "cuda:%d" % self._device
        want = set(("verts", "normals", "colors", "faces", "point_ids") if arrays is None else arrays)
        if not normals:
            want.discard("normals")
        # zeroed, one element at least: a buffer a failed call must not touch
        zeros = lambda name, shape, dt: (torch.zeros(shape, dtype=dt, device=dev)
                                         if name in want else None)
        v = [zeros("verts", (max(cv, 1), 3), torch.float32) for cv, _ in caps]
        nr = [zeros("normals", (max(cv, 1), 3), torch.float32) for cv, _ in caps]
        col = [zeros("colors", max(cv, 1), torch.int32) for cv, _ in caps]
        f = [zeros("faces", (max(cf, 1), 3), torch.int32) for _, cf in caps]
        ids = [zeros("point_ids", max(_glyph_counts(arr, garr, i, caps[i][0]), 1), torch.int32)
               for i in range(n)]
        ptrs = lambda name, xs: ((C.c_void_p * m)(*[x.data_ptr() for x in xs])
                                 if n and name in want else None)
        _fills_done()
        try:
            self._check(fn(self.h, n, arr, garr, carr, ptrs("verts", v), ptrs("normals", nr),
                           ptrs("colors", col), ptrs("faces", f), ptrs("point_ids", ids),
                           (C.c_size_t * m)(*[c[0] for c in caps]),
                           (C.c_size_t * m)(*[c[1] for c in caps]), nv, nf), "glyphs")
        except SprayRtError as e:
            e.counts = [(nv[i], nf[i]) for i in range(n)]
            e.buffers = tuple(b for b in (v, nr, col, f, ids) if n and b[0] is not None)
            raise
        cut = lambda x, k: None if x is None else x[:k]
        return [(cut(v[i], nv[i]), cut(nr[i], nv[i]), cut(col[i], nv[i]), cut(f[i], nf[i]),
                 cut(ids[i], _glyph_counts(arr, garr, i, nv[i]))) for i in range(n)]

    def glyphs_domains(self, slots, sets, glyphs, normals=True, bounds=None):
        """spray_rt_domains_glyphs: the glyph meshes of glyphs() into slots
        (empty or loaded), expanded and built on the device; a slot carries
        colours when its set has a cfield or its glyph a color.  bounds as in
        refit_domains -> (bounds result, triangle counts)."""
        slots = [int(s) for s in slots]
        n = len(slots)
        if len(sets) != n:
            e = SprayRtError("glyphs_domains: %d slots, %d sets" % (n, len(sets)))
            e.code = -1
            raise e
        arr, garr, carr, keep = _glyph_tables(sets, glyphs)
        m = max(n, 1)
        sl = (C.c_int * m)(*slots)
        out = self._bounds_out(bounds, n)
        b, k = _addr(out)
        nf = (C.c_size_t * m)()
        self._check(lib().spray_rt_domains_glyphs(
            self.h, n, sl, arr, garr, carr, 1 if normals else 0, b, nf), "domains_glyphs")
        for s in slots:
            self._nverts.pop(s, None)  # the vertex count is the expansion's
        if bounds is True:
            self.sync()
            out = out[:n].cpu().numpy()
        return out, [nf[i] for i in range(n)]

    def glyph_phase_times(self):
        """spray_rt_glyph_phase_times of the last glyph call -> [ms to the end
        of the host read, ms of the place pass and the expansion, ms of the
        device build]."""
        out = (C.c_double * 3)()
        self._check(lib().spray_rt_glyph_phase_times(self.h, out), "glyph_phase_times")
        return list(out)

    def slot_export(self, slot, what):
        """One array of a resident slot as numpy: SLOT_NODES / SLOT_QNODES4 as
        uint8 [n, 64] (the 64-B node records), SLOT_TRIS float32 [ntris, 12],
        SLOT_PRIMS uint32, SLOT_QGRID float32 [6], SLOT_NORMALS float32 [nverts, 3],
        SLOT_COLORS uint32 [nverts] (empty for a slot without colours), SLOT_FACES
        uint32 [ntris, 3]."""
        nb = C.c_size_t()
        self._check(lib().spray_rt_slot_export(self.h, int(slot), int(what), None, 0,
                                               C.byref(nb)), "slot_export")
        out = np.zeros(nb.value, np.uint8)
        if nb.value:
            self._check(lib().spray_rt_slot_export(self.h, int(slot), int(what), out.ctypes.data,
                                                   out.nbytes, C.byref(nb)), "slot_export")
        out = out.view(self._SLOT_DTYPES[int(what)])
        shape = {self.SLOT_NODES: (-1, 64), self.SLOT_QNODES4: (-1, 64), self.SLOT_TRIS: (-1, 12),
                 self.SLOT_NORMALS: (-1, 3), self.SLOT_FACES: (-1, 3)}.get(int(what))
        return out.reshape(shape) if shape else out

    def slot_sah(self, slot):
        """SAH cost of the slot's current BVH2 (spray_rt_slot_sah)."""
        v = C.c_double()
        self._check(lib().spray_rt_slot_sah(self.h, int(slot), C.byref(v)), "slot_sah")
        return v.value

    def domain_bounds(self, boxes):
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        self._check(lib().spray_rt_domain_bounds(self.h, len(b), b.ctypes.data),
                    "domain_bounds")

    def map_domain(self, domain_id, slot):
        self._check(lib().spray_rt_map_domain(self.h, int(domain_id), int(slot)),
                    "map_domain")

    def slot_info(self, slot):
        nn, nt = C.c_size_t(), C.c_size_t()
        d = C.c_int()
        self._check(lib().spray_rt_slot_info(self.h, int(slot), C.byref(nn), C.byref(d),
                                             C.byref(nt)), "slot_info")
        return {"nodes": nn.value, "depth": d.value, "tris": nt.value}

    # ---- Embree-1M streams ----
    def intersect1M(self, slot, rays, stride=96):
        a, keep = _addr(rays)
        n = _nbytes(rays) // stride
        self._check(lib().spray_rt_intersect1M(self.h, int(slot), a, n, stride),
                    "intersect1M")

    def occluded1M(self, slot, rays, stride=96):
        a, keep = _addr(rays)
        n = _nbytes(rays) // stride
        self._check(lib().spray_rt_occluded1M(self.h, int(slot), a, n, stride),
                    "occluded1M")

    def _segments(self, fn, slots, offsets, rays, stride, what):
        s = np.ascontiguousarray(slots, np.int32)
        o = np.ascontiguousarray(offsets, np.uint64)
        assert len(o) == len(s) + 1
        a, keep = _addr(rays)
        self._check(fn(self.h, s.ctypes.data, o.ctypes.data, len(s), a, stride), what)

    def intersect_segments(self, slots, offsets, rays, stride=96):
        self._segments(lib().spray_rt_intersect_segments, slots, offsets, rays, stride,
                       "intersect_segments")

    def occluded_segments(self, slots, offsets, rays, stride=96):
        self._segments(lib().spray_rt_occluded_segments, slots, offsets, rays, stride,
                       "occluded_segments")

    def domains1M(self, org, dir, maxhits):
        org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
        dir = np.ascontiguousarray(dir, np.float32).reshape(-1, 3)
        n = len(org)
        ids = np.zeros((n, maxhits), np.int32)
        ts = np.zeros((n, maxhits), np.float32)
        cnt = np.zeros(n, np.int32)
        self._check(lib().spray_rt_domains1M(self.h, org.ctypes.data, dir.ctypes.data, n,
                                             ids.ctypes.data, ts.ctypes.data,
                                             cnt.ctypes.data, int(maxhits)), "domains1M")
        return ids, ts, cnt

    # ---- fused scene path ----
    def intersect_scene(self, rays, hits=None, counters=None):
        """rays: RAY_DTYPE numpy array or uint8/float torch tensor on the GPU
        (32 B per ray); hits: HIT_DTYPE array / 48-B-per-ray tensor."""
        n = _nbytes(rays) // 32
        if hits is None:
            hits = np.zeros(n, HIT_DTYPE)
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        c, k3 = _addr(counters)
        self._check(lib().spray_rt_intersect_scene_counted(self.h, a, n, b, c),
                    "intersect_scene")
        return hits

    def occluded_scene(self, rays, occ=None, counters=None):
        n = _nbytes(rays) // 32
        if occ is None:
            occ = np.zeros(n, np.uint8)
        a, k1 = _addr(rays)
        b, k2 = _addr(occ)
        c, k3 = _addr(counters)
        self._check(lib().spray_rt_occluded_scene_counted(self.h, a, n, b, c),
                    "occluded_scene")
        return occ

    def occluded_scene_masked(self, rays, valid, occ):
        """Any hit over the rays with valid[i] != 0 (device buffers)."""
        n = _nbytes(rays) // 32
        a, k1 = _addr(rays)
        b, k2 = _addr(valid)
        c, k3 = _addr(occ)
        self._check(lib().spray_rt_occluded_scene_masked(self.h, a, n, b, c),
                    "occluded_scene_masked")

    def intersect_scene_spawn_pt(self, rays, hits, shade, out_rays, out_valid, d_count=None):
        """Closest hit + fused positional PT shadow spawn (device buffers)."""
        n = _nbytes(rays) // 32
        shade = np.ascontiguousarray(shade, np.float32)
        assert shade.size == 10
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        c, k3 = _addr(out_rays)
        d, k4 = _addr(out_valid)
        e, k5 = _addr(d_count)
        self._check(lib().spray_rt_intersect_scene_spawn_pt(self.h, a, n, b, shade.ctypes.data,
                                                            c, d, e), "intersect_scene_spawn_pt")

    def intersect_scene_shadow_pt(self, rays, hits, shade, occ, sh_valid, d_count=None):
        """Closest hit + PT shadow spawn + the shadows' any hit, one launch
        (device buffers): sh_valid[i], occ[i] positional by source ray."""
        n = _nbytes(rays) // 32
        shade = np.ascontiguousarray(shade, np.float32)
        assert shade.size == 10
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        c, k3 = _addr(occ)
        d, k4 = _addr(sh_valid)
        e, k5 = _addr(d_count)
        self._check(lib().spray_rt_intersect_scene_shadow_pt(self.h, a, n, b, shade.ctypes.data,
                                                             c, d, e),
                    "intersect_scene_shadow_pt")

    def occluded_scene_devcount(self, rays, max_rays, d_count, occ, counters=None):
        a, k1 = _addr(rays)
        b, k2 = _addr(d_count)
        c, k3 = _addr(occ)
        e, k4 = _addr(counters)
        self._check(lib().spray_rt_occluded_scene_devcount(self.h, a, int(max_rays), b, c, e),
                    "occluded_scene_devcount")

    # ---- in-situ (domain-sharded) ----
    def set_owners(self, owner):
        """Domain -> rank map (InsituPartition::rank), host int array."""
        o = np.ascontiguousarray(owner, np.int32)
        self._check(lib().spray_rt_set_owners(self.h, o.ctypes.data), "set_owners")

    def route(self, rays, rank_mask):
        """rank_mask[i] (uint64 / int64 device tensor) = ranks owning a domain
        on ray i's list."""
        n = _nbytes(rays) // 32
        a, k1 = _addr(rays)
        b, k2 = _addr(rank_mask)
        self._check(lib().spray_rt_route(self.h, a, n, b), "route")

    def exchange_plan(self, rank_mask, world, idx, starts):
        """idx = per destination rank the ascending ray indices (device int64;
        None: bounds only); starts [world + 1] int64."""
        n = rank_mask.numel()
        a, k1 = _addr(rank_mask)
        b, k2 = _addr(idx)
        c, k3 = _addr(starts)
        self._check(lib().spray_rt_exchange_plan(self.h, a, n, int(world), b, c),
                    "exchange_plan")

    def gather_rows(self, src, idx, dst):
        """dst[j] = src[idx[j]] (device tensors, rows of 4/8/16/32/48 B)."""
        n = idx.numel()
        row = _nbytes(src) // src.shape[0] if src.shape[0] else 4
        a, k1 = _addr(src)
        b, k2 = _addr(idx)
        c, k3 = _addr(dst)
        self._check(lib().spray_rt_gather_rows(self.h, a, row, b, n, c), "gather_rows")

    def intersect_scene_keyed(self, rays, hits, keys):
        """Closest hit over the resident domains + composite key (device)."""
        n = _nbytes(rays) // 32
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        c, k3 = _addr(keys)
        self._check(lib().spray_rt_intersect_scene_keyed(self.h, a, n, b, c),
                    "intersect_scene_keyed")

    def eye_rays_insitu(self, cam, image_w, spp, block, stripe, rays, pixid=None,
                        samid=None):
        cam = np.ascontiguousarray(cam, np.float32)
        bx, by, bw, bh = block
        tx, ty, tw, th = stripe
        a, k1 = _addr(rays)
        b, k2 = _addr(pixid)
        c, k3 = _addr(samid)
        self._check(lib().spray_rt_eye_rays_insitu(self.h, cam.ctypes.data, int(image_w),
                                                   int(spp), bx, by, bw, bh, tx, ty, tw, th,
                                                   a, b, c), "eye_rays_insitu")

    # ---- device ray sources ----
    def eye_rays_ooc(self, cam, image_w, spp, tile, rays, pixid=None, samid=None):
        cam = np.ascontiguousarray(cam, np.float32)
        tx, ty, tw, th = tile
        a, k1 = _addr(rays)
        b, k2 = _addr(pixid)
        c, k3 = _addr(samid)
        self._check(lib().spray_rt_eye_rays_ooc(self.h, cam.ctypes.data, int(image_w),
                                                int(spp), tx, ty, tw, th, a, b, c),
                    "eye_rays_ooc")

    def spawn_shadows_ao(self, rays, hits, pixid, n, nsamples, out_rays, out_src, d_count,
                         order=None, traced=False):
        """ooc::ShaderAo rays (nsamples per hit), compacted (device); order
        (optional, uint32/int32 device tensor): their sample-major trace order;
        traced: the rays written in that trace order instead."""
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        p, k3 = _addr(pixid)
        c, k4 = _addr(out_rays)
        d, k5 = _addr(out_src)
        e, k6 = _addr(d_count)
        if traced:
            if order is not None:
                raise ValueError("traced spawn writes no order")
            self._check(lib().spray_rt_spawn_shadows_ao_traced(self.h, a, b, p, int(n),
                                                               int(nsamples), c, d, e),
                        "spawn_shadows_ao_traced")
            return
        if order is None:
            self._check(lib().spray_rt_spawn_shadows_ao(self.h, a, b, p, int(n), int(nsamples),
                                                        c, d, e), "spawn_shadows_ao")
            return
        o, k7 = _addr(order)
        self._check(lib().spray_rt_spawn_shadows_ao_ordered(self.h, a, b, p, int(n),
                                                            int(nsamples), c, d, e, o),
                    "spawn_shadows_ao_ordered")

    def occluded_scene_order(self, rays, max_rays, order, d_count, occ):
        """Any hit of rays order[j], j < *d_count; occ[order[j]] written (device;
        order None: rays 0 .. *d_count - 1)."""
        a, k1 = _addr(rays)
        o, k2 = _addr(order) if order is not None else (None, None)
        b, k3 = _addr(d_count)
        c, k4 = _addr(occ)
        self._check(lib().spray_rt_occluded_scene_order(self.h, a, int(max_rays), o, b, c),
                    "occluded_scene_order")

    def occluded_ao(self, rays, hits, pixid, n, nsamples, out_pairs, lv, rec, d_count, occ,
                    counters=None):
        """ooc::ShaderAo's spawn fused into the any hit (device): AO ray k of
        the sample-major trace order is sample out_pairs[k] & 31 of source ray
        out_pairs[k] >> 5; occ[k] its occlusion; *d_count rays.  The rays are
        made in the any-hit lanes, never stored; lv (float32, npix * nsamples
        * 4) holds the (pixel, sample) local hemisphere samples, rec (float32,
        n * 16) the source rays' origins and frames."""
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        p, k3 = _addr(pixid)
        c, k4 = _addr(out_pairs)
        d, k5 = _addr(lv)
        r, k9 = _addr(rec)
        e, k6 = _addr(d_count)
        f, k7 = _addr(occ)
        g, k8 = _addr(counters) if counters is not None else (None, None)
        self._check(lib().spray_rt_occluded_ao(self.h, a, b, p, int(n), int(nsamples),
                                               _lv_pixels(lv, nsamples), c, d, r, e, f, g),
                    "occluded_ao")

    def spawn_shadows_ao_pairs(self, rays, hits, pixid, n, nsamples, out_pairs, lv, rec,
                               d_count):
        """The traced AO spawn as (source << 5 | sample) pairs plus the
        (pixel, sample) local hemisphere samples lv and the source rays'
        origins / frames rec (device)."""
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        p, k3 = _addr(pixid)
        c, k4 = _addr(out_pairs)
        d, k5 = _addr(lv)
        r, k7 = _addr(rec)
        e, k6 = _addr(d_count)
        self._check(lib().spray_rt_spawn_shadows_ao_pairs(self.h, a, b, p, int(n), int(nsamples),
                                                          _lv_pixels(lv, nsamples), c, d, r, e),
                    "spawn_shadows_ao_pairs")

    def occluded_ao_pairs(self, max_n, pairs, rec, lv, nsamples, d_count, occ, counters=None):
        """Any hit of the AO rays of (source << 5 | sample) pairs, each
        generated in its lane from rec / lv (device); occ[k], k < *d_count."""
        c, k4 = _addr(pairs)
        r, k9 = _addr(rec)
        d, k5 = _addr(lv)
        e, k6 = _addr(d_count)
        f, k7 = _addr(occ)
        g, k8 = _addr(counters) if counters is not None else (None, None)
        self._check(lib().spray_rt_occluded_ao_pairs(self.h, int(max_n), c, r, d, int(nsamples),
                                                     e, f, g), "occluded_ao_pairs")

    # ---- frame layer (shading, film, tiles) ----
    def set_bsdfs(self, bsdfs):
        """Per-domain BSDFs: a sequence of (type, p0, p1, p2) (Scene::getBsdf)."""
        n = len(bsdfs)
        arr = (BsdfRec * max(n, 1))()
        for i, b in enumerate(bsdfs):
            arr[i].type = int(b[0])
            for k in range(3):
                arr[i].p[k] = float(b[1 + k])
        self._check(lib().spray_rt_set_bsdfs(self.h, n, C.addressof(arr) if n else None),
                    "set_bsdfs")

    def intersect_scene_masked(self, rays, valid, hits):
        """Closest hit of the rays with valid[i] != 0 (device buffers)."""
        n = _nbytes(rays) // 32
        a, k1 = _addr(rays)
        b, k2 = _addr(valid)
        c, k3 = _addr(hits)
        self._check(lib().spray_rt_intersect_scene_masked(self.h, a, n, b, c),
                    "intersect_scene_masked")

    def shade(self, shader, bounce, rays, hits, w, valid, pixid, samid, shadows, sw, svalid,
              stats=None):
        """One ShaderPt / ShaderAo pass over positional path slots (device)."""
        n = _nbytes(rays) // 32
        ptrs = [_addr(x) for x in (rays, hits, w, valid, pixid, samid, shadows, sw, svalid,
                                   stats)]
        a = [p[0] for p in ptrs]
        self._check(lib().spray_rt_shade(self.h, C.byref(shader), int(bounce), a[0], a[1], a[2],
                                         a[3], a[4], a[5], n, a[6], a[7], a[8], a[9]), "shade")

    def film(self, image, pixid, n, spp, ns, sw, svalid, occ, scale):
        """image[pixid] += scale * unoccluded shadow weights (device)."""
        ptrs = [_addr(x) for x in (image, pixid, sw, svalid, occ)]
        a = [p[0] for p in ptrs]
        self._check(lib().spray_rt_film(self.h, a[0], a[1], int(n), int(spp), int(ns), a[2],
                                        a[3], a[4], float(scale)), "film")

    def render_tile(self, shader, cam, image_w, spp, tile, image):
        """One tile of an ooc-mode frame, enqueued on the context's stream."""
        cam = np.ascontiguousarray(cam, np.float32)
        tx, ty, tw, th = (int(v) for v in tile)
        a, k1 = _addr(image)
        self._check(lib().spray_rt_render_tile(self.h, C.byref(shader), cam.ctypes.data,
                                               int(image_w), int(spp), tx, ty, tw, th, a),
                    "render_tile")

    def render_tiles(self, shader, cam, image_w, spp, tiles, image):
        """Tiles [(x, y, w, h)] of an ooc-mode frame as one device batch
        (the same image as render_tile per tile), enqueued on the stream."""
        cam = np.ascontiguousarray(cam, np.float32)
        t = np.ascontiguousarray(np.asarray(tiles, np.int32).reshape(-1, 4))
        a, k1 = _addr(image)
        self._check(lib().spray_rt_render_tiles(self.h, C.byref(shader), cam.ctypes.data,
                                                int(image_w), int(spp), t.ctypes.data,
                                                len(t), a), "render_tiles")

    def frame_stats(self, reset=True):
        """(radiance rays, shadow rays) traced by render_tile since the last
        reset (synchronises); raises on shading cases the reference aborts on."""
        out = (C.c_ulonglong * 3)()
        self._check(lib().spray_rt_frame_stats(self.h, out, int(bool(reset))), "frame_stats")
        return int(out[0]), int(out[1])

    def spawn_shadows_pt(self, rays, hits, n, shade, out_rays, out_src, d_count):
        shade = np.ascontiguousarray(shade, np.float32)
        assert shade.size == 10
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        c, k3 = _addr(out_rays)
        d, k4 = _addr(out_src)
        e, k5 = _addr(d_count)
        self._check(lib().spray_rt_spawn_shadows_pt(self.h, a, b, int(n), shade.ctypes.data,
                                                    c, d, e), "spawn_shadows_pt")


class OocCache:
    """Out-of-core domains (spray_rt_ooc_*): every domain image in pinned host
    memory, ``cache_slots`` of them resident in HBM at a time (LruCache)."""

    def __init__(self, rt, cache_slots):
        self.rt = rt
        h = C.c_void_p()
        rt._check(lib().spray_rt_ooc_create(rt.h, int(cache_slots), C.byref(h)), "ooc_create")
        self.h = h.value
        rt._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            lib().spray_rt_ooc_destroy(self.h)
            self.h = None
            self.rt._release(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_domain(self, domain_id, verts, faces, colors=None, normals=None):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        c = None if colors is None else np.ascontiguousarray(colors, np.uint32)
        n = None if normals is None else np.ascontiguousarray(normals, np.float32)
        self.rt._check(lib().spray_rt_ooc_set_domain(
            self.h, int(domain_id), v.ctypes.data, len(v), f.ctypes.data, len(f),
            None if c is None else c.ctypes.data, None if n is None else n.ctypes.data),
            "ooc_set_domain")

    def intersect(self, rays, hits):
        n = _nbytes(rays) // 32
        a, k1 = _addr(rays)
        b, k2 = _addr(hits)
        self.rt._check(lib().spray_rt_ooc_intersect(self.h, a, n, b), "ooc_intersect")

    def occluded(self, rays, valid, occ):
        n = _nbytes(rays) // 32
        a, k1 = _addr(rays)
        b, k2 = _addr(valid)
        c, k3 = _addr(occ)
        self.rt._check(lib().spray_rt_ooc_occluded(self.h, a, n, b, c), "ooc_occluded")

    def stats(self):
        out = (C.c_ulonglong * 4)()
        self.rt._check(lib().spray_rt_ooc_stats(self.h, out), "ooc_stats")
        return {"loads": out[0], "hits": out[1], "bytes": out[2], "drains": out[3]}


def ooc_scene(desc, ply_path, cache_slots, device=0):
    """RtContext + OocCache over every domain of a scene file."""
    rt = RtContext(device)
    boxes, _ = host_parse_scene(desc, ply_path)
    rt.domain_bounds(boxes)
    oc = OocCache(rt, cache_slots)
    for d in range(len(boxes)):
        oc.set_domain(d, *host_domain_mesh(desc, ply_path, d))
    return rt, oc


class Scene:
    """GPU-backed scene (src/render/scene.h:62-251 surface)."""

    def __init__(self, desc, ply_path="", cache_size=-1, device=0):
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = lib().spray_scene_create(desc.encode(), (ply_path or "").encode(),
                                      int(cache_size), int(device), C.byref(h), err, 1024)
        if rc != 0:
            raise SprayRtError("Scene(%s) failed (%d): %s" % (desc, rc, err.value.decode()))
        self.h = h.value
        self.rt = RtContext(handle=lib().spray_scene_rt(self.h))

    def close(self):
        if getattr(self, "h", None):
            rt = getattr(self, "rt", None)
            if rt is not None:
                rt.close()  # what was created on the scene's context goes first
            lib().spray_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().spray_scene_last_error(self.h)
            raise SprayRtError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def getNumDomains(self):
        return lib().spray_scene_num_domains(self.h)

    def cache_capacity(self):
        return lib().spray_scene_cache_capacity(self.h)

    def domain_bounds(self):
        n = self.getNumDomains()
        boxes = np.zeros((n, 6), np.float32)
        bound = np.zeros(6, np.float32)
        lib().spray_scene_bounds(self.h, boxes.ctypes.data, bound.ctypes.data)
        return boxes, bound

    def getLights(self):
        out = []
        for i in range(lib().spray_scene_num_lights(self.h)):
            b = np.zeros(7, np.float32)
            lib().spray_scene_light(self.h, i, b.ctypes.data)
            out.append({"type": "point" if b[0] == 0 else "diffuse", "pos": b[1:4].copy(),
                        "rad": b[4:7].copy()})
        return out

    def load(self, domain_id):
        """Scene::load(id, SceneInfo*) -> cache block."""
        blk = C.c_int()
        self._check(lib().spray_scene_load(self.h, int(domain_id), C.byref(blk)), "load")
        return blk.value

    def intersect(self, cache_block, org, dir):
        """Scene::intersect for one ray -> (hit, RTC_ISECT_DTYPE record)."""
        rec = np.zeros(1, RTC_ISECT_DTYPE)
        o = np.asarray(org, np.float32)
        d = np.asarray(dir, np.float32)
        hit = lib().spray_scene_intersect1(self.h, int(cache_block), o.ctypes.data,
                                           d.ctypes.data, rec.ctypes.data)
        return bool(hit), rec[0]

    def occluded(self, cache_block, org, dir):
        rec = np.zeros(1, RTC_ISECT_DTYPE)
        o = np.asarray(org, np.float32)
        d = np.asarray(dir, np.float32)
        return bool(lib().spray_scene_occluded1(self.h, int(cache_block), o.ctypes.data,
                                                d.ctypes.data, rec.ctypes.data))

    def intersectDomains(self, org, dir, maxhits=None):
        """Sorted (ids, ts) per ray; org/dir [n,3]."""
        n = self.getNumDomains()
        ids, ts, cnt = self.rt.domains1M(org, dir, maxhits or n)
        return ids, ts, cnt

    def domain_mesh(self, domain_id):
        nv, nf = C.c_size_t(), C.c_size_t()
        self._check(lib().spray_scene_domain_mesh(self.h, int(domain_id), C.byref(nv),
                                                  C.byref(nf), None, None, None, None),
                    "domain_mesh")
        v = np.zeros((nv.value, 3), np.float32)
        f = np.zeros((nf.value, 3), np.uint32)
        c = np.zeros(nv.value, np.uint32)
        n = np.zeros((nv.value, 3), np.float32)
        self._check(lib().spray_scene_domain_mesh(self.h, int(domain_id), C.byref(nv),
                                                  C.byref(nf), v.ctypes.data, f.ctypes.data,
                                                  c.ctypes.data, n.ctypes.data),
                    "domain_mesh")
        return v, f, c, n

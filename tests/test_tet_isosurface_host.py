"""The host restatement of the isosurface extraction from tetrahedral meshes
(spray_rt_tet_isosurface_host; no GPU): against the numpy restatement of
tet_helpers byte for byte, against the structured extraction of section 12 on
Kuhn meshes, and the properties of the rule.
"""
import ctypes as C

import numpy as np
import pytest

import iso_helpers as ih
import tet_helpers as th

ERR_ARG, ERR_LIMIT = -1, -5
F32 = np.float32


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def meshes():
    return th.gpu_meshes()


def same(got, ref):
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()


@pytest.mark.parametrize("k", [th.SINGLE, th.CUBE, th.SMALL, th.FULL, th.PARTIAL, th.REORIENTED])
def test_host_equals_numpy(spray, meshes, k):
    m = meshes[k]
    got = th.host_mesh(spray, m)
    assert len(got[3]) > 0
    same(got, th.tet_isosurface_numpy(m))
    if m.get("cfield") is not None and m["cmap"][0].size > 1:
        assert len(np.unique(got[2])) > 3


def grid_as_mesh(g):
    nz, ny, nx = g["values"].shape
    p, t = th.kuhn_mesh((nx, ny, nz), g["origin"], g["spacing"])
    return dict(points=p, tets=t, values=g["values"].reshape(-1), iso=g["iso"],
                normals=ih.neg_gradient(g["values"], np.asarray(g["spacing"], F32)).reshape(-1, 3))


@pytest.mark.parametrize("make", [ih.sphere_grid, ih.torus_grid,
                                  lambda: ih.ramp_grid((7, 5, 6), 0.1, 4)],
                         ids=["sphere", "torus", "ramp"])
def test_kuhn_mesh_equals_the_structured_extraction(spray, make):
    g = make()
    assert not (g["values"] == F32(g["iso"])).any()
    v0, n0, f0 = spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"])
    v1, n1, _, f1 = th.host_mesh(spray, grid_as_mesh(g))
    assert len(v0) == len(v1) > 0 and len(f0) == len(f1) > 0
    # no two vertices share a position: the permutation that matches rows is unique
    assert len(np.unique(v0, axis=0)) == len(v0)
    r0, r1 = np.hstack([v0, n0]).view(np.uint32), np.hstack([v1, n1]).view(np.uint32)
    o0, o1 = np.lexsort(r0.T[::-1]), np.lexsort(r1.T[::-1])
    assert r0[o0].tobytes() == r1[o1].tobytes()       # positions and normals, bit for bit
    to1 = np.empty(len(v0), np.int64)                 # vertex id there -> vertex id here
    to1[o0] = o1
    assert np.array_equal(to1[f0.astype(np.int64)], f1.astype(np.int64))  # same rows, same winding
    assert not np.array_equal(o0, o1)                 # the vertex order does differ


def test_all_sign_cases_in_both_orientations(spray):
    p, t = th.single_tet()
    for order in ((0, 1, 2, 3), (1, 0, 2, 3), (0, 1, 3, 2), (3, 2, 1, 0)):
        pts = p[list(order)]
        for s in range(16):
            vals = np.array([(0.5 + 0.25 * v) * (1 if (s >> v) & 1 else -1) for v in range(4)], F32)
            v, _, _, f = spray.tet_isosurface_host(pts, t, vals, 0.0)
            nin = bin(s).count("1")
            assert len(f) == (0, 1, 2, 1, 0)[nin] and len(v) == (0, 3, 4, 3, 0)[nin]
            if not len(f):
                continue
            # the affine field through the four samples
            A = np.hstack([pts.astype(np.float64), np.ones((4, 1))])
            grad = np.linalg.solve(A, vals.astype(np.float64))[:3]
            ng = ih.geometric_normals(v, f)
            assert (ng @ grad < 0).all(), (order, s)


def test_closed_oriented_surfaces(spray):
    for make, grad, euler in ((ih.sphere_grid, ih.sphere_grad, 2), (ih.torus_grid, ih.torus_grad, 0)):
        m = grid_as_mesh(make())
        m = th.reoriented(m, 3)                       # mixed orientations on the way in
        v, _, _, f = th.host_mesh(spray, m)
        ih.assert_closed_oriented(f, len(v), euler)
        ng = ih.geometric_normals(v, f)
        centre = v.astype(np.float64)[f].mean(1)
        assert ((ng * grad(centre)).sum(-1) < 0).all()   # toward decreasing values


def test_reoriented_copy(spray, meshes):
    a, b = meshes[th.FULL], meshes[th.REORIENTED]
    assert not np.array_equal(a["tets"], b["tets"])
    odd = th.orientation_odd(b["points"], b["tets"].astype(np.int64))
    assert 0.3 < odd.mean() < 0.7                      # both orientations in one mesh
    ma, mb = th.host_mesh(spray, a), th.host_mesh(spray, b)
    same(ma[:3], mb[:3])                               # vertices, normals, colours: the bytes
    assert ma[3].tobytes() != mb[3].tobytes()
    # the same oriented patch per tet, never reflected (tet_helpers.patches)
    assert th.patches(a, ma[3]) == th.patches(b, mb[3])
    # and the triangles themselves wherever a tet has one
    pa, pb = th.patches(a, ma[3]), th.patches(b, mb[3])
    assert sum(len(c) == 3 for c in pa) > 50 and sum(len(c) == 4 for c in pa) > 50
    assert [c for c in pa if len(c) == 3] == [c for c in pb if len(c) == 3]


def test_empty_surface_and_no_tets(spray, meshes):
    v, n, c, f = th.host_mesh(spray, meshes[th.EMPTY])
    assert v.shape == (0, 3) and n.shape == (0, 3) and c.shape == (0,) and f.shape == (0, 3)
    p, t = th.single_tet()
    v, n, c, f = spray.tet_isosurface_host(p, t[:0], np.zeros(4, F32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    # nothing is read of a mesh without tets: not even NaN points matter
    v, n, c, f = spray.tet_isosurface_host(p * np.nan, t[:0], np.full(4, np.nan, F32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_sample_equal_to_the_isovalue(spray):
    p, t = th.kuhn_mesh((3, 3, 3))
    f = (1.0 - np.abs(p - 1.0).sum(-1)).astype(F32)   # an octahedron whose corners are samples
    assert (f == 0).sum() >= 6
    m = dict(points=p, tets=t, values=f, iso=0.0)
    v, _, _, faces = th.host_mesh(spray, m)
    same((v, faces), (lambda r: (r[0], r[3]))(th.tet_isosurface_numpy(m)))
    area = np.linalg.norm(ih.geometric_normals(v, faces), axis=-1)
    assert (area == 0).any() and (area > 0).any()      # zero-area triangles are kept
    img = spray.bvh_build_device_host(v, faces)         # and the build accepts them
    assert len(img["prims"]) == len(faces)


def test_repeated_point_and_duplicate_tets(spray):
    p, t = th.single_tet()
    vals = np.array([1, -1, -1, -1], F32)
    v, _, _, f = spray.tet_isosurface_host(p, t, vals, 0.0)
    assert len(v) == 3 and len(f) == 1
    # point 1 listed twice: the pair (1, 1) never crosses, the vertex (0, 1) is shared
    dup = np.array([[0, 1, 1, 3]], np.uint32)
    m = dict(points=p, tets=dup, values=vals, iso=0.0)
    v2, _, _, f2 = th.host_mesh(spray, m)
    same((v2, f2), (lambda r: (r[0], r[3]))(th.tet_isosurface_numpy(m)))
    assert len(v2) == 2 and len(f2) == 1 and len(set(f2[0].tolist())) == 2
    # duplicate tets: duplicate faces, the same vertices
    v3, _, _, f3 = spray.tet_isosurface_host(p, np.vstack([t, t]), vals, 0.0)
    assert v3.tobytes() == v.tobytes() and f3.tobytes() == np.vstack([f, f]).tobytes()


def test_two_meshes_agree_on_a_shared_plane(spray):
    field = lambda p: (1.9 - np.linalg.norm(p.astype(np.float64) - [3.13, 2.21, 1.37], axis=-1)).astype(F32)
    colour = lambda p: (np.sin(p.astype(np.float64) @ np.array([0.7, 1.1, 0.4]))).astype(F32)
    normal = lambda p: np.cos(p.astype(np.float64) * 0.9 + 0.2).astype(F32)
    cmap = (th.ch.table(64, 9), -1.0, 1.0)
    rows = []
    for origin, plane_i in (((0, 0, 0), 3), ((3, 0, 0), 0)):
        p, t = th.kuhn_mesh((4, 5, 4), origin)
        m = dict(points=p, tets=t, values=field(p), iso=0.0, normals=normal(p), cfield=colour(p),
                 cmap=cmap)
        assert np.abs(m["values"]).min() > 1e-3   # no vertex sits on a point: x == 3 is in-plane pairs
        v, n, c, _ = th.host_mesh(spray, m)
        on = v[:, 0] == F32(3.0)
        assert on.sum() > 4
        r = np.hstack([v[on], n[on]]).view(np.uint32)
        r = np.hstack([r, c[on, None]])
        rows.append(r[np.lexsort(r.T[::-1])])
    assert rows[0].tobytes() == rows[1].tobytes()


def test_identical_bytes_twice(spray, meshes):
    m = meshes[th.PARTIAL]
    same(th.host_mesh(spray, m), th.host_mesh(spray, m))


def raw_host(spray, p, t, vals, iso, normals=None, npoints=None, ntets=None, want_normals=False,
             gcolor=None, null=()):
    """spray_rt_tet_isosurface_host itself -> (rc, nverts, nfaces)."""
    from spray_amd._native import TetMesh, lib
    rec = TetMesh()
    rec.points = None if "points" in null else p.ctypes.data
    rec.tets = None if "tets" in null else t.ctypes.data
    rec.values = None if "values" in null else vals.ctypes.data
    rec.point_normals = None if normals is None else normals.ctypes.data
    rec.npoints = len(p) if npoints is None else npoints
    rec.ntets = len(t) if ntets is None else ntets
    rec.isovalue = iso
    nv, nf = C.c_size_t(), C.c_size_t()
    out = np.zeros((64, 3), F32)
    rc = lib().spray_rt_tet_isosurface_host(
        None if "mesh" in null else C.addressof(rec), gcolor, C.byref(nv), C.byref(nf), None,
        out.ctypes.data if want_normals else None, None, None)
    return rc, nv.value, nf.value


def test_argument_errors(spray):
    p, t = th.single_tet()
    vals = np.array([1, -1, -1, -1], F32)
    nrm = np.ones((4, 3), F32)
    assert raw_host(spray, p, t, vals, 0.0) == (0, 3, 1)
    assert raw_host(spray, p, t, vals, 0.0, nrm, want_normals=True) == (0, 3, 1)
    for null in ("mesh", "points", "tets", "values"):
        assert raw_host(spray, p, t, vals, 0.0, null=(null,))[0] == ERR_ARG, null
    assert raw_host(spray, p, t, vals, 0.0, want_normals=True)[0] == ERR_ARG   # no point_normals
    for iso in (np.nan, np.inf):
        assert raw_host(spray, p, t, vals, iso)[0] == ERR_ARG
    assert raw_host(spray, p, t, vals, 0.0, npoints=3)[0] == ERR_ARG           # index 3 >= npoints
    assert raw_host(spray, p, t, vals, 0.0, ntets=1 << 29)[0] == ERR_LIMIT
    assert raw_host(spray, p, t, vals, 0.0, npoints=1 << 32)[0] == ERR_LIMIT
    assert raw_host(spray, p, t, vals, 0.0, npoints=(1 << 32) - 1)[0] == 0

    # non-finite values at referenced points; an unreferenced one is never read
    p5 = np.vstack([p, [[np.nan, 0, 0]]]).astype(F32)
    v5 = np.append(vals, F32(np.nan))
    n5 = np.vstack([nrm, [[np.inf, 0, 0]]]).astype(F32)
    g5 = np.append(np.linspace(0, 1, 4), np.nan).astype(F32)
    cmap = (th.ch.table(8, 1), 0.0, 1.0)
    ok = spray.tet_isosurface_host(p5, t, v5, 0.0, n5, g5, cmap)
    assert len(ok[0]) == 3
    for k in range(4):
        def bad(a, value=np.nan):
            a = a.copy()
            a[k] = value
            return a
        for args in ((bad(p5), t, v5, 0.0), (p5, t, bad(v5), 0.0), (p5, t, bad(v5, np.inf), 0.0),
                     (p5, t, v5, 0.0, bad(n5)), (p5, t, v5, 0.0, None, bad(g5), cmap)):
            with pytest.raises(spray.SprayRtError) as e:
                spray.tet_isosurface_host(*args)
            assert e.value.code == ERR_ARG
    # a NaN normal is not read where normals are not written
    assert len(spray.tet_isosurface_host(p5, t, v5, 0.0, None)[0]) == 3
    assert raw_host(spray, p5, t, v5, 0.0, n5 * np.nan)[0] == 0

    # colour maps: section 13's checks
    tab = th.ch.table(8, 1)
    for cm in (None, (np.zeros(4097, np.uint32), 0.0, 1.0), (np.zeros(0, np.uint32), 0.0, 1.0),
               (tab, 1.0, 1.0), (tab, np.nan, 1.0), (tab, -3e38, 3e38), (tab, 0.0, 1e-45)):
        with pytest.raises(spray.SprayRtError) as e:
            spray.tet_isosurface_host(p, t, vals, 0.0, None, g5[:4], cm)
        assert e.value.code == ERR_ARG

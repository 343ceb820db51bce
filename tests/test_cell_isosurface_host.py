"""The split of hexahedra, wedges and pyramids into tets and the host
restatement of their isosurface extraction (spray_rt_cell_split_host,
spray_rt_cell_isosurface_host; no GPU): against the numpy restatement of
cell_helpers, against the tet extraction of the split list byte for byte, and
the properties of the rule.
"""
import ctypes as C

import numpy as np
import pytest

import cell_helpers as ch
import iso_helpers as ih
import tet_helpers as th

ERR_ARG, ERR_LIMIT = -1, -5
F32 = np.float32
TYPES = (ch.TET, ch.HEX, ch.WEDGE, ch.PYRAMID)
NSEEDS = 64


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


def same(got, ref):
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()


def geometry(m):
    return dict(points=m[0], types=m[1], offsets=m[2], conn=m[3])


def field_mesh(geom, f, iso=0.0, **kw):
    return ch.mesh(geom, f, iso, **kw)


def small_meshes():
    """Every mesh of the CPU tests: one cell of each type, the renumbered 3x3x3
    lattice, the mixed mesh, each with a field that crosses it."""
    inner = ch.sphere((0.3, 0.2, 0.1), 0.8)
    ms = [field_mesh(ch.one_cell(t, 5 + t), inner, normals=True, cmap_seed=t, ntable=16)
          for t in TYPES]
    ms.append(field_mesh(ch.hex_lattice((4, 4, 4), seed=9), ch.sphere((1.45, 1.55, 1.5), 1.2),
                         normals=True, cmap_seed=3, ntable=64))
    ms.append(field_mesh(ch.mixed_mesh(), ch.sphere((1.05, 0.95, 1.02), 1.3), normals=True,
                         color=0x00102030))
    ms.append(field_mesh(ch.mixed_mesh(11), ch.sphere((0.2, 1.8, 0.4), 1.5)))
    # through the cube's corners: the surface crosses cells of every type
    ms.append(field_mesh(ch.mixed_mesh(), ch.sphere((1.0, 0.7, 0.8), 1.7), cmap_seed=8, ntable=32))
    return ms


@pytest.mark.parametrize("ctype", TYPES)
def test_split_equals_numpy_over_renumberings(spray, ctype):
    apexes, diagonals = set(), set()
    for seed in range(NSEEDS):
        p, types, offsets, conn = ch.one_cell(ctype, seed)
        want, m, quads = ch.split_cell(ctype, conn)
        got = spray.cell_split_host(types, offsets, conn, len(p))
        assert got.dtype == np.uint32 and got.shape == (ch.NTETS[ctype], 4)
        assert got.tolist() == want, seed
        apexes.add(m)
        diagonals |= {(fi, j % 2) for fi, j in quads}
        if ctype == ch.TET:
            continue
        # integer corners: six times the absolute volumes, exact, sum to the unit
        # cell's (hex 1, wedge 1/2, pyramid 1/3)
        vol6 = np.abs(ch.det6(p, got.astype(np.int64)))
        assert (vol6 > 0).all()
        assert vol6.sum() == {ch.HEX: 6.0, ch.WEDGE: 3.0, ch.PYRAMID: 2.0}[ctype], seed
    if ctype != ch.TET:
        # the apex at every local position, both diagonals of every quad face
        assert apexes == set(range(ch.NPOINTS[ctype]))
        quad_faces = [fi for fi, q in enumerate(ch.FACES[ctype]) if len(q) == 4]
        assert diagonals == {(fi, d) for fi in quad_faces for d in (0, 1)}


def test_volumes_of_sheared_cells(spray):
    """Affine images with integer corners: the same exact sums."""
    A = np.array([[2, 1, 0], [0, 3, 1], [1, 0, 2]], np.float64)
    det = abs(round(np.linalg.det(A)))
    for ctype, share in ((ch.HEX, 6), (ch.WEDGE, 3), (ch.PYRAMID, 2)):
        for seed in range(8):
            pts = (ch.UNIT[ctype].astype(np.float64) @ A.T + [5, -3, 2]).astype(F32)
            p, types, offsets, conn = ch.one_cell(ctype, seed, pts)
            tets = spray.cell_split_host(types, offsets, conn, len(p))
            assert np.abs(ch.det6(p, tets.astype(np.int64))).sum() == share * det


@pytest.mark.parametrize("make", [lambda: ch.hex_lattice((4, 4, 4), seed=9), ch.mixed_mesh,
                                  lambda: ch.mixed_mesh(12)], ids=["lattice", "mixed", "mixed12"])
def test_split_is_conforming(spray, make):
    g = geometry(make())
    tets = ch.host_tets(spray, g)
    assert tets.tolist() == ch.split_numpy(g).tolist()
    tris, cnt = ch.tet_face_counts(tets)
    assert cnt.max() == 2                       # no triangle is shared by three tets: no crack
    ch.assert_closed_manifold(tris[cnt == 1])   # the rest is the mesh boundary
    # and the tets fill the cells: volumes, exactly
    assert (np.abs(ch.det6(g["points"], tets.astype(np.int64))) > 0).all()


def test_lattice_boundary_count(spray):
    g = geometry(ch.hex_lattice((4, 4, 4), seed=9))
    tris, cnt = ch.tet_face_counts(ch.host_tets(spray, g))
    assert (cnt == 1).sum() == 108              # 6 sides x 9 quads x 2 triangles
    p = g["points"][tris[cnt == 1]]             # each on one side of the box
    assert (((p == 0).all(1) | (p == 3).all(1)).any(1)).all()


def test_mixed_mesh_has_all_types():
    _, types, _, _ = ch.mixed_mesh()
    assert sorted(np.unique(types, return_counts=True)[1].tolist()) == [2, 2, 5, 5]
    assert set(types.tolist()) == set(TYPES)


def test_host_restatement_equals_its_definition(spray):
    for k, m in enumerate(small_meshes()):
        got = ch.host_mesh(spray, m)
        assert len(got[3]) > 0, k
        tets = ch.host_tets(spray, m)
        same(got, th.host_mesh(spray, ch.as_tets(m, tets)))
        same(got, ch.cell_isosurface_numpy(m))


@pytest.mark.parametrize("which", ["lattice", "mixed"])
def test_closed_oriented_surfaces(spray, which):
    if which == "lattice":
        c, r = np.array([2.95, 3.05, 3.0]), 2.2
        m = field_mesh(ch.hex_lattice((7, 7, 7), seed=4), ch.sphere(c, r))
    else:
        c, r = np.array([1.05, 0.95, 1.02]), 1.3
        m = field_mesh(ch.mixed_mesh(), ch.sphere(c, r))
    v, _, _, f = ch.host_mesh(spray, m)
    ih.assert_closed_oriented(f, len(v), 2)
    # consistently oriented and closed: Ng leaves the inside (toward decreasing
    # values) everywhere iff the volume the surface encloses is positive
    ng = ih.geometric_normals(v, f)
    centre = v.astype(np.float64)[f].mean(1)
    assert (ng * (centre - c)).sum() > 0
    if which == "lattice":
        assert ((ng * (centre - c)).sum(-1) > 0).all()


def test_tets_only_mesh(spray):
    meshes = th.gpu_meshes()
    for k in (th.CUBE, th.SMALL, th.REORIENTED):
        tm = meshes[k]
        m = ch.tets_only(tm)
        assert ch.host_tets(spray, m).tobytes() == np.ascontiguousarray(tm["tets"]).tobytes()
        same(ch.host_mesh(spray, m), th.host_mesh(spray, tm))


def grid_meshes(g):
    nz, ny, nx = g["values"].shape
    nrm = ih.neg_gradient(g["values"], np.asarray(g["spacing"], F32)).reshape(-1, 3)
    rng = np.random.default_rng(nx)
    extra = dict(values=g["values"].reshape(-1), iso=g["iso"], normals=nrm,
                 cfield=rng.normal(size=nx * ny * nz).astype(F32),
                 cmap=(th.ch.table(32, 5), -1.5, 1.5))
    p, t = th.kuhn_mesh((nx, ny, nz), g["origin"], g["spacing"])
    hexes = ch.hex_lattice((nx, ny, nz), g["origin"], g["spacing"])
    assert hexes[0].tobytes() == p.tobytes()
    return dict(extra, points=p, tets=t), dict(extra, **geometry(hexes))


@pytest.mark.parametrize("make", [ih.sphere_grid, ih.torus_grid,
                                  lambda: ih.ramp_grid((7, 5, 6), 0.1, 4)],
                         ids=["sphere", "torus", "ramp"])
def test_lattice_numbered_hexes_equal_the_kuhn_mesh(spray, make):
    tm, cm = grid_meshes(make())
    vt, nt, ct, ft = th.host_mesh(spray, tm)
    vc, nc, cc, fc = ch.host_mesh(spray, cm)
    assert len(vt) > 0 and len(np.unique(ct)) > 3
    same((vc, nc, cc), (vt, nt, ct))            # positions, normals, colours: the bytes
    assert fc.shape == ft.shape
    tets = ch.host_tets(spray, cm)
    # the same six tets per cell, in another order and another listing
    def per_cell(T):
        S = np.sort(np.asarray(T).reshape(-1, 6, 4).astype(np.int64), axis=2)
        return np.sort((S[..., 0] << 48) | (S[..., 1] << 32) | (S[..., 2] << 16) | S[..., 3], axis=1)

    assert np.array_equal(per_cell(tets), per_cell(np.asarray(tm["tets"])))
    assert tets.tobytes() != np.ascontiguousarray(tm["tets"]).tobytes()
    assert ch.patches(ch.as_tets(cm, tets), fc) == ch.patches(tm, ft)


def test_collapsed_hex(spray):
    p, types, offsets, conn = ch.one_cell(ch.HEX)
    conn = conn.copy()
    conn[6] = conn[5]                            # a point listed twice (a degenerate wedge)
    m = dict(points=p, types=types, offsets=offsets, conn=conn, iso=0.0,
             values=ch.sphere((0.3, 0.2, 0.1), 0.8)(p).astype(F32))
    tets = ch.host_tets(spray, m)
    assert tets.tolist() == ch.split_numpy(m).tolist() and len(tets) == 6
    assert any(len(set(t)) < 4 for t in tets.tolist())
    got = ch.host_mesh(spray, m)
    assert len(got[3]) > 0
    same(got, ch.cell_isosurface_numpy(m))
    # ties: every index equal -- the lowest positions win
    m0 = dict(m, conn=np.zeros(8, np.uint32))
    assert ch.host_tets(spray, m0).tolist() == ch.split_numpy(m0).tolist() == [[0] * 4] * 6
    assert len(ch.host_mesh(spray, m0)[0]) == 0


def test_no_cells_empty_surface_equal_sample_two_runs(spray):
    g = geometry(ch.hex_lattice((4, 3, 3)))
    m = dict(g, values=th.wave_f(g["points"]).astype(F32), iso=100.0,
             normals=np.ones_like(g["points"]))
    v, n, c, f = ch.host_mesh(spray, m)
    assert v.shape == (0, 3) and n.shape == (0, 3) and c.shape == (0,) and f.shape == (0, 3)
    # ncells == 0 reads nothing: not even NaN points matter
    none = dict(m, types=m["types"][:0], offsets=m["offsets"][:1], conn=m["conn"][:0], iso=0.3,
                points=m["points"] * np.nan, values=m["values"] * np.nan)
    v, n, c, f = ch.host_mesh(spray, none)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    assert ch.host_tets(spray, none).shape == (0, 4)
    # samples equal to the isovalue: an octahedron whose corners are lattice points
    g = geometry(ch.hex_lattice((3, 3, 3), seed=2))
    val = (1.0 - np.abs(g["points"] - 1.0).sum(-1)).astype(F32)
    assert (val == 0).sum() >= 6
    m = dict(g, values=val, iso=0.0)
    got = ch.host_mesh(spray, m)
    same(got, ch.cell_isosurface_numpy(m))
    area = np.linalg.norm(ih.geometric_normals(got[0], got[3]), axis=-1)
    assert (area == 0).any() and (area > 0).any()      # zero-area triangles are kept
    same(got, ch.host_mesh(spray, m))                  # twice: the same bytes


def raw_host(spray, m, null=(), want_normals=False, gcolor=None, **over):
    """spray_rt_cell_isosurface_host and spray_rt_cell_split_host themselves
    -> ((rc, nverts, nfaces), (rc, ntets))."""
    from spray_amd._native import CellMesh, lib
    rec = CellMesh()
    keep = {k: np.ascontiguousarray(m[k]) for k in ("points", "types", "offsets", "conn", "values")}
    for k, a in keep.items():
        setattr(rec, k, None if k in null else a.ctypes.data)
    nrm = None if m.get("normals") is None else np.ascontiguousarray(m["normals"], F32)
    rec.point_normals = None if nrm is None else nrm.ctypes.data
    rec.npoints, rec.ncells, rec.nconn = len(keep["points"]), len(keep["types"]), len(keep["conn"])
    rec.isovalue = m["iso"]
    for k, x in over.items():
        setattr(rec, k, x)
    nv, nf, nt = C.c_size_t(), C.c_size_t(), C.c_size_t()
    out = np.zeros((64, 3), F32)
    rc = lib().spray_rt_cell_isosurface_host(
        None if "mesh" in null else C.addressof(rec), gcolor, C.byref(nv), C.byref(nf), None,
        out.ctypes.data if want_normals else None, None, None)
    rc2 = lib().spray_rt_cell_split_host(None if "mesh" in null else C.addressof(rec),
                                         C.byref(nt), None)
    return (rc, nv.value, nf.value), (rc2, nt.value)


def test_argument_errors(spray):
    p, types, offsets, conn = ch.mixed_mesh()
    m = dict(points=p, types=types, offsets=offsets, conn=conn, iso=0.0,
             values=ch.sphere((1.05, 0.95, 1.02), 1.3)(p).astype(F32))
    ok = ch.host_mesh(spray, m)
    ntets = len(ch.split_numpy(m))
    assert raw_host(spray, m) == ((0, len(ok[0]), len(ok[3])), (0, ntets))
    nrm = np.ones_like(p)
    assert raw_host(spray, dict(m, normals=nrm), want_normals=True)[0][0] == 0
    for null in ("mesh", "types", "offsets", "conn"):
        assert [r[0] for r in raw_host(spray, m, null=(null,))] == [ERR_ARG, ERR_ARG], null
    for null in ("points", "values"):     # the split reads neither
        assert [r[0] for r in raw_host(spray, m, null=(null,))] == [ERR_ARG, 0], null
    assert raw_host(spray, m, want_normals=True)[0][0] == ERR_ARG   # no point_normals
    for iso in (np.nan, np.inf):
        assert raw_host(spray, dict(m, iso=iso))[0][0] == ERR_ARG
    for over in (dict(ncells=1 << 29), dict(nconn=1 << 32), dict(npoints=1 << 32)):
        assert [r[0] for r in raw_host(spray, m, **over)] == [ERR_LIMIT, ERR_LIMIT], over
    assert raw_host(spray, m, npoints=(1 << 32) - 1)[0][0] == 0

    def fails(bad):
        with pytest.raises(spray.SprayRtError) as e:
            ch.host_mesh(spray, bad)
        assert e.value.code == ERR_ARG
        return bad

    def listing_fails(bad):
        fails(bad)
        with pytest.raises(spray.SprayRtError) as e:
            ch.host_tets(spray, bad)
        assert e.value.code == ERR_ARG

    def poked(key, index, value):
        a = np.array(m[key], copy=True)
        a[index] = value
        return dict(m, **{key: a})

    listing_fails(poked("types", 3, 11))                       # an unknown type (a voxel)
    listing_fails(poked("types", 3, 0))
    hexes = np.nonzero(types == ch.HEX)[0]
    listing_fails(poked("types", hexes[0], ch.WEDGE))          # offsets against the type
    listing_fails(poked("offsets", 2, offsets[2] + 1))
    listing_fails(poked("offsets", 2, offsets[3] + 1))         # descending
    assert raw_host(spray, m, nconn=len(conn) - 1)[0][0] == ERR_ARG   # offsets[i + 1] > nconn
    assert raw_host(spray, m, nconn=len(conn) - 1)[1][0] == ERR_ARG
    listing_fails(poked("conn", 17, len(p)))                   # an index >= npoints
    assert [r[0] for r in raw_host(spray, m, npoints=len(p) - 1)] == [ERR_ARG, ERR_ARG]

    # non-finite values at the points of a cell the surface does not cross, and
    # an unreferenced NaN point that is never read
    far = ch.sphere((2.9, 0.1, 0.05), 0.5)     # around one outer corner of the wedges on +x
    mf = dict(m, values=far(p).astype(F32))
    T = np.asarray([conn[offsets[i]:offsets[i + 1]] for i in np.nonzero(types == ch.HEX)[0]])
    inside = mf["values"] >= 0
    quiet = [row for row in T if not inside[row].any()]
    assert len(quiet) == 5 and inside.any() and len(ch.host_mesh(spray, mf)[3]) > 0
    k = int(quiet[0][6])
    p1 = np.vstack([p, [[np.nan] * 3]]).astype(F32)
    v1 = np.append(mf["values"], F32(np.nan))
    n1 = np.vstack([nrm, [[np.inf, 0, 0]]]).astype(F32)
    g1 = np.append(np.linspace(0, 1, len(p)), np.nan).astype(F32)
    cmap = (th.ch.table(8, 1), 0.0, 1.0)
    full = dict(mf, points=p1, values=v1, normals=n1, cfield=g1, cmap=cmap)
    ref = ch.host_mesh(spray, dict(mf, normals=nrm, cfield=g1[:-1], cmap=cmap))
    same(ch.host_mesh(spray, full), ref)

    def bad(a, value=np.nan):
        a = a.copy()
        a[k] = value
        return a

    fails(dict(full, points=bad(p1)))
    fails(dict(full, values=bad(v1)))
    fails(dict(full, values=bad(v1, np.inf)))
    fails(dict(full, normals=bad(n1)))
    fails(dict(full, cfield=bad(g1)))
    # a NaN normal is not read where normals are not written
    same(ch.host_mesh(spray, dict(full, normals=bad(n1)), normals=False)[2:], ref[2:])

    # colour maps: section 13's checks
    tab = th.ch.table(8, 1)
    for cm in (None, (np.zeros(4097, np.uint32), 0.0, 1.0), (np.zeros(0, np.uint32), 0.0, 1.0),
               (tab, 1.0, 1.0), (tab, np.nan, 1.0), (tab, -3e38, 3e38), (tab, 0.0, 1e-45)):
        fails(dict(mf, cfield=g1[:-1], cmap=cm))

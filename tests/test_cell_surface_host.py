"""The host restatement of the boundary-surface and threshold extraction from
cell meshes (spray_rt_cell_surface_host; no GPU): every array against the numpy
restatement of surface_helpers byte for byte, and the properties of the rule
(DESIGN.md section 16).
"""
import ctypes as C

import numpy as np
import pytest

import cell_helpers as ch
import surface_helpers as sh
import tet_helpers as th

ERR_ARG, ERR_LIMIT = -1, -5
F32 = np.float32
TYPES = (ch.TET, ch.HEX, ch.WEDGE, ch.PYRAMID)
NTRIS = {ch.TET: 4, ch.HEX: 12, ch.WEDGE: 8, ch.PYRAMID: 6}
NSEEDS = 64


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


def same(got, ref):
    assert len(got) == len(ref) == 5
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()


def check(spray, m, sel=None):
    """The host restatement equals numpy, with normals and without, twice; the
    vertices are the mesh's own points, ascending -> the five arrays."""
    got = sh.host_surface(spray, m, sel)
    same(got, sh.surface_numpy(m, sel))
    same(sh.host_surface(spray, m, sel), got)
    bare = sh.host_surface(spray, m, sel, normals=False)
    same(bare, (got[0], None) + got[2:])
    v, n, col, ids, f = got
    assert (np.diff(ids.astype(np.int64)) > 0).all()
    assert v.tobytes() == np.asarray(m["points"], F32)[ids].tobytes()
    if n is not None:
        assert n.tobytes() == np.asarray(m["normals"], F32)[ids].tobytes()
    if len(f):
        assert f.max() < len(v) and len(np.unique(f)) == len(v)
    return got


def outward(m, v, f):
    """Ng = (v0 - v1) x (v2 - v0) of every triangle points away from the mesh's centroid
    (convex meshes)."""
    centre = np.asarray(m["points"], np.float64).mean(0)
    v = v.astype(np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ng = np.cross(a - b, c - a)
    return (np.einsum("ij,ij->i", ng, (a + b + c) / 3 - centre) > 0).all()


def cell_volume(spray, m):
    tets = ch.host_tets(spray, dict(m, points=m["points"]))
    return float(np.abs(ch.det6(m["points"], tets.astype(np.int64))).sum()) / 6.0


@pytest.mark.parametrize("ctype", TYPES)
def test_single_cells_over_renumberings(spray, ctype):
    firsts = set()
    for seed in range(NSEEDS):
        m = sh.mesh(ch.one_cell(ctype, seed), normals=bool(seed & 1),
                    cmap_seed=seed if seed & 2 else None, ntable=16)
        v, n, col, ids, f = check(spray, m)
        assert len(f) == NTRIS[ctype] and len(v) == ch.NPOINTS[ctype]   # every face is emitted
        assert outward(m, v, f), seed
        sh.assert_closed_oriented(f)
        ch.assert_closed_manifold(f)
        assert sh.euler(f) == 2
        firsts.add(list(m["conn"]).index(0))
    assert firsts == set(range(ch.NPOINTS[ctype]))   # the smallest index at every local position


def test_lattice_surface_is_the_boundary_of_the_tet_split(spray):
    m = sh.mesh(ch.hex_lattice((4, 4, 4), seed=9), normals=True, cmap_seed=3, ntable=64)
    v, n, col, ids, f = check(spray, m)
    assert len(f) == 108
    on_box = ((v == 0) | (v == 3)).any(1)
    assert on_box.all() and len(v) == 64 - 8
    # as sets of point triples: the faces occurring once among the split's tets
    tri, cnt = ch.tet_face_counts(ch.host_tets(spray, m))
    want = {tuple(t) for t in tri[cnt == 1].tolist()}
    got = [tuple(sorted(t)) for t in ids[f].tolist()]
    assert len(set(got)) == len(got) == 108 and set(got) == want
    ch.assert_closed_manifold(f)
    sh.assert_closed_oriented(f)
    assert sh.euler(f) == 2
    assert sh.signed_volume(v, f) == 27.0
    assert outward(m, v, f)


@pytest.mark.parametrize("seed", [3, 11, None])
def test_conforming_mixed_mesh(spray, seed):
    m = sh.mesh(sh.conforming_mesh(seed), normals=True, color=0x00102030)
    assert set(m["types"].tolist()) == {ch.HEX, ch.WEDGE, ch.PYRAMID}
    v, n, col, ids, f = check(spray, m)
    ch.assert_closed_manifold(f)
    sh.assert_closed_oriented(f)
    assert sh.euler(f) == 2
    assert sh.signed_volume(v, f) == cell_volume(spray, m) == 32.0
    assert (col == 0x00102030).all()
    # the centre and the cube's interior faces are gone: 6 hexes' outer shells
    assert len(v) == len(m["points"]) - 1


@pytest.fixture(scope="module")
def ball():
    """A 9^3-point lattice with the distance from near its centre."""
    geom = ch.hex_lattice((9, 9, 9), seed=5)
    return sh.mesh(geom, lambda p: np.linalg.norm(p.astype(np.float64) - (4.1, 3.9, 4.05), axis=-1),
                   normals=True, cmap_seed=21, ntable=4096)


def test_threshold_by_points_and_by_cells(spray, ball):
    sel = sh.select("points", 0.0, 3.4)
    kept = sh.kept_cells(ball, sel)
    assert 30 < kept.sum() < 0.5 * len(kept)
    v, n, col, ids, f = got = check(spray, ball, sel)
    sh.assert_closed_oriented(f)
    # closed and consistently oriented with a positive volume: outward
    assert sh.signed_volume(v, f) == float(kept.sum())
    assert len(np.unique(col)) > 8
    # the same kept set as cell values: the same bytes
    cv = np.where(kept, 5.0, -5.0).astype(F32)
    same(check(spray, ball, sh.select("cells", 5.0, 5.0, cv)), got)
    same(check(spray, ball, sh.select("cells", 0.0, sh.WIDE, cv)), got)
    # a shell: lo cuts an inner surface as well
    shell = sh.select("points", 1.8, 3.4)
    ks = sh.kept_cells(ball, shell)
    assert 0 < ks.sum() < kept.sum()
    v, n, col, ids, f = check(spray, ball, shell)
    sh.assert_closed_oriented(f)
    assert sh.signed_volume(v, f) == float(ks.sum())
    # bounds are inclusive
    val = float(ball["values"][17])
    one = sh.select("points", val, val)
    assert sh.kept_cells(ball, one).sum() == 0
    cv[:] = 0
    cv[7] = val
    assert len(check(spray, ball, sh.select("cells", val, val, cv))[4]) == 12


def test_empty_surfaces(spray, ball):
    for got in (check(spray, ball, sh.select("points", 100.0, 200.0)),
                check(spray, ball, sh.select("cells", 1.0, 2.0, np.zeros(512, F32)))):
        assert len(got[0]) == len(got[4]) == 0 and got[4].shape == (0, 3)
    e = dict(ball, types=ball["types"][:0], offsets=ball["offsets"][:1], conn=ball["conn"][:0])
    for sel in (None, sh.select("points", 0.0, 3.0), sh.select("cells", 0.0, 1.0, np.zeros(0, F32))):
        got = check(spray, e, sel)
        assert len(got[0]) == len(got[4]) == 0


def test_regions_touching_along_an_edge(spray):
    m = sh.mesh(ch.hex_lattice((3, 3, 2), seed=2), normals=True)
    cv = np.array([1, 0, 0, 1], F32)
    v, n, col, ids, f = check(spray, m, sh.select("cells", 1.0, 1.0, cv))
    assert len(f) == 24 and len(v) == 14
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [0, 2]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    assert sorted(set(cnt.tolist())) == [2, 4]     # non-manifold along the shared edge
    sh.assert_closed_oriented(f)
    assert sh.signed_volume(v, f) == 2.0


def test_duplicate_cells_vanish(spray):
    p, types, offsets, conn = ch.hex_lattice((3, 2, 2), seed=4)
    two = conn.reshape(2, 8)
    m = sh.mesh((p,) + ch.cells([ch.HEX] * 3, [two[0], two[0], two[1]]))
    v, n, col, ids, f = check(spray, m)
    # the doubled hex has no face left, and takes the shared face with it
    assert len(f) == 10 and set(ids.tolist()) == set(two[1].tolist())
    m = sh.mesh((p,) + ch.cells([ch.HEX] * 2, [two[0], two[0]]))
    assert len(check(spray, m)[4]) == 0


def test_collapsed_and_non_conforming_cells(spray):
    p, types, offsets, conn = ch.one_cell(ch.HEX, 6)
    for a, b in ((1, 0), (6, 2), (7, 4)):
        c2 = conn.copy()
        c2[a] = c2[b]
        check(spray, sh.mesh((p, types, offsets, c2), normals=True))
    # the existing mixed mesh: a quad of a hex faces the two triangles of a
    # pyramid cut into tets through the quad's smallest index; all three are
    # emitted (the other diagonal: test_a_quad_never_matches_a_facing_triangle)
    for seed in (3, 11):
        m = sh.mesh(ch.mixed_mesh(seed), normals=True, cmap_seed=8, ntable=32)
        v, n, col, ids, f = check(spray, m)
        assert set(m["types"].tolist()) == {ch.TET, ch.HEX, ch.WEDGE, ch.PYRAMID}
        corners = [i for i, q in enumerate(m["points"])
                   if q[0] == 0 and set(q.tolist()) <= {0.0, 2.0}]
        assert len(corners) == 4
        inner = [t for t in ids[f].tolist() if set(t) <= set(corners)]
        assert len(inner) == 4   # the quad's two triangles and the two tets' faces


@pytest.mark.parametrize("through_min", [True, False], ids=["min-diagonal", "other-diagonal"])
def test_a_quad_never_matches_a_facing_triangle(spray, through_min):
    """A hex whose quad faces two tets' triangles, cut along either diagonal: the
    quad's two triangles and both facing triangles are emitted.  Along the
    other diagonal one facing triangle lies on the quad's smallest corner and
    its two neighbours, the quad's own triple."""
    for seed in [None] + list(range(16)):
        m = sh.mesh(sh.cut_quad_mesh(through_min, seed), normals=True)
        v, n, col, ids, f = check(spray, m)
        conn = m["conn"]
        quad = set(conn[:4].tolist())
        # the face the two tets share drops, nothing else: 12 + 2 * 4 - 2 triangles
        assert len(f) == 18 and len(v) == 9, seed
        tris = [tuple(sorted(t)) for t in ids[f].tolist()]
        inner = sorted(t for t in tris if set(t) <= quad)
        facing = sorted(tuple(sorted(conn[o:o + 3].tolist())) for o in (8, 12))
        assert len(inner) == 4 and all(t in inner for t in facing), seed
        mine = sorted(t for t in inner if t not in facing) if not through_min else facing
        # the hex cuts its quad through the smallest index, whatever the tets do
        assert all(min(quad) in t for t in mine) and len(mine) == 2
        assert (len(set(inner)) == 2) == through_min
        # the triple collision the corner count settles
        faces = sh.cell_faces(m, np.ones(3, bool))
        of = lambda n: {k[1:] for k, _, _ in faces if k[0] == n}
        assert bool(of(3) & of(4)) == (not through_min), seed


@pytest.mark.parametrize("ntable", [1, 4096])
def test_colour_maps(spray, ntable):
    geom = ch.hex_lattice((5, 4, 4), seed=1)
    m = sh.mesh(geom, th.wave_f, normals=True, cmap_seed=17, ntable=ntable, clamp=0.4)
    col = check(spray, m, sh.select("points", 0.3, sh.WIDE))[2]
    assert len(col) > 0 and (len(np.unique(col)) == 1 if ntable == 1 else len(np.unique(col)) > 4)
    plain = sh.mesh(geom, th.wave_f)
    assert (check(spray, plain)[2] == 0).all()          # no colour: zeros
    const = sh.mesh(geom, th.wave_f, color=0x00ABCDEF)
    assert (check(spray, const)[2] == 0x00ABCDEF).all()


# ---- errors ----
def fails(spray, m, sel, code=ERR_ARG):
    with pytest.raises(spray.SprayRtError) as e:
        sh.host_surface(spray, m, sel)
    assert e.value.code == code


def poked(m, key, index, value):
    a = np.array(m[key], copy=True)
    a[index] = value
    return dict(m, **{key: a})


def test_argument_errors(spray):
    geom = ch.hex_lattice((5, 4, 3), seed=12)
    m = sh.mesh(geom, th.wave_f, normals=True, cmap_seed=5, ntable=8)
    nc = len(m["types"])
    cv = np.zeros(nc, F32)
    pts = sh.select("points", 0.3, sh.WIDE)
    check(spray, m, pts)
    fails(spray, m, sh.select(7, 0.0, 1.0))                              # an unknown mode
    fails(spray, m, sh.select(-1, 0.0, 1.0))
    for mode, kw in (("points", {}), ("cells", dict(cell_values=cv))):
        fails(spray, m, sh.select(mode, 1.0, 0.5, **kw))                 # lo > hi
        fails(spray, m, sh.select(mode, np.nan, 1.0, **kw))
        fails(spray, m, sh.select(mode, 0.0, np.inf, **kw))
        fails(spray, m, sh.select(mode, -np.inf, 0.0, **kw))
    check(spray, m, sh.select("all", 1.0, np.nan))                       # bounds unread in mode ALL
    bare = {k: x for k, x in m.items() if k != "values"}
    fails(spray, bare, pts)                                              # a NULL array the mode reads
    fails(spray, m, sh.select("cells", 0.0, 1.0))
    check(spray, bare, None)                                             # values unread otherwise
    check(spray, bare, sh.select("cells", 0.0, 1.0, cv))
    for sel in (None, pts, sh.select("cells", 0.0, 1.0, cv)):
        fails(spray, poked(m, "types", 7, 11), sel)                      # an unknown type
        fails(spray, poked(m, "types", 7, ch.WEDGE), sel)                # offsets against the type
        fails(spray, poked(m, "offsets", 8, m["offsets"][8] + 1), sel)
        fails(spray, dict(m, conn=m["conn"][:-1]), sel)                  # offsets[i + 1] > nconn
        fails(spray, poked(m, "conn", 8 * 5 + 1, len(m["points"])), sel)   # an index >= npoints
        fails(spray, poked(m, "points", (3, 1), np.inf), sel)
        fails(spray, poked(m, "normals", (3, 2), np.nan), sel)
        fails(spray, poked(m, "cfield", 3, np.nan), sel)
        fails(spray, dict(m, cmap=None), sel)
        fails(spray, dict(m, cmap=(m["cmap"][0], 1.0, 1.0)), sel)
    fails(spray, poked(m, "values", 3, np.nan), pts)
    check(spray, poked(m, "values", 3, np.nan), None)                    # unread in mode ALL
    fails(spray, m, sh.select("cells", 0.0, 1.0, poked(dict(cv=cv), "cv", 2, np.nan)["cv"]))


def test_nan_at_a_dropped_cell_fails_and_an_unreferenced_one_passes(spray, ball):
    sel = sh.select("points", 0.0, 3.4)
    kept = sh.kept_cells(ball, sel)
    cells = ball["conn"].reshape(-1, 8)
    used = np.zeros(len(ball["points"]), bool)
    used[cells[kept].reshape(-1)] = True
    far = int(np.nonzero(~used)[0][-1])          # a point of dropped cells only
    assert (cells == far).any()
    fails(spray, poked(ball, "points", (far, 0), np.nan), sel)
    fails(spray, poked(ball, "normals", (far, 0), np.nan), sel)
    fails(spray, poked(ball, "values", far, np.nan), sel)
    fails(spray, poked(ball, "cfield", far, np.inf), sel)
    ref = check(spray, ball, sel)
    extra = dict(ball, points=np.vstack([ball["points"], [[np.nan] * 3]]).astype(F32),
                 values=np.append(ball["values"], F32(np.nan)),
                 cfield=np.append(ball["cfield"], F32(np.nan)),
                 normals=np.vstack([ball["normals"], [[np.nan] * 3]]).astype(F32))
    same(sh.host_surface(spray, extra, sel), ref)


def test_limits(spray):
    from spray_amd._native import CellMesh, lib
    L = lib()
    nv, nf = C.c_size_t(7), C.c_size_t(7)
    args = (None, None, C.byref(nv), C.byref(nf), None, None, None, None, None)
    rec = CellMesh()
    rec.npoints = 2 ** 21 + 1                     # with ncells == 0: nothing is read
    assert L.spray_rt_cell_surface_host(C.byref(rec), *args) == ERR_LIMIT
    rec.npoints = 2 ** 21
    assert L.spray_rt_cell_surface_host(C.byref(rec), *args) == 0 and nv.value == nf.value == 0
    dummy = np.zeros(16, np.uint32)
    rec.points = rec.types = rec.offsets = rec.conn = dummy.ctypes.data
    rec.npoints, rec.ncells, rec.nconn = 8, 2 ** 29, 8
    assert L.spray_rt_cell_surface_host(C.byref(rec), *args) == ERR_LIMIT
    rec.ncells, rec.nconn = 1, 2 ** 32
    assert L.spray_rt_cell_surface_host(C.byref(rec), *args) == ERR_LIMIT
    # a NULL array with cells, and normals asked of a mesh without them
    rec.nconn, rec.conn = 8, None
    assert L.spray_rt_cell_surface_host(C.byref(rec), *args) == ERR_ARG
    assert L.spray_rt_cell_surface_host(None, *args) == ERR_ARG
    m = sh.mesh(ch.one_cell(ch.HEX, 1))
    out = np.zeros((8, 3), F32)
    from spray_amd.engine import _surf_table
    arr, sarr, carr, keep = _surf_table([m], None)
    assert L.spray_rt_cell_surface_host(C.addressof(arr), None, None, C.byref(nv), C.byref(nf), None,
                                        out.ctypes.data, None, None, None) == ERR_ARG
    assert L.spray_rt_cell_surface_host(C.addressof(arr), None, None, C.byref(nv), C.byref(nf),
                                        out.ctypes.data, None, None, None, None) == 0
    assert (nv.value, nf.value) == (8, 12) and out.tobytes() == m["points"].tobytes()

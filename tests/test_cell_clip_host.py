"""The host restatement of the clip of cell meshes by a level of their scalar
field (spray_rt_cell_clip_host, spray_rt_plane_values_host; no GPU): every
array against the numpy restatement of clip_helpers byte for byte, and the
properties of the rule.
"""
import ctypes as C

import numpy as np
import pytest

import cell_helpers as ch
import clip_helpers as clh
import color_helpers as colh
import surface_helpers as sh
import tet_helpers as th

ERR_ARG, ERR_LIMIT = -1, -5
F32 = np.float32
TYPES = (ch.TET, ch.HEX, ch.WEDGE, ch.PYRAMID)


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


def check(spray, m, invert=False):
    """The host restatement equals numpy, with normals and without, twice; the
    cap is the cell isosurface's bytes; pairs and t are as the header says ->
    the eight results."""
    got = clh.host_clip(spray, m, invert)
    clh.assert_same(got, clh.clip_numpy(m, invert), "numpy")
    clh.assert_same(clh.host_clip(spray, m, invert), got, "twice")
    bare = clh.host_clip(spray, m, invert, normals=False)
    clh.assert_same(bare, (got[0], None) + got[2:], "bare")
    v, n, col, pairs, t, f, ncv, ncf = got
    iv, inr, icol, ifaces = ch.host_mesh(spray, m)
    assert (ncv, ncf) == (len(iv), len(ifaces))
    assert v[:ncv].tobytes() == iv.tobytes() and col[:ncv].tobytes() == icol.tobytes()
    if n is not None:
        assert n[:ncv].tobytes() == inr.tobytes()
    want = ifaces[:, [0, 2, 1]] if invert else ifaces
    assert f[:ncf].tobytes() == np.ascontiguousarray(want).tobytes()
    a, b = pairs[:ncv, 0].astype(np.int64), pairs[:ncv, 1].astype(np.int64)
    assert (a < b).all() and (np.diff((a << 32) | b) > 0).all()
    own = pairs[ncv:]
    assert (own[:, 0] == own[:, 1]).all() and (np.diff(own[:, 0].astype(np.int64)) > 0).all()
    assert (t[ncv:] == 0).all()
    assert v[ncv:].tobytes() == np.asarray(m["points"], F32)[own[:, 0]].tobytes()
    kept = (np.asarray(m["values"], F32) >= F32(m["iso"])) != bool(invert)
    assert kept[own[:, 0]].all()
    if len(f):
        assert f.max() < len(v) and set(np.unique(f[ncf:]).tolist()) >= set(range(ncv, len(v)))
    return got


def solid(got):
    """A closed, consistently oriented surface -> its volume."""
    v, f = got[0], got[5]
    sh.assert_closed_oriented(f)
    return sh.signed_volume(v, f)


def cell_volume(spray, m):
    tets = ch.host_tets(spray, m)
    return float(np.abs(ch.det6(m["points"], tets.astype(np.int64))).sum()) / 6.0


@pytest.mark.parametrize("ctype", TYPES)
def test_single_cells_over_renumberings(spray, ctype):
    npts = ch.NPOINTS[ctype]
    seeds = {}
    for seed in range(256):
        seeds.setdefault(list(ch.one_cell(ctype, seed)[3]).index(0), seed)
    assert set(seeds) == set(range(npts))   # the smallest index at every local position
    for seed in seeds.values():
        geom = ch.one_cell(ctype, seed)
        conn = geom[3]
        whole = None
        for corner in range(npts):
            for sign in (1.0, -1.0):        # the single corner kept, then dropped
                def f(p, corner=corner, sign=sign):
                    out = np.full(len(p), -sign)
                    out[conn[corner]] = sign
                    return out
                m = ch.mesh(geom, f, 0.0, normals=bool(seed & 1), cmap_seed=seed if seed & 2 else None,
                            ntable=16)
                a, b = check(spray, m), check(spray, m, True)
                for got in (a, b):
                    ch.assert_closed_manifold(got[5])
                    assert sh.euler(got[5]) == 2
                va, vb = solid(a), solid(b)
                whole = whole or cell_volume(spray, m)
                assert va > 0 and vb > 0 and abs(va + vb - whole) < 1e-6


def test_isovalue_below_every_value_is_the_boundary_surface(spray):
    for geom in (ch.hex_lattice((4, 4, 3), seed=9), sh.conforming_mesh(3), ch.mixed_mesh(3)):
        m = ch.mesh(geom, th.wave_f, -50.0, normals=True, cmap_seed=3, ntable=64)
        v, n, col, pairs, t, f, ncv, ncf = check(spray, m)
        sv, sn, scol, ids, sf = sh.host_surface(spray, m)
        assert ncv == ncf == 0
        assert v.tobytes() == sv.tobytes() and n.tobytes() == sn.tobytes()
        assert col.tobytes() == scol.tobytes() and f.tobytes() == sf.tobytes()
        assert (pairs[:, 0] == ids).all() and (pairs[:, 1] == ids).all()
        # and inverted nothing is left
        e = check(spray, m, True)
        assert len(e[0]) == len(e[5]) == 0


def test_empty_clips(spray):
    m = ch.mesh(ch.hex_lattice((4, 4, 3), seed=9), th.wave_f, 50.0, normals=True, color=7)
    got = check(spray, m)
    assert len(got[0]) == len(got[5]) == 0 and got[5].shape == (0, 3) and got[6:] == (0, 0)
    e = dict(m, types=m["types"][:0], offsets=m["offsets"][:1], conn=m["conn"][:0])
    for iso in (-50.0, 0.3, 50.0):
        for invert in (False, True):
            got = check(spray, dict(e, iso=iso), invert)
            assert len(got[0]) == len(got[5]) == 0


def test_lattice_cut_by_a_plane(spray):
    m = dict(clh.lattice_4(), normals=None)
    a, b = check(spray, m), check(spray, m, True)
    for got in (a, b):
        v, f, ncv, ncf = got[0], got[5], got[6], got[7]
        ch.assert_closed_manifold(f)
        sh.assert_closed_oriented(f)
        assert sh.euler(f) == 2
        assert sh.signed_volume(v, f) == 13.5     # every coordinate is a multiple of 0.5
        assert ncv > 0 and (v[:ncv, 0] == 1.5).all()
        assert (got[4][:ncv] == 0.5).all()
    assert (a[0][a[6]:, 0] > 1.5).all() and (b[0][b[6]:, 0] < 1.5).all()
    # the two caps: the same triples reversed
    ncf = a[7]
    assert ncf == b[7] and a[5][:ncf].tobytes() == b[5][:ncf][:, [0, 2, 1]].tobytes()


def test_sphere_inside_a_lattice(spray):
    m = clh.sphere_9(seed=5)
    v, n, col, pairs, t, f, ncv, ncf = a = check(spray, m)
    assert len(v) == ncv and len(f) == ncf and ncf > 100      # the skin is empty
    ch.assert_closed_manifold(f)
    assert sh.euler(f) == 2
    inner = solid(a)
    b = check(spray, m, True)
    ch.assert_closed_manifold(b[5])
    assert clh.components(b[5]) == 2 and sh.euler(b[5]) == 4
    outer = solid(b)
    assert 0 < inner < outer and abs(inner + outer - 512.0) < 1e-8
    # the cap triangles cancel pairwise
    fwd = sorted(map(tuple, a[5][:ncf].tolist()))
    back = sorted(map(tuple, b[5][:ncf][:, [0, 2, 1]].tolist()))
    assert fwd == back
    # the outer skin is the whole box
    sv = sh.host_surface(spray, m)[0]
    assert len(b[0]) - ncv == len(sv)


@pytest.mark.parametrize("seed", [3, 11, None])
def test_conforming_mixed_mesh_cut_through_its_middle(spray, seed):
    plane = lambda p: ((p[..., 0] - 1.1) + 0.3 * (p[..., 1] - 1.0) + 0.2 * (p[..., 2] - 1.0)).astype(np.float64)
    m = ch.mesh(sh.conforming_mesh(seed), plane, 0.0, normals=True, color=0x00102030)
    assert set(m["types"].tolist()) == {ch.HEX, ch.WEDGE, ch.PYRAMID}
    a, b = check(spray, m), check(spray, m, True)
    for got in (a, b):
        ch.assert_closed_manifold(got[5])
        assert sh.euler(got[5]) == 2 and (got[2] == 0x00102030).all()
    va, vb = solid(a), solid(b)
    assert va > 0 and vb > 0 and abs(va + vb - 32.0) < 1e-8


def test_mixed_meshes_bytes(spray):
    for seed in (3, 11):
        m = ch.mesh(ch.mixed_mesh(seed), ch.sphere((1.0, 0.7, 0.8), 1.7), 0.0, normals=True,
                    cmap_seed=8, ntable=32)
        assert set(m["types"].tolist()) == {ch.TET, ch.HEX, ch.WEDGE, ch.PYRAMID}
        check(spray, m)
        check(spray, m, True)
    for through_min in (True, False):
        for seed in (None, 1, 2, 3):
            m = ch.mesh(sh.cut_quad_mesh(through_min, seed), ch.sphere((0.4, 0.6, 0.1), 0.9), 0.0,
                        normals=True)
            check(spray, m)
            check(spray, m, True)


def test_value_equal_to_the_isovalue(spray):
    geom = ch.hex_lattice((4, 4, 4), seed=6)
    f = lambda p: np.rint(p[..., 0].astype(np.float64)) - 1.0     # x == 1 is on the level
    m = ch.mesh(geom, f, 0.0, normals=True, cmap_seed=2, ntable=16)
    for invert in (False, True):
        got = check(spray, m, invert)
        v, t, faces, ncv = got[0], got[4], got[5], got[6]
        assert ncv > 0 and set(np.unique(t[:ncv]).tolist()) <= {0.0, 1.0}
        assert (v[:ncv, 0] == 1.0).all()
        sh.assert_closed_oriented(faces)          # combinatorially closed all the same
        tri = v[faces].astype(np.float64)
        area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        assert (area == 0).any() if not invert else True
        assert sh.signed_volume(v, faces) == (18.0 if not invert else 9.0)


def test_duplicate_and_collapsed_cells(spray):
    p, types, offsets, conn = ch.hex_lattice((3, 2, 2), seed=4)
    two = conn.reshape(2, 8)
    f = lambda q: th.wave_f(q) - 1.9
    m = ch.mesh((p,) + ch.cells([ch.HEX] * 3, [two[0], two[0], two[1]]), f, 0.0, normals=True)
    assert 0 < (m["values"] >= 0).sum() < len(p)
    check(spray, m)
    check(spray, m, True)
    p, types, offsets, conn = ch.one_cell(ch.HEX, 6)
    for a, b in ((1, 0), (6, 2), (7, 4)):
        c2 = conn.copy()
        c2[a] = c2[b]
        for g in (ch.sphere((0.3, 0.2, 0.1), 0.8), ch.sphere((0.9, 0.8, 0.7), 0.9)):
            m = ch.mesh((p, types, offsets, c2), g, 0.0, normals=True)
            check(spray, m)
            check(spray, m, True)


@pytest.mark.parametrize("ntable", [1, 4096])
def test_colour_maps(spray, ntable):
    geom = ch.hex_lattice((5, 4, 4), seed=1)
    m = ch.mesh(geom, th.wave_f, 0.3, normals=True, cmap_seed=17, ntable=ntable, clamp=0.4)
    col = check(spray, m)[2]
    assert len(col) > 0 and (len(np.unique(col)) == 1 if ntable == 1 else len(np.unique(col)) > 4)
    check(spray, m, True)
    plain = ch.mesh(geom, th.wave_f, 0.3)
    assert (check(spray, plain)[2] == 0).all()          # no colour: zeros
    const = ch.mesh(geom, th.wave_f, 0.3, color=0x00ABCDEF)
    assert (check(spray, const, True)[2] == 0x00ABCDEF).all()


def test_recolouring_through_pairs_and_t(spray):
    m = ch.mesh(ch.hex_lattice((5, 4, 4), seed=1), th.wave_f, 0.3, cmap_seed=17, ntable=4096)
    for invert in (False, True):
        v, n, col, pairs, t, f, ncv, ncf = check(spray, m, invert)
        h = np.asarray(m["cfield"], F32)
        a, b = pairs[:, 0], pairs[:, 1]
        g = (h[a] + (t * (h[b] - h[a]).astype(F32)).astype(F32)).astype(F32)
        table, lo, hi = m["cmap"]
        assert spray.colormap_host(g, table, lo, hi).tobytes() == col.tobytes()
        assert colh.colormap_numpy(g, table, lo, hi).astype(np.uint32).tobytes() == col.tobytes()


# ---- errors ----
def fails(spray, m, code=ERR_ARG):
    for invert in (False, True):
        with pytest.raises(spray.SprayRtError) as e:
            clh.host_clip(spray, m, invert)
        assert e.value.code == code


def poked(m, key, index, value):
    a = np.array(m[key], copy=True)
    a[index] = value
    return dict(m, **{key: a})


def test_argument_errors(spray):
    geom = ch.hex_lattice((5, 4, 3), seed=12)
    m = ch.mesh(geom, th.wave_f, 0.3, normals=True, cmap_seed=5, ntable=8)
    check(spray, m)
    fails(spray, dict(m, iso=np.nan))
    fails(spray, dict(m, iso=np.inf))
    fails(spray, poked(m, "types", 7, 11))                      # an unknown type
    fails(spray, poked(m, "types", 7, ch.WEDGE))                # offsets against the type
    fails(spray, poked(m, "offsets", 8, m["offsets"][8] + 1))
    fails(spray, dict(m, conn=m["conn"][:-1]))                  # offsets[i + 1] > nconn
    fails(spray, poked(m, "conn", 8 * 5 + 1, len(m["points"])))   # an index >= npoints
    fails(spray, poked(m, "points", (3, 1), np.inf))
    fails(spray, poked(m, "normals", (3, 2), np.nan))
    fails(spray, poked(m, "cfield", 3, np.nan))
    fails(spray, poked(m, "values", 3, np.nan))
    fails(spray, dict(m, cmap=None))
    fails(spray, dict(m, cmap=(m["cmap"][0], 1.0, 1.0)))


def test_nan_at_a_cell_without_a_kept_point_fails_and_an_unreferenced_one_passes(spray):
    m = ch.mesh(ch.hex_lattice((6, 5, 5), seed=5), clh.x_minus(3.5), 0.0, normals=True,
                cmap_seed=21, ntable=64)
    cells = m["conn"].reshape(-1, 8)
    kept = m["values"] >= 0
    part = kept[cells].any(1)
    used = np.zeros(len(m["points"]), bool)
    used[cells[part].reshape(-1)] = True
    far = int(np.nonzero(~used)[0][-1])          # a point of cells without a kept point only
    assert (cells == far).any() and 0 < part.sum() < len(part)
    with pytest.raises(spray.SprayRtError) as e:
        clh.host_clip(spray, poked(m, "points", (far, 0), np.nan))
    assert e.value.code == ERR_ARG
    for key, idx in (("normals", (far, 0)), ("values", far), ("cfield", far)):
        with pytest.raises(spray.SprayRtError) as e:
            clh.host_clip(spray, poked(m, key, idx, np.nan))
        assert e.value.code == ERR_ARG
    ref = check(spray, m)
    extra = dict(m, points=np.vstack([m["points"], [[np.nan] * 3]]).astype(F32),
                 values=np.append(m["values"], F32(np.nan)),
                 cfield=np.append(m["cfield"], F32(np.nan)),
                 normals=np.vstack([m["normals"], [[np.nan] * 3]]).astype(F32))
    clh.assert_same(clh.host_clip(spray, extra), ref)


def test_limits(spray):
    from spray_amd._native import CellMesh, lib
    from spray_amd.engine import _cell_table
    L = lib()
    counts = [C.c_size_t(7) for _ in range(4)]
    refs = [C.byref(x) for x in counts]
    args = (0, None, *refs, None, None, None, None, None, None)
    rec = CellMesh()
    rec.npoints = 2 ** 21 + 1                     # with ncells == 0: nothing is read
    assert L.spray_rt_cell_clip_host(C.byref(rec), *args) == ERR_LIMIT
    rec.npoints = 2 ** 21
    assert L.spray_rt_cell_clip_host(C.byref(rec), *args) == 0
    assert [x.value for x in counts] == [0, 0, 0, 0]
    dummy = np.zeros(16, np.uint32)
    rec.points = rec.types = rec.offsets = rec.conn = rec.values = dummy.ctypes.data
    rec.npoints, rec.ncells, rec.nconn = 8, 2 ** 29, 8
    assert L.spray_rt_cell_clip_host(C.byref(rec), *args) == ERR_LIMIT
    rec.ncells, rec.nconn = 1, 2 ** 32
    assert L.spray_rt_cell_clip_host(C.byref(rec), *args) == ERR_LIMIT
    # a NULL array with cells (values among them), and normals asked of a mesh without them
    rec.nconn, rec.conn = 8, None
    assert L.spray_rt_cell_clip_host(C.byref(rec), *args) == ERR_ARG
    rec.conn, rec.values = dummy.ctypes.data, None
    assert L.spray_rt_cell_clip_host(C.byref(rec), *args) == ERR_ARG
    assert L.spray_rt_cell_clip_host(None, *args) == ERR_ARG
    m = ch.mesh(ch.one_cell(ch.HEX, 1), th.wave_f, -50.0)
    out = np.zeros((8, 3), F32)
    arr, carr, keep = _cell_table([m])
    assert L.spray_rt_cell_clip_host(C.addressof(arr), 0, None, *refs, None, out.ctypes.data, None,
                                     None, None, None) == ERR_ARG
    assert L.spray_rt_cell_clip_host(C.addressof(arr), 0, None, *refs, out.ctypes.data, None, None,
                                     None, None, None) == 0
    assert [x.value for x in counts] == [8, 12, 0, 0] and out.tobytes() == m["points"].tobytes()


# ---- plane values ----
def test_plane_values(spray):
    rng = np.random.default_rng(4)
    pts = (rng.normal(size=(1000, 3)) * 7).astype(F32)
    for origin, normal in (((0, 0, 0), (1, 0, 0)), ((0.3, -1.7, 2.9), (0.2, -0.9, 0.4)),
                           ((1e3, 2.5, -3), (0, 0, -2.5))):
        got = spray.plane_values_host(pts, origin, normal)
        assert got.dtype == F32 and got.tobytes() == clh.plane_numpy(pts, origin, normal).tobytes()
    assert len(spray.plane_values_host(np.zeros((0, 3), F32), (0, 0, 0), (0, 0, 1))) == 0
    for origin, normal in (((np.nan, 0, 0), (1, 0, 0)), ((0, 0, 0), (0, np.inf, 0)),
                           ((0, 0, 0), (0, 0, 0)), ((0, -np.inf, 0), (0, 1, 0))):
        with pytest.raises(spray.SprayRtError) as e:
            spray.plane_values_host(pts, origin, normal)
        assert e.value.code == ERR_ARG
    from spray_amd._native import lib
    o = np.array([0, 0, 0, 1, 0, 0], F32)
    out = np.zeros(4, F32)
    L = lib()
    assert L.spray_rt_plane_values_host(None, 4, o.ctypes.data, o[3:].ctypes.data,
                                        out.ctypes.data) == ERR_ARG
    assert L.spray_rt_plane_values_host(pts.ctypes.data, 4, o.ctypes.data, o[3:].ctypes.data,
                                        None) == ERR_ARG
    assert L.spray_rt_plane_values_host(None, 0, o.ctypes.data, o[3:].ctypes.data, None) == 0


def test_slice_and_clip_by_a_plane(spray):
    m = clh.lattice_4()
    vals = spray.plane_values_host(m["points"], (1.5, 0, 0), (1, 0, 0))
    assert vals.tobytes() == m["values"].tobytes()
    m = dict(m, values=vals)
    v, n, col, f = ch.host_mesh(spray, m)
    assert len(v) > 0 and (v[:, 0] == 1.5).all()
    got = check(spray, m)
    assert sh.signed_volume(got[0], got[5]) == 13.5

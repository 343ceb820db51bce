"""Host restatement of the isosurface extraction (spray_rt_isosurface_host, no GPU).

Marching tetrahedra over the Kuhn split, vertices numbered by (point, edge
type) and faces by (cell, tetrahedron, triangle).  Checked here against an
independent numpy restatement (iso_helpers.isosurface_numpy) byte for byte and
structurally; the GPU tests then hold the kernels to this function.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import iso_helpers as ih

ERR_ARG = -1


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


def host(spray, g, normals=True):
    return spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"], normals)


def offset_grid():
    """Origin and spacing that are not 0 and 1."""
    p = ih.lattice((7, 6, 5), (1.5, -2.25, 0.3), (0.5, 0.7, 1.3))
    f = np.sin(1.1 * p[..., 0]) + np.cos(0.9 * p[..., 1]) * p[..., 2] * 0.3
    return ih.grid(f, (1.5, -2.25, 0.3), (0.5, 0.7, 1.3), iso=0.15)


def plane_grid():
    """f = x, contoured on the lattice plane x = 2: every crossing has t = 1."""
    return ih.grid(ih.lattice((5, 4, 3))[..., 0], iso=2.0)


GRIDS = {
    "cell": lambda: ih.ramp_grid((2, 2, 2), 0.0, 1),
    "strides": lambda: ih.ramp_grid((5, 4, 3), 0.1, 2),
    "sphere": ih.sphere_grid,
    "torus": ih.torus_grid,
    "offset": offset_grid,
    "plane": plane_grid,
}
CLOSED = {"sphere": (2, ih.sphere_grad), "torus": (0, ih.torus_grad)}


@pytest.fixture(scope="module")
def grids():
    return {k: make() for k, make in GRIDS.items()}


@pytest.fixture(scope="module")
def meshes(spray, grids):
    return {k: host(spray, g) for k, g in grids.items()}


@pytest.mark.parametrize("name", list(GRIDS))
def test_equals_the_numpy_restatement(grids, meshes, name):
    g = grids[name]
    v, n, f = meshes[name]
    rv, rn, rf = ih.isosurface_numpy(g["values"], g["origin"], g["spacing"], g["iso"])
    assert len(f) > 0
    assert v.tobytes() == rv.tobytes()
    assert f.tobytes() == rf.tobytes()
    assert n.tobytes() == rn.tobytes()


def test_sphere_counts(meshes):
    v, _, f = meshes["sphere"]
    assert (len(v), len(f)) == (302, 600)


@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_oriented_surfaces(grids, meshes, name):
    euler, grad = CLOSED[name]
    v, n, f = meshes[name]
    assert not (grids[name]["values"] == 0).any()
    ih.assert_closed_oriented(f, len(v), euler)
    ng = ih.geometric_normals(v, f)
    assert (np.linalg.norm(ng, axis=1) > 0).all()
    # winding: Ng leaves the region f >= iso
    centroid = v[f].astype(np.float64).mean(1)
    assert ((ng * grad(centroid)).sum(1) < 0).all()
    # the vertex normals point the same way
    assert ((n[f[:, 0]].astype(np.float64) * ng).sum(1) > 0).all()


@pytest.mark.parametrize("name", list(GRIDS))
def test_vertices_lie_on_crossing_lattice_edges(grids, meshes, name):
    g = grids[name]
    f = g["values"]
    nz, ny, nx = f.shape
    o, s = np.asarray(g["origin"], np.float64), np.asarray(g["spacing"], np.float64)
    v = meshes[name][0].astype(np.float64)
    n = 0
    for k, j, i in itertools.product(range(nz), range(ny), range(nx)):
        for dx, dy, dz in ih.EDGE:
            if i + dx >= nx or j + dy >= ny or k + dz >= nz:
                continue
            a, b = f[k, j, i], f[k + dz, j + dy, i + dx]
            if (a >= g["iso"]) == (b >= g["iso"]):
                continue
            pa = o + np.array([i, j, k]) * s
            d = np.array([dx, dy, dz]) * s
            t = (v[n] - pa) @ d / (d @ d)
            assert -1e-6 <= t <= 1 + 1e-6
            assert np.abs(pa + t * d - v[n]).max() < 1e-5
            n += 1
    assert n == len(v)


@pytest.mark.parametrize("name", list(GRIDS))
def test_sizes_and_bounds(spray, grids, meshes, name):
    from spray_amd import _native, engine
    g = grids[name]
    v, _, f = meshes[name]
    arr, keep = engine._grid_table([g])
    nv, nf = C.c_size_t(), C.c_size_t()
    rc = _native.lib().spray_rt_isosurface_host(C.addressof(arr), C.byref(nv), C.byref(nf),
                                                None, None, None)
    assert rc == 0 and (nv.value, nf.value) == (len(v), len(f))
    assert f.max() < len(v)
    assert np.array_equal(np.unique(f), np.arange(len(v)))  # every vertex is referenced
    # without normals: the same positions and faces
    v2, n2, f2 = host(spray, g, normals=False)
    assert n2 is None and v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()


def test_two_runs_give_the_same_bytes(spray, grids, meshes):
    for name in ("torus", "offset"):
        again = host(spray, grids[name])
        for a, b in zip(again, meshes[name]):
            assert a.tobytes() == b.tobytes()


def test_one_cell(meshes):
    v, _, f = meshes["cell"]
    assert 0 < len(f) <= 12 and len(v) <= 19


def test_empty_surface(spray, grids):
    g = dict(grids["sphere"], iso=float(grids["sphere"]["values"].max()) + 1.0)
    v, n, f = host(spray, g)
    assert v.shape == (0, 3) and n.shape == (0, 3) and f.shape == (0, 3)


def test_plane_on_a_lattice_plane(spray, meshes):
    v, n, f = meshes["plane"]
    assert np.isfinite(v).all() and np.isfinite(n).all()
    assert (v[:, 0] == 2.0).all()          # every vertex sits on the lattice plane
    ng = ih.geometric_normals(v, f)
    assert (np.linalg.norm(ng, axis=1) == 0).any()   # zero-area triangles are kept ...
    assert (ng[:, 0] <= 0).all() and (ng[:, 0] < 0).any()   # ... the others face decreasing x
    b = spray.bvh_build_device_host(v, f)  # ... and the device build accepts them
    assert len(b["prims"]) == len(f)


def test_shared_sample_plane_is_bitwise_equal(spray):
    o, s = (1.0, 2.0, -1.0), (0.5, 0.75, 1.25)
    p = ih.lattice((9, 6, 5), o, s)
    f = np.sin(1.3 * p[..., 0] + 0.4) * np.cos(0.8 * p[..., 1]) + 0.21 * p[..., 2]
    left = ih.grid(f[:, :, :5], o, s, iso=0.1)
    x_shared = np.float32(o[0]) + np.float32(4) * np.float32(s[0])
    right = ih.grid(f[:, :, 4:], (float(x_shared), o[1], o[2]), s, iso=0.1)
    va, vb = host(spray, left)[0], host(spray, right)[0]
    on_a, on_b = va[va[:, 0] == x_shared], vb[vb[:, 0] == x_shared]
    assert len(on_a) > 4
    key = lambda a: sorted(r.tobytes() for r in a)
    assert key(on_a) == key(on_b)


def test_errors(spray, grids):
    g = grids["strides"]

    def fails(values, spacing=(1, 1, 1)):
        with pytest.raises(spray.SprayRtError) as e:
            spray.isosurface_host(values, g["origin"], spacing, g["iso"])
        assert e.value.code == ERR_ARG

    nan = g["values"].copy()
    nan[1, 2, 3] = np.nan
    fails(nan)
    fails(g["values"][:, :, :1])           # dims < 2
    fails(g["values"], (1.0, 0.0, 1.0))    # zero spacing
    fails(g["values"], (1.0, np.inf, 1.0))

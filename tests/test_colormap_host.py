"""Host restatements of the colour map (spray_rt_isosurface_mapped_host,
spray_rt_colormap_host, no GPU).

Checked against an independent numpy restatement (color_helpers) byte for byte,
against spray_rt_isosurface_host for the geometry, and against answers worked
out on paper; the GPU tests then hold the kernels to these functions.
"""
import numpy as np
import pytest

import color_helpers as ch
import iso_helpers as ih

ERR_ARG = -1
F32 = np.float32


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


def offset_grid():
    p = ih.lattice((7, 6, 5), (1.5, -2.25, 0.3), (0.5, 0.7, 1.3))
    f = np.sin(1.1 * p[..., 0]) + np.cos(0.9 * p[..., 1]) * p[..., 2] * 0.3
    return ih.grid(f, (1.5, -2.25, 0.3), (0.5, 0.7, 1.3), iso=0.15)


GRIDS = {
    "cell": lambda: ch.mapped(ih.ramp_grid((2, 2, 2), 0.0, 1), 1, 5),
    "strides": lambda: ch.mapped(ih.ramp_grid((5, 4, 3), 0.1, 2), 2, 1),
    "sphere": lambda: ch.mapped(ih.sphere_grid(), 3, 256, 0.5),
    "torus": lambda: ch.mapped(ih.torus_grid(), 4, 4096, 0.9),
    "offset": lambda: ch.mapped(offset_grid(), 5, 33),
}


@pytest.fixture(scope="module")
def grids():
    return {k: make() for k, make in GRIDS.items()}


@pytest.fixture(scope="module")
def meshes(spray, grids):
    return {k: ch.host_mesh(spray, g) for k, g in grids.items()}


@pytest.mark.parametrize("name", list(GRIDS))
def test_colors_equal_the_numpy_restatement(grids, meshes, name):
    col = meshes[name][2]
    ref = ch.vertex_colors_numpy(grids[name])
    assert len(col) > 0 and col.dtype == np.uint32
    assert col.tobytes() == ref.tobytes()
    table = grids[name]["cmap"][0]
    assert np.isin(col, table).all()
    if len(table) > 1:
        assert len(np.unique(col)) > 1      # not one bin


@pytest.mark.parametrize("name", list(GRIDS))
def test_geometry_is_the_unmapped_extraction(spray, grids, meshes, name):
    g = grids[name]
    v, n, _, f = meshes[name]
    v0, n0, f0 = spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"])
    assert (v.tobytes(), n.tobytes(), f.tobytes()) == (v0.tobytes(), n0.tobytes(), f0.tobytes())
    v1, n1, c1, f1 = ch.host_mesh(spray, g, normals=False)
    assert n1 is None and c1.tobytes() == meshes[name][2].tobytes()
    assert (v1.tobytes(), f1.tobytes()) == (v0.tobytes(), f0.tobytes())


def test_binning_edges_exact(spray):
    """Maps whose scale is a power of two: every product is exact."""
    t8 = ch.table(8, 1)
    up, down = lambda x: np.nextafter(F32(x), F32(np.inf)), lambda x: np.nextafter(F32(x), F32(-np.inf))
    g = np.array([0, 8, -1, 9, -1e30, 1e30, down(0), up(0), down(8), up(8),
                  3, down(3), up(3), 7, down(7), up(7), 1, down(1)], F32)
    want = [0, 7, 0, 7, 0, 7, 0, 0, 7, 7, 3, 2, 3, 7, 6, 7, 1, 0]
    assert spray.colormap_host(g, t8, 0.0, 8.0).tolist() == t8[want].tolist()
    # lo = -1.5, hi = 2.5, n = 16: scale 4, bin edges at lo + k / 4
    t16 = ch.table(16, 2)
    edges = (F32(-1.5) + np.arange(17, dtype=F32) * F32(0.25)).astype(F32)
    assert spray.colormap_host(edges, t16, -1.5, 2.5).tolist() == \
        t16[np.minimum(np.arange(17), 15)].tolist()
    # (one ulp below an edge, g - lo may round back onto it: test_binning_equals_numpy)
    # one entry: everything is that entry
    t1 = ch.table(1, 3)
    assert (spray.colormap_host(g, t1, 0.0, 8.0) == t1[0]).all()


@pytest.mark.parametrize("n", [1, 2, 7, 100, 4095, 4096])
def test_binning_equals_numpy(spray, n):
    lo, hi = F32(-0.37), F32(2.91)
    tab = ch.table(n, n)
    scale = ch.map_scale(n, lo, hi)
    k = np.unique(np.linspace(0, n, min(n, 64) + 1).astype(np.int64))
    edge = (lo + (k.astype(F32) / scale).astype(F32)).astype(F32)   # about the bin edges
    near = [edge]
    for _ in range(3):
        near += [np.nextafter(near[-1], F32(np.inf))]
    for _ in range(3):
        near += [np.nextafter(near[0 if len(near) == 4 else -1], F32(-np.inf))]
    rng = np.random.default_rng(n)
    g = np.concatenate(near + [np.array([lo, hi, lo - 1, hi + 1, -3e38, 3e38], F32),
                               rng.uniform(lo - 1, hi + 1, 500).astype(F32)])
    got = spray.colormap_host(g, tab, lo, hi)
    assert got.tobytes() == ch.colormap_numpy(g, tab, lo, hi).tobytes()
    assert got[len(g) - 506] == tab[0] and got[len(g) - 505] == tab[n - 1]   # lo, hi themselves
    if n >= 7:
        assert len(np.unique(got)) >= min(n, 7)


def test_difference_overflows_to_infinity(spray):
    tab = ch.table(4096, 7)
    big = F32(3e38)
    # g - lo = +inf: the last bin; -inf: the first
    assert spray.colormap_host(np.array([big], F32), tab, -big, -1e38)[0] == tab[4095]
    assert spray.colormap_host(np.array([-big], F32), tab, big, 3.2e38)[0] == tab[0]


def test_slice_known_answer(spray):
    """values = k - 3.5 contoured at 0, coloured by g = k through 8 bins over
    [0, 8]: every vertex has t = 0.5 and g = 3.5 exactly, so colour table[3]."""
    k = np.arange(8, dtype=F32)[:, None, None] * np.ones((8, 8, 8), F32)
    tab = ch.table(8, 11)
    assert len(set(tab.tolist())) == 8
    v, n, col, f = spray.isosurface_mapped_host(k - F32(3.5), (0, 0, 0), (1, 1, 1), 0.0, k,
                                                (tab, 0.0, 8.0))
    assert len(col) == len(v) > 49 and len(f) > 0
    assert (v[:, 2] == 3.5).all()
    assert (col == tab[3]).all()


def test_shared_sample_plane_gives_the_same_colors(spray):
    o, s = (1.0, 2.0, -1.0), (0.5, 0.75, 1.25)
    p = ih.lattice((9, 6, 5), o, s)
    f = np.sin(1.3 * p[..., 0] + 0.4) * np.cos(0.8 * p[..., 1]) + 0.21 * p[..., 2]
    whole = ih.grid(f, o, s, iso=0.1)
    cf = ch.color_field(whole, 9)
    cmap = (ch.table(64, 9), float(cf.min()), float(cf.max()))
    x_shared = F32(o[0]) + F32(4) * F32(s[0])
    left = dict(ih.grid(f[:, :, :5], o, s, iso=0.1), cfield=cf[:, :, :5], cmap=cmap)
    right = dict(ih.grid(f[:, :, 4:], (float(x_shared), o[1], o[2]), s, iso=0.1),
                 cfield=cf[:, :, 4:], cmap=cmap)
    va, _, ca, _ = ch.host_mesh(spray, left)
    vb, _, cb, _ = ch.host_mesh(spray, right)
    key = lambda v, c: sorted((r.tobytes(), int(k)) for r, k in zip(v, c) if r[0] == x_shared)
    assert len(key(va, ca)) > 4 and len({k for _, k in key(va, ca)}) > 1
    assert key(va, ca) == key(vb, cb)


def test_no_field_keeps_the_constant_color(spray, grids):
    g = grids["sphere"]
    nv = len(ch.host_mesh(spray, g)[0])
    plain = dict(g, cfield=None, cmap=None, color=0x00A1B2C3)
    assert (ch.host_mesh(spray, plain)[2] == 0x00A1B2C3).all()
    assert len(ch.host_mesh(spray, plain)[2]) == nv
    # a map without a field is not read: the constant colour again
    assert (ch.host_mesh(spray, dict(plain, cmap=(ch.table(4, 1), 1.0, 0.0)))[2] == 0x00A1B2C3).all()
    # and a field overrides the constant colour
    assert ch.host_mesh(spray, dict(g, color=0x00A1B2C3))[2].tobytes() == \
        ch.host_mesh(spray, g)[2].tobytes()


def test_two_runs_give_the_same_bytes(spray, grids, meshes):
    for name in ("torus", "offset"):
        again = ch.host_mesh(spray, grids[name])
        for a, b in zip(again, meshes[name]):
            assert a.tobytes() == b.tobytes()


BAD_MAPS = {
    "empty table": (np.zeros(0, np.uint32), 0.0, 1.0),
    "4097 entries": (np.zeros(4097, np.uint32), 0.0, 1.0),
    "lo == hi": (ch.table(4, 1), 1.0, 1.0),
    "lo > hi": (ch.table(4, 1), 2.0, 1.0),
    "nan lo": (ch.table(4, 1), np.nan, 1.0),
    "inf hi": (ch.table(4, 1), 0.0, np.inf),
    "hi - lo overflows": (ch.table(4, 1), -3e38, 3e38),       # scale 0
    "scale overflows": (ch.table(4096, 1), 0.0, 1e-45),
    "subnormal scale": (ch.table(1, 1), -1e38, 1e38),
}


@pytest.mark.parametrize("name", list(BAD_MAPS))
def test_bad_maps(spray, grids, name):
    g = grids["strides"]
    with pytest.raises(spray.SprayRtError) as e:
        ch.host_mesh(spray, dict(g, cmap=BAD_MAPS[name]))
    assert e.value.code == ERR_ARG
    with pytest.raises(spray.SprayRtError) as e:
        spray.colormap_host(np.zeros(3, F32), *BAD_MAPS[name])
    assert e.value.code == ERR_ARG


def test_errors(spray, grids):
    g = grids["strides"]

    def fails(**kw):
        with pytest.raises(spray.SprayRtError) as e:
            ch.host_mesh(spray, dict(g, **kw))
        assert e.value.code == ERR_ARG

    fails(cmap=None)                                  # a field without a table
    for bad in (np.nan, np.inf, -np.inf):
        cf = g["cfield"].copy()
        cf[1, 2, 3] = bad
        fails(cfield=cf)
        with pytest.raises(spray.SprayRtError) as e:
            spray.colormap_host(np.array([0.5, bad], F32), ch.table(4, 1), 0.0, 1.0)
        assert e.value.code == ERR_ARG
    nan = g["values"].copy()
    nan[1, 2, 3] = np.nan
    fails(values=nan)                                 # the neighbours' errors stay
    with pytest.raises(ValueError):
        ch.host_mesh(spray, dict(g, cfield=g["cfield"][:, :, :2]))   # another shape

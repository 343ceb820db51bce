"""The hard mesh classes of mesh_cases.py on the CPU (no GPU): the host
restatements of the five extractions equal the numpy restatements byte for byte
on every class, the outputs are finite, and every class reaches the path it
exists for.  The path facts are computed from the inputs and the numpy side,
never from the code under test.
"""
import numpy as np
import pytest

import cell_helpers as ch
import clip_helpers as clh
import iso_helpers as ih
import mesh_cases as mc
import surface_helpers as sh
import tet_helpers as th
from test_cell_clip_host import check as clip_check
from test_cell_surface_host import check as surface_check

F32 = np.float32
TINY = float(np.finfo(F32).tiny)


@pytest.fixture(scope="module")
def spray():
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def fans():
    return mc.fans()


@pytest.fixture(scope="module")
def collapsed():
    return mc.collapsed()


def same(got, ref, what):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert (g is None) == (r is None), what
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes(), what


def finite(arrays, what):
    for a in arrays:
        if a is not None and np.asarray(a).dtype.kind == "f":
            assert np.isfinite(a).all(), what


def check_cells(spray, m):
    """Cell isosurface, both clips and the three surfaces of a case against
    numpy -> the two clips."""
    name = m["name"]
    got = ch.host_mesh(spray, m)
    same(got, ch.cell_isosurface_numpy(m), name)
    finite(got, name)
    clips = [clip_check(spray, m, invert) for invert in (False, True)]
    for c in clips:
        finite(c[:6], name)
    for sel in mc.selects(m):
        finite(surface_check(spray, m, sel), name)
    return clips


def check_tets(spray, t):
    got = th.host_mesh(spray, t)
    same(got, th.tet_isosurface_numpy(t), t["name"])
    finite(got, t["name"])
    return got


def check_grid(spray, g):
    """The structured extraction of a grid against numpy -> (verts, normals, faces)."""
    got = spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"])
    same(got, ih.isosurface_numpy(g["values"], g["origin"], g["spacing"], g["iso"]), g["name"])
    bare = spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"], normals=False)
    assert bare[0].tobytes() == got[0].tobytes() and bare[2].tobytes() == got[2].tobytes()
    finite(got, g["name"])
    return got


# ---- topology classes ----
def test_fans_reach_long_runs_and_clip_to_closed_halves(spray, fans):
    assert len(fans) == 13 and sum(m["crossing"] for m in fans) == 12
    assert {(int(m["types"][0]), m["half"], m["place"]) for m in fans if m["crossing"]} == {
        (t, h, p) for t in (ch.TET, ch.WEDGE) for h in (False, True)
        for p in ("lowest", "highest", "middle")}
    for m in fans:
        a, b = m["ab"]
        n = len(m["points"])
        assert (a, b) == {"lowest": (0, 1), "highest": (n - 2, n - 1)}.get(m["place"], (a, a + 1))
        assert 1 < a < n - 3 or m["place"] != "middle"
        assert len(m["types"]) == mc.NFAN
        keys = mc.crossing_keys(m)
        starts, lengths = mc.runs(keys)
        if not m["crossing"]:
            assert lengths.max() < 16           # the control: short runs only
            assert ((a << 32) | b) not in keys
        else:
            k = int(np.argmax(lengths))
            assert lengths[k] >= 640 and keys[starts[k]] == (a << 32) | b
            # an aligned block of 256 instances inside the run, past its first
            first = (starts[k] // 256 + 1) * 256
            assert starts[k] < first and first + 256 <= starts[k] + lengths[k]
            assert len(np.unique(keys[first - 1:first + 256])) == 1
        kept = np.asarray(m["values"]) >= 0
        if m["half"] and m["crossing"]:
            skin = clh.skin_triangles(m, np.ones(len(m["types"]), bool))
            on_ab = ((skin == a).any(1) & (skin == b).any(1)).sum()
            assert on_ab >= 2 and kept[a] != kept[b]   # skin triangles cut on (a, b)
        clips = check_cells(spray, m)
        # closed, oriented, and the two sides fill the fan.  The cap vertices
        # are the same bytes on both sides, so the caps cancel; a skin piece
        # with a cut corner differs from the exact piece by a sliver.  A cap
        # vertex is three float32 roundings of coordinates at most 1 from its
        # edge on each axis, less than 2^-22 in all; the piece's other edges
        # are shorter than 1.5, so a sliver is below 1.5 * 1.5 * 2^-22 / 6, and
        # a piece has at most two cut corners: 2^-22 per piece bounds it.
        whole = float(np.abs(ch.det6(m["points"], ch.split_numpy(m).astype(np.int64))).sum()) / 6
        vol, pieces = 0.0, 0
        for c in clips:
            sh.assert_closed_oriented(c[5])
            v = sh.signed_volume(c[0], c[5])
            assert v > 0
            vol += v
            pieces += len(c[5]) - c[7]
        assert abs(vol - whole) < pieces * 2.0 ** -22, (m["name"], vol, whole)


def test_fans_as_tets(spray, fans):
    for m in fans:
        if mc.is_tets(m):
            v, n, col, f = check_tets(spray, mc.tets_of(m))
            assert len(f) == mc.NFAN and len(v) == 1 + len(m["points"]) - 2


def test_duplicates_have_long_face_key_runs(spray):
    cases = mc.duplicates()
    assert [m["name"] for m in cases][-2:] == ["three-hex", "two-hex"]
    seen = set()
    for m in cases:
        lengths = mc.face_key_runs(m)
        seen |= set(lengths.tolist())
        check_cells(spray, m)
        if mc.is_tets(m):
            check_tets(spray, mc.tets_of(m))
    assert {2, 3} <= seen and max(seen) >= 256 and {300, 301} <= seen   # even and odd
    # instance runs as well: every crossing pair of the repeated cell
    big = [m for m in cases if m["name"] in ("hex-x300", "tet-x300")]
    for m in big:
        assert mc.runs(mc.crossing_keys(m))[1].max() >= 300
    # the host tests' facts: the doubled hex leaves nothing
    assert len(sh.surface_numpy(cases[-1])[4]) == 0 and len(sh.surface_numpy(cases[-2])[4]) == 10


def test_nonmanifold_has_runs_of_three(spray):
    edge, tets, pyramids = mc.nonmanifold()
    for m in (tets, pyramids):
        assert sorted(mc.face_key_runs(m).tolist())[-2:] == [1, 3]
    v, n, col, ids, f = sh.surface_numpy(edge, edge["cells_select"])
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [0, 2]]]), axis=1)
    assert sorted(set(np.unique(e, axis=0, return_counts=True)[1].tolist())) == [2, 4]
    for m in (edge, tets, pyramids):
        check_cells(spray, m)
    check_tets(spray, mc.tets_of(tets))


def test_nonconforming(spray):
    cases = mc.nonconforming()
    assert len(cases) == 12
    collide = []
    for m in cases:
        check_cells(spray, m)
        faces = sh.cell_faces(m, np.ones(len(m["types"]), bool))
        of = lambda n: {k[1:] for k, _, _ in faces if k[0] == n}
        collide.append(bool(of(3) & of(4)))
    # a triangle on a quad's own triple: only the corner count keeps them apart
    assert any(collide) and not all(collide)
    assert {frozenset(m["types"].tolist()) for m in cases[-2:]} == {frozenset((10, 12, 13, 14))}


def test_collapsed_family(spray, collapsed):
    live = [m for m in collapsed if len(m["types"]) and m["iso"] == 0.0]
    assert len(live) == 2 * 59 * 8 and len(collapsed) > 1000
    pairs = set()
    cut = {t: 0 for t in mc.TYPES}
    empty = 0
    for m in collapsed:
        got = ch.host_mesh(spray, m)
        same(got, ch.cell_isosurface_numpy(m), m["name"])
        finite(got, m["name"])
        empty += len(got[0]) == 0
        if len(m["types"]) == 0 or m["iso"] != 0.0:
            assert len(got[0]) == 0
            continue
        t = int(m["types"][0])
        conn = m["conn"].tolist()
        assert len(set(conn)) == len(conn) - 1
        pairs.add((t, m["name"].split("-")[1]))
        cut[t] += len(got[3]) > 0
    assert len(pairs) == 2 * 59 and min(cut.values()) > 0 and empty > 100
    # more than 900 meshes in one batch, empty ones between them
    assert sum(len(m["types"]) == 0 for m in collapsed) > 50
    assert sum(m["iso"] != 0.0 for m in collapsed) > 50


def test_collapsed_family_clips_and_surfaces(spray, collapsed):
    """The whole family through both clips and the three surfaces: no clip
    reports a cut edge without a cap vertex (the host raises on any status)."""
    for m in collapsed:
        check_cells(spray, m)
        if mc.is_tets(m):
            check_tets(spray, mc.tets_of(m))


def test_flat_cells_sit_on_the_sign_boundary(spray):
    cases = mc.flat()
    rel = []
    for m in cases:
        T = ch.split_numpy(m).astype(np.int64)
        p = m["points"].astype(np.float64)
        d = ch.det6(p, T)
        e = [np.linalg.norm(p[T[:, v]] - p[T[:, 0]], axis=1) for v in (1, 2, 3)]
        assert min(x.min() for x in e) > 0
        rel.append(d / (e[0] * e[1] * e[2]))
        if "-flat" in m["name"]:
            assert (d == 0).all(), m["name"]
            # and in float32 as the rule computes it: not odd
            assert not th.orientation_odd(m["points"], T).any()
        check_cells(spray, m)
        if mc.is_tets(m):
            check_tets(spray, mc.tets_of(m))
    rel = np.concatenate(rel)
    assert (rel == 0).sum() >= 24
    assert ((rel > 0) & (rel < 1e-6)).sum() > 5 and ((rel < 0) & (rel > -1e-6)).sum() > 5
    assert any(m["points"].min() > 9e5 for m in cases)


# ---- field classes ----
def crossing_values(m):
    a, b = mc.crossing_pairs(m)
    f = np.asarray(m["values"], F32)
    return f[a], f[b]


def field_facts(klass, name, fa, fb, verts, faces):
    """The facts a field class exists for, from its crossing samples and the
    numpy restatement's triangles."""
    with np.errstate(all="ignore"):
        diff = (fb - fa).astype(F32)
    assert klass in ("onlevel", "zeros", "subnormal", "huge", "ulps", "constant"), name
    if klass in ("onlevel", "zeros"):
        area = mc.triangle_areas(verts, faces)
        assert (area == 0).any() and (area > 0).any(), name
    if klass == "huge":
        assert np.isinf(diff).any() and np.isfinite(diff).any(), name
        assert np.isfinite(fa).all() and np.isfinite(fb).all()
    if klass == "subnormal":
        assert ((np.abs(diff) < TINY) & (diff != 0)).any(), name
        assert (np.abs(np.concatenate([fa, fb])) < TINY).all()
    if klass == "ulps":
        near = (np.abs(fa.view(np.int32).astype(np.int64) - fb.view(np.int32)) == 1)
        assert near.any() and (~near).any(), name
    if klass == "constant":
        assert len(fa) == 0 and len(faces) == 0


def test_field_classes_on_cells(spray):
    cases = mc.field_cells()
    assert [m["klass"] for m in cases] == ["onlevel", "zeros", "zeros", "subnormal", "subnormal",
                                           "huge", "ulps", "constant"]
    assert np.signbit(cases[2]["iso"]) and not np.signbit(cases[1]["iso"])
    assert np.signbit(cases[1]["values"]).any() and (cases[1]["values"] == 0).sum() > 20
    assert float(np.abs(cases[5]["values"]).max()) == float(F32(3e38))
    assert (cases[7]["values"] == F32(cases[7]["iso"])).all()
    # renumbered
    assert not np.array_equal(cases[0]["conn"][:8], ch.hex_lattice(mc.LATTICE)[3][:8])
    for m in cases:
        check_cells(spray, m)
        v, n, col, f = ch.cell_isosurface_numpy(m)
        field_facts(m["klass"], m["name"], *crossing_values(m), v, f)


def test_field_classes_on_tets(spray):
    for m in mc.field_tets():
        assert mc.is_tets(m) and len(m["types"]) == 6 * 5 * 4 * 3
        v, n, col, f = check_tets(spray, mc.tets_of(m))
        field_facts(m["klass"], m["name"], *crossing_values(m), v, f)
        if m["klass"] in ("onlevel", "huge"):
            check_cells(spray, m)


def test_field_classes_on_grids(spray):
    for g in mc.field_grids():
        assert g["values"].shape == mc.LATTICE[::-1]
        v, n, f = check_grid(spray, g)
        field_facts(g["klass"], g["name"], *mc.grid_crossing_pairs(g), v, f)


def test_pencils(spray):
    shapes = set()
    for g in mc.pencils():
        shapes.add(g["values"].shape)
        v, n, f = check_grid(spray, g)
        assert len(f) > 256
        # the level is crossed at the last point, one past a block of 256
        ins = np.moveaxis(g["values"] >= F32(g["iso"]), int(np.argmax(g["values"].shape)), 0)
        assert (ins[256] != ins[255]).any() and (ins[1] != ins[0]).any()
    assert shapes == {(2, 2, 257), (2, 257, 2), (257, 2, 2)}


# ---- batches ----
def test_batches_hold_every_class_and_twins():
    cells, tets, grids = mc.cell_batch(), mc.tet_batch(), mc.grid_batch()
    topo = {"fan", "duplicates", "nonmanifold", "nonconforming", "collapsed", "flat"}
    fld = {"onlevel", "zeros", "subnormal", "huge", "ulps", "constant"}
    assert {m["klass"] for m in cells} == topo | fld
    assert {m["klass"] for m in tets} == (topo - {"nonconforming"}) | fld
    assert {g["klass"] for g in grids} == fld | {"pencil"}
    for batch in (cells, tets, grids):
        names = [m["name"] for m in batch]
        assert len(set(names)) == len(names)
        twins = [k for k, m in enumerate(batch) if "twin_of" in m]
        assert len(twins) == 2
        for k in twins:
            assert batch[k - 1]["name"] == batch[k]["twin_of"]
            assert batch[k]["klass"] in topo | fld | {"pencil"}
    assert max(len(m["types"]) for m in cells) <= 3000
    assert {m.get("normals") is not None for m in cells} == {True, False}
    sizes = {m["cmap"][0].size for m in cells if m.get("cfield") is not None}
    assert sizes == {1, 16, 4096}
    assert any(m.get("color") is not None for m in cells)
    assert any(m.get("color") is None and m.get("cfield") is None for m in cells)

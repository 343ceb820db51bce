"""The device build and refit kernels on the classes of build_cases.py.

References, each bit for bit: the host restatements
(spray_rt_bvh_build_device_host, spray_rt_bvh_refit_host) for the slot images,
the numpy forms of build_helpers for the refit of `million`, and the oracle's
brute force for queries.  test_build_cases.py holds the restatements to numpy
and the cases to their boundaries; nothing here has a tolerance.
"""
import numpy as np
import pytest

import build_cases as bc
import build_helpers as bh
import refit_helpers as rh

pytestmark = pytest.mark.gpu

SMALL = sorted(bc.small())
NEIGHBOUR, SLOT = 0, 1


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


class Meshes:
    """(verts, faces, colors, normals) and the restatement of a case, made once."""

    def __init__(self, oracle):
        self.oracle, self.m, self.r = oracle, {}, {}

    def mesh(self, c):
        if c.name not in self.m:
            with np.errstate(all="ignore"):
                n = rh.vertex_normals(self.oracle, c.verts, c.faces) if len(c.verts) else \
                    np.zeros((0, 3), np.float32)
            self.m[c.name] = (c.verts, c.faces, rh.vertex_colors(len(c.verts)), n)
        return self.m[c.name]

    def restated(self, c):
        """The image, or the error code of a refused case."""
        import spray_amd
        if c.name not in self.r:
            try:
                self.r[c.name] = bh.build_device_host(c.verts, c.faces)
            except spray_amd.SprayRtError as e:
                self.r[c.name] = e.code
        return self.r[c.name]


@pytest.fixture(scope="module")
def meshes(oracle):
    return Meshes(oracle)


def to_dev(x):
    """numpy -> GPU tensor (uint32 arrays travel as their int32 bits)."""
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def columns(ms, device):
    """[(v, f, col, n)] -> the four lists of build_domains."""
    cols = [[m[k] for m in ms] for k in range(4)]
    return [[to_dev(x) for x in col] for col in cols] if device else cols


def assert_image(c, slot, want, normals):
    got = bh.export_all(c, slot)
    assert got["NODES"] == want["nodes"].tobytes()
    assert got["TRIS"] == want["tris"].tobytes()
    assert got["PRIMS"] == want["prims"].tobytes()
    assert got["QNODES4"] == want["qnodes4"].tobytes()
    assert got["QGRID"] == want["grid"].tobytes()
    assert got["NORMALS"] == normals.tobytes()
    info = c.slot_info(slot)
    assert info == {"nodes": len(want["nodes"]), "depth": want["depth"], "tris": len(want["prims"])}
    return got


def exported(spray, c, slot):
    """export_all, None for a slot that is not loaded."""
    try:
        return bh.export_all(c, slot)
    except spray.SprayRtError:
        return None


def exact_bounds(v, f):
    ref = v[np.unique(f)]
    return np.concatenate([ref.min(0), ref.max(0)]).tobytes()


@pytest.fixture(scope="module")
def ctx(spray, meshes):
    """Slot 0 holds grid12 (the neighbour), slot 1 whatever case came last."""
    c = spray.RtContext(0)
    m = meshes.mesh(bc.named("grid12"))
    c.build_domains([NEIGHBOUR], *columns([m], False))
    yield c
    c.close()


# ---- images ----

@pytest.mark.parametrize("name", SMALL)
def test_image_equals_the_restatement(spray, meshes, ctx, name):
    """A call of the case alone, from tensors and from numpy arrays: the image
    of the restatement, or its refusal with the neighbour's bytes kept."""
    case = bc.small()[name]
    v, f, col, n = m = meshes.mesh(case)
    want = meshes.restated(case)
    assert (want if isinstance(want, int) else 0) == bc.OUTCOME.get(name, 0)
    neighbour = meshes.mesh(bc.named("grid12"))
    before = bh.export_all(ctx, NEIGHBOUR)
    for device in (True, False):
        if isinstance(want, int):
            held = exported(spray, ctx, SLOT)
            with pytest.raises(spray.SprayRtError) as e:
                ctx.build_domains([NEIGHBOUR, SLOT], *columns([neighbour, m], device))
            assert e.value.code == want and "slot %d" % SLOT in str(e.value)
            assert exported(spray, ctx, SLOT) == held
        else:
            bounds = ctx.build_domains([SLOT], *columns([m], device), bounds=True)
            assert_image(ctx, SLOT, want, n)
            assert bounds[0].tobytes() == exact_bounds(v, f)
        assert bh.export_all(ctx, NEIGHBOUR) == before


@pytest.fixture(scope="module")
def million(spray, meshes):
    """`million` built once, from tensors, in a context of its own."""
    case = bc.million()
    m = meshes.mesh(case)
    c = spray.RtContext(0)
    dev = columns([m], True)
    bounds = c.build_domains([0], *dev, bounds=True)
    yield c, case, m, bounds
    c.close()


def test_million_image(meshes, million):
    c, case, (v, f, col, n), bounds = million
    assert_image(c, 0, meshes.restated(case), n)
    assert bounds[0].tobytes() == exact_bounds(v, f)


# ---- queries ----

@pytest.mark.parametrize("name", bc.QUERIED)
def test_queries_match_the_oracle(spray, oracle, meshes, ctx, name):
    case = bc.small()[name]
    v, f, col, n = m = meshes.mesh(case)
    cols = columns([m], True)
    ctx.build_domains([SLOT], *cols)
    bh.check_queries(spray, oracle, ctx, SLOT, v, f, col, n, 500 + bc.QUERIED.index(name),
                     ray_verts=bc.ray_verts(name))
    del cols   # alive until the queries have synchronised


# ---- batches ----

def test_mixed_call_in_three_orders(spray, meshes):
    """levels3 sizes the grids, so most blocks see none of the small slots'
    triangles; slot k holds mesh k of mixed() whatever the order of the call."""
    base = bc.mixed()
    slot_of = {c.name: k for k, c in enumerate(base)}
    c = spray.RtContext(0)
    first = None
    for device, order in ((True, "as_listed"), (False, "reversed"), (True, "rotated"),
                          (True, "as_listed")):
        cases = bc.mixed_orders()[order]
        ms = [meshes.mesh(x) for x in cases]
        slots = [slot_of[x.name] for x in cases]
        bounds = c.build_domains(slots, *columns(ms, device), bounds=True)
        got = {}
        for x, s, m, row in zip(cases, slots, ms, bounds):
            if len(x.faces) == 0:
                assert c.slot_info(s) == {"nodes": 0, "depth": 0, "tris": 0}
                continue
            got[s] = assert_image(c, s, meshes.restated(x), m[3])
            assert row.tobytes() == exact_bounds(m[0], m[1])
        if first is None:
            first = got
        assert got == first
    c.close()


@pytest.mark.parametrize("nslots", bc.MANY_CALLS)
def test_many_slots_either_side_of_the_sort_partition(spray, meshes, nslots):
    cases = bc.many(nslots)
    distinct = {x.name: x for x in bc.many_meshes()}
    dev = {k: [to_dev(a) for a in meshes.mesh(x)] for k, x in distinct.items()}
    c = spray.RtContext(0)
    cols = [[dev[x.name][k] for x in cases] for k in range(4)]
    c.build_domains(list(range(nslots)), *cols)
    images = {}
    for s, x in enumerate(cases):
        if len(x.faces) == 0:
            assert c.slot_info(s) == {"nodes": 0, "depth": 0, "tris": 0}
        elif x.name not in images:
            images[x.name] = assert_image(c, s, meshes.restated(x), meshes.mesh(x)[3])
        else:
            assert bh.export_all(c, s) == images[x.name], (s, x.name)
    assert len(images) == len(distinct) - 1
    c.close()


@pytest.mark.parametrize("kind", ["face", "nan"])
def test_poisoned_calls_fail_and_change_nothing(spray, meshes, kind):
    """A bad element at the block and stride boundaries of build_check, the bad
    mesh first, last and fifth in the call: ERR_ARG naming its slot, every slot
    as it was, and the good call afterwards goes through."""
    base = bc.mixed()
    slot_of = {c.name: k for k, c in enumerate(base)}
    c = spray.RtContext(0)

    def good():
        ms = [meshes.mesh(x) for x in base]
        c.build_domains(list(range(len(base))), *columns(ms, True))
        out = {}
        for s, (x, m) in enumerate(zip(base, ms)):
            if len(x.faces):
                out[s] = assert_image(c, s, meshes.restated(x), m[3])
        return out

    before = good()
    text = "face index out of range" if kind == "face" else "non-finite coordinate"
    for i, tri in enumerate(bc.poison_positions()):
        bad = bc.poisoned(kind, tri)
        order = list(bc.mixed_orders().values())[i % 3]
        cases = [bad if x.name == "levels3" else x for x in order]
        ms = [(bad.verts, bad.faces, rh.vertex_colors(len(bad.verts)),
               np.zeros_like(bad.verts)) if x is bad else meshes.mesh(x) for x in cases]
        slots = [slot_of["levels3" if x is bad else x.name] for x in cases]
        with pytest.raises(spray.SprayRtError) as e:
            c.build_domains(slots, *columns(ms, i % 2 == 0))
        assert e.value.code == bc.ERR_ARG, (kind, tri)
        assert "slot %d)" % slot_of["levels3"] in str(e.value) and text in str(e.value)
        for s, img in before.items():
            assert bh.export_all(c, s) == img, (kind, tri, s)
        assert c.slot_info(slot_of["empty"])["tris"] == 0
    assert good() == before
    c.close()


# ---- refit at scale ----

@pytest.mark.parametrize("g", [100, 363], ids=["levels3", "grid363"])
def test_refit_of_uploaded_slots_at_scale(spray, oracle, g):
    """spray_rt_bvh_refit_host byte for byte on 20,000 and 263,538 triangles."""
    v, f = rh._grid(g)
    col, n = rh.vertex_colors(len(v)), rh.vertex_normals(oracle, v, f)
    c = spray.RtContext(0)
    c.upload_domain(2, v, f, col, n)
    built = bh.export_all(c, 2)
    for i, d in enumerate(("sin", "shear", "flatten", "identity")):
        v1 = rh.deform(d, v)
        n1 = rh.vertex_normals(oracle, v1, f)
        new = (to_dev(v1), to_dev(n1)) if i % 2 else (v1, n1)
        c.refit_domains([2], [new[0]], [new[1]])
        got = bh.export_all(c, 2)
        want = spray.bvh_refit_host(v, v1, f)
        assert got["NODES"] == want["nodes"].tobytes(), d
        assert got["TRIS"] == want["tris"].tobytes(), d
        assert got["QGRID"] == want["grid"].tobytes(), d
        assert got["QNODES4"] == want["qnodes4"].tobytes(), d
        assert got["NORMALS"] == n1.tobytes() and got["PRIMS"] == built["PRIMS"]
    assert got == built   # back at the original vertices: the uploaded image
    c.close()


def test_million_refit(oracle, meshes, million):
    """The one place where refit_tris and refit_commit stride: `million`
    refitted to the sin deformation against the by-level numpy forms, and back
    to the built image."""
    c, case, (v, f, col, n), _ = million
    b = meshes.restated(case)
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    new = (to_dev(v1), to_dev(n1))
    bounds = c.refit_domains([0], [new[0]], [new[1]], bounds=True)
    assert bounds[0].tobytes() == exact_bounds(v1, f)
    got = bh.export_all(c, 0)
    nodes = np.frombuffer(got["NODES"], rh.NODE_DTYPE)
    for k in ("left", "right", "pad"):
        assert np.array_equal(nodes[k], b["nodes"][k])
    assert got["PRIMS"] == b["prims"].tobytes() and got["NORMALS"] == n1.tobytes()
    plo, phi, rng = bh.expected_boxes_by_level(b["nodes"], b["prims"], f, v1)
    assert np.stack([nodes["l_lo"], nodes["r_lo"]], 1).tobytes() == plo.tobytes()
    assert np.stack([nodes["l_hi"], nodes["r_hi"]], 1).tobytes() == phi.tobytes()
    tris = np.frombuffer(got["TRIS"], np.float32).reshape(-1, 12)
    ff = f[b["prims"]]
    assert np.array_equal(tris[:, 0:3], v1[ff[:, 0]])
    assert np.array_equal(tris[:, 3:6], v1[ff[:, 0]] - v1[ff[:, 1]])
    assert np.array_equal(tris[:, 6:9], v1[ff[:, 2]] - v1[ff[:, 0]])
    pick = np.sort(np.random.default_rng(9).choice(len(f), 20000, replace=False))
    assert tris[pick].tobytes() == rh.expected_tris(b["prims"][pick], f, v1).tobytes()
    q4 = np.frombuffer(got["QNODES4"], rh.QNODE4_DTYPE)
    assert np.array_equal(q4["child"], b["qnodes4"]["child"])
    bh.check_qnodes4(q4, np.frombuffer(got["QGRID"], np.float32), rng, plo, phi, len(f))
    old = (to_dev(v), to_dev(n))
    c.refit_domains([0], [old[0]], [old[1]])
    assert_image(c, 0, b, n)
    del new, old

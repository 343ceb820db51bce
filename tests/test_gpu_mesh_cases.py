"""The five mesh extractions on the GPU over the hard classes of mesh_cases.py
(spray_rt_isosurface, spray_rt_tet_isosurface, spray_rt_cell_isosurface,
spray_rt_cell_surface, spray_rt_cell_clip and their slot forms).

References, each bit for bit: the host restatements (themselves checked against
numpy on these classes in test_mesh_cases.py) for the extracted arrays, a
build_domains of the restated arrays in a second context for the slot images,
the oracle's brute force for queries.
"""
import ctypes as C

import numpy as np
import pytest

import build_helpers as bh
import cell_helpers as ch
import clip_helpers as clh
import mesh_cases as mc
import surface_helpers as sh
import tet_helpers as th

pytestmark = pytest.mark.gpu

WHAT = bh.WHAT + ("COLORS", "FACES")
F32 = np.float32
NORMALS = 1   # the place of the normals in every call's results


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def ctx(spray):
    c = spray.RtContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def other(spray):
    """A second context: build_domains of the restated arrays."""
    c = spray.RtContext(0)
    yield c
    c.close()


def grids_on_device(grids):
    import torch
    return [dict(g, values=torch.from_numpy(g["values"]).cuda()) for g in grids]


class Extraction:
    """One call of the engine under one setting: how to run a batch of cases on
    a context, the host restatement of one case, the slot form."""

    def __init__(self, name, kind, extra=None):
        self.name, self.kind, self.extra = name, kind, extra

    def cases(self):
        return {"grid": mc.grid_batch, "tet": mc.tet_batch}.get(self.kind, mc.cell_batch)()

    def extras(self, ms):
        """The per-mesh argument beside the meshes: selects, invert flags."""
        if self.kind == "surface":
            return [mc.selects(m)[self.extra] for m in ms]
        if self.kind == "clip":
            return [self.extra] * len(ms)
        return None

    def on_device(self, ms, ex):
        if self.kind == "grid":
            return grids_on_device(ms), ex
        if self.kind == "tet":
            return th.on_device(ms), ex
        if self.kind == "surface":
            return sh.on_device(ms, ex)
        return ch.on_device(ms), ex

    def run(self, c, ms, ex, **kw):
        if self.kind == "grid":
            out = c.isosurface(ms, **kw)
        elif self.kind == "tet":
            out = c.tet_isosurface(ms, **kw)
        elif self.kind == "cell":
            out = c.cell_isosurface(ms, **kw)
        elif self.kind == "surface":
            out = c.cell_surface(ms, ex, **kw)
        else:
            out = c.cell_clip(ms, ex, **kw)
        c.sync()   # the calls are enqueued on the context's stream; torch reads on another
        return out

    def host(self, spray, m, ex, normals=True):
        if self.kind == "grid":
            return spray.isosurface_host(m["values"], m["origin"], m["spacing"], m["iso"], normals)
        if self.kind == "tet":
            return th.host_mesh(spray, m, normals)
        if self.kind == "cell":
            return ch.host_mesh(spray, m, normals)
        if self.kind == "surface":
            return sh.host_surface(spray, m, ex, normals)
        return clh.host_clip(spray, m, ex, normals)

    def counts(self, r):
        """What the count-only form reports for restated results r."""
        if self.kind == "clip":
            return (len(r[0]), len(r[5]), r[6], r[7])
        return (len(r[0]), len(r[{"grid": 2, "tet": 3, "cell": 3, "surface": 4}[self.kind]]))

    def slots(self, c, slots, ms, ex, bounds):
        if self.kind == "grid":
            return c.isosurface_domains(slots, ms, bounds=bounds)
        if self.kind == "tet":
            return c.tet_isosurface_domains(slots, ms, bounds=bounds)
        if self.kind == "cell":
            return c.cell_isosurface_domains(slots, ms, bounds=bounds)
        if self.kind == "surface":
            return c.cell_surface_domains(slots, ms, ex, bounds=bounds)
        return c.cell_clip_domains(slots, ms, ex, bounds=bounds)

    def mesh_of(self, m, r):
        """(verts, faces, colors or None, normals) a slot of case m holds, of restated results r."""
        if self.kind == "grid":
            col = None if m["color"] is None else np.full(len(r[0]), m["color"], np.uint32)
            return r[0], r[2], col, r[1]
        faces = r[{"tet": 3, "cell": 3, "surface": 4, "clip": 5}[self.kind]]
        col = r[2] if m.get("cfield") is not None or m.get("color") is not None else None
        return r[0], faces, col, r[1]


EXTRACTIONS = [Extraction("grid", "grid"), Extraction("tet", "tet"), Extraction("cell", "cell"),
               Extraction("surface-all", "surface", 0), Extraction("surface-points", "surface", 1),
               Extraction("surface-cells", "surface", 2), Extraction("clip", "clip", False),
               Extraction("clip-inverted", "clip", True)]
IDS = [e.name for e in EXTRACTIONS]
UNSTRUCTURED = [e for e in EXTRACTIONS if e.kind != "grid"]


def to_bytes(r):
    """Results of one mesh, from the device or the host, as comparable bytes."""
    out = []
    for x in r:
        if x is None or isinstance(x, (int, np.integer)):
            out.append(x if x is None else int(x))
        elif hasattr(x, "cpu"):
            out.append(x.cpu().numpy().tobytes())
        else:
            out.append(np.ascontiguousarray(x).tobytes())
    return tuple(out)


def without_normals(b):
    return b[:NORMALS] + (None,) + b[NORMALS + 1:]


@pytest.fixture(scope="module")
def batches(spray):
    """name -> (cases, extras, restated bytes with normals, restated results)."""
    out = {}
    for e in EXTRACTIONS:
        ms = e.cases()
        ex = e.extras(ms)
        res = [e.host(spray, m, None if ex is None else ex[k]) for k, m in enumerate(ms)]
        out[e.name] = (ms, ex, [to_bytes(r) for r in res], res)
    return out


@pytest.fixture(scope="module")
def family():
    return mc.collapsed()


def first_difference(got, want, names):
    """For the message of a failed comparison: (mesh, array, first differing byte)."""
    for k, (g, w) in enumerate(zip(got, want)):
        for i, (x, y) in enumerate(zip(g, w)):
            if x != y:
                at = None
                if isinstance(x, bytes) and isinstance(y, bytes):
                    n = min(len(x), len(y))
                    a, b = np.frombuffer(x[:n], np.uint8), np.frombuffer(y[:n], np.uint8)
                    d = np.nonzero(a != b)[0]
                    at = (int(d[0]) if len(d) else n, len(x), len(y))
                return names[k], i, at
    return None


def assert_equal(got, want, names):
    assert len(got) == len(want)
    assert got == want, first_difference(got, want, names)


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
@pytest.mark.parametrize("e", EXTRACTIONS, ids=IDS)
def test_kernels_equal_the_host_restatement(ctx, batches, e, device):
    """Every class in one batch, with normals; the same batch reversed, without."""
    ms, ex, want, _ = batches[e.name]
    names = [m["name"] for m in ms]
    dm, dx = e.on_device(ms, ex) if device else (ms, ex)
    got = [to_bytes(r) for r in e.run(ctx, dm, dx)]
    assert_equal(got, want, names)
    rx = None if dx is None else dx[::-1]
    rev = [to_bytes(r) for r in e.run(ctx, dm[::-1], rx, normals=False)][::-1]
    assert_equal(rev, [without_normals(w) for w in want], names)


@pytest.mark.parametrize("e", EXTRACTIONS, ids=IDS)
def test_twins_give_the_bytes_each_gives_alone(ctx, batches, e):
    ms, ex, want, _ = batches[e.name]
    twins = [k for k, m in enumerate(ms) if "twin_of" in m]
    assert len(twins) == 2
    dm, dx = e.on_device(ms, ex)
    for k in twins:
        assert want[k] == want[k - 1]
        alone = e.run(ctx, [dm[k]], None if dx is None else [dx[k]])
        assert to_bytes(alone[0]) == want[k], ms[k]["name"]
        pair = e.run(ctx, dm[k - 1:k + 1], None if dx is None else dx[k - 1:k + 1])
        assert [to_bytes(r) for r in pair] == [want[k], want[k]], ms[k]["name"]


def family_call(e, family):
    """The collapsed family with its empty neighbours as one batch of the
    call: the splits for the tet call, selects of the three modes in turn,
    invert flags in turn."""
    if e.kind == "tet":
        return [mc.split_of(m) for m in family], None
    if e.kind == "surface":
        return family, [mc.selects(m)[k % 3] for k, m in enumerate(family)]
    if e.kind == "clip":
        return family, [bool(k & 1) for k in range(len(family))]
    return family, None


MANY = [e for e in EXTRACTIONS if e.name in ("tet", "cell", "surface-all", "clip")]


@pytest.mark.parametrize("e", MANY, ids=[e.name for e in MANY])
def test_many_segments(spray, ctx, family, e):
    """About a thousand meshes of one cell or none in one call, then the same
    call again on the same context: its scratch is reused."""
    ms, ex = family_call(e, family)
    assert len(ms) > 1000
    names = [m["name"] for m in ms]
    res = [e.host(spray, m, None if ex is None else ex[k]) for k, m in enumerate(ms)]
    want = [to_bytes(r) for r in res]
    assert sum(len(w[0]) == 0 for w in want) > 100 and sum(len(w[0]) > 0 for w in want) > 300
    dm, dx = e.on_device(ms, ex)
    got = [to_bytes(r) for r in e.run(ctx, dm, dx)]
    assert_equal(got, want, names)
    again = [to_bytes(r) for r in e.run(ctx, dm, dx)]
    assert_equal(again, want, names)
    counted = e.run(ctx, dm, dx, count_only=True)
    assert counted == [e.counts(r) for r in res]


@pytest.mark.parametrize("e", UNSTRUCTURED, ids=[e.name for e in UNSTRUCTURED])
def test_count_only_form(ctx, batches, e):
    ms, ex, _, res = batches[e.name]
    pick = [k for k, m in enumerate(ms) if m["klass"] in ("fan", "duplicates", "collapsed")]
    assert {ms[k]["klass"] for k in pick} == {"fan", "duplicates", "collapsed"}
    sub = [ms[k] for k in pick]
    sx = None if ex is None else [ex[k] for k in pick]
    want = [e.counts(res[k]) for k in pick]
    if e.name != "surface-points":   # every cell of a fan holds a and b: all of them or none
        assert max(w[0] for w in want) > 600
    assert e.run(ctx, sub, sx, count_only=True) == want
    dm, dx = e.on_device(sub, sx)
    assert e.run(ctx, dm, dx, count_only=True) == want


def test_count_only_form_of_the_structured_call(ctx, batches):
    from spray_amd import _native, engine
    ms, _, _, res = batches["grid"]
    n = len(ms)
    arr, keep = engine._grid_table(grids_on_device(ms))
    nv, nf = (C.c_size_t * n)(), (C.c_size_t * n)()
    rc = _native.lib().spray_rt_isosurface(ctx.h, n, arr, None, None, None, None, None, nv, nf)
    assert rc == 0
    assert [(nv[k], nf[k]) for k in range(n)] == [(len(r[0]), len(r[2])) for r in res]


SLOT_CASES = {"grid": ("grid-onlevel", "grid-huge"),
              "tet": ("fan-tet-full-middle", "tet-x300", "kuhn-onlevel", "kuhn-huge"),
              "cell": ("fan-tet-half-middle", "fan-wedge-half-middle", "hex-x300", "tet-x300",
                       "cells-onlevel", "cells-huge")}


def slot_ready(m):
    """The case with point normals and a colour, so that the queries' shading is compared too."""
    if "origin" in m:
        return m if m["color"] is not None else dict(m, color=0x00C08040)
    m = mc.with_normals(m)
    if m.get("cfield") is None and m.get("color") is None:
        m = dict(m, color=0x00C08040)
    return m


SLOTTED = [e for e in EXTRACTIONS if e.name in ("grid", "tet", "cell", "surface-all", "clip",
                                                "clip-inverted")]


@pytest.mark.parametrize("e", SLOTTED, ids=[e.name for e in SLOTTED])
def test_slot_images_and_queries(spray, oracle, ctx, other, batches, e):
    """Slots filled on the device equal a build of the restated arrays, zero-area
    and duplicate triangles included, and answer rays as the brute force does."""
    by_name = {m["name"]: m for m in batches[e.name][0]}
    ms = [slot_ready(by_name[n]) for n in SLOT_CASES.get(e.kind, SLOT_CASES["cell"])]
    ex = e.extras(ms)
    res = [e.host(spray, m, None if ex is None else ex[k]) for k, m in enumerate(ms)]
    parts = [e.mesh_of(m, r) for m, r in zip(ms, res)]
    n = len(ms)
    slots = list(range(n))
    dm, dx = e.on_device(ms, ex)
    bounds = e.slots(ctx, slots, dm, dx, True)
    ref = other.build_domains(slots, [p[0] for p in parts], [p[1] for p in parts],
                              [p[2] for p in parts], [p[3] for p in parts], bounds=True)
    assert bounds.tobytes() == ref.tobytes()
    for k in slots:
        name = ms[k]["name"]
        got = {w: ctx.slot_export(k, getattr(ctx, "SLOT_" + w)).tobytes() for w in WHAT}
        want = {w: other.slot_export(k, getattr(other, "SLOT_" + w)).tobytes() for w in WHAT}
        assert got == want, name
        assert ctx.slot_info(k) == other.slot_info(k), name
        assert got["FACES"] == np.ascontiguousarray(parts[k][1]).tobytes(), name
        v, f, col, nrm = parts[k]
        assert len(f) > 0, name
        bh.check_queries(spray, oracle, ctx, k, v, f, col, nrm, 900 + k)
    # the degenerate triangles the classes are there for went through the build
    if e.name in ("grid", "tet", "cell", "clip"):
        assert ms[-2]["klass"] == "onlevel"
        assert (mc.triangle_areas(parts[-2][0], parts[-2][1]) == 0).any()
    if e.kind != "grid":
        dup = -3 if e.kind == "tet" else 2
        tri = np.sort(np.asarray(parts[dup][1], np.int64), axis=1)
        assert ms[dup]["klass"] == "duplicates"
        if e.kind != "surface":
            assert np.unique(tri, axis=0, return_counts=True)[1].max() >= 300
    for k in slots:
        ctx.release_domain(k)
        other.release_domain(k)

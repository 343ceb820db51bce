"""A time-step session as data: one context, several filters per step, moving
boxes and maps, for test_session_host.py (the
conditions, on the CPU) and test_gpu_session.py (the context against its twin).

A session is a list of steps.  A step is a dict: "ops" (a list of operations),
"maps" (domain -> slot updates, -1 unmaps), "boxes" ("slack" or "exact") and,
for a call that must be rejected, "reject".  An operation is a dict naming its
call kind ("kind"), its target ("slot"), a unique "name" and its inputs, which
come from the helper modules of the per-filter tests.

    apply(c, session, k, device)   the step's calls on a context, batched by kind
    restate(op)                    (verts, faces, colors, normals) from the host forms
    chain(session, k, slot)        the operations that made the slot's content
    content(session, k, slot)      the chain folded into one mesh
    replay(c, session, k, device)  every live slot's chain alone on a fresh context
    boxes / maps                   the scene state after step k

The domains lie in two rows of three (place()); a domain's slack box holds
everything the slots mapped to it contain over the whole session."""
import functools

import numpy as np

import block_stream_helpers as bsh
import build_helpers as bh
import cell_helpers as cellh
import clip_helpers as clh
import color_helpers as colh
import glyph_helpers as gh
import iso_helpers as ih
import refit_helpers as rh
import stream_helpers as sth
import surface_helpers as sfh
import tet_helpers as th

F32 = np.float32
NDOM = 6           # fixed for the whole session; domain 5 starts unmapped
PITCH, ROW = 12.0, 15.0   # domain d's contents sit around (PITCH * (d % 3), ROW * (d // 3), 0)
SLACK = 0.5
EXTRACTIONS = ("iso", "tet", "cell", "surface", "clip", "stream", "bstream", "glyphs")
BASES = EXTRACTIONS + ("build", "upload")
KINDS = BASES + ("refit", "recolor", "release")
BSDFS = ((0, 0.8, 0.7, 0.6),) * NDOM
MIB, MIRROR0 = 1 << 20, 64 << 10   # ensure()'s and the pinned mirrors' first sizes

# The scratch each kind of call lays out or stages through (rt_ctx.h): every
# *_domains call ends in domains_build; host pointers pass d_stage.
SCRATCH = {
    "iso": {"d_isomesh", "build", "d_sort", "d_stage"},
    "tet": {"d_isomesh", "build", "d_sort", "d_stage"},
    "cell": {"d_isomesh", "build", "d_sort", "d_stage"},
    "surface": {"d_isomesh", "build", "d_sort", "d_surfinst", "d_stage"},
    "clip": {"d_isomesh", "build", "d_sort", "d_surfinst", "d_stage"},
    "stream": {"d_isomesh", "build", "d_sort", "d_stage"},
    "bstream": {"d_isomesh", "build", "d_sort", "d_stage"},
    "glyphs": {"d_isomesh", "build", "d_sort", "d_stage"},
    "build": {"build", "d_sort", "d_stage"},
    "refit": {"d_stage", "slots"},
    "recolor": {"d_stage", "slots"},
    "upload": {"slots"},      # the slot table and the slots' own memory
    "release": {"slots"},
}
for _k in BASES:
    SCRATCH[_k] = SCRATCH[_k] | {"slots"}


def align256(n):
    return (int(n) + 255) & ~255


# ---- placing inputs in a domain's region ----
def place(kind, x, d):
    """The inputs of one operation moved into domain d's region."""
    off = np.array([PITCH * (d % 3), ROW * (d // 3), 0.0], F32)
    add = lambda o: tuple(float(v) for v in (np.asarray(o, F32) + off))
    if kind == "iso":
        return dict(x, origin=add(x["origin"]))
    if kind in ("tet", "cell", "surface", "clip"):
        return dict(x, points=(x["points"] + off).astype(F32))
    if kind == "stream":
        return dict(x, origin=add(x["origin"]), seeds=(x["seeds"] + off).astype(F32))
    if kind == "bstream":
        return dict(x, blocks=[dict(b, origin=add(b["origin"])) for b in x["blocks"]],
                    seeds=(x["seeds"] + off).astype(F32))
    if kind == "glyphs":
        return dict(x, points=(x["points"] + off).astype(F32))
    return (x + off).astype(F32)   # vertices


def op(kind, slot, name, **inputs):
    assert kind in KINDS + ("glyph_buffers",)
    return dict(kind=kind, slot=slot, name=name, **inputs)


# ---- the host restatements ----
_RESTATED = {}


def _spray():
    import spray_amd
    return spray_amd


def has_colors(o):
    k = o["kind"]
    if k == "iso":
        g = o["grid"]
        return g.get("cfield") is not None or g.get("color") is not None
    if k in ("tet", "cell", "surface", "clip"):
        m = o["mesh"]
        return m.get("cfield") is not None or m.get("color") is not None
    if k == "stream":
        return o["field"].get("cfield") is not None or o["tube"].get("color") is not None
    if k == "bstream":
        return (any(b.get("cfield") is not None for b in o["set"]["blocks"])
                or o["tube"].get("color") is not None)
    if k == "glyphs":
        return o["set"].get("cfield") is not None or o["glyph"].get("color") is not None
    return o.get("colors") is not None


def _restate(o):
    spray, k = _spray(), o["kind"]
    if k == "iso":
        v, n, c, f = colh.host_mesh(spray, o["grid"])
    elif k == "tet":
        v, n, c, f = th.host_mesh(spray, o["mesh"])
    elif k == "cell":
        v, n, c, f = cellh.host_mesh(spray, o["mesh"])
    elif k == "surface":
        v, n, c, _, f = sfh.host_surface(spray, o["mesh"], o.get("select"))
    elif k == "clip":
        v, n, c, _, _, f = clh.host_clip(spray, o["mesh"], o["invert"])[:6]
    elif k == "stream":
        t = o["tube"]
        v, n, c, f = spray.stream_tubes_host(*sth.host_args(o["field"]), t["radius"], t["nsides"],
                                             color=t.get("color"), cfield=o["field"].get("cfield"),
                                             cmap=o["field"].get("cmap"),
                                             **sth.host_kw(o["field"]))
    elif k == "bstream":
        t = o["tube"]
        v, n, c, f = spray.block_stream_tubes_host(*bsh.host_args(o["set"]), t["radius"],
                                                   t["nsides"], color=t.get("color"),
                                                   cmap=o["set"].get("cmap"),
                                                   **bsh.host_kw(o["set"]))
    elif k == "glyphs":
        v, n, c, f, _ = spray.glyphs_host(o["set"], o["glyph"])
    elif k in ("build", "upload"):
        return o["verts"], o["faces"], o.get("colors"), o.get("normals")
    elif k == "refit":
        if "set" in o:   # the moving-particle recipe: the glyphs of the moved set
            v, n = spray.glyphs_host(o["set"], o["glyph"])[:2]
            return v, None, None, n
        return o["verts"], None, None, o.get("normals")
    elif k == "recolor":
        table, lo, hi = o["cmap"]
        return None, None, spray.colormap_host(o["scalars"], table, lo, hi), None
    else:
        raise KeyError(k)
    return v, f, (c if has_colors(o) else None), n


def restate(o):
    """(verts, faces, colors, normals) of one operation from the host forms
    (entries it does not set are None), computed once per operation name."""
    if o["name"] not in _RESTATED:
        _RESTATED[o["name"]] = (o, _restate(o))
    kept, out = _RESTATED[o["name"]]
    assert kept is o, "two operations named " + o["name"]
    return out


def corrupted(o, other):
    """o restated from another operation's inputs: what carried state looks like."""
    return _restate(dict(other, name=o["name"] + "/corrupted"))


def mesh_bytes(o):
    """The size of an operation's result (0 for a release): what 'larger' means."""
    if o["kind"] == "release":
        return 0
    if o["kind"] == "glyph_buffers":
        return sum(12 * len(m[0]) + 12 * len(m[3]) for m in restate_buffers(o))
    return sum(0 if a is None else np.asarray(a).nbytes for a in restate(o))


def restate_buffers(o):
    """[(verts, normals, colors, faces, point_ids)] of a caller-buffer glyph call."""
    if o["name"] not in _RESTATED:
        spray = _spray()
        _RESTATED[o["name"]] = (o, [spray.glyphs_host(S, o["glyph"]) for S in o["sets"]])
    return _RESTATED[o["name"]][1]


# ---- the bytes a call lays out in d_isomesh, from the restated counts ----
def _mesh_take(o, with_normals=True):
    v, f, c, n = restate(o)
    nv, nf = len(v), len(f)
    return (align256(12 * nv) + (align256(12 * nv) if with_normals and n is not None else 0)
            + (align256(4 * nv) if has_colors(o) else 0) + align256(12 * nf))


def _tube_scratch(npoints, nseeds):
    return 3 * align256(12 * npoints) + align256(4 * npoints) + 3 * align256(4 * (nseeds + 1))


def isomesh_bytes(o, device=True):
    """The Layout of one job in d_isomesh (the *_domains entry points'
    `Layout M`): the mesh at its exact size, before it the tubes' line
    scratch or the glyphs' records."""
    spray, k = _spray(), o["kind"]
    if k in ("iso", "tet", "cell", "surface", "clip"):
        return _mesh_take(o)
    if k == "stream":
        pts = spray.streamlines_host(*sth.host_args(o["field"]), **sth.host_kw(o["field"]))[0]
        return _tube_scratch(len(pts), len(o["field"]["seeds"])) + _mesh_take(o)
    if k == "bstream":
        pts = spray.block_streamlines_host(*bsh.host_args(o["set"]), **bsh.host_kw(o["set"]))[0]
        return _tube_scratch(len(pts), len(o["set"]["seeds"])) + _mesh_take(o)
    if k == "glyphs":
        nglyphs = len(spray.glyphs_host(o["set"], o["glyph"])[4])
        return align256(48 * nglyphs) + _mesh_take(o)
    if k == "glyph_buffers":   # into caller buffers: the records alone
        return sum(align256(48 * len(m[4])) for m in restate_buffers(o))
    if k == "refit" and "set" in o and device:   # glyphs(arrays=("verts", "normals"))
        return align256(48 * len(spray.glyphs_host(o["set"], o["glyph"])[4]))
    return 0


def step_isomesh_bytes(step, device=True):
    """The largest layout a call of the step asks of d_isomesh (a call batches
    the step's operations of one kind)."""
    per_kind = {}
    for o in step["ops"]:
        per_kind[o["kind"]] = per_kind.get(o["kind"], 0) + isomesh_bytes(o, device)
    return max(per_kind.values(), default=0)


# sizeof(GlyphJob) + a status word + sizeof(GlyphCount) + sizeof(GlyphOut)
# (glyph_kernels.h): the head of the glyph arena holds one of each per job
GLYPH_HEAD_PER_JOB = 304 + 4 + 16 + 96


def glyph_head_bytes(njobs):
    return (align256(304 * njobs) + align256(4 * njobs) + align256(16 * njobs)
            + align256(96 * njobs))


# ---- the session's state after a step ----
def good(step):
    return step.get("reject") is None


def slot_ops(session, k, slot):
    return [o for step in session[:k + 1] if good(step) for o in step["ops"]
            if o.get("slot") == slot]


def chain(session, k, slot):
    """The operations that produced the slot's content after step k: its last
    build, upload or extraction, then only the refits and recolours that
    followed ([] for a slot that is not live)."""
    ops = slot_ops(session, k, slot)
    last = max((i for i, o in enumerate(ops) if o["kind"] in BASES + ("release",)), default=None)
    if last is None or ops[last]["kind"] == "release":
        return []
    return ops[last:]


def live_slots(session, k):
    slots = sorted({o["slot"] for step in session[:k + 1] if good(step) for o in step["ops"]
                    if o.get("slot") is not None})
    return [s for s in slots if chain(session, k, s)]


def fold(ops, restated=restate):
    """A chain as one mesh (verts, faces, colors, normals)."""
    v, f, c, n = restated(ops[0])
    for o in ops[1:]:
        rv, _, rc, rn = restated(o)
        if o["kind"] == "refit":
            v, n = rv, (rn if rn is not None else n)
        else:
            c = rc
    return v, f, c, n


def content(session, k, slot):
    ops = chain(session, k, slot)
    return fold(ops) if ops else None


def maps(session, k):
    """{domain: slot} after step k (unmapped domains absent)."""
    m = {}
    for step in session[:k + 1]:
        if good(step):
            m.update(step.get("maps", {}))
    return {d: s for d, s in m.items() if s >= 0}


def exact_box(v, f):
    ref = v[np.unique(f)]
    return np.concatenate([ref.min(0), ref.max(0)]).astype(F32)


@functools.lru_cache(maxsize=None)
def _slack_boxes(key):
    session = _SESSIONS[key]
    lo = np.full((NDOM, 3), np.inf)
    hi = np.full((NDOM, 3), -np.inf)
    for k in range(len(session)):
        for d, s in maps(session, k).items():
            m = content(session, k, s)
            if m is not None and len(m[1]):
                b = exact_box(m[0], m[1])
                lo[d], hi[d] = np.minimum(lo[d], b[:3]), np.maximum(hi[d], b[3:])
    for d in range(NDOM):
        assert np.isfinite(lo[d]).all(), "domain %d never holds anything" % d
    return np.concatenate([lo - SLACK, hi + SLACK], 1).astype(F32)


_SESSIONS = {}


def slack_boxes(session):
    key = id(session)
    _SESSIONS[key] = session
    return _slack_boxes(key)


def boxes(session, k):
    """The [NDOM, 6] boxes after step k: slack boxes, or in an "exact" step the
    exact bounds of every mapped non-empty domain."""
    mode = [s for s in session[:k + 1] if good(s)][-1].get("boxes", "slack")
    out = slack_boxes(session).copy()
    if mode == "exact":
        for d, s in maps(session, k).items():
            m = content(session, k, s)
            if m is not None and len(m[1]):
                out[d] = exact_box(m[0], m[1])
    return out


def merged(session, k):
    """(verts, faces) of every mapped non-empty domain's mesh after step k."""
    vs, fs, base = [], [], 0
    for d, s in sorted(maps(session, k).items()):
        m = content(session, k, s)
        if m is not None and len(m[1]):
            vs.append(m[0])
            fs.append(m[1].astype(np.int64) + base)
            base += len(m[0])
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.uint32)


# ---- the calls ----
def to_dev(x):
    """numpy -> GPU tensor (uint32 arrays travel as their int32 bits)."""
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def on_device(x):
    """The arrays of an input dict (or a list of them) as GPU tensors; colour
    tables and scalars stay on the host."""
    if isinstance(x, (list, tuple)):
        return [on_device(y) for y in x]
    if isinstance(x, dict):
        return {k: (v if k == "cmap" else on_device(v)) if isinstance(v, (np.ndarray, list, dict))
                else v for k, v in x.items()}
    return to_dev(x) if isinstance(x, np.ndarray) else x


def _inputs(xs, device):
    return on_device(xs) if device else list(xs)


def _call(c, kind, ops, device):
    """One batched call for the operations of one kind -> {slot: bounds row}
    (refits too; recolours, uploads and releases return nothing)."""
    slots = [o["slot"] for o in ops]
    n = len(ops)
    rows = lambda b: {s: np.asarray(b[i]) for i, s in enumerate(slots)}
    if kind == "iso":
        return rows(c.isosurface_domains_mapped(slots, _inputs([o["grid"] for o in ops], device),
                                                bounds=True))
    if kind == "tet":
        return rows(c.tet_isosurface_domains(slots, _inputs([o["mesh"] for o in ops], device),
                                             bounds=True))
    if kind == "cell":
        return rows(c.cell_isosurface_domains(slots, _inputs([o["mesh"] for o in ops], device),
                                              bounds=True))
    if kind == "surface":
        sels = [o.get("select") for o in ops]
        return rows(c.cell_surface_domains(slots, _inputs([o["mesh"] for o in ops], device),
                                           None if all(s is None for s in sels)
                                           else _inputs(sels, device), bounds=True))
    if kind == "clip":
        return rows(c.cell_clip_domains(slots, _inputs([o["mesh"] for o in ops], device),
                                        [o["invert"] for o in ops], bounds=True))
    if kind == "stream":
        return rows(c.stream_tubes_domains(slots, _inputs([o["field"] for o in ops], device),
                                           [o["tube"] for o in ops], bounds=True)[0])
    if kind == "bstream":
        return rows(c.block_stream_tubes_domains(slots, _inputs([o["set"] for o in ops], device),
                                                 [o["tube"] for o in ops], bounds=True)[0])
    if kind == "glyphs":
        return rows(c.glyphs_domains(slots, _inputs([o["set"] for o in ops], device),
                                     [o["glyph"] for o in ops], bounds=True)[0])
    if kind == "build":
        cols = [o.get("colors") for o in ops]
        nrms = [o.get("normals") for o in ops]
        arrays = [[o["verts"] for o in ops], [o["faces"] for o in ops], cols, nrms]
        for j in range(n):   # device: tensors; else host and device mixed inside each job
            for a, arr in enumerate(arrays):
                if arr[j] is not None and (device or (a + j) % 2):
                    arr[j] = to_dev(arr[j])
        return rows(c.build_domains(slots, *arrays, bounds=True))
    if kind == "refit":
        vs, ns = [], []
        for o in ops:
            if "set" in o and device:   # verts and normals alone, straight into the refit
                (gv, gn, _, _, _), = c.glyphs(on_device([o["set"]]), [o["glyph"]],
                                              arrays=("verts", "normals"))
            else:
                gv, _, _, gn = restate(o)
                if device:
                    gv, gn = to_dev(gv), (None if gn is None else to_dev(gn))
            vs.append(gv)
            ns.append(gn)
        return rows(c.refit_domains(slots, vs, None if all(x is None for x in ns) else ns,
                                    bounds=True))
    if kind == "recolor":
        cols = []
        for o in ops:
            if device:
                cols.append(c.colormap_apply(to_dev(o["scalars"]), o["cmap"]))
            else:
                cols.append(restate(o)[2])
        c.recolor_domains(slots, cols)
        return {}
    if kind == "upload":
        for o in ops:
            c.upload_domain(o["slot"], o["verts"], o["faces"], o.get("colors"), o.get("normals"))
        return {}
    if kind == "release":
        for o in ops:
            c.release_domain(o["slot"])
        return {}
    raise KeyError(kind)


def buffers_call(c, o, device=True):
    """A caller-buffer glyph call: the list glyphs() returns (not synchronised)."""
    return c.glyphs(_inputs(o["sets"], device), [o["glyph"]] * len(o["sets"]))


def set_scene(c, session, k, box_rows=None):
    """The step's boxes (box_rows: rows from returned bounds replace the
    computed ones), maps, owners and BSDFs."""
    b = boxes(session, k)
    for d, row in (box_rows or {}).items():
        b[d] = row
    c.domain_bounds(b)   # also unmaps every domain
    for d, s in sorted(maps(session, k).items()):
        c.map_domain(d, s)
    c.set_owners(np.zeros(NDOM, np.int32))
    c.set_bsdfs(list(BSDFS))
    return b


def apply(c, session, k, device):
    """Step k's calls on context c, the slots of one kind batched into one
    call in the order the kinds first appear, then the step's scene state
    -> ({slot: bounds}, [glyph_buffers results], boxes).  In an "exact" step
    the boxes of the slots just written are the returned bounds."""
    step = session[k]
    assert good(step)
    order = []
    for o in step["ops"]:
        if o["kind"] not in order:
            order.append(o["kind"])
    bounds, outs = {}, []
    for kind in order:
        ops = [o for o in step["ops"] if o["kind"] == kind]
        if kind == "glyph_buffers":
            outs += [(o, buffers_call(c, o, device)) for o in ops]
        else:
            bounds.update(_call(c, kind, ops, device))
    rows = {}
    if step.get("boxes") == "exact":
        for d, s in maps(session, k).items():
            m = content(session, k, s)
            if s in bounds and m is not None and len(m[1]):
                rows[d] = bounds[s]
    return bounds, outs, set_scene(c, session, k, rows)


def attempt(c, step, device):
    """The rejected call of a step -> the error."""
    import pytest
    spray = _spray()
    r = step["reject"]
    with pytest.raises(spray.SprayRtError) as e:
        _call(c, r["kind"], r["ops"], device)
    return e.value


def replay(c, session, k, device):
    """The twin: on a fresh context each live slot's chain alone, one
    single-slot call at a time, then step k's scene state.  No history and
    another batch composition: what differs from the session context is
    carried state or batch dependence."""
    for s in live_slots(session, k):
        for o in chain(session, k, s):
            _call(c, o["kind"], [o], device)
    return set_scene(c, session, k)


def written(step):
    return sorted({o["slot"] for o in step["ops"] if o.get("slot") is not None})


def compare_slots(got, want, step, what="slot"):
    """{slot: bytes-or-dict} against another: the mismatches are named by step
    and slot."""
    bad = [(step, s) for s in sorted(set(got) | set(want)) if got.get(s) != want.get(s)]
    assert not bad, "%s bytes differ at (step, slot): %s" % (what, bad)


def mesh_image(m):
    """A restated mesh as the bytes compare_slots compares."""
    v, f, c, n = m
    return {"VERTS": v.tobytes(), "FACES": np.ascontiguousarray(f, np.uint32).tobytes(),
            "COLORS": b"" if c is None else np.ascontiguousarray(c, np.uint32).tobytes(),
            "NORMALS": b"" if n is None else np.ascontiguousarray(n, F32).tobytes()}


# ---- the session ----
def _mesh_op(kind, slot, name, oracle, which, d, deform=None):
    v, f = bh.mesh(which, oracle)
    v = place("build", v, d)
    if deform:
        v = rh.deform(deform, v)
    return op(kind, slot, name, verts=v, faces=f, colors=rh.vertex_colors(len(v)),
              normals=rh.vertex_normals(oracle, v, f))


def _glyph_cloud(n, seed, d, color_seed=None, arrows=False):
    p = gh.cloud(n, seed)
    S = gh.pset(p, vectors=gh.swirl(p, seed) if arrows else None)
    if color_seed is not None:
        S = gh.with_color(S, color_seed)
    return place("glyphs", S, d)


@functools.lru_cache(maxsize=None)
def session(oracle):
    """The session of test_session_host.py and test_gpu_session.py (domain d
    <-> slot d; slot 6 is never mapped)."""
    P = place
    sphere = cellh.sphere
    hex995 = cellh.hex_lattice((9, 9, 5), (-1, 2, 0.5), (0.5, 0.75, 1.25))
    spaced = sth.with_color(sth.small_cases()["spaced"], 7)
    tube = dict(radius=0.05, nsides=5, color=None)

    first = [
        op("iso", 0, "s0.iso0", grid=P("iso", colh.mapped(ih.ramp_grid((5, 5, 5), 0.0, 11), 21, 16), 0)),
        op("iso", 1, "s0.iso1", grid=P("iso", dict(ih.ramp_grid((5, 5, 5), 0.1, 12),
                                                   color=0x00C08040), 1)),
        _mesh_op("build", 2, "s0.build2", oracle, "grid12", 2),
        op("glyphs", 3, "s0.glyphs3", set=_glyph_cloud(12, 1, 3, 31), glyph=gh.sphere(0.4, 1)),
        op("stream", 4, "s0.stream4", field=P("stream", spaced, 4), tube=tube),
    ]
    s0 = dict(name="first", ops=first, maps={0: 0, 1: 1, 2: 2, 3: 3, 4: 4})

    grid12 = first[2]
    moved12 = rh.deform("sin", grid12["verts"])
    tet_big = th.mesh(*th.kuhn_mesh((7, 7, 7), (0, 0, 0), (0.6, 0.6, 0.6)), th.busy_f, 0.1,
                      normals=True, cmap_seed=14, ntable=256)
    surf_big = sfh.mesh(hex995, normals=True, cmap_seed=12, ntable=4096, clamp=0.3)
    g3 = restate(first[3])
    s1 = dict(name="map5", maps={5: 5}, ops=[
        op("tet", 0, "s1.tet0", mesh=P("tet", tet_big, 0)),
        op("cell", 1, "s1.cell1", mesh=P("cell", cellh.mesh(cellh.mixed_mesh(), sphere((1.0, 0.7, 0.8), 1.7),
                                                            0.0, normals=True, cmap_seed=16,
                                                            ntable=64), 1)),
        op("surface", 5, "s1.surface5", mesh=P("surface", surf_big, 5)),
        op("bstream", 4, "s1.bstream4", set=P("bstream", bsh.case("refined"), 4), tube=bsh.tube_of(0)),
        _mesh_op("upload", 6, "s1.upload6", oracle, "tri5", 0),
        op("refit", 2, "s1.refit2", verts=moved12,
           normals=rh.vertex_normals(oracle, moved12, grid12["faces"])),
        op("recolor", 3, "s1.recolor3", scalars=np.ascontiguousarray(g3[0][:, 1] + g3[0][:, 2]),
           cmap=(colh.table(64, 5), -3.0, 5.0)),
    ])

    bad_set = _glyph_cloud(9, 4, 1)
    bad_set["points"] = bad_set["points"].copy()
    bad_set["points"][5, 1] = np.nan
    r1 = dict(name="reject-glyphs", ops=[], reject=dict(kind="glyphs", expect=("set 1, slot 1",), ops=[
        op("glyphs", 3, "r1.good", set=_glyph_cloud(9, 3, 3), glyph=gh.sphere(0.3, 0, 0x00334455)),
        op("glyphs", 1, "r1.bad", set=bad_set, glyph=gh.sphere(0.3, 0, 0x00334455))]))

    clip_small = cellh.mesh(cellh.hex_lattice((4, 4, 4), seed=5), clh.x_minus(1.5), 0.0,
                            normals=True, cmap_seed=19, ntable=32)
    s2 = dict(name="samekey-rebuilt", ops=[
        op("clip", 1, "s2.clip1", mesh=P("clip", clip_small, 1), invert=False),
        _mesh_op("build", 2, "s2.build2", oracle, "grid12", 2, deform="flatten"),
        op("release", 6, "s2.release6"),
        op("glyphs", 3, "s2.glyphs3", set=_glyph_cloud(20, 2, 3, arrows=True),
           glyph=gh.arrow(0.6, 5, color=0x0040C0F0)),
    ])

    miss = ih.grid(ih.sphere_f(ih.lattice((6, 5, 4))), iso=100.0)
    dropped = gh.small_cases()["all_dropped"]
    s3 = dict(name="exact-boxes-empties", boxes="exact", ops=[
        op("surface", 5, "s3.surface5", mesh=P("surface", sfh.mesh(cellh.one_cell(cellh.HEX, 2), normals=True,
                                                                    cmap_seed=15, ntable=8), 5)),
        op("tet", 0, "s3.tet0", mesh=P("tet", th.mesh(*th.five_tet_cube(), sphere((0.2, 0.1, 0.3), 0.9), 0.0,
                                                      normals=True, color=0x00123456), 0)),
        op("iso", 1, "s3.iso1-empty", grid=P("iso", miss, 1)),
        op("glyphs", 3, "s3.glyphs3-empty", set=P("glyphs", dropped[0], 3), glyph=dropped[1]),
        op("stream", 4, "s3.stream4", field=P("stream", sth.small_cases()["dyadic"], 4),
           tube=dict(radius=0.125, nsides=3, color=0x00F0A020)),
    ])

    bad_build = _mesh_op("build", 6, "r2.bad", oracle, "grid12", 2)
    bad_build["faces"] = bad_build["faces"].copy()
    bad_build["faces"][7, 2] = len(bad_build["verts"])
    r2 = dict(name="reject-build", ops=[], reject=dict(kind="build", expect=("slot 6",), ops=[
        _mesh_op("build", 2, "r2.good", oracle, "tri1", 2), bad_build]))

    big = _glyph_cloud(140, 6, 2, 33)
    big_glyph = gh.sphere(0.25, 2)
    s4 = dict(name="large", boxes="slack", ops=[
        op("glyphs", 2, "s4.glyphs2-large", set=big, glyph=big_glyph),
        op("cell", 1, "s4.cell1", mesh=P("cell", cellh.mesh(cellh.hex_lattice((5, 5, 5), seed=7),
                                                            sphere((2.0, 2.1, 1.9), 1.5), 0.0,
                                                            normals=True, cmap_seed=11, ntable=16), 1)),
        op("stream", 3, "s4.stream3", field=P("stream", spaced, 3), tube=tube),
        _mesh_op("upload", 6, "s4.upload6", oracle, "tri4", 0),
    ])

    moved = dict(big, points=(big["points"] + np.array([0.25, -0.125, 0.375], F32)).astype(F32))
    s5v = restate(s3["ops"][0])[0]
    s5 = dict(name="samekey", ops=[
        op("refit", 2, "s5.refit2-glyphs", set=moved, glyph=big_glyph),
        op("recolor", 5, "s5.recolor5", scalars=np.ascontiguousarray(s5v[:, 0] + 2 * s5v[:, 1]),
           cmap=(colh.table(7, 9), float(s5v[:, 0].min()), float(s5v[:, 0].max() + 3.0))),
    ])

    ones = [P("glyphs", gh.pset(gh.cloud(1, 100 + i)), 0) for i in range(300)]
    s6 = dict(name="release-unmap", maps={4: -1}, ops=[
        op("release", 4, "s6.release4"),
        op("glyph_buffers", None, "s6.glyphs-300", sets=ones, glyph=gh.sphere(0.2, 0, 0x00203040)),
        op("bstream", 0, "s6.bstream0", set=P("bstream", bsh.case("one_block"), 0), tube=bsh.tube_of(3)),
        op("iso", 5, "s6.iso5", grid=P("iso", dict(ih.sphere_grid(), color=0x00123456), 5)),
    ])

    good_cell = cellh.mesh(cellh.one_cell(cellh.HEX, 2), sphere((0.3, 0.2, 0.1), 0.8), 0.0,
                           normals=True, color=0x00123456)
    bad_cell = cellh.mesh(cellh.hex_lattice((4, 3, 3)), th.wave_f, 0.3, normals=True)
    bad_cell["conn"] = bad_cell["conn"].copy()
    bad_cell["conn"][8 * 5 + 1] = len(bad_cell["points"])
    r3 = dict(name="reject-cell", ops=[], reject=dict(
        kind="cell", expect=("cell isosurface (mesh 1, slot 0)",),
        ops=[op("cell", 1, "r3.good", mesh=good_cell), op("cell", 0, "r3.bad", mesh=bad_cell)]))

    s7 = dict(name="remap4", maps={4: 4}, ops=[
        op("glyphs", 3, "s7.glyphs3-single", set=_glyph_cloud(5, 8, 3, 35), glyph=gh.sphere(0.5, 1)),
        op("stream", 4, "s7.stream4", field=P("stream", sth.with_color(sth.small_cases()["spaced"], 3), 4),
           tube=dict(radius=0.3, nsides=6, color=None)),
        op("tet", 0, "s7.tet0", mesh=P("tet", th.mesh(*th.kuhn_mesh((5, 5, 5)), sphere((2.1, 1.9, 2.2), 1.6), 0.0,
                                                      normals=True, cmap_seed=11, ntable=16), 0)),
        op("cell", 1, "s7.cell1", mesh=s1["ops"][1]["mesh"]),
        op("surface", 5, "s7.surface5", mesh=P("surface", sfh.mesh(sfh.conforming_mesh(), normals=True,
                                                                    cmap_seed=16, ntable=64), 5)),
        op("clip", 2, "s7.clip2", mesh=P("clip", cellh.mesh(hex995, th.wave_f, 0.3, normals=True,
                                                            cmap_seed=12, ntable=4096, clamp=0.3), 2),
           invert=True),
        _mesh_op("build", 6, "s7.build6", oracle, "tri5", 0),
    ])

    s8 = dict(name="round-trip", ops=list(first))
    return (s0, s1, r1, s2, s3, r2, s4, s5, s6, r3, s7, s8)


# the steps the tests name
FIRST, MAP5, SAMEKEY, LARGE, ANCHOR = 0, 1, 7, 6, 10

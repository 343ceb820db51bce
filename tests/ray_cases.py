"""A small multi-domain scene, the hard ray classes and a float64 reference
for the scene-path tests (test_ray_cases.py, test_gpu_ray_cases.py), and the
same classes as the eye rays of in-situ frames with their partitions,
shading set-up and whole-scene reference frame (test_insitu_ray_cases.py,
test_gpu_insitu_ray_cases.py).  The scene, the classes and the float64
reference are pure numpy; whatever needs the oracle (the `extents` and
`nonfinite` classes start from hitting rays) takes the oracle's scene as an
argument, and the in-situ helpers (frame_reference, cross_rank_ties) import
insitu_helpers, and with it torch, when they are called.

Scene: eight touching domains in a 2 x 2 x 2 arrangement of 4-unit cells plus
one curved domain.  A lattice domain is the welded surface of three cubes
with integer vertex coordinates:
  A  2 x 2 x 2 in 1 x 1 quads (48 triangles), one face in the cell's inner x
     plane: the x neighbour's A has the same face there, so the two domains
     hold coincident triangles, their boxes touch in that plane and the
     leaves of those faces have zero thickness;
  B  2 x 2 x 2 in 2 x 2 quads (12 triangles), one face in the inner z plane
     (coincident with the z neighbour's), one face partly on a face of A
     (coplanar, overlapping triangles inside one domain);
  C  2 x 2 x 2 in 1 x 1 quads (48 triangles) towards the outer corner, at a
     position that differs per domain.
The curved domain is the `grid` bump of refit_helpers (8 x 8 quads), scaled
and set across the top four domains.  A domain's box is its mesh bound.
"""
import numpy as np

from conftest import edge_rays, random_rays
from refit_helpers import _grid

F32 = np.float32
CELL = 4
NDOM = 9
LARGE = 1.0e4  # the large-coordinate variant's translation (every axis)
CLASSES = ("axis_off", "axis_lattice", "tiny", "edge", "surface", "extents", "random")
TNEAR, TFAR = F32(0.001), F32(np.inf)
# the in-situ partitions of the scene over two ranks (test_insitu_ray_cases.py):
# domain 4i + 2j + k on rank (i + j + k) % 2 and the curved domain on rank 0,
# so every x pair and z pair that shares coincident triangles is split; and
# every domain on rank 1 (rank 0 holds rays only)
OWNER_CHECKER = tuple((i + j + k) % 2 for i in (0, 1) for j in (0, 1) for k in (0, 1)) + (0,)
OWNER_ONE = (1,) * NDOM


# --------------------------------------------------------------------------
# scene
# --------------------------------------------------------------------------
def _cube(lo, size, step):
    """Quads of an axis-aligned cube's surface, `step` units wide, as
    triangles over unwelded integer corner points."""
    lo = np.asarray(lo, np.int64)
    tris = []
    for ax in range(3):
        o1, o2 = (ax + 1) % 3, (ax + 2) % 3
        for side in (0, size):
            for s in range(0, size, step):
                for t in range(0, size, step):
                    q = []
                    for ds, dt in ((0, 0), (step, 0), (step, step), (0, step)):
                        p = lo.copy()
                        p[ax] += side
                        p[o1] += s + ds
                        p[o2] += t + dt
                        q.append(p)
                    tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.array(tris, np.int64)  # [nt, 3, 3]


def _lattice_domain(i, j, k):
    """Local coordinates count away from the scene's centre planes: global =
    4 - local for cell index 0, 4 + local for cell index 1."""
    a_lo = (0, (j + k) % 2, 2 * j)           # A: the face local x = 0
    b_lo = (2, 1, 0)                         # B: the face local z = 0
    c_lo = (1 + (i + j) % 2, 2, 2 - (k + i) % 2)
    tris = np.concatenate([_cube(a_lo, 2, 1), _cube(b_lo, 2, 2), _cube(c_lo, 2, 1)])
    sign = np.array([1 if c else -1 for c in (i, j, k)], np.int64)
    pts = CELL + tris.reshape(-1, 3) * sign
    verts, inv = np.unique(pts, axis=0, return_inverse=True)  # weld
    return verts.astype(F32), inv.reshape(-1, 3).astype(np.uint32)


def build_scene(offset=0.0):
    """[(verts float32 [nv, 3], faces uint32 [nf, 3])] * NDOM, boxes [NDOM, 6]."""
    meshes = [_lattice_domain(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    gv, gf = _grid(8)
    gv = (gv * F32(0.6) + np.array([4.3, 3.9, 6.6], F32)).astype(F32)
    meshes.append((gv, gf))
    off = F32(offset)
    meshes = [((v + off).astype(F32), np.ascontiguousarray(f)) for v, f in meshes]
    boxes = np.stack([np.concatenate([v.min(0), v.max(0)]) for v, _ in meshes]).astype(F32)
    return meshes, boxes


def merged(meshes):
    """All domains as one mesh (faces re-indexed), for the float64 reference
    and the builders that aim at triangles."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f.astype(np.int64) + base)
        base += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.uint32)


def lattice_planes(meshes):
    """[(axis, coordinate)] of the lattice planes that hold whole triangles."""
    out = set()
    for v, f in meshes[:8]:
        tri = v[f]  # [nf, 3, 3]
        for ax in range(3):
            flat = (tri[:, 0, ax] == tri[:, 1, ax]) & (tri[:, 0, ax] == tri[:, 2, ax])
            out |= {(ax, float(c)) for c in np.unique(tri[flat, 0, ax])}
    return sorted(out)


# --------------------------------------------------------------------------
# ray classes: dict(org, dir, tnear, tfar), float32
# --------------------------------------------------------------------------
def _pack(org, d, tnear=None, tfar=None, **extra):
    n = len(org)
    r = dict(org=np.ascontiguousarray(org, F32), dir=np.ascontiguousarray(d, F32),
             tnear=np.full(n, TNEAR, F32) if tnear is None else np.ascontiguousarray(tnear, F32),
             tfar=np.full(n, TFAR, F32) if tfar is None else np.ascontiguousarray(tfar, F32))
    r.update(extra)
    return r


def _signed_zero(rng, n):
    return np.where(rng.integers(0, 2, n) == 0, F32(0.0), F32(-0.0)).astype(F32)


def _axis(rng, n, offset, planes=None):
    off = float(offset)
    ax = rng.integers(0, 3, n)
    fwd = rng.integers(0, 2, n) == 0
    # transverse coordinates off the lattice: integer + [0.05, 0.95]
    org = rng.integers(-1, 9, size=(n, 3)) + rng.uniform(0.05, 0.95, size=(n, 3)) + off
    if planes is not None:  # one transverse coordinate exactly on a plane
        pick = rng.integers(0, len(planes), n)
        for r in range(n):
            pa, pc = planes[pick[r]]
            if pa == ax[r]:  # a plane across the ray: use the next axis instead
                pa = (pa + 1) % 3
                pc = [c for a, c in planes if a == pa][pick[r] % sum(a == pa for a, _ in planes)]
            org[r, pa] = pc
    inside = rng.uniform(size=n) < 0.25  # a quarter starts inside the scene
    rows = np.arange(n)
    start = np.where(fwd, -3.0, 11.0) + off
    org[rows, ax] = np.where(inside, org[rows, ax], start)
    d = np.stack([_signed_zero(rng, n) for _ in range(3)], 1)
    d[rows, ax] = np.where(fwd, 1.0, -1.0)
    return _pack(org, d)


def axis_off(rng, n, meshes, offset=0.0):
    """Axis-parallel rays, both travel directions, the two zero components
    drawn from {+0.0, -0.0}, origins off the lattice."""
    return _axis(rng, n, offset)


def axis_lattice(rng, n, meshes, offset=0.0):
    """axis_off with one origin coordinate exactly on a lattice plane that
    holds triangles: the ray lies in that plane (grazing)."""
    return _axis(rng, n, offset, lattice_planes(meshes))


TINY = (1e-30, -1e-30, 1e-40, -1e-40, 1e-20, -1e-20, 1.0000001e-20, -1.0000001e-20, 3e-39,
        1e-8, -1e-8)


def tiny(rng, n, meshes, offset=0.0):
    """One dominant direction component, the others from TINY: below, at and
    just above the kernels' direction clamp (1e-20), subnormals, and 1e-8."""
    r = _axis(rng, n, offset)
    vals = np.array(TINY, np.float64).astype(F32)  # 1e-40, 3e-39 stay subnormal
    small = r["dir"] == 0
    r["dir"][small] = vals[rng.integers(0, len(vals), int(small.sum()))]
    return r


def edge(rng, n, meshes, offset=0.0):
    """conftest.edge_rays over the merged mesh (aimed at vertices and edge
    midpoints), half from the near shell, half moved back along the ray to
    about 1000 scene extents."""
    v, f = merged(meshes)
    org, d = edge_rays(rng, v, f, n)
    ext = float(np.linalg.norm(v.max(0) - v.min(0)))
    far = np.arange(n) % 2 == 1
    o64 = org.astype(np.float64)
    o64[far] -= d[far].astype(np.float64) * 1000.0 * ext
    return _pack(o64.astype(F32), d)


def surface(rng, n, meshes, offset=0.0):
    """Origins on triangles of the lattice domains (v0 + u e1 + v e2 in
    float32 is exactly in such a triangle's plane; on a curved triangle at
    coordinates of 1e4 it is up to 1e-3 off it, as far as tnear), random
    directions: shadow rays, whose t = 0 self-hit must fall to tnear."""
    v, f = merged(meshes[:8])
    tri = v[f[rng.integers(0, len(f), n)]]
    uv = rng.uniform(0.02, 0.98, size=(n, 2))
    flip = uv.sum(1) > 1.0
    uv[flip] = 1.0 - uv[flip]
    u, w = uv[:, :1].astype(F32), uv[:, 1:].astype(F32)
    org = (tri[:, 0] + u * (tri[:, 1] - tri[:, 0]) + w * (tri[:, 2] - tri[:, 0])).astype(F32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _pack(org, d)


def random(rng, n, meshes, offset=0.0):
    c = np.array([4.0, 4.0, 4.0]) + float(offset)
    return _pack(*random_rays(rng, n, c, 9.0))


def _hitting(rng, n, meshes, offset, osc):
    """n generic rays that hit with the default extents, and their hits."""
    r = random(rng, 4 * n, meshes, offset)
    h, _ = osc.intersect(r["org"], r["dir"])
    sel = np.flatnonzero(h["domain"] >= 0)[:n]
    assert len(sel) == n
    return r["org"][sel], r["dir"][sel], h[sel]


EXTENT_CASES = ("tfar_eq", "tfar_below", "tnear_eq", "bracket_later", "tfar_lt_tnear",
                "tfar_zero", "tnear_zero", "tnear_neg")


def extents(rng, n, meshes, offset, osc, domain_query, boxes):
    """Generic hitting rays with extents derived from the oracle's own hit
    distances under the default extents (t1: the first surface):
      tfar_eq        tfar = t1                      accepted
      tfar_below     tfar = nextafter(t1, 0)        a miss
      tnear_eq       tnear = t1                     strict: the next surface
      bracket_later  (tnear, tfar] holds only a hit of a later entry of the
                     ray's domain list
      tfar_lt_tnear  tnear past t1, tfar before it  a miss
      tfar_zero      tfar = 0                       a miss
      tnear_zero, tnear_neg   tnear = 0, -1         the default hit
    Returns the class with `case` (index into EXTENT_CASES) and `t1`."""
    org, d, h1 = _hitting(rng, 2 * n, meshes, offset, osc)
    t1 = h1["t"].copy()
    # the surface after t1, and the one after that (t = +inf: none)
    h2, _ = osc.intersect(org, d, tnear=t1 * F32(1.001))
    t2 = h2["t"]
    h3, _ = osc.intersect(org, d, tnear=t2 * F32(1.001))
    t3 = h3["t"]
    ids, _, cnt, _ = domain_query(org, d, boxes, len(boxes))
    pos2 = np.array([list(ids[r, :cnt[r]]).index(h2["domain"][r]) if h2["domain"][r] >= 0 else -1
                     for r in range(len(org))])
    later = np.flatnonzero((pos2 >= 1) & (h2["domain"] != h1["domain"]))[: n // 8]
    assert len(later) >= n // 16, len(later)
    rest = np.setdiff1d(np.arange(len(org)), later)[: n - len(later)]
    others = [c for c in range(len(EXTENT_CASES)) if c != 3]
    case = np.concatenate([np.full(len(later), 3), np.array(others)[np.arange(len(rest)) % 7]])
    sel = np.concatenate([later, rest])
    perm = rng.permutation(n)
    sel, case = sel[perm], case[perm]
    org, d, t1, t2, t3 = org[sel], d[sel], t1[sel], t2[sel], t3[sel]
    tn = np.full(n, TNEAR, F32)
    tf = np.full(n, TFAR, F32)
    c = case
    tf[c == 0] = t1[c == 0]
    tf[c == 1] = np.nextafter(t1[c == 1], F32(0))
    tn[c == 2] = t1[c == 2]
    tn[c == 3] = (t1[c == 3] + t2[c == 3]) * F32(0.5)
    end3 = np.where(np.isfinite(t3), (t2 + t3) * F32(0.5), t2 * F32(2.0)).astype(F32)
    tf[c == 3] = end3[c == 3]
    tn[c == 4] = t1[c == 4] * F32(1.5)
    tf[c == 4] = t1[c == 4] * F32(0.5)
    tf[c == 5] = F32(0.0)
    tn[c == 6] = F32(0.0)
    tn[c == 7] = F32(-1.0)
    return _pack(org, d, tn, tf, case=case, t1=t1)


PLANTS = ("org_nan", "org_pinf", "org_ninf", "dir_nan", "dir_pinf", "dir_ninf", "dir_zero",
          "tnear_nan", "tfar_nan")


def nonfinite(rng, n, meshes, offset, osc):
    """Ordinary hitting rays; every fourth record has one of PLANTS planted
    (`planted`: index into PLANTS, -1 for the untouched neighbours)."""
    org, d, _ = _hitting(rng, n, meshes, offset, osc)
    r = _pack(org.copy(), d.copy())
    planted = np.full(n, -1)
    rows = np.arange(0, n, 4)
    planted[rows] = np.arange(len(rows)) % len(PLANTS)
    comp = rng.integers(0, 3, n)
    bad = {0: np.nan, 1: np.inf, 2: -np.inf}
    for i in rows:
        p = planted[i]
        if p < 3:
            r["org"][i, comp[i]] = bad[p]
        elif p < 6:
            r["dir"][i, comp[i]] = bad[p - 3]
        elif p == 6:
            r["dir"][i] = 0.0
        elif p == 7:
            r["tnear"][i] = np.nan
        else:
            r["tfar"][i] = np.nan
    r["planted"] = planted
    return r


def mixed(classes):
    """Round-robin interleaving of the given classes (dicts): neighbouring
    lanes of a wave hold different classes."""
    k = len(classes)
    n = min(len(c["org"]) for c in classes) * k
    out = {}
    for key in ("org", "dir", "tnear", "tfar"):
        a = np.stack([c[key][: n // k] for c in classes], 1)
        out[key] = np.ascontiguousarray(a.reshape((n,) + a.shape[2:]))
    return out


def make_classes(seed, n, meshes, boxes, offset, osc, domain_query):
    """Every class of CLASSES plus `nonfinite` and `mixed`, seeded."""
    out = {}
    for k, name in enumerate(CLASSES):
        rng = np.random.default_rng(1000 * seed + k)
        if name == "extents":
            out[name] = extents(rng, n, meshes, offset, osc, domain_query, boxes)
        else:
            out[name] = globals()[name](rng, n, meshes, offset)
    out["nonfinite"] = nonfinite(np.random.default_rng(1000 * seed + 99), n, meshes, offset, osc)
    out["mixed"] = mixed([out[c] for c in CLASSES])
    return out


# --------------------------------------------------------------------------
# float64 reference
# --------------------------------------------------------------------------
BARY_MARGIN = 1e-5  # tests/test_oracle.py, oracle.c or_f64_intersect
T_RTOL = 1e-4       # the north-star tolerance on t
EPS32 = 2.0 ** -24  # float32 unit roundoff


def f64_reference(verts, faces, org, d, tnear, tfar, chunk=256):
    """Brute force over all triangles in double, from the float32 inputs.
    Returns dict(hit, t, ambiguous): for a ray that is not ambiguous, `hit`
    says whether a surface lies in (tnear, tfar] and `t` is the nearest.

    A candidate is a crossing with every barycentric >= -margin; it is
    robust with every barycentric >= margin and within the margin otherwise.
    A ray is ambiguous when
      * a candidate within the margin is nearer than its nearest robust hit
        (or is its only candidate);
      * it lies in the plane of a triangle whose interior or boundary its
        line crosses inside the extents;
      * a candidate's t is within T_RTOL relative of tnear or tfar;
      * float32 cannot resolve its nearest robust hit's t to T_RTOL.

    margin is BARY_MARGIN, or what float32 can resolve where that is more:
    with C = v0 - org rounded to float32 (relative error eps = 2^-24 per
    component), R = dir x C carries about 3 eps |dir| |C|, U = R . e (one
    more product and two sums) about 6 eps |dir| |C| |e|, and den = Ng . dir
    with Ng = e1 x e2 rounded about 4 eps |Ng| |dir|, so
      |du| <= 8 eps (|dir| |C| (|e1| + |e2|) + |Ng| |dir|) / |den|
    (8: the 6 above and slack for the division).  For a ray from 1000 scene
    extents away this is about 1e-3, a hundred times BARY_MARGIN: which of
    two triangles at an edge such a ray hits is not decided in float32, by
    this intersector or any other.  Likewise T = Ng . C carries 4 eps |Ng|
    |C|, so the relative error of t = T / den is bounded by
      8 eps (|Ng| |C| / |Ng . C| + |Ng| |dir| / |den|),
    beyond T_RTOL only for far origins at grazing incidence."""
    v = verts.astype(np.float64)
    A, B, C = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2 = B - A, C - A
    nrm = np.cross(e1, e2)
    nlen = np.linalg.norm(nrm, axis=1)
    elen = np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)
    n = len(org)
    hit = np.zeros(n, bool)
    tout = np.full(n, np.inf)
    amb = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            o = org[s:s + chunk].astype(np.float64)[:, None, :]
            dd = d[s:s + chunk].astype(np.float64)[:, None, :]
            tn = tnear[s:s + chunk].astype(np.float64)[:, None]
            tf = tfar[s:s + chunk].astype(np.float64)[:, None]
            p = np.cross(dd, e2[None])
            det = (e1[None] * p).sum(-1)
            sv = o - A[None]
            u = (sv * p).sum(-1) / det
            q = np.cross(sv, e1[None])
            w = (dd * q).sum(-1) / det
            t = (e2[None] * q).sum(-1) / det
            m = np.minimum(np.minimum(u, w), 1.0 - u - w)
            # what float32 can resolve (see the docstring)
            dl = np.linalg.norm(dd, axis=-1)
            sl = np.linalg.norm(sv, axis=-1)
            shape = dl * nlen[None] / np.abs(det)
            mg = np.maximum(BARY_MARGIN, 8 * EPS32 * (dl * sl * elen[None] / np.abs(det) + shape))
            t_err = 8 * EPS32 * (nlen[None] * sl / np.abs((sv * nrm[None]).sum(-1)) + shape)
            cand = (det != 0) & (m >= -mg)
            near_tn = np.abs(t - tn) <= T_RTOL * np.maximum(np.abs(t), np.abs(tn))
            near_tf = np.isfinite(tf) & \
                (np.abs(t - tf) <= T_RTOL * np.maximum(np.abs(t), np.abs(tf)))
            inside = cand & (t > tn) & (t <= tf)
            robust = inside & (m >= mg)
            marginal = inside & ~robust
            k_rob = np.where(robust, t, np.inf).argmin(1)
            t_rob = np.where(robust, t, np.inf).min(1)
            t_mar = np.where(marginal, t, np.inf).min(1)
            a = t_mar <= t_rob * (1.0 + T_RTOL)
            a &= np.isfinite(t_mar)
            a |= (cand & (near_tn | near_tf)).any(1)
            a |= np.isfinite(t_rob) & (t_err[np.arange(len(o)), k_rob] > T_RTOL)
            # rays in a triangle's plane: clip the line to the triangle
            dlen = np.linalg.norm(dd, axis=-1)
            scale = np.abs(A).max() + 1.0
            copl = (np.abs((dd * nrm[None]).sum(-1)) <= 1e-6 * dlen * nlen[None]) & \
                   (np.abs((sv * nrm[None]).sum(-1)) <= 1e-6 * scale * nlen[None])
            if copl.any():
                r_i, t_i = np.nonzero(copl)
                lo = np.full(len(r_i), -np.inf)
                hi = np.full(len(r_i), np.inf)
                P = [A[t_i], B[t_i], C[t_i]]
                oo, dv = o[r_i, 0], dd[r_i, 0]
                for k in range(3):
                    ev = P[(k + 1) % 3] - P[k]
                    inward = np.cross(nrm[t_i], ev)  # in-plane, towards the inside
                    f0 = ((oo - P[k]) * inward).sum(-1)
                    f1 = (dv * inward).sum(-1)
                    slack = 1e-6 * np.linalg.norm(inward, axis=1) * scale
                    tc = -(f0 + slack) / f1
                    lo = np.where(f1 > 0, np.maximum(lo, tc), lo)
                    hi = np.where(f1 < 0, np.minimum(hi, tc), hi)
                    dead = (f1 == 0) & (f0 + slack < 0)
                    hi = np.where(dead, -np.inf, hi)
                over = (lo <= hi) & (hi > tn[r_i, 0]) & (lo <= tf[r_i, 0])
                a[np.unique(r_i[over])] = True
            hit[s:s + chunk] = np.isfinite(t_rob)
            tout[s:s + chunk] = t_rob
            amb[s:s + chunk] = a
    return dict(hit=hit, t=tout, ambiguous=amb)


# --------------------------------------------------------------------------
# the fixture both test modules share (built once per process and variant)
# --------------------------------------------------------------------------
SEED, NRAYS = 7, 1024
_VARIANTS = {}


def variant(oracle, offset):
    """dict(meshes, boxes, colors, normals, osc, classes, verts, faces) of the
    scene translated by `offset`; nobody may write into it."""
    from refit_helpers import vertex_colors, vertex_normals
    if offset not in _VARIANTS:
        meshes, boxes = build_scene(offset)
        colors = [vertex_colors(len(v)) for v, _ in meshes]
        normals = [vertex_normals(oracle, v, f) for v, f in meshes]
        osc = oracle.Scene(NDOM)
        for i, (v, f) in enumerate(meshes):
            osc.set_domain(i, v, f, colors[i], normals[i], boxes[i])
        classes = make_classes(SEED, NRAYS, meshes, boxes, offset, osc, oracle.domain_query)
        V, F = merged(meshes)
        _VARIANTS[offset] = dict(meshes=meshes, boxes=boxes, colors=colors, normals=normals,
                                 osc=osc, classes=classes, verts=V, faces=F, ref={})
    return _VARIANTS[offset]


def oracle_results(var, name):
    """(hits, occluded, counts of intersect, counts of occluded) of the
    extended oracle on class `name`, computed once."""
    if name not in var["ref"]:
        c = var["classes"][name]
        h, hc = var["osc"].intersect(c["org"], c["dir"], tnear=c["tnear"], tfar=c["tfar"])
        o, oc = var["osc"].occluded(c["org"], c["dir"], tnear=c["tnear"], tfar=c["tfar"])
        var["ref"][name] = (h, o, hc, oc)
    return var["ref"][name]


def frame_inputs(var, name, spp=2):
    """Class `name` as the eye rays of an in-situ frame: dict(org, dir, pix,
    sam, w, h, spp) with pixid = i // spp (a pixel's samples adjacent, the
    in-situ order), samid = i, and the smallest near-square image that holds
    ceil(n / spp) pixels.  The in-situ forms take radiance rays with the
    default extents (tnear 0.001, tfar +inf), so the class's own tnear / tfar
    are not part of the frame."""
    c = var["classes"][name]
    n = len(c["org"])
    npix = -(-n // spp)
    w = int(np.ceil(np.sqrt(npix)))
    h = -(-npix // w)
    i = np.arange(n, dtype=np.int32)
    return dict(org=c["org"], dir=c["dir"], pix=(i // spp).astype(np.int32), sam=i, w=w, h=h,
                spp=spp)


# the shading set-up of the in-situ frames on this scene, the same on the
# oracle's and the engine's side: one point light that moves with the scene,
# every domain diffuse, ks 0.4, shininess 10
SHADING = {"pt1": ("pt", 1, 1), "pt3": ("pt", 3, 2), "ao4": ("ao", 1, 4)}  # kind, bounces, samples
BSDFS = ((0, 0.8, 0.7, 0.6),) * NDOM
KS, SHININESS = (0.4, 0.4, 0.4), 10.0


def frame_lights(offset):
    off = float(offset)
    return [(0, 4.0 + off, 30.0 + off, 60.0 + off, 1.0, 1.0, 1.0)]


def frame_shader(make, offset, case):
    """make: pyoracle.shader or spray_amd.frame.make_shader."""
    kind, bounces, samples = SHADING[case]
    return make(kind, bounces, samples, KS, SHININESS, frame_lights(offset))


def frame_reference(oracle, var, offset, name, case, inputs=None):
    """(records, image, totals) of the whole-scene reference frame
    (insitu_helpers.reference_frame_rays) on frame_inputs(var, name), or on
    `inputs` (then `name` is only a label); computed once per set of eye
    rays and shading case."""
    import hashlib
    import insitu_helpers as H
    fi = frame_inputs(var, name) if inputs is None else inputs
    rays = hashlib.sha1(np.ascontiguousarray(fi["org"]).tobytes() +
                        np.ascontiguousarray(fi["dir"]).tobytes()).hexdigest()
    key = ("frame", name, case, rays, fi["w"], fi["h"], fi["spp"])
    if key not in var["ref"]:
        sh = frame_shader(oracle.shader, offset, case)
        var["ref"][key] = H.reference_frame_rays(oracle, sh, list(BSDFS), var["osc"], fi["org"],
                                                 fi["dir"], fi["pix"], fi["sam"], fi["w"],
                                                 fi["h"], fi["spp"])
    return var["ref"][key]


def bounce_counts(ref, bounce):
    """(hits, shadow rays, occluded shadow rays) of one bounce of a frame's
    reference records."""
    rows = [v for (b, _), v in ref.items() if b == bounce]
    return (len(rows), sum(bin(v[1]).count("1") for v in rows),
            sum(bin(v[2]).count("1") for v in rows))


def cross_rank_ties(oracle, var, owner, org, d):
    """Indices of the rays on which both ranks of the two-rank partition
    `owner` hit at the same t bits (the winning ones: the list position
    decides), from the oracle alone."""
    import insitu_helpers as H
    meshes = (var["meshes"], var["boxes"], var["colors"], var["normals"])
    rays = H.rays_tensor(org, d)
    keys = [H.OracleLocal(oracle, owner, r, meshes=meshes).intersect_keyed(rays)[1].numpy()
            for r in (0, 1)]
    both = (keys[0] != H.MISS_KEY) & (keys[1] != H.MISS_KEY)
    return np.flatnonzero(both & ((keys[0] >> 32) == (keys[1] >> 32)))


def check_against_f64(var, name, hit, t=None):
    """The float64 statement on robust rays: the same hit or miss, and t
    (closest hit; None for an any hit) within T_RTOL relative.  Returns the
    ambiguous flags."""
    c = var["classes"][name]
    key = ("f64", name)
    if key not in var["ref"]:
        var["ref"][key] = f64_reference(var["verts"], var["faces"], c["org"], c["dir"],
                                        c["tnear"], c["tfar"])
    ref = var["ref"][key]
    ok = ~ref["ambiguous"]
    bad = np.flatnonzero(ok & (hit != ref["hit"]))
    assert len(bad) == 0, (name, len(bad), bad[:8])
    if t is None:
        return ref["ambiguous"]
    both = ok & hit
    rel = np.abs(t[both] - ref["t"][both]) / np.abs(ref["t"][both])
    assert len(rel) == 0 or rel.max() < T_RTOL, (name, rel.max())
    return ref["ambiguous"]

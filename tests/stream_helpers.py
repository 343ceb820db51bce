"""A numpy restatement of the streamline rule and the fields and seeds shared
by the streamline tests (test_streamlines_host.py, test_gpu_streamlines.py,
test_stream_cases.py, test_gpu_stream_cases.py; the hard classes are in
stream_cases.py).

Written from the rule in include/spray_rt.h, step by step, not from the C
code: sample, step, lines, tangent and frame, tube.  Every operation is one
numpy operation on scalars or 3-vectors of one dtype (float32 for the byte
comparisons, float64 for the error estimate of the rotation test), so nothing
is contracted and division and square root are correctly rounded.  The ring
table is the library's (spray_amd.tube_ring).  `stats` counts the paths a case
reaches.
"""
import collections

import numpy as np

import color_helpers as ch

F32 = np.float32
FORWARD, BACKWARD, BOTH = 0, 1, 2
GRID, STEPS, SPEED, SEED = 0, 1, 2, 3


def field(vectors, seeds, step, max_steps, direction=FORWARD, min_speed=1e-6,
          origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), cfield=None, cmap=None):
    return dict(vectors=np.ascontiguousarray(vectors, F32),
                seeds=np.ascontiguousarray(seeds, F32).reshape(-1, 3), step=step,
                max_steps=max_steps, direction=direction, min_speed=min_speed, origin=origin,
                spacing=spacing, cfield=cfield, cmap=cmap)


def host_args(f):
    """The positional arguments of the host forms."""
    return (f["vectors"], f["origin"], f["spacing"], f["seeds"], f["step"], f["max_steps"])


def host_kw(f):
    return dict(direction=f["direction"], min_speed=f["min_speed"])


# ---- the rule ----

def lerp(a, b, t):
    return a + t * (b - a)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


class Rule:
    """The rule over one field in dtype F."""

    def __init__(self, f, F=F32, stats=None):
        self.F = F
        self.v = np.asarray(f["vectors"], F)
        self.dims = self.v.shape[2], self.v.shape[1], self.v.shape[0]
        self.origin = np.asarray(f["origin"], F32).astype(F)
        self.spacing = np.asarray(f["spacing"], F32).astype(F)
        self.step = F(F32(f["step"]))
        self.max_steps = int(f["max_steps"])
        ms = F(F32(f["min_speed"]))
        self.msq = ms * ms
        self.cfield = None if f.get("cfield") is None else np.asarray(f["cfield"], F)
        self.cmap = f.get("cmap")
        self.stats = collections.Counter() if stats is None else stats

    def locate(self, p):
        """(inside, cell indices, fractions)."""
        F = self.F
        g = (p - self.origin) / self.spacing
        inside, idx, fr = True, [], []
        for a in range(3):
            n = self.dims[a]
            if not (g[a] >= 0 and g[a] <= F(n - 1)):
                return False, None, None
            i = min(int(np.floor(g[a])), n - 2)
            if g[a] == F(n - 1):
                self.stats["upper_face"] += 1
            idx.append(i)
            fr.append(g[a] - F(i))
        return inside, idx, fr

    def sample(self, arr, idx, fr):
        """Trilinear: the four x-lerps, the two y-lerps, the z-lerp (per component)."""
        i, j, k = idx
        c = lambda dx, dy, dz: arr[k + dz, j + dy, i + dx]
        x00 = lerp(c(0, 0, 0), c(1, 0, 0), fr[0])
        x10 = lerp(c(0, 1, 0), c(1, 1, 0), fr[0])
        x01 = lerp(c(0, 0, 1), c(1, 0, 1), fr[0])
        x11 = lerp(c(0, 1, 1), c(1, 1, 1), fr[0])
        y0, y1 = lerp(x00, x10, fr[1]), lerp(x01, x11, fr[1])
        return lerp(y0, y1, fr[2])

    def v_at(self, p):
        ok, idx, fr = self.locate(p)
        return self.sample(self.v, idx, fr) if ok else None

    def usable(self, k1):
        d = dot(k1, k1)
        return bool(self.msq <= d and d < np.inf), d

    def try_step(self, p, k1, h, steps):
        """(p', None) where the step is taken, else (None, reason)."""
        F = self.F
        ok, d = self.usable(k1)
        if not ok:
            self.stats["speed_overflow" if not d < np.inf else "speed_low"] += 1
            return None, SPEED
        hh, h6 = F(0.5) * h, h / F(6.0)
        k2 = self.v_at(p + hh * k1)
        if k2 is None:
            self.stats["grid_q2"] += 1
            return None, GRID
        k3 = self.v_at(p + hh * k2)
        if k3 is None:
            self.stats["grid_q3"] += 1
            return None, GRID
        k4 = self.v_at(p + h * k3)
        if k4 is None:
            self.stats["grid_q4"] += 1
            return None, GRID
        pn = p + h6 * (((k1 + F(2) * k2) + F(2) * k3) + k4)
        if not self.locate(pn)[0]:
            self.stats["grid_pn"] += 1
            return None, GRID
        if pn.tobytes() == p.tobytes():
            self.stats["no_motion"] += 1
            return None, SPEED
        if steps >= self.max_steps:
            return None, STEPS
        return pn, None

    def axis_normal(self, T):
        F = self.F
        a = 0
        for b in (1, 2):
            if abs(T[b]) < abs(T[a]):
                a = b
        if sum(abs(T[b]) == abs(T[a]) for b in range(3)) > 1:
            self.stats["axis_tie"] += 1   # the smallest |T_a| on two or three axes
        self.stats["axis_%d" % a] += 1
        e = np.zeros(3, F)
        e[a] = 1
        w = e - T[a] * T
        return w / np.sqrt(dot(w, w))

    def half(self, seed, h):
        """Points, tangents, normals, colours of a half-line from the seed
        (the seed first) and its end reason."""
        F = self.F
        p, T, N = seed, np.zeros(3, F), np.zeros(3, F)
        out, steps = [], 0
        while True:
            _, idx, fr = self.locate(p)
            k1 = self.sample(self.v, idx, fr)
            ok, d = self.usable(k1)
            if ok:
                T = k1 / np.sqrt(d)
            elif steps:
                self.stats["tangent_kept"] += 1
            if steps == 0:
                N = self.axis_normal(T)
            else:
                w = N - dot(N, T) * T
                if dot(w, w) >= F(0.25):
                    self.stats["carried"] += 1
                    N = w / np.sqrt(dot(w, w))
                else:
                    self.stats["repick"] += 1
                    N = self.axis_normal(T)
            g = None if self.cfield is None else self.sample(self.cfield, idx, fr)
            out.append((p, T, N, g))
            pn, why = self.try_step(p, k1, h, steps)
            if pn is None:
                return out, why
            p, steps = pn, steps + 1

    def lines(self, seeds, direction):
        """dict(points, tangents, normals, scalars [np(, 3)], off [ns + 1], info [ns, 2])."""
        F = self.F
        pts, off, info = [], [0], []
        with np.errstate(all="ignore"):
            for s in np.asarray(seeds, F32).astype(F):
                if not self.locate(s)[0]:
                    self.stats["seed_outside"] += 1
                    info.append((0, SEED | SEED << 8))
                    off.append(len(pts))
                    continue
                back, eb = ([], STEPS) if direction == FORWARD else self.half(s, -self.step)
                fwd, ef = ([], STEPS) if direction == BACKWARD else self.half(s, self.step)
                seedrec = (fwd or back)[0]
                line = back[:0:-1] + [seedrec] + fwd[1:]
                if direction == BOTH and len(back) == 1 and len(fwd) > 1:
                    self.stats["empty_back"] += 1
                if direction == BOTH and len(fwd) == 1 and len(back) > 1:
                    self.stats["empty_fwd"] += 1
                self.stats["line_%d" % min(len(line), 3)] += 1
                info.append((max(len(back) - 1, 0), eb | ef << 8))
                pts += line
                off.append(len(pts))
        col = lambda k, w: np.array([r[k] for r in pts], F).reshape(-1, w)
        return dict(points=col(0, 3), tangents=col(1, 3), normals=col(2, 3),
                    scalars=None if self.cfield is None else col(3, 1)[:, 0],
                    off=np.array(off, np.uint32), info=np.array(info, np.uint32).reshape(-1, 2))


def lines_numpy(f, F=F32, stats=None):
    return Rule(f, F, stats).lines(f["seeds"], f["direction"])


def tubes_numpy(f, L, radius, nsides, ring, color=0, F=F32):
    """(verts, normals, colors, faces) of the lines L = lines_numpy(f)."""
    radius = F(F32(radius))
    ring = np.asarray(ring, F32).astype(F)
    if f.get("cfield") is not None:
        pcol = ch.colormap_numpy(L["scalars"].astype(F32), *f["cmap"])
    else:
        pcol = np.full(len(L["points"]), color, np.uint32)
    V, Nr, C, Fc = [], [], [], []
    ns = nsides
    for l in range(len(L["off"]) - 1):
        p0, m = int(L["off"][l]), int(L["off"][l + 1]) - int(L["off"][l])
        if m < 2:
            continue
        v0 = len(V)
        for j in range(m):
            P, T, N = (L[k][p0 + j] for k in ("points", "tangents", "normals"))
            B = np.array([T[1] * N[2] - T[2] * N[1], T[2] * N[0] - T[0] * N[2],
                          T[0] * N[1] - T[1] * N[0]], F)
            for k in range(ns):
                o = ring[k, 0] * N + ring[k, 1] * B
                V.append(P + radius * o)
                Nr.append(o)
                C.append(pcol[p0 + j])
        for j, sign in ((0, F(-1)), (m - 1, F(1))):
            V.append(L["points"][p0 + j])
            Nr.append(-L["tangents"][p0 + j] if sign < 0 else L["tangents"][p0 + j])
            C.append(pcol[p0 + j])
        for j in range(m - 1):
            for k in range(ns):
                a, b = j * ns + k, j * ns + (k + 1) % ns
                c, d = a + ns, b + ns
                Fc += [(v0 + a, v0 + c, v0 + b), (v0 + b, v0 + c, v0 + d)]
        for k in range(ns):
            Fc.append((v0 + m * ns, v0 + k, v0 + (k + 1) % ns))
        for k in range(ns):
            r = (m - 1) * ns
            Fc.append((v0 + m * ns + 1, v0 + r + (k + 1) % ns, v0 + r + k))
    return (np.array(V, F).reshape(-1, 3), np.array(Nr, F).reshape(-1, 3),
            np.array(C, np.uint32), np.array(Fc, np.uint32).reshape(-1, 3))


# ---- fields and seeds ----

def lattice(nx, ny, nz):
    """x, y, z index arrays of shape [nz, ny, nx]."""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)


def uniform(nx, ny, nz, v):
    out = np.zeros((nz, ny, nx, 3), F32)
    out[...] = np.asarray(v, F32)
    return out


def rotation(n, omega=1.0, lift=0.0):
    """Rigid rotation about the z axis through the centre of an n^3 grid."""
    x, y, z = lattice(n, n, n)
    c = (n - 1) / 2.0
    return np.stack([-omega * (y - c), omega * (x - c), np.full_like(x, lift)], -1).astype(F32)


def abc(n, A=1.0, B=0.8, C=0.6):
    """The ABC flow sampled on the lattice of [0, 2 pi]^3."""
    x, y, z = (2.0 * np.pi * a / (n - 1) for a in lattice(n, n, n))
    return np.stack([A * np.sin(z) + C * np.cos(y), B * np.sin(x) + A * np.cos(z),
                     C * np.sin(y) + B * np.cos(x)], -1).astype(F32)


def sink(nx=3, ny=2, nz=2):
    """v = (c - x, 0, 0), c between two cells: lines converge on the plane x = c."""
    x, y, z = lattice(nx, ny, nz)
    out = np.zeros((nz, ny, nx, 3), F32)
    out[..., 0] = (nx - 1) / 2.0 - x
    return out


def corner_turn():
    """A 4 x 4 x 2 field that flows along +x up to x = 1 and along +y from
    x = 2: one step of 1.5 from x = 1 turns the tangent by more than 60
    degrees, so the carried normal is dropped and the axis rule picks again."""
    out = np.zeros((2, 4, 4, 3), F32)
    out[:, :, :2, 0] = 1.0
    out[:, :, 2:, 1] = 1.0
    return out


def scalar_field(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, shape).astype(F32)


def random_seeds(n, dims, seed, margin=0.0):
    rng = np.random.default_rng(seed)
    hi = np.asarray(dims, np.float64) - 1.0
    return (margin + rng.uniform(0.0, 1.0, (n, 3)) * (hi - 2 * margin)).astype(F32)


def small_cases():
    """The small fields of the host test, as {name: field}."""
    u = uniform(5, 2, 2, (1, 0, 0))
    cases = {}
    cases["dyadic"] = field(u, [[0.25, 0.5, 0.5]], 0.5, 100)
    cases["cell2"] = field(rotation(2, 1.0, 0.25), [[0.5, 0.25, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]],
                           0.125, 9, BOTH)
    for name, dims in (("322", (3, 2, 2)), ("232", (2, 3, 2)), ("223", (2, 2, 3))):
        v = abc(3)[:dims[2], :dims[1], :dims[0]].copy()
        hi = np.asarray(dims, F32) - 1
        seeds = [[0, 0, 0], hi, [hi[0], 0.5, 0.5], [0.5, hi[1], 0.5], [0.5, 0.5, hi[2]],
                 [-0.0, 0.25, 0.75], [1.0, 1.0, 1.0], [np.nextafter(hi[0], F32(9)), 0.5, 0.5],
                 [0.5, np.nextafter(F32(0), F32(-1)), 0.5], [0.5, 0.5, -1e-3]]
        cases["abc" + name] = field(v, seeds, 0.25, 6, BOTH)
    seeds3 = [[0.25, 0.5, 0.5], [3.75, 0.5, 0.5], [2.0, 1.0, 0.0]]
    cases["steps0"] = field(u, seeds3, 0.5, 0, BOTH)
    cases["steps1"] = field(u, seeds3, 0.5, 1, BOTH)
    cases["steps1_fwd"] = field(u, seeds3, 0.5, 1, FORWARD)
    cases["back"] = field(u, seeds3, 0.5, 40, BACKWARD)
    cases["ends"] = field(u, [[0.0, 0.5, 0.5], [4.0, 0.5, 0.5], [3.9, 0.5, 0.5]], 0.5, 40, BOTH)
    cases["zero"] = field(uniform(3, 3, 3, (0, 0, 0)), [[1, 1, 1], [0.5, 1.5, 0.25]], 0.5, 5, BOTH)
    cases["slow"] = field(uniform(3, 3, 3, (1e-4, 0, 0)), [[1, 1, 1]], 0.5, 5, BOTH, min_speed=1e-3)
    cases["huge"] = field(uniform(3, 3, 3, (2e19, 2e19, 0)), [[1, 1, 1]], 0.5, 5, BOTH)
    cases["underflow"] = field(uniform(3, 3, 3, (1e-9, 0, 0)), [[1.5, 1, 1]], 1e-3, 5, BOTH,
                               min_speed=1e-12)
    cases["sink"] = field(sink(), [[0.25, 0.5, 0.5], [1.9, 0.25, 0.75], [1.0, 0.5, 0.5]], 0.5, 60,
                          BOTH)
    cases["turn"] = field(corner_turn(), [[1.0, 0.25, 0.5], [0.5, 0.125, 0.25]], 1.5, 3, BOTH)
    cases["spaced"] = field(abc(5), random_seeds(7, (5, 5, 5), 11), 0.0625, 20, BOTH,
                            origin=(-1.5, 2.0, 0.25), spacing=(0.5, 0.25, 2.0))
    cases["spaced"]["seeds"] = (cases["spaced"]["seeds"] * np.array([0.5, 0.25, 2.0], F32)
                                + np.array([-1.5, 2.0, 0.25], F32)).astype(F32)
    return cases


def with_color(f, seed, ntable=37):
    """f with a colour field and a map that clamps at both ends."""
    g = dict(f)
    g["cfield"] = scalar_field(f["vectors"].shape[:3], seed)
    g["cmap"] = (ch.table(ntable, seed), -0.5, 0.625)
    return g

"""A numpy restatement of the block rule of the multi-block streamline filter
and the cases shared by its tests (test_block_streamlines_host.py,
test_gpu_block_streamlines.py).

Written from the rule in include/spray_rt.h: everything of the single-grid rule
(stream_helpers.Rule: locate, sample, usable, the axis rule) per block, and on
top of it only "which grid": a half-line carries a current block, a point is
sampled there if it is inside it, else in the lowest-indexed block it is
inside, which becomes the current one.  `stats` counts the paths a case
reaches; "on_shared_face" counts the located points that lie on a face of
their block and in another block as well (for plane-sharing splits: on a shared
plane).
"""
import collections
import functools

import numpy as np

import color_helpers as ch
import stream_helpers as sh

F32 = np.float32
FORWARD, BACKWARD, BOTH = sh.FORWARD, sh.BACKWARD, sh.BOTH
GRID, STEPS, SPEED, SEED = sh.GRID, sh.STEPS, sh.SPEED, sh.SEED


def block(vectors, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), cfield=None):
    return dict(vectors=np.ascontiguousarray(vectors, F32), origin=tuple(origin),
                spacing=tuple(spacing), cfield=cfield)


def block_set(blocks, seeds, step, max_steps, direction=FORWARD, min_speed=1e-6, cmap=None):
    return dict(blocks=list(blocks), seeds=np.ascontiguousarray(seeds, F32).reshape(-1, 3),
                step=step, max_steps=max_steps, direction=direction, min_speed=min_speed,
                cmap=cmap)


def host_args(s):
    """The positional arguments of the host forms."""
    return (s["blocks"], s["seeds"], s["step"], s["max_steps"])


def host_kw(s):
    return dict(direction=s["direction"], min_speed=s["min_speed"])


def as_field(s, b=0):
    """Block b of a set as a field of stream_helpers (the single-grid forms)."""
    B = s["blocks"][b]
    return sh.field(B["vectors"], s["seeds"], s["step"], s["max_steps"], s["direction"],
                    s["min_speed"], B["origin"], B["spacing"], B.get("cfield"), s.get("cmap"))


def split(vectors, spacing, parts=(2, 2, 2), cfield=None):
    """The index sub-boxes of a grid at origin 0, parts per axis (x, y, z),
    sharing planes; block index = px + parts_x * (py + parts_y * pz)."""
    nz, ny, nx = vectors.shape[:3]
    cuts = [np.linspace(0, n - 1, p + 1).astype(int) for n, p in zip((nx, ny, nz), parts)]
    out = []
    for pz in range(parts[2]):
        for py in range(parts[1]):
            for px in range(parts[0]):
                lo = [cuts[0][px], cuts[1][py], cuts[2][pz]]
                hi = [cuts[0][px + 1], cuts[1][py + 1], cuts[2][pz + 1]]
                sl = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
                out.append(block(vectors[sl].copy(),
                                 [float(F32(spacing[a]) * F32(lo[a])) for a in range(3)], spacing,
                                 None if cfield is None else np.ascontiguousarray(cfield[sl])))
    return out


# ---- the rule ----

class BlockRule:
    """The block rule over one set in dtype F."""

    def __init__(self, s, F=F32, stats=None):
        self.F = F
        self.stats = collections.Counter() if stats is None else stats
        self.rules = [sh.Rule(dict(vectors=b["vectors"], origin=b["origin"],
                                   spacing=b["spacing"], step=s["step"],
                                   max_steps=s["max_steps"], min_speed=s["min_speed"],
                                   cfield=b.get("cfield")), F, collections.Counter())
                      for b in s["blocks"]]
        r0 = self.rules[0]
        r0.stats = self.stats          # usable / axis_normal count into the set's stats
        self.step, self.max_steps, self.r0 = r0.step, r0.max_steps, r0
        self.colored = s["blocks"][0].get("cfield") is not None

    def locate(self, q, cur):
        """(block, cell indices, fractions) or None; cur None: a seed."""
        found = None
        if cur is not None:
            ok, idx, fr = self.rules[cur].locate(q)
            if ok:
                found = cur, idx, fr
                if any(r.locate(q)[0] for r in self.rules[:cur]):
                    self.stats["sticky_over_lower"] += 1   # it stays where it is
        if found is None:
            if cur is not None:
                self.stats["miss"] += 1
            for k, r in enumerate(self.rules):
                ok, idx, fr = r.locate(q)
                if ok:
                    found = k, idx, fr
                    break
        if found is None:
            return None
        k, idx, fr = found
        dims = self.rules[k].dims
        if any((idx[a] == 0 and fr[a] == 0) or (idx[a] == dims[a] - 2 and fr[a] == 1)
               for a in range(3)):     # on a face of its block: in another one as well?
            if sum(r.locate(q)[0] for r in self.rules) > 1:
                self.stats["on_shared_face"] += 1
        if cur is not None and k != cur:
            self.stats["switch"] += 1
        return found

    def v_at(self, q, cur):
        """(value, block) or (None, cur)."""
        got = self.locate(q, cur)
        if got is None:
            return None, cur
        k, idx, fr = got
        return self.rules[k].sample(self.rules[k].v, idx, fr), k

    def try_step(self, p, k1, h, steps, cur):
        """(p', block of p', None) where the step is taken, else (None, None, reason)."""
        F = self.F
        ok, d = self.r0.usable(k1)
        if not ok:
            return None, None, SPEED
        hh, h6 = F(0.5) * h, h / F(6.0)
        seen = [cur]
        k2, cur = self.v_at(p + hh * k1, cur)
        if k2 is None:
            self.stats["grid_q2"] += 1
            return None, None, GRID
        seen.append(cur)
        k3, cur = self.v_at(p + hh * k2, cur)
        if k3 is None:
            self.stats["grid_q3"] += 1
            return None, None, GRID
        seen.append(cur)
        k4, cur = self.v_at(p + h * k3, cur)
        if k4 is None:
            self.stats["grid_q4"] += 1
            return None, None, GRID
        seen.append(cur)
        pn = p + h6 * (((k1 + F(2) * k2) + F(2) * k3) + k4)
        got = self.locate(pn, cur)
        if got is None:
            self.stats["grid_pn"] += 1
            return None, None, GRID
        seen.append(got[0])
        if len({seen[1], seen[3], seen[4]}) == 3:
            self.stats["three_blocks_in_step"] += 1
        if pn.tobytes() == p.tobytes():
            return None, None, SPEED
        if steps >= self.max_steps:
            return None, None, STEPS
        return pn, got, None

    def half(self, seed, start, h):
        """Points, tangents, normals, scalars, blocks of a half-line from the
        seed located as `start` (the seed first) and its end reason."""
        F = self.F
        p, T, N = seed, np.zeros(3, F), np.zeros(3, F)
        out, steps = [], 0
        cur, idx, fr = start
        while True:
            R = self.rules[cur]
            k1 = R.sample(R.v, idx, fr)
            ok, d = self.r0.usable(k1)
            if ok:
                T = k1 / np.sqrt(d)
            if steps == 0:
                N = self.r0.axis_normal(T)
            else:
                w = N - sh.dot(N, T) * T
                N = w / np.sqrt(sh.dot(w, w)) if sh.dot(w, w) >= F(0.25) else self.r0.axis_normal(T)
            g = R.sample(R.cfield, idx, fr) if self.colored else None
            out.append((p, T, N, g, cur))
            pn, got, why = self.try_step(p, k1, h, steps, cur)
            if pn is None:
                return out, why
            p, steps = pn, steps + 1
            cur, idx, fr = got

    def lines(self, seeds, direction):
        """stream_helpers.Rule.lines' dict and blocks uint32 [np]."""
        F = self.F
        pts, off, info = [], [0], []
        with np.errstate(all="ignore"):
            for s in np.asarray(seeds, F32).astype(F):
                start = self.locate(s, None)
                if start is None:
                    self.stats["seed_outside"] += 1
                    info.append((0, SEED | SEED << 8))
                    off.append(len(pts))
                    continue
                back, eb = ([], STEPS) if direction == FORWARD else self.half(s, start, -self.step)
                fwd, ef = ([], STEPS) if direction == BACKWARD else self.half(s, start, self.step)
                line = back[:0:-1] + [(fwd or back)[0]] + fwd[1:]
                self.stats["end_%d" % eb] += direction != FORWARD
                self.stats["end_%d" % ef] += direction != BACKWARD
                info.append((max(len(back) - 1, 0), eb | ef << 8))
                pts += line
                off.append(len(pts))
        col = lambda k, w: np.array([r[k] for r in pts], F).reshape(-1, w)
        return dict(points=col(0, 3), tangents=col(1, 3), normals=col(2, 3),
                    scalars=col(3, 1)[:, 0] if self.colored else None,
                    blocks=np.array([r[4] for r in pts], np.uint32),
                    off=np.array(off, np.uint32), info=np.array(info, np.uint32).reshape(-1, 2))


def lines_numpy(s, stats=None):
    return BlockRule(s, F32, stats).lines(s["seeds"], s["direction"])


def tubes_numpy(s, L, radius, nsides, ring, color=0):
    colored = s["blocks"][0].get("cfield") is not None
    return sh.tubes_numpy(dict(cfield=True if colored else None, cmap=s.get("cmap")), L, radius,
                          nsides, ring, color)


# ---- the cases ----

SPACING = (0.25, 0.25, 0.25)


def lattice9(name):
    return {"rotation": sh.rotation(9, 0.25), "abc": sh.abc(9)}[name]


def world_seeds(n, seed, margin=0.03):
    """Seeds inside the 9^3 lattice at spacing 0.25, on no lattice plane."""
    return (sh.random_seeds(n, (9, 9, 9), seed, margin=margin * 4) * F32(0.25)).astype(F32)


def unsplit(s, name):
    """The field the 9^3 splits below are sub-boxes of, with s's seeds and trace."""
    return sh.field(lattice9(name), s["seeds"], s["step"], s["max_steps"], s["direction"],
                    s["min_speed"], (0.0, 0.0, 0.0), SPACING)


def hop_blocks(n=6):
    """n 2 x 2 x 2-point blocks in a row along x, the speed growing with x."""
    out = []
    for k in range(n):
        v = np.zeros((2, 2, 2, 3), F32)
        v[..., 0, 0] = 1.0 + 0.75 * k
        v[..., 1, 0] = 1.0 + 0.75 * (k + 1)
        out.append(block(v, (float(k), 0.0, 0.0)))
    return out


def refined_blocks():
    """A 3^3 block at spacing 1 next to a 5^3 block at spacing 0.5."""
    def sampled(n, origin, h):
        x, y, z = (origin[a] + h * c for a, c in enumerate(sh.lattice(n, n, n)))
        return np.stack([1.0 + 0.125 * y, 0.25 * np.cos(2.0 * x), 0.125 * np.sin(x + z)],
                        -1).astype(F32)
    return [block(sampled(3, (0, 0, 0), 1.0)),
            block(sampled(5, (2, 0, 0), 0.5), (2.0, 0.0, 0.0), (0.5, 0.5, 0.5))]


def overlap_blocks():
    """x in [0, 5] and x in [3, 8]: two cell layers in common, with other data."""
    return [block(sh.uniform(6, 3, 3, (1, 0, 0))),
            block(sh.uniform(6, 3, 3, (1, 0.25, 0)), (3.0, 0.0, 0.0))]


def gap_blocks():
    u = sh.uniform(3, 3, 3, (1, 0, 0))
    return [block(u), block(u, (3.0, 0.0, 0.0))]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: set}."""
    c = {}
    rot, abc = split(lattice9("rotation"), SPACING), split(lattice9("abc"), SPACING)
    c["rotation_both"] = block_set(rot, world_seeds(130, 1), 0.25, 14, BOTH)
    c["rotation_fwd"] = block_set(rot, world_seeds(9, 2), 0.25, 60, FORWARD)
    c["rotation_back"] = block_set(rot, world_seeds(9, 3), 0.25, 60, BACKWARD)
    c["abc_both"] = block_set(abc, world_seeds(12, 4), 0.03125, 40, BOTH)
    c["abc_fwd"] = block_set(abc, world_seeds(7, 5), 0.03125, 40, FORWARD)
    c["abc_back"] = block_set(abc, world_seeds(7, 6), 0.03125, 40, BACKWARD)
    on = [[1.0, 0.3, 0.3], [1.0, 1.0, 1.0], [0.3, 1.0, 1.7], [2.0, 2.0, 2.0], [0.0, 0.0, 0.0]]
    c["on_planes"] = block_set(abc, on, 0.03125, 10, BOTH)
    c["reversed"] = block_set(abc[::-1], np.concatenate([world_seeds(12, 4), np.asarray(on, F32)]),
                              0.03125, 40, BOTH)
    c["overlap"] = block_set(overlap_blocks(), [[0.5, 0.5, 1.0], [4.0, 0.5, 1.0], [7.0, 0.75, 1.0],
                                                [3.5, 0.25, 0.5]], 0.5, 40, BOTH)
    c["refined"] = block_set(refined_blocks(), [[0.25, 1.0, 1.0], [1.9, 0.4, 1.3], [3.8, 1.5, 0.3],
                                                [2.0, 1.0, 1.0], [2.25, 1.75, 1.25]], 0.125, 60,
                             BOTH)
    # seeds on the faces of the refined blocks, and one float beyond and before each
    up, down = lambda x: np.nextafter(F32(x), F32(99)), lambda x: np.nextafter(F32(x), F32(-99))
    ulps = [[f(x), 0.75, 1.25] for x in (0.0, 2.0, 4.0) for f in (F32, up, down)]
    ulps += [[2.75, f(y), 0.5] for y in (0.0, 2.0) for f in (F32, up, down)]
    ulps += [[1.5, 0.5, f(z)] for z in (-0.0, 2.0) for f in (F32, up, down)]
    c["face_ulps"] = block_set(refined_blocks(), ulps, 0.125, 3, BOTH)
    c["gap"] = block_set(gap_blocks(), [[0.5, 1.0, 1.0], [2.5, 1.0, 1.0], [4.5, 0.5, 1.5],
                                        [3.25, 1.0, 1.0]], 0.5, 40, BOTH)
    c["hop3"] = block_set(hop_blocks(), [[0.4, 0.5, 0.5], [0.375, 0.25, 0.75]], 1.5, 5, BOTH)
    uniform9 = split(sh.uniform(9, 9, 9, (1, 0, 0)), SPACING)
    c["aligned"] = block_set(uniform9, [[0.25, 0.5, 0.5], [0.5, 1.0, 1.0], [1.0, 0.25, 1.5],
                                        [1.75, 1.0, 0.75]], 0.25, 12, BOTH)
    c["steps0"] = block_set(abc, world_seeds(5, 7), 0.03125, 0, BOTH)
    c["steps1"] = block_set(abc, world_seeds(5, 8), 0.5, 1, BOTH)
    c["steps1_fwd"] = block_set(uniform9, [[0.875, 0.5, 0.5], [1.0, 1.0, 1.0]], 0.25, 1, FORWARD)
    c["one_block"] = block_set([block(sh.abc(5), (-1.5, 2.0, 0.25), (0.5, 0.25, 2.0))],
                               (sh.random_seeds(9, (5, 5, 5), 11) * np.array([0.5, 0.25, 2.0], F32)
                                + np.array([-1.5, 2.0, 0.25], F32)).astype(F32), 0.0625, 20, BOTH)
    c["no_seeds"] = block_set(rot, np.zeros((0, 3), F32), 0.25, 10, BOTH)
    return c


def colored(s, seed, ntable=37):
    """s with a colour field on every block and a map that clamps at both ends."""
    g = dict(s)
    g["blocks"] = [dict(b, cfield=sh.scalar_field(b["vectors"].shape[:3], seed + k))
                   for k, b in enumerate(s["blocks"])]
    g["cmap"] = (ch.table(ntable, seed), -0.5, 0.625)
    return g


COLORED = ("abc_both", "refined", "overlap", "one_block")


def case(name):
    """A case, with colour fields where COLORED lists it."""
    s = cases()[name]
    return colored(s, 30 + sorted(cases()).index(name)) if name in COLORED else s


def tube_of(k):
    return dict(radius=0.015625 * (1 + k % 3), nsides=3 + (5 * k) % 14,
                color=None if k % 3 == 1 else 0x00102030 + k)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(lines dict, stats) of the numpy restatement of case(name)."""
    stats = collections.Counter()
    return lines_numpy(case(name), stats), stats

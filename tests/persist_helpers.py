"""Batch sizes and batches for the tests of the persistent body of the scene
kernel (test_persist_shapes.py, test_gpu_persist.py).  Pure numpy.

The launcher runs the plain grid (one packet per wave) while a batch has no
more packets than the resident grid has waves, i.e. up to grid * 256 rays,
and the persistent grid above it: 64 work queues over bands of band_size(M)
rays, dealt in chunks of 64 rays while M < grid * 4 * chunk * 4 (`small`)
and of `chunk` rays from there on.  `grid` (resident blocks of the launched
instantiation) and `chunk` are read from RtContext.scene_launch_info() at run
time; sizes() turns them into the two batch sizes the tests use, and
tiling() makes a batch of any such size out of a class of a few thousand
rays whose oracle results are known, so that the expected result of every
positional output is ref[sel]."""
import numpy as np

QUEUES = 64       # work queues (bands) of a persistent launch
WAVES = 4         # waves per block
RESIDUE = 37      # live lanes of the last packet of every size of sizes()


def band_size(M):
    """Rays per band: ceil(ceil(M / 64) / 64) * 64 (a whole number of
    packets; restated from the kernel's band_size)."""
    per_queue = -(-M // QUEUES)
    return -(-per_queue // 64) * 64


def persists(M, grid):
    """A closest-hit batch without a device count runs the persistent grid."""
    return -(-M // 64) > grid * WAVES


def small(M, grid, chunk):
    """The persistent grid deals packets (64 rays), not chunks."""
    return M < grid * WAVES * chunk * 4


def _next_residue(M):
    """The smallest value >= M that is RESIDUE modulo 64."""
    return M + (RESIDUE - M) % 64


def sizes(grid, chunk):
    """(M_small, M_big) for a resident grid of `grid` blocks and chunks of
    `chunk` rays.
    M_small: the smallest M > grid * 256 with M % 64 == 37 -- persistent,
             `small`, chunks of 64 rays.
    M_big:   the smallest M >= grid * 4 * chunk * 4 with M % 64 == 37 and
             band_size(M) % chunk == 64 -- persistent, chunks of `chunk`
             rays; every band ends 64 rays into a chunk and the last band
             ends inside a packet."""
    m_small = _next_residue(grid * 256 + 1)
    m = _next_residue(grid * WAVES * chunk * 4)
    while band_size(m) % chunk != 64:
        m += 64
    return m_small, m


def tiling(n, M, seed):
    """Index array `sel` of length M into a class of n rays.  The first part
    is as many whole consecutive copies of 0 .. n-1 as fit into M // 2 rays
    (the class's neighbouring-lane structure: coherent waves); the rest is a
    seeded draw with repetition (incoherent waves: masked, non-finite and
    ordinary records side by side in one packet)."""
    copies = (M // 2) // n
    head = np.tile(np.arange(n, dtype=np.int64), copies)
    rng = np.random.default_rng(seed)
    tail = rng.integers(0, n, M - len(head), dtype=np.int64)
    return np.concatenate([head, tail])


def halves(n, M):
    """(slice of the whole copies, slice of the seeded draw) of tiling(n, M, .)."""
    k = ((M // 2) // n) * n
    return slice(0, k), slice(k, M)


def copies_and_prefix(n, M):
    """M = k * n + p, p < n: a batch of k whole copies of a class and a
    prefix of p of its rays (the counted form: counters add up)."""
    return M // n, M % n


def take(c, sel):
    """Class `c` (dict of org, dir, tnear, tfar) at the indices `sel`."""
    return {k: np.ascontiguousarray(c[k][sel]) for k in ("org", "dir", "tnear", "tfar")}

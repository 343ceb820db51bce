"""CPU tests of persist_helpers.py: the batch sizes that put a launch into the
persistent body of the scene kernel, with packets and with chunks, and the
tiled batches whose expected results are ref[sel] -- checked against the
oracle itself before any GPU sees them (test_gpu_persist.py)."""
import numpy as np
import pytest

import persist_helpers as PH
import ray_cases as RC

GRIDS = range(256, 2049, 128)  # resident blocks: 1 .. 8 per CU of a 256-CU part
CHUNKS = (128, 256)            # the any-hit and the closest-hit chunk


@pytest.fixture(scope="module", params=(0.0, RC.LARGE), ids=["origin", "large"])
def var(request, oracle):
    return RC.variant(oracle, request.param)


def test_band_size():
    """ceil(ceil(M / 64) / 64) * 64 at the edges: 64 bands of whole packets
    that cover M."""
    assert [PH.band_size(m) for m in (1, 64, 65, 4096, 4097, 8192, 8193)] == \
        [64, 64, 64, 64, 128, 128, 192]
    for m in (37, 4133, 262181, 8388608, 8388609):
        s = PH.band_size(m)
        assert s % 64 == 0 and 64 * s >= m and 64 * (s - 64) < m


@pytest.mark.parametrize("chunk", CHUNKS)
def test_sizes(chunk):
    for grid in GRIDS:
        m_small, m_big = PH.sizes(grid, chunk)
        waves = grid * PH.WAVES
        for m in (m_small, m_big):
            assert m % 64 == PH.RESIDUE, (grid, m)
            assert -(-m // 64) > waves and PH.persists(m, grid), (grid, m)  # persistent
        # the smallest such sizes
        assert not PH.persists(m_small - 64, grid), grid
        assert m_small < grid * PH.WAVES * chunk * 4 and PH.small(m_small, grid, chunk), grid
        assert m_big >= grid * PH.WAVES * chunk * 4 and not PH.small(m_big, grid, chunk), grid
        assert m_big - grid * PH.WAVES * chunk * 4 < 64 * 64 * (chunk // 64) + 64, grid
        s = PH.band_size(m_big)
        assert s % chunk == 64, (grid, s)  # every band ends 64 rays into a chunk
        # all 64 bands hold rays; the last one ends inside a packet and is no
        # longer than the others
        last = m_big - 63 * s
        assert 0 < last <= s and last % 64 == PH.RESIDUE, (grid, last)
        assert m_big * 80 < 1_000_000_000, (grid, m_big)  # rays + hit records


def test_tiling_layout():
    n, m = 1024, 3000
    sel = PH.tiling(n, m, 5)
    a, b = PH.halves(n, m)
    assert sel.dtype == np.int64 and len(sel) == m and sel.min() >= 0 and sel.max() < n
    assert a == slice(0, 1024) and np.array_equal(sel[a], np.arange(n))
    assert len(np.unique(sel[b])) > n // 2 and not np.array_equal(sel[b][:n], np.arange(n))
    assert np.array_equal(sel, PH.tiling(n, m, 5)) and not np.array_equal(sel, PH.tiling(n, m, 6))
    # fewer than two copies' worth: the seeded draw only
    assert PH.halves(7168, 4133) == (slice(0, 0), slice(0, 4133))
    k, p = PH.copies_and_prefix(1024, 262181)
    assert k * 1024 + p == 262181 and 0 < p < 1024


def test_tiled_oracle_is_tiled_reference(var):
    """The oracle on a 3,000-ray tiling of `mixed` gives ref[sel], byte for
    byte: a ray's result does not depend on its place in the batch."""
    ref, occ, _, _ = RC.oracle_results(var, "mixed")
    sel = PH.tiling(len(ref), 3000, 17)
    c = PH.take(var["classes"]["mixed"], sel)
    h, _ = var["osc"].intersect(c["org"], c["dir"], tnear=c["tnear"], tfar=c["tfar"])
    o, _ = var["osc"].occluded(c["org"], c["dir"], tnear=c["tnear"], tfar=c["tfar"])
    assert h.tobytes() == ref[sel].tobytes()
    assert np.array_equal(o, occ[sel])
    dom = ref["domain"][sel]
    assert len(np.unique(dom[dom >= 0])) >= 8 and (dom < 0).any() and 0 < occ[sel].mean() < 1


def test_tiled_nonfinite_keeps_every_plant(var):
    planted = var["classes"]["nonfinite"]["planted"]
    sel = PH.tiling(len(planted), 3000, 17)
    for part in PH.halves(len(planted), 3000):
        kinds = set(planted[sel[part]].tolist())
        assert kinds >= set(range(len(RC.PLANTS))) and -1 in kinds, kinds

"""bench.py --dump-outputs (no GPU): the arrays written for a step's buffers
are a fixed seeded sample in float32 / float64, within the 64 MB limit at the
bench frame's size, with the fields the interface leaves undefined zeroed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from spray_amd._native import HIT_DTYPE  # noqa: E402

NAMES = {"sample_index", "hit_domain", "hit_prim", "hit_color", "hit_t", "hit_uv", "hit_ng",
         "hit_ns", "shadow_valid", "shadow_occluded", "shadow_rays"}


def _buffers(n, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, HIT_DTYPE)
    for k in ("t", "u", "v", "ng", "ns"):
        rec[k] = rng.uniform(-1, 1, size=rec[k].shape)
    rec["prim"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    rec["color"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    rec["domain"] = rng.integers(-1, 64, n)
    rec["t"][rec["domain"] < 0] = np.inf  # a miss: nothing but domain is defined
    valid = (rng.integers(0, 2, n) * (rec["domain"] >= 0)).astype(np.uint8)
    occ = rng.integers(0, 256, n).astype(np.uint8)  # junk where no shadow ray was spawned
    return (rec, valid, occ, torch.from_numpy(rec.view(np.uint8).copy()),
            torch.from_numpy(valid.copy()), torch.from_numpy(occ.copy()))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_is_a_fixed_sample_of_the_step_outputs(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_RAYS", 257)
    rec, valid, occ, th, tv, to = _buffers(1000, 1)
    bench.dump_outputs(str(tmp_path / "a"), th, tv, to, int(valid.sum()))
    bench.dump_outputs(str(tmp_path / "b"), th, tv, to, int(valid.sum()))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == NAMES
    for k in NAMES:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
        assert np.isfinite(a[k]).all(), k
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == 257 and np.all(np.diff(idx) > 0) and idx[-1] < 1000
    r, hit = rec[idx], rec["domain"][idx] >= 0
    assert np.array_equal(a["hit_domain"], r["domain"])
    assert np.array_equal(a["hit_prim"], np.where(hit, r["prim"], 0))  # exact in float64
    assert np.array_equal(a["hit_color"], np.where(hit, r["color"], 0))
    assert np.array_equal(a["hit_t"], np.where(hit, r["t"], 0))
    assert np.array_equal(a["hit_uv"][:, 1], np.where(hit, r["v"], 0))
    assert np.array_equal(a["hit_ng"], np.where(hit[:, None], r["ng"], 0))
    assert np.array_equal(a["hit_ns"], np.where(hit[:, None], r["ns"], 0))
    assert np.array_equal(a["shadow_valid"], valid[idx] != 0)
    assert np.array_equal(a["shadow_occluded"], (occ[idx] != 0) & (valid[idx] != 0))
    assert a["shadow_rays"].tolist() == [float(valid.sum())]


def test_dump_takes_every_ray_of_a_small_output(tmp_path):
    rec, valid, occ, th, tv, to = _buffers(100, 2)
    bench.dump_outputs(str(tmp_path), th, tv, to, 0)
    a = _load(tmp_path)
    assert np.array_equal(a["sample_index"], np.arange(100))
    assert np.array_equal(a["hit_domain"], rec["domain"])


def test_dump_stays_within_64_mb_at_the_bench_frame(tmp_path):
    # bytes per sampled ray over all arrays, measured on a small dump
    _, valid, _, th, tv, to = _buffers(64, 3)
    bench.dump_outputs(str(tmp_path), th, tv, to, 0)
    per_ray = sum(a.nbytes for k, a in _load(tmp_path).items() if k != "shadow_rays") / 64
    assert bench.DUMP_RAYS <= bench.W * bench.H * bench.SPP
    assert bench.DUMP_RAYS * per_ray + 8 <= 64e6

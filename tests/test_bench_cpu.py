"""bench.py's command line and output dump, on the host (no GPU): what a
plain run leaves to --full, and the arrays --dump-outputs writes."""
import os
import sys

import numpy as np
import pytest
import torch


def _bench():
    import bench

    return bench


def _launch(B, seed):
    g = torch.Generator().manual_seed(seed)
    T, N = 10, 4
    return {
        "rewards": torch.randint(-30, 1, (T, B, N), dtype=torch.int32, generator=g),
        "done": torch.randint(0, 2, (T, B), dtype=torch.uint8, generator=g),
        "actions": torch.randint(1, 105, (T, B, N), dtype=torch.uint8, generator=g),
        "obs": torch.randint(-128, 128, (T, B, N, 48), dtype=torch.int8, generator=g),
    }


def test_dump_outputs_writes_float32_arrays_whole_when_small(tmp_path):
    bench = _bench()
    last = _launch(37, 0)
    bench.dump_outputs(str(tmp_path / "d"), last)
    assert sorted(os.listdir(tmp_path / "d")) == ["actions.npy", "done.npy", "obs.npy", "rewards.npy"]
    for name, t in last.items():
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.numpy().astype(np.float32))


def test_dump_outputs_samples_the_same_games_of_a_large_array(tmp_path, monkeypatch):
    """above the per-array cap an array keeps a sorted, seeded sample of its
    games (axis 1): the same games in every run, every kept game whole"""
    bench = _bench()
    B = 64
    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 10 * 4 * 48 * 4 * 20)  # 20 games of obs; the other arrays fit
    last = _launch(B, 1)
    bench.dump_outputs(str(tmp_path / "a"), last)
    bench.dump_outputs(str(tmp_path / "b"), last)
    obs = np.load(tmp_path / "a" / "obs.npy")
    assert obs.shape == (10, 20, 4, 48) and obs.nbytes <= bench.DUMP_ARRAY_BYTES
    assert np.array_equal(obs, np.load(tmp_path / "b" / "obs.npy"))
    keep = np.sort(np.random.default_rng(0).choice(B, size=20, replace=False))
    assert np.array_equal(obs, last["obs"].numpy()[:, keep].astype(np.float32))
    assert np.load(tmp_path / "a" / "rewards.npy").shape == (10, B, 4)


def test_dump_of_the_headline_shape_stays_under_64_mb():
    bench = _bench()
    T, B, N = bench.STEPS_PER_LAUNCH, 65536, bench.N_PLAYERS
    total = 0
    for per_game in (T * N, T, T * N, T * N * 48):  # rewards, done, actions, obs
        games = B if per_game * 4 * B <= bench.DUMP_ARRAY_BYTES else bench.DUMP_ARRAY_BYTES // (per_game * 4)
        total += games * per_game * 4 + 128  # + the .npy header
    assert total <= 64_000_000


def test_plain_run_options_and_full(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x", "--only", "puct"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "x" and a.only == "puct"


def test_extra_legs_are_refused_without_full(monkeypatch):
    """--only with a leg beside the headline is an error in a plain run (no
    silent headline-only run, no extra leg behind the driver's back)"""
    bench = _bench()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--only", "puct"])
    monkeypatch.setattr(bench, "dist_setup", lambda args: (1, 0, 0))  # no GPU touched
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "--full" in str(e.value)

"""GPU checks of the device prioritised replay (csrc/sechs_replay.hip).

* the drop-in PriorityReplayBuffer replays the reference's recorded traces
  (golden F15) from the recorded uniforms: indices, len and beta exactly,
  weights, priorities and tree snapshots to 1e-12;
* DevicePER against the numpy model of the contract (test_replay_cpu.PerModel)
  at capacities 4099 (no power of two: leaves at two depths, more than one LDS
  subtree) and 4096, with a batched store that wraps, 256 samples, a round in
  which most indices repeat (the last position must win), indices outside the
  leaf range, and a capacity-2 buffer.  The device pow may differ from numpy's
  in the last place, so after every update the leaves are held to 1e-12, then
  the model adopts the device's leaves and the device's internal nodes must
  equal the model's pairwise sums bit for bit -- the samples that follow are
  compared exactly;
* payload rows (16 and 112 bytes) through a wrap: a sampled row is the newest
  one stored in its slot;
* the flow of the reference's own tests/test_pbr.py.
"""
import random

import numpy as np
import pytest
import torch

from test_replay_cpu import PerModel, per_traces

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ti", range(4))
def test_priority_replay_buffer_replays_reference_traces(ti, monkeypatch):
    from rl_6_nimmt.utils.replay_buffer import PriorityReplayBuffer

    tr = per_traces()[ti]
    cap, n = tr["capacity"], tr["n"]
    buf = PriorityReplayBuffer(max_length=cap)
    stores = 0
    for _ in range(tr["nstore"]):
        buf.store(k=stores)
        stores += 1
    for r, rd in enumerate(tr["rounds"]):
        buf.store(k=stores)
        stores += 1
        feed = iter(rd["u"])
        monkeypatch.setattr(random, "random", lambda: next(feed))
        idx, w, batch = buf.sample(n)
        assert next(feed, None) is None  # exactly n uniforms drawn
        assert idx.dtype == np.uint32 and idx.tolist() == rd["idx"], (ti, r)
        assert w.dtype == np.float64 and np.allclose(w, rd["weights"], rtol=1e-12, atol=0), (ti, r)
        slots = idx.astype(np.int64) - (cap - 1)  # each holds the newest store whose count = slot (mod capacity)
        last = stores - 1
        assert [int(k) for k in batch["k"]] == (last - (last - slots) % cap).tolist(), (ti, r)
        prio = buf.per.tree().cpu().numpy()[idx.astype(np.int64)]
        assert np.allclose(prio, rd["priorities"], rtol=1e-12, atol=0), (ti, r)
        assert buf.beta == rd["beta"] and len(buf) == rd["len"], (ti, r)
        errors = np.array(rd["errors"])
        buf.batch_update(idx, errors)
        assert np.array_equal(errors, rd["errors"])  # the caller's array is left alone
        if str(r) in tr["tree"]:
            assert np.allclose(buf.per.tree().cpu().numpy(), tr["tree"][str(r)], rtol=1e-12, atol=0), (ti, r)


def _adopt(per, model):
    """leaves to 1e-12; then the device's internal nodes == pairwise sums of its own leaves, exactly"""
    got = per.tree().cpu().numpy()
    lo = model.cap - 1
    assert np.allclose(got[lo:], model.tree[lo:], rtol=1e-12, atol=0)
    model.tree[lo:] = got[lo:]
    model.rebuild()
    assert np.array_equal(got, model.tree)
    assert (len(per), per.pointer) == (model.num_items, model.pointer)


def _same_sample(per, model, n, rng):
    u = rng.random_sample(n)
    idx, prio, w, _ = per.sample(n, u)
    midx, mprio, mw = model.sample(n, u)
    assert np.array_equal(idx.cpu().numpy(), midx)
    assert np.array_equal(prio.cpu().numpy(), mprio)
    assert np.allclose(w.cpu().numpy(), mw, rtol=1e-12, atol=0)
    assert per.beta == model.beta
    return midx


@pytest.mark.parametrize("cap", [4099, 4096])
def test_device_per_equals_the_model(cap):
    from rl_6_nimmt.replay import DevicePER

    rng = np.random.RandomState(cap)
    per, model = DevicePER(cap), PerModel(cap)
    for m in (3000, 3000):  # the second call wraps mid-batch
        per.store(count=m)
        model.store(m)
        _adopt(per, model)
    assert len(per) == 5999 and per.pointer == 6000 - cap
    for _ in range(2):
        idx = _same_sample(per, model, 256, rng)
        err = rng.random_sample(256) * 1.5
        per.update(idx, err)
        model.update(idx, err)
        _adopt(per, model)
    per.store(count=700)  # enters at the maximum leaf, not at 1.0
    model.store(700)
    _adopt(per, model)
    # one leaf holds nearly all the priority: most samples repeat it, and of the repeats the last error stays
    heavy = cap - 1 + 1234
    for p in (per, model):
        p.update([heavy], [1e7], epsilon=0.0, upper=float("inf"), alpha=1.0)
    _adopt(per, model)
    idx = _same_sample(per, model, 256, rng)
    assert (idx == heavy).sum() > 200
    err = np.linspace(0.05, 0.9, 256)  # distinct: first-wins or any-wins gives another leaf
    per.update(torch.as_tensor(idx, device=per.device), torch.as_tensor(err, device=per.device))
    model.update(idx, err)
    _adopt(per, model)
    assert model.tree[heavy] == pytest.approx((err[np.nonzero(idx == heavy)[0][-1]] + 0.01) ** 0.6, rel=1e-12)
    # indices outside the leaf range are skipped
    before = per.tree().cpu().numpy()
    outside = torch.tensor([0, cap - 2, 2 * cap - 1, 2**31 - 1, -1], device=per.device)
    per.update(outside, torch.full((5,), 0.5, dtype=torch.float64, device=per.device))
    assert np.array_equal(per.tree().cpu().numpy(), before)
    _same_sample(per, model, 256, rng)
    with pytest.raises(ValueError):
        per.store(count=cap + 1)


def test_device_per_capacity_two():
    from rl_6_nimmt.replay import DevicePER

    rng = np.random.RandomState(2)
    with pytest.raises(ValueError):
        DevicePER(2).sample(2, [0.1, 0.2])  # empty: the reference's np.min raises
    per, model = DevicePER(2), PerModel(2)
    for _ in range(3):
        per.store()
        model.store()
        _adopt(per, model)
        idx = _same_sample(per, model, 4, rng)
        err = rng.random_sample(4)
        per.update(idx, err)
        model.update(idx, err)
        _adopt(per, model)
    assert len(per) == 2 and per.pointer == 1  # three stores, one wrap


@pytest.mark.parametrize("row_bytes", [16, 112])
def test_sampled_payload_rows_are_the_newest_of_their_slot(row_bytes):
    from rl_6_nimmt.replay import DevicePER

    cap, words = 4099, row_bytes // 4
    per = DevicePER(cap, row_bytes=row_bytes)
    newest = np.full(cap, -1, dtype=np.int64)
    count = 0
    for m in (3000, 3000):
        ids = torch.arange(count, count + m, dtype=torch.int32, device="cuda")
        per.store(ids[:, None].repeat(1, words))  # every 4-byte word of a row = its global store count
        newest[(per.pointer - m + np.arange(m)) % cap] = np.arange(count, count + m)
        count += m
    idx, _, _, rows = per.sample(256)
    assert rows.shape == (256, row_bytes) and rows.dtype == torch.uint8
    got = rows.view(torch.int32).cpu().numpy()
    slots = idx.cpu().numpy().astype(np.int64) - (cap - 1)
    assert (newest[slots] >= 0).all() and (newest[slots] >= cap).any() and (newest[slots] < 3000).any()
    assert np.array_equal(got, np.repeat(newest[slots][:, None], words, axis=1))
    with pytest.raises(ValueError):
        per.store(torch.zeros((3, row_bytes + 16), dtype=torch.uint8, device="cuda"))


def test_reference_pbr_flow_runs_through():
    """tests/test_pbr.py of the reference: a one-element error tensor per round"""
    from rl_6_nimmt.utils.replay_buffer import PriorityReplayBuffer

    np.random.seed(0)
    random.seed(0)
    pbr = PriorityReplayBuffer(max_length=100, dtype=torch.double)
    experience = {"a": torch.tensor([20]), "b": torch.tensor([30])}
    for _ in range(10):
        pbr.store(**experience)
    for _ in range(200):
        pbr.store(**experience)
        b_idx, weights, minibatch = pbr.sample(10)
        assert weights.mean() != 0 and np.isfinite(weights).all()
        assert len(minibatch["a"]) == 10
        pbr.batch_update(b_idx, torch.from_numpy(np.random.random_sample((1,))))
    assert len(pbr) == 208 and pbr.beta == pytest.approx(0.6)

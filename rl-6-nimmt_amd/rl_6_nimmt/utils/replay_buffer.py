"""Replay buffers of the DQN family (reference: rl_6_nimmt/utils/replay_buffer.py).

`PriorityReplayBuffer` (replay_buffer.py:122-203) with the reference's
interface; the sum tree lives on the GPU (`DevicePER`, csrc/sechs_replay.hip),
the experience dicts stay in a host array like the reference's
`SumTree.data`:
  * `store(**experience)` enters at the maximum leaf priority (1.0 in an
    empty tree);
  * `sample(n)` draws its n uniforms from Python's global `random.random()`
    in order (and nothing else from that stream), advances `beta`, and
    returns (tree indices uint32 ndarray, importance weights f64 ndarray,
    minibatch dict of lists);
  * `batch_update(tree_idx, abs_errors)` sets leaf = min(|err| + epsilon,
    upper) ** alpha in the dtype of `abs_errors`, as numpy does there (the
    agents pass float32 tensors); a shorter `abs_errors` updates only that many
    entries (the reference's zip); the caller's tensor is left as it was (the
    reference adds epsilon in place); host indices outside the leaf range
    raise ValueError (the reference corrupts an inner node or raises
    IndexError);
  * `len` is stores minus pointer wraps, past the capacity (replay_buffer.py:
    98-104) -- the agents' `len(history) > minibatch` test sees that number.

`History` here is the DQN replay ring (replay_buffer.py:206-271), indexed as
the reference's so that `sample(n)` (`random.sample(range(len))`) addresses
the same transitions: `len` is the pointer while filling, `max_length` at the
store that wraps, and the pointer again from the next store on (the older
transitions in slots >= pointer are then out of `sample`'s reach).  The
list-like `History` of utils/history.py is what the other agents use.
"""
import random

import numpy as np
import torch

from ..replay import DevicePER


class PriorityReplayBuffer:
    def __init__(self, max_length=None, dtype=torch.float, device=torch.device("cpu"), per_device=None):
        self.dtype = dtype
        self.device = device  # the agent's (host) device; the tree is on the GPU `per_device`
        if max_length is None:
            raise ValueError("PriorityReplayBuffer needs max length!")
        self.max_length = int(max_length)
        self.per = DevicePER(self.max_length, row_bytes=0, device=per_device)
        self.data = np.zeros(self.max_length, dtype=object)  # SumTree.data: 0 = never written

    # the reference's hyper-parameters (replay_buffer.py:143-148) live on the DevicePER
    absolute_error_upper = property(lambda s: s.per.absolute_error_upper,
                                    lambda s, v: setattr(s.per, "absolute_error_upper", v))
    epsilon = property(lambda s: s.per.epsilon, lambda s, v: setattr(s.per, "epsilon", v))
    alpha = property(lambda s: s.per.alpha, lambda s, v: setattr(s.per, "alpha", v))
    beta = property(lambda s: s.per.beta, lambda s, v: setattr(s.per, "beta", v))
    beta_increment = property(lambda s: s.per.beta_increment, lambda s, v: setattr(s.per, "beta_increment", v))

    @property
    def total_priority(self):
        return float(self.per.tree()[0])

    def store(self, **experience):
        self.data[self.per.pointer] = experience
        self.per.store(count=1)

    def sample(self, n):
        u = [random.random() for _ in range(n)]
        idx, _, weights, _ = self.per.sample(n, u)
        leaf_idx = idx.cpu().numpy().astype(np.uint32)
        data_batch = self.data[leaf_idx.astype(np.int64) - (self.max_length - 1)]
        assert all(isinstance(d, dict) for d in data_batch), "Wrong data in sample detected"
        minibatch = {k: [dic[k] for dic in data_batch] for k in data_batch[0]}
        return leaf_idx, weights.cpu().numpy(), minibatch

    def batch_update(self, tree_idx, abs_errors):
        """must be called to update priorities"""
        if isinstance(abs_errors, torch.Tensor):
            errs = abs_errors.detach().reshape(-1)
            wide = errs.dtype == torch.float64
        else:
            errs = np.asarray(abs_errors).reshape(-1)
            wide = errs.dtype == np.float64
        k = min(len(tree_idx), len(errs))
        tree_idx, errs = tree_idx[:k], errs[:k]
        if not isinstance(tree_idx, torch.Tensor):
            tree_idx = np.asarray(tree_idx, dtype=np.int64)
            bad = (tree_idx < self.max_length - 1) | (tree_idx > 2 * self.max_length - 2)
            if bad.any():
                raise ValueError(f"tree index {int(tree_idx[bad][0])} is no leaf of a capacity-{self.max_length} tree "
                                 f"({self.max_length - 1}..{2 * self.max_length - 2})")
        if wide:
            self.per.update(tree_idx, errs)
            return
        # numpy keeps the errors' dtype through `+= epsilon`, the clip and the power
        # (replay_buffer.py:192-197): the same arithmetic here, the leaves then go in as they are
        if isinstance(errs, torch.Tensor):
            errs = (errs.cpu() + self.epsilon).numpy()
        else:
            errs = errs + self.epsilon
        ps = np.minimum(errs, self.absolute_error_upper) ** self.alpha
        self.per.update(tree_idx, ps.astype(np.float64), epsilon=0.0, upper=float("inf"), alpha=1.0)

    def __len__(self):
        return len(self.per)


class History:
    """Generic replay ring. Can accommodate arbitrary fields."""

    def __init__(self, max_length=None, dtype=torch.float, device=torch.device("cpu")):
        self.max_length = max_length
        self.device = device
        self.dtype = dtype
        self.is_full = False
        self.clear()

    def clear(self):
        self.memories = [None] * (self.max_length or 0)
        self.data_pointer = 0  # is_full stays as it is (replay_buffer.py:255-260)

    def store(self, **kwargs):
        if self.max_length is None:
            self.memories.append(kwargs)
            self.data_pointer += 1
            return
        self.memories[self.data_pointer] = kwargs
        self.data_pointer += 1
        self.is_full = False
        if self.data_pointer >= self.max_length:
            self.data_pointer = 0
            self.is_full = True

    @staticmethod
    def _collate(items):
        return {k: [it[k] for it in items] for k in items[0]}

    def sample(self, n):
        idx = random.sample(range(len(self)), k=n)
        return idx, None, self._collate([self.memories[i] for i in idx])

    def rollout(self, n=None):
        """When n is not None, returns only the last n entries"""
        m = len(self)
        return self._collate(self.memories[:m] if n is None else self.memories[m - n: m])

    def __len__(self):
        if self.max_length is None:
            return self.data_pointer
        return self.max_length if self.is_full else self.data_pointer

"""Device prioritised replay: the reference's SumTree + PriorityReplayBuffer
(utils/replay_buffer.py:15-203) as HIP kernels (csrc/sechs_replay.hip, the
sn_per_* entry points of include/sechs.h).

`DevicePER(capacity, row_bytes)` holds the f64 sum tree in the reference's
heap layout and, with `row_bytes` > 0, a ring of fixed-size payload rows
(observations, action, reward, done packed by the caller) that `sample`
gathers on the device and `gather` returns for given slots: the batched
league DQN learner (dqn.BatchedDQN) stores its 112-byte transition rows
there, the prioritised variants sampling, the uniform ones gathering.  The
drop-in `PriorityReplayBuffer` (utils/replay_buffer.py) uses it with
`row_bytes=0` and keeps its experience dicts on the host.

Kept from the reference: the hyper-parameters and their defaults, `beta`
advancing on every `sample`, `len` = stores minus pointer wraps (it passes the
capacity), and the importance weights' minimum taken over the first
min(len, capacity) leaves.  Every call only enqueues work on the current
stream of the device; nothing synchronises.

There is no CPU fallback: the handle is created on first use and that needs
the GPU.  Constructing a `DevicePER` touches nothing.

Clones: `inherit(parent)` takes the parent's leaves, rows and
hyper-parameters on the device (sn_per_inherit) -- verbatim at equal
capacity, else the newest rows re-homed, oldest first; `inherit_host` is the
torch model of that rule and the kernel is held to it.  `copy.deepcopy` is
`clone()`, an equal-capacity `inherit`.  Pickling (`torch.save` of an agent)
exports the leaves and the ring to CPU tensors, which synchronises; loading
keeps them on the host until the handle is next created (sn_per_import), so
unpickling touches no GPU either.
"""
import ctypes

import numpy as np
import torch

from . import _native as nat


_HYPER = ("absolute_error_upper", "epsilon", "alpha", "beta", "beta_increment")


def inherit_host(leaves, rows, pointer, num_items, capacity):
    """sn_per_inherit in torch: what a replay of `capacity` slots takes from a
    parent with `leaves` f64 [cap], `rows` [cap, row_bytes] (or None) and the
    counters `pointer`, `num_items` -> (leaves', rows', pointer', num_items').
    Equal capacities: everything as it is.  Else the newest h = min(held,
    capacity) slots, oldest first, into slots 0 .. h-1 with the parent's
    priorities, zeros behind them, and the counters of h stores into an empty
    ring; held = cap once the parent has wrapped (num_items != pointer), its
    pointer before."""
    leaves = torch.as_tensor(leaves, dtype=torch.float64).reshape(-1)
    cap_src, cap, pointer, num_items = int(leaves.numel()), int(capacity), int(pointer), int(num_items)
    if rows is not None:
        rows = torch.as_tensor(rows).reshape(cap_src, -1)
    if cap == cap_src:
        return leaves.clone(), None if rows is None else rows.clone(), pointer, num_items
    held = cap_src if num_items != pointer else pointer
    h = min(held, cap)
    src = (pointer - h + torch.arange(h, device=leaves.device)) % cap_src
    new_leaves = torch.zeros(cap, dtype=torch.float64, device=leaves.device)
    new_leaves[:h] = leaves[src]
    new_rows = None
    if rows is not None:
        new_rows = torch.zeros((cap, rows.shape[1]), dtype=rows.dtype, device=rows.device)
        new_rows[:h] = rows[src.to(rows.device)]
    return new_leaves, new_rows, h % cap, h - (1 if h == cap else 0)


class DevicePER:
    def __init__(self, capacity, row_bytes=0, device=None):
        capacity, row_bytes = int(capacity), int(row_bytes)
        if capacity < 2:
            raise ValueError("capacity must be >= 2 (the reference cannot sample from a one-slot buffer)")
        if row_bytes < 0 or row_bytes % 16:
            raise ValueError("row_bytes must be 0 or a multiple of 16")
        self.capacity, self.row_bytes = capacity, row_bytes
        self._device_arg = device
        self.device = None
        self._h = None
        self._saved = None  # (leaves, ring or None, pointer, num_items) on the host, loaded when the handle is created
        # replay_buffer.py:143-148
        self.absolute_error_upper = 1.0
        self.epsilon = 0.01
        self.alpha = 0.6
        self.beta = 0.4
        self.beta_increment = 0.001

    # ------------------------------------------------------------ lifecycle
    def _handle(self):
        if self._h is None:
            nat.require_gpu()
            d = torch.device("cuda" if self._device_arg is None else self._device_arg)
            if d.type != "cuda":
                raise nat.NativeError(f"DevicePER lives on the GPU, not on {d} (no CPU fallback)")
            idx = d.index if d.index is not None else torch.cuda.current_device()
            self.device = torch.device("cuda", idx)
            h = ctypes.c_void_p()
            with torch.cuda.device(self.device):
                nat.check(nat.lib().sn_per_create(ctypes.byref(h), self.capacity, self.row_bytes, idx), "sn_per_create")
            self._h = h
            if self._saved is not None:  # an unpickled state (or a clone of one)
                leaves, ring, pointer, num_items = self._saved
                leaves = leaves.to(self.device, torch.float64).contiguous()
                ring = None if ring is None else ring.to(self.device).contiguous()
                nat.check(nat.lib().sn_per_import(h, nat.ptr(leaves), nat.ptr(ring), pointer, num_items,
                                                  self._stream()), "sn_per_import")
                self._saved = None
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            nat.lib().sn_per_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ clones
    def inherit(self, parent):
        """take over `parent`'s replay and hyper-parameters; whatever this
        one held is gone.  Equal capacities: verbatim, slot for slot, with
        the parent's counters.  Else the parent's newest rows, oldest first,
        up to this capacity, at the parent's priorities (inherit_host; DESIGN
        §4c).  Enqueued on the current stream, where the parent's own calls
        went.  A parent nothing was ever stored into leaves this one empty
        and touches no GPU."""
        if parent is self:
            raise ValueError("a replay cannot inherit from itself")
        if parent.row_bytes != self.row_bytes:
            raise ValueError(f"the parent's rows hold {parent.row_bytes} bytes, not {self.row_bytes}")
        for k in _HYPER:
            setattr(self, k, getattr(parent, k))
        if parent._h is None:  # nothing on the device: empty, or a loaded state still on the host
            self.close()
            self._saved = None
            if parent._saved is not None:
                self._saved = inherit_host(*parent._saved, self.capacity)
            return
        self._saved = None  # loaded state this one never used: overwritten like the rest
        h = self._handle()
        nat.check(nat.lib().sn_per_inherit(h, parent._h, self._stream()), "sn_per_inherit")

    def clone(self):
        """a new DevicePER of the same capacity, row_bytes and device holding
        the same replay: same uniforms, same samples; from there on the two
        are independent.  Of one without a handle: another without a handle."""
        new = DevicePER(self.capacity, self.row_bytes, device=self._device_arg if self.device is None else self.device)
        new.inherit(self)
        return new

    def __deepcopy__(self, memo):
        memo[id(self)] = new = self.clone()
        return new

    def __getstate__(self):
        """constructor arguments, hyper-parameters, counters and -- when a
        handle exists -- the leaves (f64) and the ring (uint8) as CPU tensors:
        this waits for the device"""
        state = {"capacity": self.capacity, "row_bytes": self.row_bytes, "device": self._device_arg,
                 **{k: getattr(self, k) for k in _HYPER}}
        if self._h is not None:
            _, pointer, num_items = self._counters()
            leaves = self.tree()[self.capacity - 1:].cpu()
            ring = None
            if self.row_bytes:
                ring = self.gather(torch.arange(self.capacity, dtype=torch.int32, device=self.device)).cpu()
            state["saved"] = (leaves, ring, pointer, num_items)
        elif self._saved is not None:
            state["saved"] = self._saved
        return state

    def __setstate__(self, state):
        """touches no GPU: the arrays stay on the host until the handle is
        next created; `len` and `pointer` answer from the kept counters"""
        self.capacity, self.row_bytes, self._device_arg = state["capacity"], state["row_bytes"], state["device"]
        self.device, self._h = None, None
        self._saved = state.get("saved")
        for k in _HYPER:
            setattr(self, k, state[k])

    def _stream(self):
        return nat.stream_handle(self.device)

    def _counters(self):
        if self._h is None:
            return (self.capacity, 0, 0) if self._saved is None else (self.capacity,) + tuple(self._saved[2:])
        c, p, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        nat.check(nat.lib().sn_per_info(self._h, ctypes.byref(c), ctypes.byref(p), ctypes.byref(n)), "sn_per_info")
        return c.value, p.value, n.value

    @property
    def pointer(self):
        return self._counters()[1]

    def __len__(self):
        return self._counters()[2]

    # ------------------------------------------------------------ replay
    def store(self, rows=None, count=None):
        """`count` reference stores in one call (1 <= count <= capacity), each
        at the maximum leaf priority (1.0 in an empty tree).  rows: a device
        tensor of count x row_bytes bytes (any dtype / shape), count defaults
        to its first dimension."""
        h = self._handle()
        if rows is not None:
            if self.row_bytes == 0:
                raise ValueError("this replay holds no payload rows (row_bytes=0)")
            rows = rows.to(self.device).contiguous()
            m = int(rows.shape[0]) if count is None else int(count)
            if rows.numel() * rows.element_size() != m * self.row_bytes:
                raise ValueError(f"rows hold {rows.numel() * rows.element_size()} bytes, not {m} x {self.row_bytes}")
        else:
            m = 1 if count is None else int(count)
        nat.check(nat.lib().sn_per_store(h, m, nat.ptr(rows), self._stream()), "sn_per_store")

    def sample(self, n, u=None):
        """-> (tree_idx int32 [n], priority f64 [n], is_weight f64 [n], rows
        uint8 [n][row_bytes] or None), device tensors.  u: n f64 uniforms in
        [0, 1) (drawn on the device when None)."""
        h = self._handle()
        n = int(n)
        if n < 1:
            raise ValueError("n must be >= 1")
        if u is None:
            u = torch.rand(n, dtype=torch.float64, device=self.device)
        else:
            u = torch.as_tensor(u, dtype=torch.float64).to(self.device).contiguous()
            if u.numel() != n:
                raise ValueError(f"u holds {u.numel()} uniforms, not {n}")
        self.beta = min(1.0, self.beta + self.beta_increment)  # replay_buffer.py:162
        idx = torch.empty(n, dtype=torch.int32, device=self.device)
        prio = torch.empty(n, dtype=torch.float64, device=self.device)
        weight = torch.empty(n, dtype=torch.float64, device=self.device)
        rows = torch.empty((n, self.row_bytes), dtype=torch.uint8, device=self.device) if self.row_bytes else None
        nat.check(nat.lib().sn_per_sample(h, n, nat.ptr(u), float(self.beta), nat.ptr(idx), nat.ptr(prio),
                                          nat.ptr(weight), nat.ptr(rows), self._stream()), "sn_per_sample")
        return idx, prio, weight, rows

    def gather(self, slots):
        """-> the payload rows uint8 [n][row_bytes] of the data slots `slots`
        (int32 [n] on the device; slot = tree index - capacity + 1); a slot
        outside [0, capacity) gives a zero row.  The uniform replay of
        DQNVanilla / DDQNAgent: the caller draws the slots."""
        h = self._handle()
        if self.row_bytes == 0:
            raise ValueError("this replay holds no payload rows (row_bytes=0)")
        slots = torch.as_tensor(slots).to(self.device).reshape(-1)
        if slots.dtype != torch.int32:
            slots = slots.to(torch.int64).clamp(-1, 2**31 - 1).to(torch.int32)
        slots = slots.contiguous()
        n = int(slots.numel())
        if n < 1:
            raise ValueError("n must be >= 1")
        rows = torch.empty((n, self.row_bytes), dtype=torch.uint8, device=self.device)
        nat.check(nat.lib().sn_per_gather(h, n, nat.ptr(slots), nat.ptr(rows), self._stream()), "sn_per_gather")
        return rows

    def update(self, tree_idx, abs_err, epsilon=None, upper=None, alpha=None):
        """Leaf tree_idx[i] = min(abs_err[i] + epsilon, upper) ** alpha; of a
        repeated index the last entry counts; indices outside the leaf range
        are skipped.  The keywords default to the attributes."""
        h = self._handle()
        if isinstance(tree_idx, np.ndarray):
            tree_idx = tree_idx.astype(np.int64)
        idx = torch.as_tensor(tree_idx).to(self.device).reshape(-1)
        if idx.dtype != torch.int32:
            idx = idx.to(torch.int64).clamp(-1, 2**31 - 1).to(torch.int32)
        err = torch.as_tensor(abs_err).to(self.device, torch.float64).reshape(-1)
        if idx.numel() != err.numel():
            raise ValueError(f"{idx.numel()} indices but {err.numel()} errors")
        if idx.numel() == 0:
            return
        idx, err = idx.contiguous(), err.contiguous()
        nat.check(nat.lib().sn_per_update(h, idx.numel(), nat.ptr(idx), nat.ptr(err),
                                          float(self.epsilon if epsilon is None else epsilon),
                                          float(self.absolute_error_upper if upper is None else upper),
                                          float(self.alpha if alpha is None else alpha), self._stream()),
                  "sn_per_update")

    def tree(self):
        """the 2*capacity-1 nodes, f64 on the device"""
        h = self._handle()
        out = torch.empty(2 * self.capacity - 1, dtype=torch.float64, device=self.device)
        nat.check(nat.lib().sn_per_tree(h, nat.ptr(out), self._stream()), "sn_per_tree")
        return out

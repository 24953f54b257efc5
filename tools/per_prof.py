#!/usr/bin/env python3
"""Device prioritised replay (DevicePER, csrc/sechs_replay.hip) against the
obvious PyTorch-ROCm form of the same cycle on the same inputs.

One process; every call is timed with device events after a warm-up; the native
and the torch leg of an operation alternate; medians over `--reps`.
  big    capacity 2^20, 112-byte rows (two int8 observations, action, reward,
         done), store / sample / update of 65 536 -- the batched learner's shape;
  small  capacity 100 000, no rows, n = 64 -- the drop-in agents' shape: a
         launch-overhead figure, not a bandwidth one;
  inherit  a clone's replay (DevicePER.inherit) at the big shape,
         into the same and into half the capacity: see run_inherit.
The torch yardstick (TorchPER) keeps flat leaves and the ring: store = max +
scatter + index_copy_; sample = cumsum + searchsorted + index_select (+ the
weights); update = clamp + pow + scatter.  For time only: a cumsum orders the
additions differently from the tree, and its scatter of a repeated index is
not ordered.  Algorithmic bytes: algorithmic_bytes() below.

Usage:  python tools/per_prof.py [--reps 30] [--warmup 5] [--only big|small|inherit]
        [--native-only] [--out per_prof.json]
(--native-only: the native legs alone, for a kernel trace of its own:
 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/per_prof.py --native-only --reps 5)
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-6-nimmt_amd"))

SHAPES = {"big": (1 << 20, 112, 65536), "small": (100000, 0, 64)}
EPS, UPPER, ALPHA, BETA = 0.01, 1.0, 0.6, 0.4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


class TorchPER:
    """the yardstick: leaves + ring as plain tensors"""

    def __init__(self, cap, row_bytes, dev):
        self.cap, self.pointer = cap, 0
        self.leaves = torch.zeros(cap, dtype=torch.float64, device=dev)
        self.ring = torch.zeros((cap, row_bytes), dtype=torch.uint8, device=dev) if row_bytes else None
        self.ar = {}

    def _arange(self, n):
        if n not in self.ar:
            self.ar[n] = torch.arange(n, device=self.leaves.device)
        return self.ar[n]

    def store(self, m, rows):
        top = self.leaves.max()
        top = torch.where(top == 0, torch.ones_like(top), top)
        slots = (self._arange(m) + self.pointer) % self.cap
        self.leaves.scatter_(0, slots, top.expand(m))
        if rows is not None:
            self.ring.index_copy_(0, slots, rows)
        self.pointer = (self.pointer + m) % self.cap

    def sample(self, n, u):
        cs = torch.cumsum(self.leaves, 0)
        total = cs[-1]
        seg = total / n
        v = seg * self._arange(n) + u * seg
        slot = torch.searchsorted(cs, v).clamp_(max=self.cap - 1)
        prio = self.leaves.index_select(0, slot)
        w = torch.pow((prio / total) / (self.leaves.min() / total), -BETA)
        rows = self.ring.index_select(0, slot) if self.ring is not None else None
        return slot, prio, w, rows

    def update(self, slot, err):
        self.leaves.scatter_(0, slot, torch.clamp(err + EPS, max=UPPER) ** ALPHA)


def levels(cap):
    d = 0
    while (1 << d) < 2 * cap - 1:
        d += 1
    return d


def algorithmic_bytes(cap, rb, n):
    """what each call has to move: store = rows in + ring out, leaves, the max over the leaves, the rebuild (leaves
    read, inner nodes written); sample = the min over the leaves, the descent's loads, u / index / priority /
    weight, the gather; update = index + error, leaves, the rebuild"""
    return {"store": 2 * n * rb + 8 * n + 8 * cap + 16 * cap,
            "sample": 8 * cap + 8 * n * levels(cap) + 28 * n + 2 * n * rb,
            "update": 12 * n + 8 * n + 16 * cap}


def run_shape(name, reps, warmup, native_only):
    from rl_6_nimmt.replay import DevicePER

    cap, rb, n = SHAPES[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    per = DevicePER(cap, row_bytes=rb, device=dev)
    ref = None if native_only else TorchPER(cap, rb, dev)
    rows = torch.randint(0, 256, (n, rb), dtype=torch.uint8, device=dev, generator=g) if rb else None
    chunk = min(cap, 1 << 16)
    fill = torch.zeros((chunk, rb), dtype=torch.uint8, device=dev) if rb else None
    for at in range(0, cap, chunk):  # steady state: a full buffer with spread-out priorities
        m = min(chunk, cap - at)
        per.store(fill[:m] if rb else None, count=m)
        if ref:
            ref.store(m, fill[:m] if rb else None)
    spread = torch.rand(cap, dtype=torch.float64, device=dev, generator=g)
    per.update(torch.arange(cap - 1, 2 * cap - 1, device=dev), spread)
    if ref:
        ref.update(torch.arange(cap, device=dev), spread)
    u = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    err = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * 1.5
    idx = per.sample(n, u)[0]
    slot = idx.long() - (cap - 1)
    legs = {"store": (lambda: per.store(rows, count=n), lambda: ref.store(n, rows)),
            "sample": (lambda: per.sample(n, u), lambda: ref.sample(n, u)),
            "update": (lambda: per.update(idx, err), lambda: ref.update(slot, err))}
    out = {"capacity": cap, "row_bytes": rb, "n": n, "reps": reps, "bytes": algorithmic_bytes(cap, rb, n)}
    for op, (native, yard) in legs.items():
        t_n, t_y = [], []
        for r in range(warmup + reps):
            a = timed(native)
            b = None if native_only else timed(yard)
            if r >= warmup:
                t_n.append(a)
                t_y.append(b)
        res = {"native_us": statistics.median(t_n), "native_min_us": min(t_n), "native_max_us": max(t_n)}
        res["native_GBps"] = out["bytes"][op] / res["native_us"] / 1e3
        if not native_only:
            res.update(torch_us=statistics.median(t_y), torch_min_us=min(t_y), torch_max_us=max(t_y))
            res["torch_GBps"] = out["bytes"][op] / res["torch_us"] / 1e3
            res["torch_over_native"] = res["torch_us"] / res["native_us"]
        out[op] = res
    return out


def run_inherit(reps, warmup, native_only):
    """DevicePER.inherit (one k_per_inherit launch + the rebuild) at the big shape, into a child of the same
    capacity (verbatim) and of half of it (the newest half re-homed), against the same result put together
    from PyTorch ops: the parent's leaves (tree() slice) and rows (gather(arange)), an index_select into the
    child's order, sn_per_import.  Once per clone, not per step: a correctness path, timed for the record."""
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.replay import DevicePER

    cap, rb, n = SHAPES["big"]
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    parent = DevicePER(cap, row_bytes=rb, device=dev)
    for at in range(0, cap + n, n):  # wrapped, the pointer at n
        parent.store(torch.randint(0, 256, (n, rb), dtype=torch.uint8, device=dev, generator=g))
    parent.update(torch.arange(cap - 1, 2 * cap - 1, device=dev), torch.rand(cap, dtype=torch.float64, device=dev, generator=g))
    every = torch.arange(cap, dtype=torch.int32, device=dev)
    out = {"capacity": cap, "row_bytes": rb, "reps": reps}
    for name, c in (("equal", cap), ("halved", cap // 2)):
        h = min(cap, c)
        child, built = DevicePER(c, row_bytes=rb, device=dev), DevicePER(c, row_bytes=rb, device=dev)
        src = torch.arange(cap, device=dev) if c == cap else (parent.pointer - h + torch.arange(h, device=dev)) % cap
        counters = (parent.pointer, len(parent)) if c == cap else (h % c, h - (h == c))

        def native():
            child.inherit(parent)

        def yard():
            leaves = parent.tree()[cap - 1:].index_select(0, src)
            rows = parent.gather(every).index_select(0, src)
            nat.check(nat.lib().sn_per_import(built._handle(), nat.ptr(leaves), nat.ptr(rows), *counters,
                                              built._stream()), "sn_per_import")

        t_n, t_y = [], []
        for r in range(warmup + reps):
            a = timed(native)
            b = None if native_only else timed(yard)
            if r >= warmup:
                t_n.append(a)
                t_y.append(b)
        nbytes = h * (8 + rb) + c * (8 + rb) + 16 * c  # kept slots read, every child slot written, the rebuild
        res = {"child_capacity": c, "bytes": nbytes, "native_us": statistics.median(t_n), "native_min_us": min(t_n),
               "native_max_us": max(t_n)}
        res["native_GBps"] = nbytes / res["native_us"] / 1e3
        if not native_only:
            assert torch.equal(child.tree(), built.tree()) and torch.equal(child.gather(every[:c]), built.gather(every[:c]))
            assert (child.pointer, len(child)) == (built.pointer, len(built))
            res.update(torch_us=statistics.median(t_y), torch_min_us=min(t_y), torch_max_us=max(t_y))
            res["torch_over_native"] = res["torch_us"] / res["native_us"]
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("per_prof: no GPU -- times are taken on the device or not at all")
    result = {name: run_shape(name, args.reps, args.warmup, args.native_only)
              for name in SHAPES if not args.only or name == args.only}
    if not args.only or args.only == "inherit":
        result["inherit"] = run_inherit(args.reps, args.warmup, args.native_only)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

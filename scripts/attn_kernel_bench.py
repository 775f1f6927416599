"""Microbench of the attention kernels at the flagship shape (device events,
median): forward and backward (dQ + dKV, which one launcher call issues
back to back; rocprofv3 --kernel-trace splits the two) at B16 H32 S2048,
D in {64, 80, 96, 128}. D = 80 runs the packed entry points, the mode the
flagship uses; the others the [B, H, S, D] ones.

Prints microseconds and TF/s per call (causal FLOPs: 2 * B * H * S^2 * D
forward, 5 of those products backward). To compare two builds, run it in
several fresh processes per build, alternated, with --root pointing at each
tree, and keep a change only if its slowest run beats the other's fastest.

Usage: python scripts/attn_kernel_bench.py [--root TREE] [--dims 64 80 96 128]
                                           [--iters 50] [--warmup 5] [--json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

B, H, S = 16, 32, 2048
PACKED_DIMS = (80,)


def _time(fn, iters, warmup):
    """Median device-event time (us) of `iters` calls after `warmup`."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(iters):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in evs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))),
        help="tree to import metis_amd from")
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 80, 96, 128])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", action="store_true",
                    help="also print one JSON line {name: us}")
    args = ap.parse_args()
    assert args.iters >= 50, "time at least 50 calls"

    sys.path.insert(0, os.path.abspath(args.root))
    from metis_amd.ops import require_extension

    ext = require_extension()
    results = {}
    for d in args.dims:
        g = torch.Generator(device="cuda").manual_seed(d)
        scale = 1.0 / math.sqrt(d)
        bf16 = dict(device="cuda", dtype=torch.bfloat16, generator=g)
        if d in PACKED_DIMS:
            qkv = torch.randn(B, S, 3 * H * d, **bf16)
            d_o = torch.randn(B, S, H * d, **bf16)
            o, lse = ext.attn_fwd_packed(qkv, H, H, d, scale)
            delta = ext.attn_bwd_delta_packed(o, d_o, H)
            calls = {
                "fwd": lambda: ext.attn_fwd_packed(qkv, H, H, d, scale),
                "bwd": lambda: ext.attn_bwd_packed(qkv, d_o, lse, delta, H, H,
                                                   d, scale),
            }
        else:
            q, k, v, d_o = (torch.randn(B, H, S, d, **bf16) for _ in range(4))
            o, lse = ext.attn_fwd(q, k, v, scale)
            delta = ext.attn_bwd_delta(o, d_o)
            calls = {
                "fwd": lambda: ext.attn_fwd(q, k, v, scale),
                "bwd": lambda: ext.attn_bwd(q, k, v, d_o, lse, delta, scale),
            }
        for name, fn in calls.items():
            us = _time(fn, args.iters, args.warmup)
            flops = 2 * B * H * S * S * d * (1 if name == "fwd" else 5)
            mode = "packed" if d in PACKED_DIMS else "unpacked"
            results[f"{name} D={d}"] = us
            print(f"{name} D={d:<3d} {mode:8s} {us:9.1f} us "
                  f"{flops / us * 1e-6:7.1f} TF/s", flush=True)
        del calls
    if args.json:
        print("ATTN_KERNEL_BENCH " + json.dumps(results), flush=True)


if __name__ == "__main__":
    main()

"""Microbench of the fused bias / residual / LayerNorm / GeLU-backward calls
against the eager compositions they replace (device events, median).

At 32768 x 2560 (the flagship's tokens x hidden):
  bias_residual_layernorm_fwd   vs  residual + (y + bias), layernorm_fwd
  bias_residual_add             vs  residual + (y + bias)
  layernorm_bwd_add             vs  layernorm_bwd, dres + dx
  layernorm_bwd_add + colsum    vs  layernorm_bwd, dres + dx, g.sum(0)
and at 32768 x 10240:
  gelu_tanh_bwd_bgrad           vs  aten gelu_backward, dh.sum(0)

For each call it prints microseconds, the bytes the operation needs (from
the shapes), the floor at the 6.3 TB/s achievable HBM bandwidth and the
achieved share of it; for each pair the time saved. Run it in several
fresh processes and compare the saving with the eager side's spread.

Usage: python scripts/fused_bench.py [--iters 50] [--warmup 5] [--json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

HBM_ACHIEVABLE = 6.3e12     # bytes/s, MI355X achievable HBM bandwidth
ROWS, HIDDEN, FFN = 32768, 2560, 10240


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", action="store_true",
                    help="also print one JSON line {name: us}")
    args = ap.parse_args()
    assert args.iters >= 50, "time at least 50 calls"

    from metis_amd.ops import require_extension

    ext = require_extension()
    torch.manual_seed(0)
    results = {}

    def pair(name, fused, eager, need):
        """`need`: bytes of the fused call (each tensor once)."""
        for tag, fn in (("fused", fused), ("eager", eager)):
            us = _time(fn, args.iters, args.warmup)
            results[f"{name} {tag}"] = us
            bps = need / (us * 1e-6)
            print(f"{name + ' ' + tag:36s} {us:8.1f} us  need {need / 1e6:7.1f} MB"
                  f"  floor {need / HBM_ACHIEVABLE * 1e6:6.1f} us  "
                  f"{100 * bps / HBM_ACHIEVABLE:5.1f}% of achievable",
                  flush=True)
        saved = results[f"{name} eager"] - results[f"{name} fused"]
        print(f"{name + ' saved':36s} {saved:8.1f} us", flush=True)

    bf16 = dict(device="cuda", dtype=torch.bfloat16)
    y = torch.randn(ROWS, HIDDEN, **bf16)
    res = torch.randn(ROWS, HIDDEN, **bf16)
    dy = torch.randn(ROWS, HIDDEN, **bf16)
    bias = torch.randn(HIDDEN, **bf16)
    gamma = torch.randn(HIDDEN, device="cuda")
    beta = torch.randn(HIDDEN, device="cuda")
    t = ROWS * HIDDEN * 2                       # one bf16 [rows, H]
    stats = 2 * ROWS * 4
    x, _, mean, rstd = ext.bias_residual_layernorm_fwd(
        y, bias, res, gamma, beta, 1e-5)

    us = _time(lambda: ext.layernorm_fwd(x, gamma, beta, 1e-5),
               args.iters, args.warmup)
    results["layernorm_fwd"] = us
    print(f"{'layernorm_fwd':36s} {us:8.1f} us  need {(2 * t + stats) / 1e6:7.1f}"
          f" MB  floor {(2 * t + stats) / HBM_ACHIEVABLE * 1e6:6.1f} us",
          flush=True)

    pair("bias_residual_layernorm_fwd",
         lambda: ext.bias_residual_layernorm_fwd(y, bias, res, gamma, beta, 1e-5),
         lambda: ext.layernorm_fwd(res + (y + bias), gamma, beta, 1e-5),
         4 * t + stats)
    pair("bias_residual_add",
         lambda: ext.bias_residual_add(y, bias, res),
         lambda: res + (y + bias), 3 * t)
    pair("layernorm_bwd_add",
         lambda: ext.layernorm_bwd_add(dy, res, x, gamma, mean, rstd, False),
         lambda: res + ext.layernorm_bwd(dy, x, gamma, mean, rstd)[0],
         4 * t + stats)
    pair("layernorm_bwd_add colsum",
         lambda: ext.layernorm_bwd_add(dy, res, x, gamma, mean, rstd, True),
         lambda: (res + ext.layernorm_bwd(dy, x, gamma, mean, rstd)[0]).sum(0),
         4 * t + stats)
    del y, res, dy, x

    h = torch.randn(ROWS, FFN, **bf16)
    da = torch.randn(ROWS, FFN, **bf16)
    pair("gelu_tanh_bwd_bgrad",
         lambda: ext.gelu_tanh_bwd_bgrad(h, da),
         lambda: torch.ops.aten.gelu_backward(
             da, h, approximate="tanh").sum(0),
         3 * ROWS * FFN * 2)
    if args.json:
        print("FUSED_BENCH " + json.dumps(results), flush=True)


if __name__ == "__main__":
    main()

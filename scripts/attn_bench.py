"""Attention fwd/bwd microbench: our HIP flash kernels vs PyTorch SDPA.

Prints one line per (D, direction, impl) with ms and achieved TF/s
(causal FLOP count: 2*B*H*S^2*D per matmul pair, halved for causal,
x2 for QK^T+PV; bwd counts 2.5x fwd as is conventional).

With --packed each shape also gets, on a qkv [B, S, 3*H*D] holding the same
values: the packed entry points (impl "packed"), and the relayout copies
they replace as arms of their own (impl "copy": split + merge for fwd,
unmerge + split_bwd for bwd), so packed - hip can be read next to copy.

Usage: python scripts/attn_bench.py [--iters 20] [--json OUT] [--packed]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

import metis_amd._hip_ops as ext


def bench(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def run_packed(q, k, v, do, iters, results):
    B, H, S, D = q.shape
    sc = 1 / math.sqrt(D)
    fwd_fl = 4 * B * H * S * S * D / 2
    qkv = torch.cat([t.transpose(1, 2).reshape(B, S, H * D) for t in (q, k, v)],
                    dim=-1).contiguous()
    d_o = do.transpose(1, 2).reshape(B, S, H * D).contiguous()
    o, lse = ext.attn_fwd_packed(qkv, H, H, D, sc)
    delta = ext.attn_bwd_delta_packed(o, d_o, H)
    dq = torch.randn_like(q)

    def row(op, impl, t, fl):
        results.append(dict(op=op, impl=impl, B=B, H=H, S=S, D=D, ms=t * 1e3,
                            tflops=fl / t / 1e12))

    t = bench(lambda: ext.attn_fwd_packed(qkv, H, H, D, sc), iters)
    row("fwd", "packed", t, fwd_fl)
    t = bench(lambda: ext.attn_bwd_packed(qkv, d_o, lse, delta, H, H, D, sc),
              iters)
    row("bwd", "packed", t, fwd_fl * 2.5)
    t = (bench(lambda: ext.qkv_split_transpose(qkv, H, H, D), iters)
         + bench(lambda: ext.heads_merge(q), iters))
    row("fwd", "copy", t, 0.0)
    t = (bench(lambda: ext.heads_unmerge(d_o, H), iters)
         + bench(lambda: ext.qkv_split_transpose_bwd(dq, k, v, D), iters))
    row("bwd", "copy", t, 0.0)


def run(B, H, S, D, iters, results, packed=False):
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    do = torch.randn_like(q)
    sc = 1 / math.sqrt(D)
    fwd_fl = 4 * B * H * S * S * D / 2            # causal
    bwd_fl = fwd_fl * 2.5

    t = bench(lambda: ext.attn_fwd(q, k, v, sc), iters)
    results.append(dict(op="fwd", impl="hip", B=B, H=H, S=S, D=D,
                        ms=t * 1e3, tflops=fwd_fl / t / 1e12))

    t = bench(lambda: F.scaled_dot_product_attention(
        q, k, v, is_causal=True), iters)
    results.append(dict(op="fwd", impl="sdpa", B=B, H=H, S=S, D=D,
                        ms=t * 1e3, tflops=fwd_fl / t / 1e12))

    o, lse = ext.attn_fwd(q, k, v, sc)
    delta = (do.float() * o.float()).sum(-1).contiguous()
    t = bench(lambda: ext.attn_bwd(q, k, v, do, lse, delta, sc), iters)
    results.append(dict(op="bwd", impl="hip", B=B, H=H, S=S, D=D,
                        ms=t * 1e3, tflops=bwd_fl / t / 1e12))
    if packed:
        run_packed(q, k, v, do, iters, results)

    qs = q.clone().requires_grad_(True)
    ks = k.clone().requires_grad_(True)
    vs = v.clone().requires_grad_(True)
    out = F.scaled_dot_product_attention(qs, ks, vs, is_causal=True)

    def sdpa_bwd():
        qs.grad = ks.grad = vs.grad = None
        torch.autograd.grad(out, (qs, ks, vs), do, retain_graph=True)

    t = bench(sdpa_bwd, iters)
    results.append(dict(op="bwd", impl="sdpa", B=B, H=H, S=S, D=D,
                        ms=t * 1e3, tflops=bwd_fl / t / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--packed", action="store_true",
                    help="also time the packed entry points and the copies "
                         "they replace")
    args = ap.parse_args()
    results = []
    # flagship-relevant shapes: gpt3-2.7b (H=32, D=80), llama/gpt D=128, D=64;
    # the last is the flagship microbatch itself
    for B, H, S, D in [(4, 32, 2048, 64), (4, 32, 2048, 80),
                       (4, 32, 2048, 128), (2, 32, 4096, 128),
                       (16, 32, 2048, 80)]:
        run(B, H, S, D, args.iters, results, args.packed)
    for r in results:
        print(f"{r['op']:>3} {r['impl']:>6} B{r['B']} H{r['H']} S{r['S']} "
              f"D{r['D']:<3} {r['ms']:8.3f} ms  {r['tflops']:7.1f} TF/s")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Decode-path microbench: tokens/s for KV-cache generation on 1 GPU.

A/B driver for METIS_DECODE_KERNEL (single-query decode attention
kernel vs the SDPA fallback): run once with the env unset and once =1.

Usage: python scripts/decode_bench.py [--model llama3-1b] [--new 64]

Two further modes:

  --kernel   device-event timing of ext.attn_decode (decode.hip) against
             ext.attn_decode_ragged (decode_ragged.hip) over a shape grid,
             alternating the two; prints microseconds, achieved bytes/s
             (bytes needed = 2 * sum_b kv_len_b * Hkv * D * 2) and that as
             a share of the 6.3 TB/s achievable HBM bandwidth.
  --ragged   the continuous-batching workload (llama3-1b, 8 requests,
             prompts 64-183 tokens, 32 new each, ContinuousBatcher), once
             per METIS_DECODE_KERNEL value in fresh child processes,
             alternated; prints tok/s per repeat and the spread.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from metis_amd.cli.plan_runner import MODEL_SPECS
from metis_amd.models.gpt import GPTModel, GPTModelSpec
from metis_amd.models.llama import LlamaModel, LlamaModelSpec
from metis_amd.runtime.generate import generate

HBM_ACHIEVABLE = 6.3e12     # bytes/s, MI355X achievable HBM read bandwidth
RESULT_TAG = "RAGGED_RESULT "


def _time_alternating(fns, iters, warmup):
    """Median device-event time (us) of each callable, calls interleaved
    so drift and neighbours hit all of them alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    evs = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[i].append((a, b))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) * 1e3 for a, b in e)
            for e in evs]


def kernel_mode(args):
    from metis_amd.ops import require_extension

    ext = require_extension()
    torch.manual_seed(0)
    print("kernel  B   H Hkv   D      S  lens     |   dense us  TB/s  %HBM |"
          "  ragged us  TB/s  %HBM  splits=auto | speedup")

    def report(B, H, Hkv, D, S, lens_list, tag):
        q = torch.randn(B, H, 1, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn_like(k)
        lens = torch.tensor(lens_list, device="cuda", dtype=torch.int32)
        scale = 1.0 / math.sqrt(D)
        need = 2 * sum(lens_list) * Hkv * D * 2          # K and V, bf16
        fns = [lambda: ext.attn_decode_ragged(q, k, v, lens, scale)]
        dense = tag == "full"     # decode.hip has no per-row length
        if dense:
            fns.insert(0, lambda: ext.attn_decode(q, k, v, scale))
        us = _time_alternating(fns, args.iters, args.warmup)

        def cols(t):
            bps = need / (t * 1e-6)
            return f"{t:10.1f} {bps / 1e12:5.2f} {100 * bps / HBM_ACHIEVABLE:5.1f}"

        d = cols(us[0]) if dense else " " * 10 + "  n/a   n/a"
        sp = f"{us[0] / us[-1]:6.2f}x" if dense else "   n/a"
        print(f"kernel {B:2d} {H:3d} {Hkv:3d} {D:3d} {S:6d}  {tag:8s} | {d} | "
              f"{cols(us[-1])}              | {sp}", flush=True)

    for H, Hkv, D in ((32, 8, 64), (32, 8, 128)):
        for B in (1, 8, 64):
            for S in (512, 4096, 16384):
                report(B, H, Hkv, D, S, [S] * B, "full")
        g = torch.Generator().manual_seed(1)
        for B, S in ((8, 4096), (64, 4096)):
            lens = torch.randint(S // 8, S + 1, (B,), generator=g).tolist()
            report(B, H, Hkv, D, S, lens, "S/8..S")


def _ragged_child(args):
    """One process, one METIS_DECODE_KERNEL value (from the environment):
    warm up once, then time whole ContinuousBatcher runs."""
    from metis_amd.models.llama import LLAMA_SPECS
    from metis_amd.runtime.generate import ContinuousBatcher

    spec = LLAMA_SPECS["llama3-1b"]
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LlamaModel(spec, tp=1, dtype=torch.bfloat16)
    model.eval()
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, spec.vocab_size, (64 + 17 * i,),
                             generator=g).tolist() for i in range(8)]
    new = 32

    def run():
        cb = ContinuousBatcher(model, capacity=256, max_batch=8,
                               device="cuda")
        for p in prompts:
            cb.submit(p, new, temperature=0.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = cb.run_until_done()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert all(len(done[i]) == len(p) + new
                   for i, p in enumerate(prompts))
        return len(prompts) * new / dt

    with torch.no_grad():
        run()                                   # warmup
        tps = [run() for _ in range(args.inner)]
    print(RESULT_TAG + json.dumps({"tok_s": tps}), flush=True)


def ragged_mode(args):
    """Parent: never touches the GPU; starts one fresh child per
    measurement, alternating METIS_DECODE_KERNEL=0 / 1."""
    results = {"0": [], "1": []}
    for rep in range(args.repeats):
        for flag in ("0", "1"):
            env = dict(os.environ, METIS_DECODE_KERNEL=flag)
            out = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "--ragged-child",
                 "--inner", str(args.inner)],
                env=env, check=True, capture_output=True, text=True).stdout
            line = [ln for ln in out.splitlines()
                    if ln.startswith(RESULT_TAG)][-1]
            tps = json.loads(line[len(RESULT_TAG):])["tok_s"]
            med = statistics.median(tps)
            results[flag].append(med)
            print(f"ragged repeat {rep} METIS_DECODE_KERNEL={flag}: "
                  f"median {med:.1f} tok/s of "
                  f"{[round(t, 1) for t in tps]}", flush=True)
    summary = {}
    for flag, name in (("0", "mask-SDPA"), ("1", "ragged kernel")):
        r = results[flag]
        summary[flag] = (statistics.median(r), max(r) - min(r))
        print(f"ragged METIS_DECODE_KERNEL={flag} ({name}): "
              f"median {summary[flag][0]:.1f} tok/s, "
              f"spread {summary[flag][1]:.1f} (min {min(r):.1f}, "
              f"max {max(r):.1f}) over {len(r)} processes")
    spread = max(summary["0"][1], summary["1"][1])
    gain = summary["1"][0] / summary["0"][0] - 1.0
    keep = summary["1"][0] >= summary["0"][0] - spread
    print(f"ragged verdict: kernel {100 * gain:+.1f}% vs mask-SDPA, "
          f"repeat-to-repeat spread {spread:.1f} tok/s -> "
          f"{'default ON' if keep else 'opt-in'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-1b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--kernel", action="store_true",
                    help="decode.hip vs decode_ragged.hip kernel timing")
    ap.add_argument("--ragged", action="store_true",
                    help="continuous-batching A/B over METIS_DECODE_KERNEL")
    ap.add_argument("--ragged-child", action="store_true",
                    help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()

    if args.kernel:
        assert args.iters >= 50, "--kernel times at least 50 iterations"
        return kernel_mode(args)
    if args.ragged_child:
        return _ragged_child(args)
    if args.ragged:
        assert args.repeats >= 3, "--ragged needs at least 3 repeats"
        return ragged_mode(args)

    spec = MODEL_SPECS[args.model]
    cls = LlamaModel if isinstance(spec, LlamaModelSpec) else GPTModel
    torch.manual_seed(0)
    model = cls(spec, tp=1, dtype=torch.bfloat16).to("cuda")
    tokens = torch.randint(0, spec.vocab_size, (args.batch, args.prompt),
                           device="cuda")
    # warmup
    generate(model, tokens, 8, temperature=0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = generate(model, tokens, args.new, temperature=0.0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tps = args.batch * args.new / dt
    flag = os.environ.get("METIS_DECODE_KERNEL", "1(default)")
    print(f"decode {args.model} b{args.batch} p{args.prompt} n{args.new} "
          f"METIS_DECODE_KERNEL={flag}: {dt*1e3:.1f} ms, {tps:.0f} tok/s")
    assert out.shape == (args.batch, args.prompt + args.new)


if __name__ == "__main__":
    main()

"""Decode-path microbench: tokens/s for KV-cache generation on 1 GPU.

A/B driver for METIS_DECODE_KERNEL (single-query decode attention
kernel vs the SDPA fallback): run once with the env unset and once =1.

Usage: python scripts/decode_bench.py [--model llama3-1b] [--new 64]

Two further modes:

  --kernel   device-event timing of ext.attn_decode (decode.hip) against
             ext.attn_decode_ragged (decode_ragged.hip) over a shape grid,
             alternating the two; prints microseconds, achieved bytes/s
             (bytes needed = 2 * sum_b kv_len_b * Hkv * D * 2) and that as
             a share of the 6.3 TB/s achievable HBM bandwidth. With
             --kv-dtype fp8 the fp8-cache kernel (decode_ragged_fp8.hip)
             runs on the same K/V quantised per row, alternated call by
             call with the other two (bytes needed = 2 * sum_b kv_len_b *
             Hkv * (D + 4)); its speedup column is against the bf16 ragged
             kernel.
  --ragged   the continuous-batching workload (llama3-1b, 8 requests,
             prompts 64-183 tokens, 32 new each, ContinuousBatcher), once
             per METIS_DECODE_KERNEL value in fresh child processes,
             alternated; prints tok/s per repeat and the spread. With
             --ab-weights the two arms are bf16 and fp8 weights instead
             (METIS_DECODE_KERNEL left alone), and peak allocated memory
             is reported per arm. With --ab-kv the two arms are a bf16 and
             an fp8 KV cache (ContinuousBatcher kv_dtype) in the same way;
             --long-context swaps the workload for 8 prompts of 3072-3968
             tokens in a cache of capacity 4096.
  --linear   device-event timing of the fp8 weight-only decode linear
             (w8_linear.hip) against bf16 F.linear (hipBLASLt) on the
             llama3-1b / llama3-8b linears at M in {1, 4, 8, 16}, the two
             alternated call by call while rotating through enough distinct
             weight buffers that either arm's set exceeds the 256 MiB
             last-level cache; --sweep-splits adds explicit split counts.

  --steady   steady decoding, bf16 against fp8 weights in one process:
             batch 8, a 64-token prefill into a KVCache, then 64 timed
             single-token steps per arm, arms alternated; ms/step.

--weight-dtype fp8 quantises the model (runtime.quantize) in the
end-to-end modes.
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

    from metis_amd.ops.kv8 import quantize_kv_e4m3

    ext = require_extension()
    torch.manual_seed(0)
    fp8 = args.kv_dtype == "fp8"
    print("kernel  B   H Hkv   D      S  lens     |   dense us  TB/s  %HBM |"
          "  ragged us  TB/s  %HBM  splits=auto | speedup"
          + (" |     fp8 us  TB/s  %HBM | fp8 vs ragged" if fp8 else ""))

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
        if fp8:
            k8, ks = quantize_kv_e4m3(k)
            v8, vs = quantize_kv_e4m3(v)
            need8 = 2 * sum(lens_list) * Hkv * (D + 4)   # bytes + scales
            fns.append(lambda: ext.attn_decode_ragged_fp8(
                q, k8, v8, ks, vs, lens, scale))
        us = _time_alternating(fns, args.iters, args.warmup)
        rag = us[1] if dense else us[0]

        def cols(t, need=need):
            bps = need / (t * 1e-6)
            return f"{t:10.1f} {bps / 1e12:5.2f} {100 * bps / HBM_ACHIEVABLE:5.1f}"

        d = cols(us[0]) if dense else " " * 10 + "  n/a   n/a"
        sp = f"{us[0] / rag:6.2f}x" if dense else "   n/a"
        f8 = (f" | {cols(us[-1], need8)} | {rag / us[-1]:6.2f}x"
              if fp8 else "")
        print(f"kernel {B:2d} {H:3d} {Hkv:3d} {D:3d} {S:6d}  {tag:8s} | {d} | "
              f"{cols(rag)}              | {sp}{f8}", flush=True)

    for H, Hkv, D in ((32, 8, 64), (32, 8, 128)):
        for B in (1, 8, 64):
            for S in (512, 4096, 16384):
                report(B, H, Hkv, D, S, [S] * B, "full")
        g = torch.Generator().manual_seed(1)
        for B, S in ((8, 4096), (64, 4096)):
            lens = torch.randint(S // 8, S + 1, (B,), generator=g).tolist()
            report(B, H, Hkv, D, S, lens, "S/8..S")


LINEAR_SPLIT_SWEEP = (1, 2, 4, 8, 16)
LLC_BYTES = 256 << 20


def linear_mode(args):
    import torch.nn.functional as F

    from metis_amd.models.llama import LLAMA_SPECS
    from metis_amd.ops import require_extension
    from metis_amd.ops.w8 import quantize_weight_e4m3

    ext = require_extension()
    torch.manual_seed(0)
    sweep = LINEAR_SPLIT_SWEEP if args.sweep_splits else ()
    print("linear model      layer       N      K   M bufs splits |"
          "    fp8 us  TB/s  %HBM |   bf16 us  TB/s  %HBM | speedup"
          + ("".join(f" | ns={n:<2d} us" for n in sweep)), flush=True)
    for name in ("llama3-1b", "llama3-8b"):
        spec = LLAMA_SPECS[name]
        h, f, d = spec.hidden_size, spec.ffn_hidden_size, spec.head_dim
        layers = (("qkv", (spec.num_heads + 2 * spec.num_kv_heads) * d, h),
                  ("proj", h, h), ("gate_up", 2 * f, h), ("down", h, f),
                  ("head", spec.vocab_size, h))
        for layer, N, K in layers:
            # distinct buffers: the fp8 set alone exceeds the cache
            nbuf = max(2, -(-(LLC_BYTES * 5 // 4) // (N * K)))
            w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
            w8, scale = quantize_weight_e4m3(w)
            bias = torch.zeros(N, device="cuda", dtype=torch.bfloat16)
            w8s = [w8.clone() for _ in range(nbuf)]
            wbs = [w.clone() for _ in range(nbuf)]
            del w, w8
            ns_auto = ext.w8_linear_auto_splits(N, K)
            for M in (1, 4, 8, 16):
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
                # each arm starts elsewhere in the ring, so no arm finds
                # a buffer another arm has just pulled into the cache
                arms = 2 + len(sweep)
                turn = [a * nbuf // arms for a in range(arms)]

                def nxt(arm):
                    turn[arm] = (turn[arm] + 1) % nbuf
                    return turn[arm]

                fns = [lambda: ext.w8_linear(x, w8s[nxt(0)], scale, bias),
                       lambda: F.linear(x, wbs[nxt(1)], bias)]
                for j, ns in enumerate(sweep):
                    fns.append(lambda ns=ns, j=j: ext.w8_linear(
                        x, w8s[nxt(2 + j)], scale, bias, ns))
                us = _time_alternating(fns, args.iters, args.warmup)

                def cols(t, nbytes):
                    bps = nbytes / (t * 1e-6)
                    return (f"{t:9.1f} {bps / 1e12:5.2f} "
                            f"{100 * bps / HBM_ACHIEVABLE:5.1f}")

                print(f"linear {name:10s} {layer:8s} {N:6d} {K:6d} {M:3d} "
                      f"{nbuf:4d} {ns_auto:6d} | {cols(us[0], N * K)} | "
                      f"{cols(us[1], 2 * N * K)} | {us[1] / us[0]:6.2f}x"
                      + "".join(f" | {t:8.1f}" for t in us[2:]), flush=True)
            del w8s, wbs
            torch.cuda.empty_cache()


def steady_mode(args):
    """Decode steps only (no prefill in the timed window): what the fp8
    weight-only kernel buys once a batch is running."""
    from metis_amd.models.llama import LLAMA_SPECS
    from metis_amd.runtime.generate import KVCache
    from metis_amd.runtime.quantize import quantize_for_decode

    spec = LLAMA_SPECS[args.model]
    with torch.device("cuda"):
        torch.manual_seed(0)
        dense = LlamaModel(spec, tp=1, dtype=torch.bfloat16).eval()
        torch.manual_seed(0)
        quant = LlamaModel(spec, tp=1, dtype=torch.bfloat16).eval()
    quantize_for_decode(quant)
    torch.cuda.empty_cache()
    B, P, steps = args.batch, 64, 64
    toks = torch.randint(0, spec.vocab_size, (B, P), device="cuda")
    nxt = torch.randint(0, spec.vocab_size, (B, 1), device="cuda")
    res = {"bf16": [], "fp8": []}
    with torch.no_grad():
        for rep in range(args.repeats + 1):         # first round warms up
            for label, model in (("bf16", dense), ("fp8", quant)):
                cache = KVCache()
                model(toks, cache=cache, pos_offset=0)
                for i in range(4):                  # warm the step shapes
                    model(nxt, cache=cache, pos_offset=P + i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    model(nxt, cache=cache, pos_offset=P + 4 + i)
                torch.cuda.synchronize()
                if rep:
                    res[label].append(
                        (time.perf_counter() - t0) * 1e3 / steps)
    for label in ("bf16", "fp8"):
        r = res[label]
        med = statistics.median(r)
        print(f"steady {args.model} batch {B} weights={label}: ms/step "
              f"{[round(x, 3) for x in r]}, median {med:.3f} "
              f"({B / med * 1e3:.0f} tok/s)", flush=True)


def _ragged_child(args):
    """One process, one METIS_DECODE_KERNEL value (from the environment):
    warm up once, then time whole ContinuousBatcher runs."""
    from metis_amd.models.llama import LLAMA_SPECS
    from metis_amd.runtime.generate import ContinuousBatcher

    spec = LLAMA_SPECS[args.model]
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LlamaModel(spec, tp=1, dtype=torch.bfloat16)
    model.eval()
    if args.weight_dtype == "fp8":
        from metis_amd.runtime.quantize import quantize_for_decode

        quantize_for_decode(model)
        torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    g = torch.Generator().manual_seed(0)
    if args.long_context:       # multiples of 128: flash-attention prefill
        plens, capacity = [3072 + 128 * i for i in range(8)], 4096
    else:
        plens, capacity = [64 + 17 * i for i in range(8)], 256
    prompts = [torch.randint(0, spec.vocab_size, (n,),
                             generator=g).tolist() for n in plens]
    new = 32

    def run():
        cb = ContinuousBatcher(model, capacity=capacity, max_batch=8,
                               device="cuda", kv_dtype=args.kv_dtype)
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
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print(RESULT_TAG + json.dumps({"tok_s": tps, "peak_gib": peak}),
          flush=True)


def _run_child(args, env, weight_dtype, kv_dtype="bf16"):
    out = subprocess.run(
        [sys.executable, os.path.abspath(__file__), "--ragged-child",
         "--inner", str(args.inner), "--model", args.model,
         "--weight-dtype", weight_dtype, "--kv-dtype", kv_dtype]
        + (["--long-context"] if args.long_context else []),
        env=env, check=True, capture_output=True, text=True).stdout
    line = [ln for ln in out.splitlines() if ln.startswith(RESULT_TAG)][-1]
    return json.loads(line[len(RESULT_TAG):])


def ragged_weights_mode(args):
    """Parent: never touches the GPU; one fresh child per measurement,
    alternating bf16 and fp8 weights."""
    results = {"bf16": [], "fp8": []}
    peaks = {"bf16": [], "fp8": []}
    for rep in range(args.repeats):
        for wd in ("bf16", "fp8"):
            res = _run_child(args, dict(os.environ), wd, args.kv_dtype)
            med = statistics.median(res["tok_s"])
            results[wd].append(med)
            peaks[wd].append(res["peak_gib"])
            print(f"ragged {args.model} repeat {rep} weights={wd}: median "
                  f"{med:.1f} tok/s of {[round(t, 1) for t in res['tok_s']]}, "
                  f"peak {res['peak_gib']:.2f} GiB", flush=True)
    for wd in ("bf16", "fp8"):
        r = results[wd]
        print(f"ragged {args.model} weights={wd}: median "
              f"{statistics.median(r):.1f} tok/s, spread {max(r) - min(r):.1f} "
              f"(min {min(r):.1f}, max {max(r):.1f}) over {len(r)} processes, "
              f"peak allocated {max(peaks[wd]):.2f} GiB")
    gain = statistics.median(results["fp8"]) / statistics.median(results["bf16"])
    print(f"ragged {args.model} verdict: fp8 weights {100 * (gain - 1):+.1f}% "
          f"tok/s vs bf16 (opt-in either way: fp8 changes the numerics)")


def ragged_kv_mode(args):
    """Parent: never touches the GPU; one fresh child per measurement,
    alternating a bf16 and an fp8 KV cache (weights as --weight-dtype)."""
    results = {"bf16": [], "fp8": []}
    peaks = {"bf16": [], "fp8": []}
    ctx = "long-context " if args.long_context else ""
    for rep in range(args.repeats):
        for kd in ("bf16", "fp8"):
            res = _run_child(args, dict(os.environ), args.weight_dtype, kd)
            med = statistics.median(res["tok_s"])
            results[kd].append(med)
            peaks[kd].append(res["peak_gib"])
            print(f"ragged {ctx}{args.model} repeat {rep} kv={kd}: median "
                  f"{med:.1f} tok/s of {[round(t, 1) for t in res['tok_s']]}, "
                  f"peak {res['peak_gib']:.2f} GiB", flush=True)
    for kd in ("bf16", "fp8"):
        r = results[kd]
        print(f"ragged {ctx}{args.model} weights={args.weight_dtype} kv={kd}: "
              f"median {statistics.median(r):.1f} tok/s, spread "
              f"{max(r) - min(r):.1f} (min {min(r):.1f}, max {max(r):.1f}) "
              f"over {len(r)} processes, peak allocated "
              f"{max(peaks[kd]):.2f} GiB")
    gain = statistics.median(results["fp8"]) / statistics.median(results["bf16"])
    print(f"ragged {ctx}{args.model} verdict: fp8 KV cache "
          f"{100 * (gain - 1):+.1f}% tok/s vs bf16 (opt-in either way: fp8 "
          f"changes the numerics)")


def ragged_mode(args):
    """Parent: never touches the GPU; starts one fresh child per
    measurement, alternating METIS_DECODE_KERNEL=0 / 1."""
    results = {"0": [], "1": []}
    for rep in range(args.repeats):
        for flag in ("0", "1"):
            env = dict(os.environ, METIS_DECODE_KERNEL=flag)
            tps = _run_child(args, env, args.weight_dtype,
                             args.kv_dtype)["tok_s"]
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
    ap.add_argument("--linear", action="store_true",
                    help="w8_linear.hip vs bf16 F.linear kernel timing")
    ap.add_argument("--steady", action="store_true",
                    help="decode-steps-only ms/step, bf16 vs fp8 weights")
    ap.add_argument("--sweep-splits", action="store_true",
                    help="--linear: also time explicit num_splits values")
    ap.add_argument("--weight-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="fp8: weight-only quantised linears (end-to-end modes)")
    ap.add_argument("--ab-weights", action="store_true",
                    help="--ragged: alternate bf16 / fp8 weights instead of "
                         "METIS_DECODE_KERNEL")
    ap.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="--kernel: add the fp8-cache kernel's columns; "
                         "--ragged: KV cache of the ContinuousBatcher")
    ap.add_argument("--ab-kv", action="store_true",
                    help="--ragged: alternate a bf16 / fp8 KV cache instead "
                         "of METIS_DECODE_KERNEL")
    ap.add_argument("--long-context", action="store_true",
                    help="--ragged: 8 prompts of 3072-3968 tokens, capacity "
                         "4096, instead of 64-183 tokens in 256")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    args = ap.parse_args()

    if args.kernel:
        assert args.iters >= 50, "--kernel times at least 50 iterations"
        return kernel_mode(args)
    if args.linear:
        assert args.iters >= 50, "--linear times at least 50 iterations"
        return linear_mode(args)
    if args.steady:
        return steady_mode(args)
    if args.ragged_child:
        return _ragged_child(args)
    if args.ragged:
        assert args.repeats >= 3, "--ragged needs at least 3 repeats"
        if args.ab_weights:
            return ragged_weights_mode(args)
        if args.ab_kv:
            return ragged_kv_mode(args)
        return ragged_mode(args)

    spec = MODEL_SPECS[args.model]
    cls = LlamaModel if isinstance(spec, LlamaModelSpec) else GPTModel
    torch.manual_seed(0)
    model = cls(spec, tp=1, dtype=torch.bfloat16).to("cuda")
    model.eval()
    if args.weight_dtype == "fp8":
        from metis_amd.runtime.quantize import quantize_for_decode

        quantize_for_decode(model)
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
          f"METIS_DECODE_KERNEL={flag} weights={args.weight_dtype}: "
          f"{dt*1e3:.1f} ms, {tps:.0f} tok/s")
    assert out.shape == (args.batch, args.prompt + args.new)


if __name__ == "__main__":
    main()

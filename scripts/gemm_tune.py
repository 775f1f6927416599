#!/usr/bin/env python3
"""Tune the linear layers' backward GEMMs and write the algorithm table.

For each (op, M, N, K) — op is ``dgrad`` (dx = dy @ w) or ``wgrad``
(dw = dy^T @ x), with dy [M,N], w [N,K], x [M,K] — the tuner times

* the aten call autograd makes today (three rounds: its spread is the bar),
* hipBLASLt's heuristic default in the same layout (algo -1),
* for dgrad, the TN route on a transposed weight copy (``lt_tn``), with the
  transpose kernel timed beside it,
* every algorithm ``getAllAlgos`` lists that ``matmulIsAlgoSupported``
  accepts for the shape, capped at the first ``--max-algos`` (default 64;
  the output says when the cap cut the list).

Timing: device events, 3 warm-up and 10 timed calls per arm, cycling
through at least three operand sets sized so that no arm finds its operands
in the 256 MiB last-level cache. A candidate whose first timed call is more
than three times the heuristic default is dropped as slow without the
remaining calls. A candidate is rejected if three calls on the same inputs
are not bitwise equal, or if it fails the per-block conformance criterion
    max|got - ref| <= 2 max|base - ref| + 2^-8 max|ref|   per (row, 256 cols)
against the float64 product, base being the aten bf16 result. A candidate
whose call raises is skipped and never retried.

A route other than ``aten`` is written only where it beats the aten median
by more than the aten arm's spread (max - min of its three round medians,
at least 1 % of the median).

Also probes whether a weight-gradient algorithm with the BGRADB epilogue
(bias gradient in the same GEMM) exists at the fc2, qkv and head shapes.

    python scripts/gemm_tune.py --out profiles/mi355x/gemm_algos.json \
        --report gemm_tune_report.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

LLC_BYTES = 256 << 20
WARMUP, ITERS = 3, 10
ULP_BF16 = 2.0 ** -8
COL_BLOCK = 256

# flagship: GPT-3 2.7B, 16 x 2048 tokens; (layer, N, K) of y = x @ W^T
FLAGSHIP_M = 32768
FLAGSHIP_LAYERS = (("qkv", 7680, 2560), ("proj", 2560, 2560),
                   ("fc1", 10240, 2560), ("fc2", 2560, 10240),
                   ("head", 51200, 2560))


def _block_max(e, block=COL_BLOCK):
    e = e.abs()
    pad = -e.size(-1) % block
    if pad:
        e = torch.cat([e, e.new_zeros(*e.shape[:-1], pad)], dim=-1)
    return e.reshape(*e.shape[:-1], -1, block).amax(-1)


def conformance_ratio(got, base, ref):
    """Worst (row, 256-column) block of the criterion above; <= 1 passes."""
    eg = _block_max(got.double() - ref)
    eb = _block_max(base.double() - ref)
    bound = 2.0 * eb + ULP_BF16 * _block_max(ref)
    ratio = torch.where(eg == 0, torch.zeros_like(eg), eg / bound)
    ratio = torch.where(torch.isfinite(ratio), ratio,
                        torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def _events(n):
    return [(torch.cuda.Event(enable_timing=True),
             torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def time_calls(fn, sets, iters=ITERS, warmup=WARMUP, start=0):
    """Device-event times (us) of ``iters`` calls of fn(i), i cycling through
    the operand sets."""
    for j in range(warmup):
        fn((start + j) % sets)
    evs = _events(iters)
    for j, (a, b) in enumerate(evs):
        a.record()
        fn((start + warmup + j) % sets)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]


def tune_shape(ext, op, M, N, K, max_algos, log):
    dev, bf16 = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1234)
    flops = 2.0 * M * N * K
    other = (N, K) if op == "dgrad" else (M, K)     # w or x
    set_bytes = 2 * (M * N + other[0] * other[1])
    nset = max(3, -(-(LLC_BYTES * 5 // 4) // set_bytes))
    dys = [torch.randn(M, N, device=dev, dtype=bf16, generator=g)
           for _ in range(nset)]
    # weights at the scale of the model's init, activations at unit scale
    scale = K ** -0.5 if op == "dgrad" else 1.0
    oth = [torch.randn(*other, device=dev, dtype=bf16, generator=g) * scale
           for _ in range(nset)]

    if op == "dgrad":
        aten = lambda i: dys[i] @ oth[i]
        lt = lambda algo: (lambda i: ext.lt_linear_dgrad(dys[i], oth[i], algo))
        ref = dys[0].double() @ oth[0].double()
    else:
        aten = lambda i: dys[i].t() @ oth[i]
        lt = lambda algo: (lambda i: ext.lt_linear_wgrad(dys[i], oth[i], algo))
        ref = dys[0].double().t() @ oth[0].double()
    base = aten(0)

    def pf(us):
        return flops / (us * 1e-6) / 1e15 if us else 0.0

    def check(fn):
        """(repeatable, conformance ratio) of fn on operand set 0."""
        outs = [fn(0) for _ in range(3)]
        rep = all(torch.equal(outs[0], o) for o in outs[1:])
        return rep, conformance_ratio(outs[0], base, ref)

    res = {"op": op, "M": M, "N": N, "K": K, "operand_sets": nset}
    aten_rounds = [statistics.median(time_calls(aten, nset))]

    # heuristic default in the same layout
    t_def = statistics.median(time_calls(lt(-1), nset))
    rep, ratio = check(lt(-1))
    res["default"] = {"algo": int(ext.lt_heuristic_algo(op, M, N, K)),
                      "us": t_def, "pf": pf(t_def), "repeatable": rep,
                      "ratio": ratio}

    arms = []       # (route, algo, us)
    if rep and ratio <= 1.0:
        arms.append(("lt", -1, t_def))

    if op == "dgrad":
        wts = [ext.transpose_bf16(w) for w in oth]
        tn = lambda i: ext.lt_linear_dgrad_tn(dys[i], wts[i])
        t_tn = statistics.median(time_calls(tn, nset))
        rep, ratio = check(tn)
        tbuf = torch.empty_like(wts[0])
        t_tr = statistics.median(time_calls(
            lambda i: ext.transpose_bf16_out(oth[i], tbuf), nset))
        res["lt_tn"] = {"us": t_tn, "pf": pf(t_tn), "repeatable": rep,
                        "ratio": ratio, "transpose_us": t_tr,
                        "transpose_tbps": 4.0 * N * K / (t_tr * 1e-6) / 1e12}
        if rep and ratio <= 1.0:
            arms.append(("lt_tn", -1, t_tn))
        del wts, tbuf

    aten_rounds.append(statistics.median(time_calls(aten, nset, start=1)))

    algos = [int(a) for a in ext.lt_supported_algos(op, M, N, K)]
    res["supported"] = len(algos)
    res["capped"] = len(algos) > max_algos
    if res["capped"]:
        log(f"  {len(algos)} supported algorithms, trying the first "
            f"{max_algos}")
        algos = algos[:max_algos]
    cands, counts = [], {"tried": 0, "slow": 0, "error": 0,
                         "not_repeatable": 0, "not_conformant": 0}
    for algo in algos:
        counts["tried"] += 1
        fn = lt(algo)
        try:
            first = time_calls(fn, nset, iters=1, warmup=1)[0]
            if first > 3.0 * t_def:
                counts["slow"] += 1
                cands.append({"algo": algo, "us": first, "status": "slow"})
                continue
            us = statistics.median(time_calls(fn, nset, warmup=2))
            rep, ratio = check(fn)
        except RuntimeError as e:       # an error status: skip, never retry
            counts["error"] += 1
            cands.append({"algo": algo, "status": "error",
                          "error": str(e).splitlines()[0][:120]})
            continue
        status = ("not_repeatable" if not rep else
                  "not_conformant" if ratio > 1.0 else "ok")
        if status != "ok":
            counts[status] += 1
        else:
            arms.append(("lt", algo, us))
        cands.append({"algo": algo, "us": us, "pf": pf(us), "ratio": ratio,
                      "status": status})
    res["candidates"], res["counts"] = cands, counts

    aten_rounds.append(statistics.median(time_calls(aten, nset, start=2)))
    t_aten = statistics.median(aten_rounds)
    spread = max(max(aten_rounds) - min(aten_rounds), 0.01 * t_aten)
    res["aten"] = {"us": t_aten, "pf": pf(t_aten), "rounds": aten_rounds,
                   "spread_us": spread}

    best = min(arms, key=lambda a: a[2]) if arms else None
    res["best"] = ({"route": best[0], "algo": best[1], "us": best[2],
                    "pf": pf(best[2])} if best else None)
    if best is not None and best[2] < t_aten - spread:
        route, algo, us = best
    else:
        route, algo, us = "aten", -1, t_aten
    res["entry"] = {"op": op, "M": M, "N": N, "K": K, "route": route,
                    "algo": algo, "best_us": round(us, 1),
                    "default_us": round(t_def, 1),
                    "aten_us": round(t_aten, 1)}
    if op == "dgrad":
        res["entry"]["lt_tn_us"] = round(res["lt_tn"]["us"], 1)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None,
                    help="table file to write (default: print only)")
    ap.add_argument("--report", default=None,
                    help="full per-candidate report (JSON)")
    ap.add_argument("--ops", default="dgrad,wgrad")
    ap.add_argument("--shapes", default=None,
                    help="M,N,K;M,N,K;... (default: the flagship layers)")
    ap.add_argument("--max-algos", type=int, default=64)
    args = ap.parse_args()

    from metis_amd.ops import require_extension
    from metis_amd.ops.linear import device_id

    ext = require_extension()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_tune.py needs a GPU")

    if args.shapes:
        shapes = [tuple(int(v) for v in s.split(","))
                  for s in args.shapes.split(";")]
    else:
        shapes = [(FLAGSHIP_M, n, k) for _, n, k in FLAGSHIP_LAYERS]
    t0 = time.time()

    def log(msg):
        print(f"[{time.time() - t0:6.1f}s] {msg}", flush=True)

    header = {"hipblaslt_version": int(ext.lt_version()),
              "device": device_id()}
    log(f"hipBLASLt {header['hipblaslt_version']} on {header['device']}")
    results = []
    for op in args.ops.split(","):
        for M, N, K in shapes:
            log(f"{op} M={M} N={N} K={K}")
            r = tune_shape(ext, op, M, N, K, args.max_algos, log)
            results.append(r)
            e, c = r["entry"], r["counts"]
            log(f"  aten {r['aten']['us']:.0f} us ({r['aten']['pf']:.2f} PF/s,"
                f" spread {r['aten']['spread_us']:.0f}) | default "
                f"{r['default']['us']:.0f} us | "
                + (f"lt_tn {r['lt_tn']['us']:.0f} us + transpose "
                   f"{r['lt_tn']['transpose_us']:.0f} us "
                   f"({r['lt_tn']['transpose_tbps']:.2f} TB/s) | "
                   if op == "dgrad" else "")
                + f"best {r['best']} | tried {c['tried']} slow {c['slow']} "
                f"error {c['error']} not-repeatable {c['not_repeatable']} "
                f"not-conformant {c['not_conformant']} -> {e['route']} "
                f"{e['algo']}")
            torch.cuda.empty_cache()

    bgradb = {}
    for name, n, k in FLAGSHIP_LAYERS:
        if name in ("fc2", "qkv", "head"):
            bgradb[name] = int(ext.lt_wgrad_bgradb_algos(FLAGSHIP_M, n, k))
    log(f"BGRADB weight-gradient algorithms offered: {bgradb}")

    table = dict(header, entries=[r["entry"] for r in results])
    print(json.dumps(table, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    if args.report:
        with open(args.report, "w") as f:
            json.dump(dict(header, bgradb_algos=bgradb, shapes=results), f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Tune the linear layers' backward GEMMs and write the algorithm table.

For each (op, M, N, K) — op is ``dgrad`` (dx = dy @ w) or ``wgrad``
(dw = dy^T @ x), with dy [M,N], w [N,K], x [M,K] — the tuner times

* the aten call autograd makes today (three rounds: its spread is the bar),
* hipBLASLt's heuristic default in the same layout (algo -1),
* for dgrad, the TN route on a transposed weight copy (``lt_tn``), with the
  transpose kernel timed beside it,
* for wgrad, the four routes on transposed activations (``lt_dyt``,
  ``lt_xt``, ``lt_xt_nn``, ``lt_dyt_xt``; metis_amd/ops/linear.py). The
  activation changes with every call, so the transposes a route needs (and
  the transpose of dwT back for ``lt_xt_nn``) run inside its timed region,
  into a reused buffer; they are also timed alone and reported beside it,
* every algorithm ``getAllAlgos`` lists that ``matmulIsAlgoSupported``
  accepts for the shape: in the op's own layout capped at the first
  ``--max-algos`` (default 64), in each transposed wgrad layout at the first
  ``--max-route-algos`` (default 64); the output says when a cap cut a list.

Timing: device events, 3 warm-up and 10 timed calls per arm, cycling
through at least three operand sets sized so that no arm finds its operands
in the 256 MiB last-level cache. A candidate whose first timed call is more
than three times the heuristic default of its route is dropped as slow
without the remaining calls. A candidate is rejected if three calls on the
same inputs are not bitwise equal, or if it fails the per-block conformance
criterion
    max|got - ref| <= 2 max|base - ref| + 2^-8 max|ref|   per (row, 256 cols)
against the float64 product, base being the aten bf16 result. A candidate
whose call raises is skipped and never retried.

A route other than ``aten`` is written only where it beats the aten median
by more than the aten arm's spread (max - min of its three round medians,
at least 1 % of the median).

Every (op, shape) is tuned in a fresh child process under its own time
limit (``--shape-timeout``); the first child that fails or runs out of time
ends the run: no table is written, and the report holds the shapes that
finished.

Also probes whether a weight-gradient algorithm with the BGRADB epilogue
(bias gradient in the same GEMM) exists at the fc2, qkv and head shapes.

    python scripts/gemm_tune.py --out profiles/mi355x/gemm_algos.json \
        --report gemm_tune_report.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
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

# wgrad route -> (problem name in lt_gemm.cpp, transposes dy, transposes x)
WGRAD_ROUTES = {"lt_dyt": ("wgrad_dyt", True, False),
                "lt_xt": ("wgrad_xt", False, True),
                "lt_xt_nn": ("wgrad_xt_nn", False, True),
                "lt_dyt_xt": ("wgrad_tn", True, True)}


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


def wgrad_route_fn(ext, route, dys, xs, scratch):
    """algo -> fn(i): the whole ``route`` on operand set i, transposes
    included, as ops/linear.py runs it. ``scratch`` holds the reused flat
    buffers for dy^T and x^T."""
    M, N = dys[0].shape
    K = xs[0].size(1)

    def dyt(i):
        out = scratch["dy"][:M * N].view(N, M)
        ext.transpose_bf16_out(dys[i], out)
        return out

    def xt(i):
        out = scratch["x"][:M * K].view(K, M)
        ext.transpose_bf16_out(xs[i], out)
        return out

    if route == "lt_dyt":
        return lambda a: (lambda i: ext.lt_linear_wgrad_dyt(dyt(i), xs[i], a))
    if route == "lt_xt":
        return lambda a: (lambda i: ext.lt_linear_wgrad_xt(dys[i], xt(i), a))
    if route == "lt_xt_nn":
        return lambda a: (lambda i: ext.transpose_bf16(
            ext.lt_linear_wgrad_xt_nn(dys[i], xt(i), a)))
    if route == "lt_dyt_xt":
        return lambda a: (lambda i: ext.lt_linear_wgrad_tn(dyt(i), xt(i), a))
    raise ValueError(route)


def tune_shape(ext, op, M, N, K, max_algos, max_route_algos, log,
               routes=tuple(WGRAD_ROUTES)):
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

    arms = []       # (route, algo, us)

    def default_arm(route, make, problem):
        t = statistics.median(time_calls(make(-1), nset))
        rep, ratio = check(make(-1))
        if rep and ratio <= 1.0:
            arms.append((route, -1, t))
        return {"algo": int(ext.lt_heuristic_algo(problem, M, N, K)),
                "us": t, "pf": pf(t), "repeatable": rep, "ratio": ratio}

    def sweep(route, make, problem, t_def, cap):
        """Every supported algorithm of ``problem`` (first ``cap``) through
        the filters; the ones that pass join ``arms``."""
        algos = [int(a) for a in ext.lt_supported_algos(problem, M, N, K)]
        out = {"supported": len(algos), "capped": len(algos) > cap}
        if out["capped"]:
            log(f"  {route}: {len(algos)} supported algorithms, trying the "
                f"first {cap}")
            algos = algos[:cap]
        cands, counts = [], {"tried": 0, "slow": 0, "error": 0,
                             "not_repeatable": 0, "not_conformant": 0}
        for algo in algos:
            counts["tried"] += 1
            fn = make(algo)
            try:
                first = time_calls(fn, nset, iters=1, warmup=1)[0]
                if first > 3.0 * t_def:
                    counts["slow"] += 1
                    cands.append({"algo": algo, "us": first, "status": "slow"})
                    continue
                us = statistics.median(time_calls(fn, nset, warmup=2))
                rep, ratio = check(fn)
            except RuntimeError as e:   # an error status: skip, never retry
                counts["error"] += 1
                cands.append({"algo": algo, "status": "error",
                              "error": str(e).splitlines()[0][:120]})
                continue
            status = ("not_repeatable" if not rep else
                      "not_conformant" if ratio > 1.0 else "ok")
            if status != "ok":
                counts[status] += 1
            else:
                arms.append((route, algo, us))
            cands.append({"algo": algo, "us": us, "pf": pf(us),
                          "ratio": ratio, "status": status})
        out["candidates"], out["counts"] = cands, counts
        return out

    def best_of(route):
        mine = [a for a in arms if a[0] == route]
        return min(mine, key=lambda a: a[2]) if mine else None

    res = {"op": op, "M": M, "N": N, "K": K, "operand_sets": nset}
    aten_rounds = [statistics.median(time_calls(aten, nset))]

    # heuristic default in the same layout
    res["default"] = default_arm("lt", lt, op)
    t_def = res["default"]["us"]

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

    res.update(sweep("lt", lt, op, t_def, max_algos))

    if op == "wgrad" and M % 8 == 0 and N % 8 == 0 and K % 8 == 0:
        scratch = {"dy": torch.empty(M * N, device=dev, dtype=bf16),
                   "x": torch.empty(M * K, device=dev, dtype=bf16)}
        dwt = torch.empty(K, N, device=dev, dtype=bf16)
        dw = torch.empty(N, K, device=dev, dtype=bf16)
        tr = {}     # the transposes alone: us and TB/s (read + write)
        for name, srcs, dst in (
                ("dy", dys, scratch["dy"].view(N, M)),
                ("x", oth, scratch["x"].view(K, M)),
                ("dwT", [dwt] * nset, dw)):
            t = statistics.median(time_calls(
                lambda i: ext.transpose_bf16_out(srcs[i], dst), nset))
            tr[name] = {"us": t,
                        "tbps": 4.0 * dst.numel() / (t * 1e-6) / 1e12}
        res["transposes"] = tr
        del dwt, dw
        res["routes"] = {}
        for route in routes:
            problem, t_dy, t_x = WGRAD_ROUTES[route]
            make = wgrad_route_fn(ext, route, dys, oth, scratch)
            r = {"default": default_arm(route, make, problem)}
            r["transpose_us"] = (t_dy * tr["dy"]["us"] + t_x * tr["x"]["us"]
                                 + (route == "lt_xt_nn") * tr["dwT"]["us"])
            r.update(sweep(route, make, problem, r["default"]["us"],
                           max_route_algos))
            b = best_of(route)
            r["best"] = ({"algo": b[1], "us": b[2], "pf": pf(b[2])}
                         if b else None)
            res["routes"][route] = r
            log(f"  {route}: default {r['default']['us']:.0f} us, best "
                f"{r['best']}, of which transposes {r['transpose_us']:.0f} us,"
                f" counts {r['counts']}")
        del scratch

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
    else:
        b = best_of("lt")
        if b:
            res["entry"]["lt_us"] = round(b[2], 1)
            res["entry"]["lt_algo"] = b[1]
        for r in res.get("routes", {}):
            b = best_of(r)
            if b:
                res["entry"][r + "_us"] = round(b[2], 1)
    return res


def child(args):
    """Tune one (op, shape), or run the BGRADB probe, in this process and
    write the result to ``--child-out``."""
    from metis_amd.ops import require_extension
    from metis_amd.ops.linear import device_id

    ext = require_extension()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_tune.py needs a GPU")
    out = {"hipblaslt_version": int(ext.lt_version()), "device": device_id()}
    t0 = time.time()

    def log(msg):
        print(f"[{time.time() - t0:6.1f}s] {msg}", flush=True)

    if args.child == "bgradb":
        out["bgradb"] = {
            name: int(ext.lt_wgrad_bgradb_algos(FLAGSHIP_M, n, k))
            for name, n, k in FLAGSHIP_LAYERS
            if name in ("fc2", "qkv", "head")}
    else:
        op, M, N, K = args.child.split(",")
        M, N, K = int(M), int(N), int(K)
        r = tune_shape(ext, op, M, N, K, args.max_algos,
                       args.max_route_algos, log, args.routes.split(","))
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
        out["shape"] = r
    with open(args.child_out, "w") as f:
        json.dump(out, f)


def run_child(args, what, tmpdir):
    """One child under the time limit; any failure ends the whole run."""
    path = os.path.join(tmpdir, "child.json")
    if os.path.exists(path):
        os.remove(path)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what,
           "--child-out", path, "--max-algos", str(args.max_algos),
           "--max-route-algos", str(args.max_route_algos),
           "--routes", args.routes]
    try:
        rc = subprocess.run(cmd, timeout=args.shape_timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"gemm_tune.py: {what} exceeded "
                         f"{args.shape_timeout} s; stopping")
    if rc != 0:
        raise SystemExit(f"gemm_tune.py: {what} ended with status {rc}; "
                         "stopping")
    with open(path) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None,
                    help="table file to write (default: print only)")
    ap.add_argument("--report", default=None,
                    help="full per-candidate report (JSON)")
    ap.add_argument("--ops", default="dgrad,wgrad")
    ap.add_argument("--shapes", default=None,
                    help="M,N,K;M,N,K;... (default: the flagship layers)")
    ap.add_argument("--max-algos", type=int, default=64,
                    help="cap of the sweep in the op's own layout")
    ap.add_argument("--max-route-algos", type=int, default=64,
                    help="cap of the sweep in each transposed wgrad layout")
    ap.add_argument("--routes", default=",".join(WGRAD_ROUTES),
                    help="transposed wgrad routes to time (default: all)")
    ap.add_argument("--shape-timeout", type=int, default=300,
                    help="time limit of one (op, shape) child, seconds")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child:
        return child(args)

    if args.shapes:
        shapes = [tuple(int(v) for v in s.split(","))
                  for s in args.shapes.split(";")]
    else:
        shapes = [(FLAGSHIP_M, n, k) for _, n, k in FLAGSHIP_LAYERS]

    # this process never opens the GPU: one fresh child per step
    header, results, bgradb = None, [], None

    def write_report():
        if args.report:
            with open(args.report, "w") as f:
                json.dump(dict(header, bgradb_algos=bgradb, shapes=results),
                          f, indent=1)
                f.write("\n")

    with tempfile.TemporaryDirectory() as tmpdir:
        for op in args.ops.split(","):
            for M, N, K in shapes:
                print(f"{op} M={M} N={N} K={K}", flush=True)
                r = run_child(args, f"{op},{M},{N},{K}", tmpdir)
                results.append(r.pop("shape"))
                if header is None:
                    header = r
                elif header != r:
                    raise SystemExit("library version or device changed "
                                     "between shapes")
                write_report()
        bgradb = run_child(args, "bgradb", tmpdir)["bgradb"]
    print(f"BGRADB weight-gradient algorithms offered: {bgradb}", flush=True)

    table = dict(header, entries=[r["entry"] for r in results])
    print(json.dumps(table, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    write_report()


if __name__ == "__main__":
    main()

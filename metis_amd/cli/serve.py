"""Minimal completion server over the KV-cache decode path.

Serves a trained checkpoint (cli/train.py's per-rank format) or a
random-init model for smoke testing:

  python -m metis_amd.cli.serve --model gpt2-small \
      --checkpoint ckpts/step_1000/rank0.pt --port 8000

  POST /generate {"tokens": [[...]], "max_new_tokens": 32,
                  "temperature": 0.8, "top_k": 40}
  -> {"tokens": [[prompt + continuation]]}

Scope: single process (tp=pp=1), token-id interface (tokenizers are
deployment-specific). The single-query decode kernel (decode.hip) is
the default GPU decode path of per-request generate() calls;
``--continuous`` serves every request through one shared
ContinuousBatcher decode loop (requests join and leave the running
batch between steps), whose padded ragged cache is read by the split-S
ragged kernel (decode_ragged.hip) instead. ``--weight-dtype fp8`` quantises
the linear weights once at load (e4m3fn, per-channel scales) and decodes
through the weight-only fp8 kernel (w8_linear.hip); the default stays bf16.
``--kv-dtype fp8`` (with ``--continuous`` only) holds the batcher's KV cache
as e4m3fn bytes plus per-position scales (kv_quant.hip writes it,
decode_ragged_fp8.hip reads it); the default stays bf16 and the two fp8
options compose.
"""

from __future__ import annotations

import argparse

import torch

from metis_amd.models.gpt import GPTModel, MODEL_SPECS as _GPT_SPECS
from metis_amd.models.llama import LlamaModel, LlamaModelSpec, LLAMA_SPECS

MODEL_SPECS = {**_GPT_SPECS, **LLAMA_SPECS}
from metis_amd.runtime.generate import (ContinuousBatcher, generate,  # noqa: E402
                                         generate_ragged)
from metis_amd.runtime.quantize import (quantize_for_decode,  # noqa: E402
                                         weight_dtype_of)


class BatcherWorker:
    """One background decode loop shared by all requests: /generate
    submits into the ContinuousBatcher and blocks until its request
    retires; the loop steps whenever work is queued."""

    def __init__(self, model, capacity: int, max_batch: int = 8,
                 device=None, eos_id=None, kv_dtype: str = "bf16"):
        import threading

        self.cb = ContinuousBatcher(model, capacity, max_batch=max_batch,
                                    device=device, eos_id=eos_id,
                                    kv_dtype=kv_dtype)
        self.lock = threading.Lock()
        self.events = {}
        self.results = {}
        self._threading = threading
        t = threading.Thread(target=self._loop, daemon=True)
        t.start()

    def submit(self, prompt, max_new, temperature, top_k, generator=None):
        with self.lock:
            rid = self.cb.submit(prompt, max_new, temperature=temperature,
                                 top_k=top_k, generator=generator)
            self.events[rid] = self._threading.Event()
        return rid

    def wait(self, rid, timeout=600.0):
        ev = self.events[rid]
        if not ev.wait(timeout):
            raise TimeoutError("generation timed out")
        with self.lock:
            self.events.pop(rid, None)
            return self.results.pop(rid)

    def submit_and_wait(self, prompt, max_new, temperature, top_k,
                        generator=None, timeout=600.0):
        return self.wait(self.submit(prompt, max_new, temperature, top_k,
                                     generator), timeout)

    def _loop(self):
        import time as _time

        while True:
            with self.lock:
                busy = self.cb.active > 0 or bool(self.cb._pending)
                done = self.cb.step() if busy else {}
                for rid, toks in done.items():
                    self.results[rid] = toks
                    if rid in self.events:
                        self.events[rid].set()
                self.cb.finished.clear()   # served via results; don't
                                           # accumulate forever
            if not busy:
                _time.sleep(0.002)


def load_model(model_name: str, checkpoint: str = None,
               dtype=torch.bfloat16, device=None, weight_dtype: str = "bf16",
               kv_dtype: str = "bf16"):
    assert weight_dtype in ("bf16", "fp8"), weight_dtype
    assert kv_dtype in ("bf16", "fp8"), kv_dtype
    spec = MODEL_SPECS[model_name]
    cls = LlamaModel if isinstance(spec, LlamaModelSpec) else GPTModel
    model = cls(spec, dtype=dtype)
    if checkpoint:
        state = torch.load(checkpoint, map_location="cpu", weights_only=True)
        plan = state.get("plan", {})
        assert plan.get("tp", 1) == 1 and plan.get("pp", 1) == 1, (
            "serve v1 loads tp=pp=1 checkpoints")
        model.load_state_dict(state["model"])
    model.eval()
    if weight_dtype == "fp8":   # after the checkpoint, before the move
        quantize_for_decode(model)
    if device is not None:
        model = model.to(device)
    model.kv_dtype = kv_dtype       # build_app's default for the batcher
    return model, spec


try:  # module level so FastAPI can resolve the (string) annotation
    from pydantic import BaseModel

    class GenRequest(BaseModel):
        tokens: list
        max_new_tokens: int = 32
        temperature: float = 0.0
        top_k: int = 0
        seed: int = 0
except ImportError:  # pragma: no cover - fastapi/pydantic are optional
    GenRequest = None


def build_app(model, spec, device=None, continuous: bool = False,
              max_batch: int = 8, kv_dtype: str = None):
    from fastapi import FastAPI

    if kv_dtype is None:
        kv_dtype = getattr(model, "kv_dtype", "bf16")
    assert kv_dtype in ("bf16", "fp8"), kv_dtype
    if kv_dtype == "fp8" and not continuous:
        raise ValueError("kv_dtype='fp8' needs continuous=True: only the "
                         "continuous batcher's ragged cache is quantised")
    app = FastAPI(title="metis_amd serve")
    worker = (BatcherWorker(model, spec.seq_length, max_batch=max_batch,
                            device=device, kv_dtype=kv_dtype)
              if continuous else None)
    app.state.worker = worker

    @app.get("/health")
    def health():
        return {"status": "ok", "model": spec.name,
                "seq_length": spec.seq_length,
                "weight_dtype": weight_dtype_of(model),
                "kv_dtype": kv_dtype}

    @app.post("/generate")
    def gen(req: GenRequest):
        from fastapi import HTTPException

        g = torch.Generator().manual_seed(req.seed) if req.seed else None
        if not req.tokens or any(len(p) == 0 for p in req.tokens):
            raise HTTPException(400, "empty prompt")
        lens = {len(p) for p in req.tokens}
        if max(lens) >= spec.seq_length:
            raise HTTPException(
                400, f"prompt length {max(lens)} >= context {spec.seq_length}")
        budget = spec.seq_length - max(lens)
        n = max(0, min(req.max_new_tokens, budget))
        if worker is not None:
            # continuous batching: each prompt becomes one request in
            # the shared decode loop (requests from other HTTP calls
            # interleave in the same batch)
            g = None
            if req.seed:
                g = torch.Generator().manual_seed(req.seed)
            # submit every prompt first so they decode as ONE batch,
            # then collect
            rids = [worker.submit(p, n, req.temperature, req.top_k,
                                  generator=g) for p in req.tokens]
            return {"tokens": [worker.wait(r) for r in rids]}
        if len(lens) > 1:   # ragged batch: padded-cache batched decode
            out = generate_ragged(model, req.tokens, n,
                                  temperature=req.temperature,
                                  top_k=req.top_k, generator=g,
                                  device=device)
            return {"tokens": out}
        toks = torch.tensor(req.tokens, dtype=torch.long)
        if device is not None:
            toks = toks.to(device)
        out = generate(model, toks, n, temperature=req.temperature,
                       top_k=req.top_k, generator=g)
        return {"tokens": out.cpu().tolist()}

    return app


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="gpt2-small", choices=sorted(MODEL_SPECS))
    p.add_argument("--checkpoint", default=None)
    p.add_argument("--host", default="127.0.0.1")
    p.add_argument("--port", type=int, default=8000)
    p.add_argument("--continuous", action="store_true",
                   help="serve through one shared continuous-batching "
                        "decode loop")
    p.add_argument("--max-batch", type=int, default=8)
    p.add_argument("--weight-dtype", choices=("bf16", "fp8"), default="bf16",
                   help="fp8: weight-only e4m3fn linears, quantised at load")
    p.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16",
                   help="fp8: e4m3fn KV cache with per-position scales "
                        "(needs --continuous)")
    args = p.parse_args(argv)
    if args.kv_dtype == "fp8" and not args.continuous:
        p.error("--kv-dtype fp8 requires --continuous")
    return args


def main() -> None:
    args = parse_args()

    device = "cuda:0" if torch.cuda.is_available() else None
    dtype = torch.bfloat16 if torch.cuda.is_available() else torch.float32
    model, spec = load_model(args.model, args.checkpoint, dtype, device,
                             weight_dtype=args.weight_dtype,
                             kv_dtype=args.kv_dtype)

    import uvicorn

    uvicorn.run(build_app(model, spec, device, continuous=args.continuous,
                          max_batch=args.max_batch,
                          kv_dtype=args.kv_dtype), host=args.host,
                port=args.port, log_level="warning")


if __name__ == "__main__":
    main()

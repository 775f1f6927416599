"""Linear layer whose backward GEMMs run in layouts the library is fast at.

``linear(x, weight, bias)`` is ``F.linear`` in the forward. Its backward
looks each GEMM up in a committed table (``profiles/mi355x/gemm_algos.json``,
written by ``scripts/gemm_tune.py``) keyed by (op, M, N, K):

* ``aten``  – the calls autograd makes for ``F.linear``: ``dy @ w`` and
  ``dy.t() @ x``. Every shape without an entry takes this route, so it
  computes the bits it always did.
* ``lt``    – the same layout through hipBLASLt with the algorithm index the
  tuner chose (``ext.lt_linear_dgrad`` / ``ext.lt_linear_wgrad``).
* ``lt_tn`` – data gradient: ``dx = dy @ Wt^T`` on a contiguous transposed
  copy ``Wt`` of the weight, the TN product the forward runs.
* ``lt_dyt`` / ``lt_xt`` / ``lt_xt_nn`` / ``lt_dyt_xt`` – weight gradient on
  a transposed activation (docs/KERNELS.md "Linear backward"): ``dy^T``,
  ``x^T``, ``x^T`` with the result transposed back, or both (the TN product;
  ``lt_tn`` names a data-gradient route only). The transposed activation
  changes with every call, so it is written into a reused scratch buffer
  inside the backward and kept nowhere.

No timing happens at run time: which kernel runs depends on the table file
alone, so two processes compute the same bits.

The transposed copy is kept per weight and refreshed in the backward when
its stamp no longer matches. The stamp is (epoch, ``weight._version``,
``weight.data_ptr()``, forward count): the epoch is advanced by everything
in this project that writes weights behind autograd's back
(``FusedAdamW.step`` / ``load_state_dict``, checkpoint loads), the version
counter sees in-place autograd ops, the pointer sees re-bound storage. A
write through ``weight.data`` leaves no trace in any of them, so a forward
through the weight also invalidates the copy: it is rebuilt at most once per
forward, and a repeated backward of one forward reuses it.
"""

from __future__ import annotations

import json
import logging
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from metis_amd import ops as _ops

_log = logging.getLogger(__name__)

TABLE_PATH = os.path.join(
    os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
    "profiles", "mi355x", "gemm_algos.json")

OPS = ("dgrad", "wgrad")
ROUTES = {"dgrad": ("aten", "lt", "lt_tn"),
          "wgrad": ("aten", "lt", "lt_dyt", "lt_xt", "lt_xt_nn", "lt_dyt_xt")}

Key = Tuple[str, int, int, int]


class GemmTable:
    """Parsed algorithm table: (op, M, N, K) -> (route, algo)."""

    def __init__(self, lt_version: int, device: str,
                 entries: Dict[Key, Tuple[str, int]]):
        self.lt_version = lt_version
        self.device = device
        self.entries = entries

    @classmethod
    def empty(cls) -> "GemmTable":
        return cls(-1, "", {})

    @classmethod
    def parse(cls, obj) -> "GemmTable":
        """Strict: any malformed field raises ValueError (the caller then
        applies no entry at all, never half a table)."""
        if not isinstance(obj, dict):
            raise ValueError("table is not an object")
        version, device = obj.get("hipblaslt_version"), obj.get("device")
        if not _is_int(version) or not isinstance(device, str):
            raise ValueError("header needs hipblaslt_version (int) and device")
        raw = obj.get("entries")
        if not isinstance(raw, list):
            raise ValueError("entries is not a list")
        entries: Dict[Key, Tuple[str, int]] = {}
        for e in raw:
            if not isinstance(e, dict):
                raise ValueError("entry is not an object")
            op, route, algo = e.get("op"), e.get("route"), e.get("algo", -1)
            dims = (e.get("M"), e.get("N"), e.get("K"))
            if op not in OPS or route not in ROUTES[op]:
                raise ValueError(f"bad op/route {op!r}/{route!r}")
            if not all(_is_int(d) and d > 0 for d in dims):
                raise ValueError(f"bad shape {dims!r}")
            if not _is_int(algo) or algo < -1:
                raise ValueError(f"bad algo {algo!r}")
            key = (op,) + dims
            if key in entries:
                raise ValueError(f"duplicate entry {key!r}")
            entries[key] = (route, algo)
        return cls(version, device, entries)

    def matches(self, lt_version: int, device: str) -> bool:
        return self.lt_version == lt_version and self.device == device

    def lookup(self, op: str, M: int, N: int, K: int) -> Tuple[str, int]:
        return self.entries.get((op, M, N, K), ("aten", -1))


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def load_table(path: str) -> GemmTable:
    """Read a table file; a missing or malformed file gives the empty table
    (every GEMM on the aten route) and one warning."""
    try:
        with open(path) as f:
            return GemmTable.parse(json.load(f))
    except (OSError, ValueError) as e:   # JSONDecodeError is a ValueError
        _log.warning("gemm table %s not used (%s): linear backward GEMMs "
                     "take the aten route", path, e)
        return GemmTable.empty()


def resolve_table(table: GemmTable, lt_version: int, device: str) -> GemmTable:
    """The table if it was tuned for this library version and device,
    otherwise the empty table and one warning."""
    if not table.entries or table.matches(lt_version, device):
        return table
    _log.warning(
        "gemm table was tuned for hipBLASLt %s on %r, this is %s on %r: "
        "linear backward GEMMs take the aten route",
        table.lt_version, table.device, lt_version, device)
    return GemmTable.empty()


# METIS_GEMM_TABLE names another table file (probing entries one at a time)
_FILE_TABLE = load_table(os.environ.get("METIS_GEMM_TABLE") or TABLE_PATH)
_ACTIVE: Optional[GemmTable] = None         # resolved at the first GPU backward


def device_id() -> str:
    """What the table's ``device`` field is compared with: the ISA name and
    the CU count, e.g. ``gfx950-256cu``. The marketing name is not used: it
    comes from a lookup file that may be absent (every AMD GPU is then
    "AMD Radeon Graphics") and is empty under rocprofv3."""
    p = torch.cuda.get_device_properties(torch.cuda.current_device())
    return f"{p.gcnArchName.split(':')[0]}-{p.multi_processor_count}cu"


def _active_table() -> GemmTable:
    global _ACTIVE
    if _ACTIVE is None:
        ext = _ops.require_extension()
        _ACTIVE = resolve_table(_FILE_TABLE, int(ext.lt_version()),
                                device_id())
    return _ACTIVE


class use_table:
    """Context manager: route by ``table`` instead of the committed file
    (tests, and probing one entry at a time)."""

    def __init__(self, table: GemmTable):
        self.table = table

    def __enter__(self):
        global _ACTIVE
        self._saved = _ACTIVE
        _ACTIVE = self.table
        return self.table

    def __exit__(self, *exc):
        global _ACTIVE
        _ACTIVE = self._saved
        return False


def enabled() -> bool:
    return os.environ.get("METIS_LT_BWD", "1") != "0"


# --- the transposed weight copy ---------------------------------------------
_epoch = 0
transpose_refreshes = 0     # how often a Wt copy was (re)built; tests read it


def bump_epoch() -> None:
    """Call after writing weights without autograd seeing it (the fused
    optimizer step, state loads): every transposed copy becomes stale."""
    global _epoch
    _epoch += 1


def _stamp(weight: torch.Tensor):
    return (_epoch, weight._version, weight.data_ptr(),
            getattr(weight, "_metis_fwd_count", 0))


def transposed_weight(weight: torch.Tensor) -> torch.Tensor:
    """The contiguous [K, N] copy of ``weight`` [N, K], rebuilt if stale."""
    global transpose_refreshes
    ext = _ops.require_extension()
    stamp = _stamp(weight)
    cached = getattr(weight, "_metis_wt", None)
    if cached is not None and cached[0] == stamp:
        return cached[1]
    w = weight.detach()
    if (cached is not None and cached[1].device == w.device
            and cached[1].shape == (w.size(1), w.size(0))):
        wt = cached[1]
    else:
        wt = torch.empty(w.size(1), w.size(0), dtype=w.dtype, device=w.device)
    ext.transpose_bf16_out(w, wt)
    weight._metis_wt = (stamp, wt)
    transpose_refreshes += 1
    return wt


def _lt_ok(*tensors: torch.Tensor) -> bool:
    """The hipBLASLt routes take CUDA bf16 only, and not under stream
    capture (a refresh decided at capture time would be replayed blindly)."""
    if not all(t.is_cuda and t.dtype == torch.bfloat16 for t in tensors):
        return False
    return not torch.cuda.is_current_stream_capturing()


def _lt_operand(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


# --- transposed activations for the weight gradient ---------------------------
# One flat bf16 buffer per (device, stream, slot), grown to the largest
# activation seen. A transposed activation is written and read inside one
# backward call on one stream, so the next call may overwrite it: stream
# order alone makes the reuse safe.
_scratch: Dict[Tuple[int, int, int], torch.Tensor] = {}


def _transposed_scratch(t: torch.Tensor, slot: int) -> torch.Tensor:
    """``t`` [R, C] transposed into the scratch buffer, as a [C, R] view."""
    key = (t.device.index, torch.cuda.current_stream(t.device).cuda_stream,
           slot)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < t.numel():
        del buf
        _scratch.pop(key, None)      # free the smaller one before allocating
        buf = _scratch[key] = torch.empty(t.numel(), dtype=t.dtype,
                                          device=t.device)
    out = buf[:t.numel()].view(t.size(1), t.size(0))
    _ops.require_extension().transpose_bf16_out(t, out)
    return out


def _wgrad(route: str, algo: int, dy2: torch.Tensor,
           x2: torch.Tensor) -> torch.Tensor:
    """dw [N,K] = dy2^T @ x2 by a hipBLASLt route of ROUTES["wgrad"]."""
    ext = _ops.require_extension()
    dy2, x2 = _lt_operand(dy2), _lt_operand(x2)
    if route == "lt":
        return ext.lt_linear_wgrad(dy2, x2, algo)
    if route == "lt_dyt":
        return ext.lt_linear_wgrad_dyt(_transposed_scratch(dy2, 0), x2, algo)
    if route == "lt_xt":
        return ext.lt_linear_wgrad_xt(dy2, _transposed_scratch(x2, 0), algo)
    if route == "lt_xt_nn":
        return ext.transpose_bf16(
            ext.lt_linear_wgrad_xt_nn(dy2, _transposed_scratch(x2, 0), algo))
    if route == "lt_dyt_xt":
        return ext.lt_linear_wgrad_tn(_transposed_scratch(dy2, 0),
                                      _transposed_scratch(x2, 1), algo)
    raise ValueError(f"unknown wgrad route {route!r}")


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        weight._metis_fwd_count = getattr(weight, "_metis_fwd_count", 0) + 1
        ctx.weight_ref = weight     # the object that carries the Wt copy
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, K = w.shape
        dy2 = dy.reshape(-1, N)
        x2 = x.reshape(-1, K)
        M = dy2.size(0)
        lt = _lt_ok(dy2, x2, w)
        table = _active_table() if lt else None
        dx = dw = db = None

        if ctx.needs_input_grad[0]:
            route, algo = table.lookup("dgrad", M, N, K) if lt else ("aten", -1)
            if route == "lt_tn" and N % 8 == 0 and K % 8 == 0:
                wt = transposed_weight(ctx.weight_ref)
                dx2 = _ops.require_extension().lt_linear_dgrad_tn(
                    _lt_operand(dy2), wt)
            elif route == "lt":
                dx2 = _ops.require_extension().lt_linear_dgrad(
                    _lt_operand(dy2), _lt_operand(w), algo)
            else:
                dx2 = dy2 @ w
            dx = dx2.view(x.shape)
        if ctx.needs_input_grad[1]:
            route, algo = table.lookup("wgrad", M, N, K) if lt else ("aten", -1)
            # the transposing routes need every size a multiple of 8
            # (transpose_bf16_out); other shapes make autograd's own call
            if route == "lt" or (route != "aten" and M % 8 == 0
                                 and N % 8 == 0 and K % 8 == 0):
                dw = _wgrad(route, algo, dy2, x2)
            else:
                dw = dy2.t() @ x2
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy2.sum(0, keepdim=True).view(N)
        return dx, dw, db


def linear(x: torch.Tensor, weight: torch.Tensor,
           bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear`` with table-routed backward GEMMs (module docstring).
    ``METIS_LT_BWD=0`` restores plain ``F.linear``."""
    if not enabled():
        return F.linear(x, weight, bias)
    return _Linear.apply(x, weight, bias)

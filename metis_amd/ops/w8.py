"""fp8 (OCP e4m3fn) weight-only linear with PERSISTENT weight quantisation.

Weights are quantised once, per output channel; activations stay bf16.
A decode step runs its linears at M = batch <= 16 rows, where a linear
layer is a weight stream: fp8 weights halve the bytes (and the resident
weight memory). The hot path is the hand-written kernel w8_linear.hip;
ops/fp8.py (both operands quantised per call, hipBLASLt fp8) is a
different, training-side experiment and is not used here.

    y[m, n] = scale[n] * sum_k x[m, k] * decode(w8[n, k]) + bias[n]

The fp8 decode is exact and the scale is applied once after the K sum, so
every route below computes the same formula:

* GPU, bf16, 1 <= M <= 16: ext.w8_linear (fp32 accumulation, bf16 out);
* GPU, bf16, M > 16 (prefill chunks) or METIS_W8_KERNEL=0: the library
  GEMM on the exactly decoded weights, scale and bias in fp32;
* CPU or any other dtype: fp32 eager.
"""

from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from metis_amd import ops as _ops

_E4M3_MAX = 448.0
# Floor of the per-row amax: keeps the scale of an all-zero row finite and
# positive. Rows whose amax is below it quantise to zeros.
_AMAX_TINY = 2.0 ** -100
KERNEL_MAX_M = 16


def quantize_weight_e4m3(w: torch.Tensor):
    """Per-output-channel symmetric quantisation of w [N, K].

    Returns (w8 float8_e4m3fn [N, K], scale fp32 [N]) with
    scale[n] = max(amax_n, tiny) / 448 and w ~= w8 * scale[:, None]. The
    quotient is clamped to +-448 BEFORE the cast (e4m3fn has no inf: an
    out-of-range cast gives NaN). Round trip: |w - w8*scale| <= amax_n/28
    (half an ulp of the top binade, 16, times the scale)."""
    assert w.dim() == 2, "weight must be [N, K]"
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1).clamp(min=_AMAX_TINY)
    scale = amax / _E4M3_MAX
    q = (wf / scale[:, None]).clamp(-_E4M3_MAX, _E4M3_MAX)
    return q.to(torch.float8_e4m3fn).contiguous(), scale.contiguous()


def _eager(x2, w8, scale, bias):
    """The formula in fp32 eager (CPU, non-bf16 dtypes)."""
    y = F.linear(x2.float(), w8.float()) * scale
    if bias is not None:
        y = y + bias.float()
    return y.to(x2.dtype)


def _library_gemm(x2, w8, scale, bias):
    """The formula through the bf16 library GEMM on exactly decoded
    weights; scale and bias in fp32, one cast at the end."""
    y = F.linear(x2, w8.to(x2.dtype)).float() * scale
    if bias is not None:
        y = y + bias.float()
    return y.to(x2.dtype)


def w8_linear(x: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor,
              bias: torch.Tensor = None) -> torch.Tensor:
    """x [..., K] -> [..., N] against w8 [N, K] (float8_e4m3fn), scale
    fp32 [N], bias [N] or None. Leading dims are flattened and restored."""
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.size(-1))
    if x.is_cuda and x.dtype == torch.bfloat16:
        m = x2.size(0)
        if 1 <= m <= KERNEL_MAX_M and os.environ.get("METIS_W8_KERNEL") != "0":
            ext = _ops.require_extension()
            x2 = x2.contiguous()
            if x2.data_ptr() % 16:
                x2 = x2.clone()
            b = None if bias is None else bias.to(torch.bfloat16)
            y = ext.w8_linear(x2, w8, scale, b)
        else:
            y = _library_gemm(x2, w8, scale, bias)
    else:
        y = _eager(x2, w8, scale, bias)
    return y.reshape(*lead, w8.size(0))


class W8Linear(nn.Module):
    """Drop-in for ColumnParallelLinear / RowParallelLinear at tp = 1 with
    the weight held as e4m3fn + per-channel scale (buffers, no grads)."""

    def __init__(self, w8: torch.Tensor, scale: torch.Tensor,
                 bias: torch.Tensor = None):
        super().__init__()
        self.out_features, self.in_features = w8.shape
        self.register_buffer("w8", w8)
        self.register_buffer("scale", scale)
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, linear: nn.Module) -> "W8Linear":
        """Quantise a module that holds .weight [N, K] and .bias [N]."""
        w8, scale = quantize_weight_e4m3(linear.weight)
        bias = getattr(linear, "bias", None)
        return cls(w8, scale, None if bias is None else bias.detach().clone())

    def forward(self, x: torch.Tensor, tp_group=None) -> torch.Tensor:
        return w8_linear(x, self.w8, self.scale, self.bias)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, weight=e4m3fn")

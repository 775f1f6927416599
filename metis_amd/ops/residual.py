"""Bias, residual and LayerNorm passes of a transformer block, fused.

Between the GEMMs of a pre-LN block the eager composition runs a broadcast
bias add, a residual add and a LayerNorm forward, and in the backward one
gradient add where the residual branch meets LayerNorm's dx plus one column
reduce per bias. Each is a pass over a [tokens, H] tensor that a
neighbouring kernel can do on data it already holds:

  norm_passthrough          x -> (x, LN(x)); the backward adds the gradient
                            of the passed-through x inside the norm backward
  bias_residual_layer_norm  (y, bias, residual) -> (x, LN(x)) with
                            x = residual + (y + bias); the backward also
                            returns the bias gradient as the column sum of
                            the gradient it writes
  bias_residual_add         x = residual + (y + bias) alone
  gelu_bgrad                tanh GeLU whose backward also sums dh by columns,
                            the gradient of the bias added in front of it

The forward values and every gradient except the two bias gradients are
bitwise those of the eager composition (both bf16 roundings of the two adds
are kept); the bias gradients are fp32 column sums in another order.
dh of gelu_bgrad is the same formula in fp32 with one rounding, not
bitwise aten's.

METIS_FUSED_RESIDUAL=0 (read per call) selects the eager composition; so do
CPU and non-bf16 inputs.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from metis_amd import ops as _ops

MAX_HIDDEN = 8192


def fused_enabled(x: torch.Tensor) -> bool:
    """True where the fused kernels take `x` as the block's hidden state."""
    return (x.is_cuda and x.dtype == torch.bfloat16
            and x.size(-1) % 8 == 0 and x.size(-1) <= MAX_HIDDEN
            and os.environ.get("METIS_FUSED_RESIDUAL", "1") != "0")


class _NormPassthroughFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ext = _ops.require_extension()
        x = x.contiguous()
        z, mean, rstd = ext.layernorm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.set_materialize_grads(False)
        return x, z

    @staticmethod
    def backward(ctx, dx_pass, dz):
        if dz is None:
            return dx_pass, None, None, None
        ext = _ops.require_extension()
        x, weight, mean, rstd = ctx.saved_tensors
        if dx_pass is None:
            g, dgamma, dbeta = ext.layernorm_bwd(dz, x, weight, mean, rstd)
        else:
            g, dgamma, dbeta, _ = ext.layernorm_bwd_add(
                dz, dx_pass.contiguous(), x, weight, mean, rstd, False)
        return g, dgamma.to(weight.dtype), dbeta.to(weight.dtype), None


class _BiasResidualNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, residual, weight, ln_bias, eps):
        ext = _ops.require_extension()
        x, z, mean, rstd = ext.bias_residual_layernorm_fwd(
            y.contiguous(), bias, residual.contiguous(), weight, ln_bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.bias_dtype = bias.dtype
        ctx.set_materialize_grads(False)
        return x, z

    @staticmethod
    def backward(ctx, dx, dz):
        x, weight, mean, rstd = ctx.saved_tensors
        want = ctx.needs_input_grad[1]
        if dz is None:
            if dx is None:
                return (None,) * 6
            db = dx.sum(tuple(range(dx.dim() - 1))) if want else None
            return dx, db, dx, None, None, None
        ext = _ops.require_extension()
        if dx is None:
            g, dgamma, dbeta = ext.layernorm_bwd(dz, x, weight, mean, rstd)
            db = g.sum(tuple(range(g.dim() - 1))) if want else None
        else:
            g, dgamma, dbeta, colsum = ext.layernorm_bwd_add(
                dz, dx.contiguous(), x, weight, mean, rstd, want)
            db = colsum.to(ctx.bias_dtype) if want else None
        # y and residual receive the same tensor: no copy
        return (g, db, g, dgamma.to(weight.dtype), dbeta.to(weight.dtype),
                None)


class _BiasResidualAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, bias, residual):
        ext = _ops.require_extension()
        return ext.bias_residual_add(y.contiguous(), bias,
                                     residual.contiguous())

    @staticmethod
    def backward(ctx, dx):
        # the bias gradient stays a column reduce: dx is produced by the
        # next block's backward
        db = (dx.sum(tuple(range(dx.dim() - 1)))
              if ctx.needs_input_grad[1] else None)
        return dx, db, dx


class _GeluBgradFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, bias):
        ctx.save_for_backward(h)
        ctx.bias_dtype = bias.dtype
        return F.gelu(h, approximate="tanh")

    @staticmethod
    def backward(ctx, da):
        ext = _ops.require_extension()
        (h,) = ctx.saved_tensors
        dh, dbias = ext.gelu_tanh_bwd_bgrad(h.contiguous(), da.contiguous())
        db = dbias.to(ctx.bias_dtype) if ctx.needs_input_grad[1] else None
        return dh, db


def norm_passthrough(x, weight, bias, eps: float = 1e-5):
    """(x, LayerNorm(x)). Take the residual branch from the returned x: its
    gradient is then added inside the norm backward."""
    if fused_enabled(x):
        return _NormPassthroughFn.apply(x, weight, bias, eps)
    return x, _ops.layer_norm(x, weight, bias, eps)


def bias_residual_layer_norm(y, bias, residual, weight, ln_bias,
                             eps: float = 1e-5):
    """(x, LayerNorm(x)) with x = residual + (y + bias)."""
    if fused_enabled(y) and bias.dtype == torch.bfloat16:
        return _BiasResidualNormFn.apply(y, bias, residual, weight, ln_bias,
                                         eps)
    x = residual + (y + bias)
    return x, _ops.layer_norm(x, weight, ln_bias, eps)


def bias_residual_add(y, bias, residual):
    """residual + (y + bias), both roundings kept."""
    if fused_enabled(y) and bias.dtype == torch.bfloat16:
        return _BiasResidualAddFn.apply(y, bias, residual)
    return residual + (y + bias)


def gelu_bgrad(h, bias):
    """gelu(h, tanh) for h = linear(x, W, bias.detach()): `bias` is an input
    only to receive its gradient, the column sum of dh."""
    return _GeluBgradFn.apply(h, bias)

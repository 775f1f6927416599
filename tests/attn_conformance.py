"""Reference, yardstick and comparators for the causal flash-attention tests.

Plain test support (not a conftest): imported by test_attn_conformance_cpu.py
and test_attn_conformance_gpu.py. Everything here runs on whatever device the
inputs live on.

  reference_fp64   the operation itself, written out in float64
  baseline_bf16    the same formula in bf16 tensors: what rounding at the
                   kernels' I/O precision costs on these very inputs
  blockwise_ratio / assert_blockwise_close
                   per 16-row block (the kernels' own row-block granularity):
                   max|got - ref| <= factor * max|base - ref| + 2**-8 * max|ref|
  lse_error / assert_lse_close
                   fp32 LSE against the fp64 one, absolute
"""

from __future__ import annotations

import torch

ROW_BLOCK = 16

# Absolute bound on |lse_kernel - lse_fp64| (natural log units).
#
# LSE is fp32 end to end, so there is no bf16 yardstick; the yardstick is a
# plain fp32 eager logsumexp of the same bf16 inputs. Measured on an MI355X
# over the whole grid of test_attn_conformance_gpu.py (main grid, late rows,
# peaked softmax, non-default scale; |lse| <= 22.8, reached by the peaked
# cases): eager fp32 is at most 4.7e-6 off the fp64 value, the kernel at
# most 4.1e-6 (0.80e-6 and 0.89e-6 without the peaked cases; the per-D
# figures are in docs/KERNELS.md). The bound is
#
#     4 * 4.7e-6 = 1.9e-5   a small multiple of the fp32-eager figure
#   + 2.2e-6                __expf(x): the ROCm device library's native exp
#                           is v_exp_f32(x * log2(e)), documented to about
#                           1 ulp, and rounding the product x * log2(e) adds
#                           |x| * 2**-24 relative to the result. Terms that
#                           carry weight have |x| = m - s <= 32, so l, and
#                           with it log l, is off by <= 32 * 2**-24 + 2**-23
#   + 1.9e-6                __logf(l) = v_log_f32(l) * ln 2: budget 2 ulp of
#                           a result up to log(1024) < 8, 2 * 2**-23 * 8
#   + 1.9e-6                rounding the sum m + log l, half an ulp of 32
#   = 2.5e-5
#
# Losing one key out of 384 moves a row's LSE by about 1/384 = 2.6e-3, a
# hundred times this bound; test_attn_conformance_cpu.py checks that such a
# row is rejected.
LSE_ATOL = 2.5e-5


def causal_mask(s: int, device=None) -> torch.Tensor:
    """[S, S] bool, True where key j is hidden from query i (j > i)."""
    return torch.ones(s, s, dtype=torch.bool, device=device).triu(1)


def _attention(q, k, v, scale, mask=None):
    """Explicit masked-softmax attention in the dtype of q/k/v.
    q [B,H,S,D], k/v [B,Hkv,S,D]; GQA by repeat_interleave (q-head h reads
    kv-head h // G). Returns o [B,H,S,D] and lse [B,H,S]."""
    g = q.size(1) // k.size(1)
    if g != 1:
        k = k.repeat_interleave(g, dim=1)
        v = v.repeat_interleave(g, dim=1)
    if mask is None:
        mask = causal_mask(q.size(2), q.device)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    s = s.masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, v), lse


def _run(q, k, v, scale, d_o, dtype, mask):
    need_grad = d_o is not None
    q_, k_, v_ = (t.detach().to(dtype).requires_grad_(need_grad)
                  for t in (q, k, v))
    with torch.set_grad_enabled(need_grad):
        o, lse = _attention(q_, k_, v_, scale, mask)
    if not need_grad:
        return o, lse, None, None, None
    dq, dk, dv = torch.autograd.grad(o, (q_, k_, v_), d_o.detach().to(dtype))
    return o.detach(), lse.detach(), dq, dk, dv


def reference_fp64(q, k, v, scale, d_o=None, mask=None):
    """(o, lse, dq, dk, dv) in float64; the grads are None without d_o."""
    return _run(q, k, v, scale, d_o, torch.float64, mask)


def baseline_bf16(q, k, v, scale, d_o=None):
    """(o, dq, dk, dv) of the same formula run entirely in bf16 tensors
    (bf16 matmuls, bf16 softmax, bf16 autograd)."""
    o, _, dq, dk, dv = _run(q, k, v, scale, d_o, torch.bfloat16, None)
    return o, dq, dk, dv


def eager_lse_fp32(q, k, v, scale):
    """Plain fp32 eager logsumexp of the scores: the LSE yardstick."""
    return _run(q, k, v, scale, None, torch.float32, None)[1]


def _block_max(x: torch.Tensor) -> torch.Tensor:
    b, h, s, d = x.shape
    assert s % ROW_BLOCK == 0, s
    return x.abs().reshape(b, h, s // ROW_BLOCK, ROW_BLOCK * d).amax(-1)


def blockwise_ratio(got, base, ref, factor=2.0):
    """Worst block of max|got-ref| / (factor*max|base-ref| + 2**-8*max|ref|).

    got/base/ref are [B, H, S, D]; the maxima run over one 16-row block of
    one (batch, head). Returns (ratio, (b, h, row_block), err_got, err_base);
    <= 1 passes. A NaN/inf anywhere in got gives ratio inf."""
    ref = ref.double()
    err_got = _block_max(got.double() - ref)
    err_base = _block_max(base.double() - ref)
    bound = factor * err_base + 2.0 ** -8 * _block_max(ref)
    ratio = err_got / bound
    ratio = torch.where(torch.isfinite(ratio), ratio,
                        torch.full_like(ratio, float("inf")))
    flat = int(ratio.argmax())
    nh, nrb = ratio.size(1), ratio.size(2)
    where = (flat // (nh * nrb), flat // nrb % nh, flat % nrb)
    return (float(ratio[where]), where, float(err_got[where]),
            float(err_base[where]))


def assert_blockwise_close(got, base, ref, factor=2.0, what=""):
    """Assert the blockwise criterion; returns the worst ratio."""
    ratio, where, e_got, e_base = blockwise_ratio(got, base, ref, factor)
    assert ratio <= 1.0, (
        f"{what}: worst block (b, h, row-block)={where}: "
        f"|got-ref|={e_got:.3e}, bf16-baseline |base-ref|={e_base:.3e}, "
        f"ratio to bound (factor {factor:g}) = {ratio:.3f}")
    return ratio


def lse_error(lse, lse64) -> float:
    """max |lse - lse64|; inf if lse holds a non-finite value."""
    err = (lse.double() - lse64.double()).abs().max()
    return float(err) if bool(torch.isfinite(err)) else float("inf")


def assert_lse_close(lse, lse64, atol=LSE_ATOL, what="lse"):
    err = lse_error(lse, lse64)
    assert err <= atol, f"{what}: max |lse - lse_fp64| = {err:.3e} > {atol:g}"
    return err

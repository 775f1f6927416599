"""GPU conformance of the flash-attention forward and backward kernels.

Every numerics case runs flash_attention forward + backward once on bf16
randn inputs, then compares o, dq, dk, dv per 16-row block against a float64
reference with the bf16-eager error on the same inputs as yardstick
(tests/attn_conformance.py), and attn_fwd's LSE against the float64 one
within LSE_ATOL. Shapes are the smallest that reach each code path:

  S=128  one q tile; one 128-wide KV tile (D <= 80 forward) or two 64-wide
  S=256  two q tiles, the (w, 7-w) pairing across a tile boundary
  S=384  odd tile count; dKV blocks of 128 (D=64) vs 64 rows disagree with
         the 128-row q tiles
  D      64 (8-wave dKV block), 80 and 96 (zero-padded third 32-chunk: 80
         pads half of it, 96 fills it), 128
  heads  MHA, G=2, MQA (G=4) and the non-power-of-two G=3

Each case prints its worst ratio per quantity (run with -s); the figures
recorded in docs/KERNELS.md come from these lines.

LSE bound (LSE_ATOL = 2.5e-5, absolute, against the float64 LSE). LSE is
fp32, so its yardstick is a plain fp32 eager logsumexp on the same inputs,
printed next to the kernel's error by every case. Measured over this file's
grid: fp32 eager <= 4.7e-6, kernel <= 4.1e-6 (both in the peaked cases,
|lse| <= 23; 0.80e-6 and 0.89e-6 otherwise). The bound is 4 x 4.7e-6 for
the fp32 arithmetic itself plus 6e-6 for what the kernel does differently:
__expf as v_exp_f32(x * log2 e), about 1 ulp plus |x| * 2**-24 from
rounding the product, with |x| <= 32 for every term that carries weight
(2.2e-6 on log l); __logf at 2 ulp of a result below 8 (1.9e-6); and the
fp32 sum m + log l, half an ulp of 32 (1.9e-6). The full derivation stands
beside LSE_ATOL in attn_conformance.py. One key lost out of 384 moves LSE
by about 2.6e-3 (test_attn_conformance_cpu.py checks it is rejected).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from attn_conformance import (LSE_ATOL, assert_blockwise_close,
                                  assert_lse_close, baseline_bf16,
                                  eager_lse_fp32, lse_error, reference_fp64)
    from metis_amd.ops import require_extension
    from metis_amd.ops.attention import flash_attention
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

DIMS = (64, 80, 96, 128)
HEADS = ((4, 4), (4, 2), (4, 1), (6, 2))


def _inputs(b, h, hkv, s, d, q_mul=1.0, layout="bhsd"):
    """bf16 randn q, k, v, d_o; one fixed seed per (shape, q_mul)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed((((d * 4096 + s) * 16 + h) * 16 + hkv) * 16 + b
                    + int(q_mul * 1000) * 2 ** 32)

    def rn(heads, mul=1.0):
        shape = (b, heads, s, d) if layout == "bhsd" else (b, s, heads, d)
        x = torch.randn(shape, device="cuda", generator=gen) * mul
        return x.to(torch.bfloat16)

    return rn(h, q_mul), rn(hkv), rn(hkv), rn(h)


def _fwd_bwd(q, k, v, d_o, scale=None):
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = flash_attention(q, k, v, causal=True, scale=scale)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o)
    return o.detach(), dq, dk, dv


def _check(kind, b, h, hkv, s, d, q_mul=1.0, scale_mul=1.0, lse=True):
    q, k, v, d_o = _inputs(b, h, hkv, s, d, q_mul)
    scale = scale_mul / math.sqrt(d)
    got = dict(zip(("o", "dq", "dk", "dv"),
                   _fwd_bwd(q, k, v, d_o, None if scale_mul == 1.0 else scale)))
    ref = dict(zip(("o", "lse", "dq", "dk", "dv"),
                   reference_fp64(q, k, v, scale, d_o)))
    base = dict(zip(("o", "dq", "dk", "dv"), baseline_bf16(q, k, v, scale, d_o)))

    line = f"CONF kind={kind} D={d} H={h} Hkv={hkv} S={s}"
    failures = []
    for n in ("o", "dq", "dk", "dv"):
        assert got[n].shape == ref[n].shape and got[n].dtype == torch.bfloat16
        try:
            ratio = assert_blockwise_close(got[n], base[n], ref[n], what=n)
        except AssertionError as e:
            failures.append(str(e))
            ratio = float("nan")
        line += f" {n}={ratio:.3f}"
    if lse:
        o2, lse_k = require_extension().attn_fwd(q, k, v, scale)
        assert torch.equal(o2, got["o"])
        assert lse_k.dtype == torch.float32 and lse_k.shape == ref["lse"].shape
        e_k = lse_error(lse_k, ref["lse"])
        e_e = lse_error(eager_lse_fp32(q, k, v, scale), ref["lse"])
        line += (f" lse_err={e_k:.2e} lse_eager_fp32_err={e_e:.2e}"
                 f" lse_absmax={float(ref['lse'].abs().max()):.1f}")
    print(line)
    assert not failures, "\n".join(failures)
    if lse:
        assert_lse_close(lse_k, ref["lse"], LSE_ATOL)


@pytest.mark.parametrize("s", (128, 256, 384))
@pytest.mark.parametrize("h,hkv", HEADS)
@pytest.mark.parametrize("d", DIMS)
def test_main_grid(d, h, hkv, s):
    _check("main", 2, h, hkv, s, d)


@pytest.mark.parametrize("d", DIMS)
def test_late_rows(d):
    """S=1024: |o| of the last row blocks is ~0.2, where a global max-abs
    bound is loosest and the per-block one is not."""
    _check("late", 1, 2, 1, 1024, d)


@pytest.mark.parametrize("h,hkv", HEADS)
@pytest.mark.parametrize("d", DIMS)
def test_peaked_softmax(d, h, hkv):
    """q x 4: low-entropy softmax, large running-max jumps, small l."""
    _check("peaked", 2, h, hkv, 384, d, q_mul=4.0)


@pytest.mark.parametrize("d", DIMS)
def test_non_default_scale(d):
    _check("scale", 2, 4, 2, 256, d, scale_mul=0.7)


@pytest.mark.parametrize("d", (32, 112))
def test_uninstantiated_head_dim_falls_back(d):
    """Head dims the kernels are not instantiated for go through SDPA,
    forward and backward, and meet the same comparator."""
    _check("fallback", 2, 4, 2, 128, d, lse=False)


def _assert_bitwise(a, b, what):
    for n, x, y in zip(("o", "dq", "dk", "dv", "lse"), a, b):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: {n} differs"


@pytest.mark.parametrize("d", (64, 96))
def test_non_contiguous_inputs_bitwise(d):
    """[B, S, H, D] storage passed as transposed views, d_o too."""
    b, h, hkv, s = 2, 4, 2, 256
    q, k, v, d_o = _inputs(b, h, hkv, s, d, layout="bshd")
    views = [t.transpose(1, 2) for t in (q, k, v, d_o)]
    assert not any(t.is_contiguous() for t in views)
    got = _fwd_bwd(*views)
    want = _fwd_bwd(*(t.contiguous() for t in views))
    _assert_bitwise(got, want, f"D={d} transposed views")
    ext = require_extension()
    scale = 1.0 / math.sqrt(d)
    _assert_bitwise(ext.attn_fwd(*views[:3], scale),
                    ext.attn_fwd(*(t.contiguous() for t in views[:3]), scale),
                    f"D={d} attn_fwd on views")


@pytest.mark.parametrize("h,hkv,s,d", [(4, 2, 384, 64), (4, 4, 256, 128)])
def test_forward_backward_deterministic(h, hkv, s, d):
    q, k, v, d_o = _inputs(2, h, hkv, s, d)
    ext = require_extension()
    scale = 1.0 / math.sqrt(d)
    runs = [_fwd_bwd(q, k, v, d_o) + (ext.attn_fwd(q, k, v, scale)[1],)
            for _ in range(2)]
    _assert_bitwise(runs[0], runs[1], f"D={d} repeated run")


@pytest.mark.parametrize("d", (64, 96))
def test_batch_element_alone_matches_batched(d):
    """Batch element 1 run alone reproduces row [1] of the batched result:
    catches a cross-batch / cross-head base-offset slip that random data
    could mask."""
    q, k, v, d_o = _inputs(2, 4, 2, 256, d)
    full = _fwd_bwd(q, k, v, d_o)
    alone = _fwd_bwd(*(t[1:2].contiguous() for t in (q, k, v, d_o)))
    _assert_bitwise(alone, [t[1:2] for t in full], f"D={d} batch element 1")


def test_head_dim_32_trains_a_step():
    q, k, v, _ = _inputs(2, 4, 4, 128, 32)
    # fp32 master weight: the step must be visible, not rounded away
    w = torch.nn.Parameter(torch.ones(32, device="cuda"))
    opt = torch.optim.SGD([w], lr=1.0)
    loss = flash_attention(q * w.to(torch.bfloat16), k, v).float().square().mean()
    loss.backward()
    assert torch.isfinite(w.grad).all() and bool(w.grad.abs().max() > 0)
    opt.step()
    assert torch.isfinite(loss) and torch.isfinite(w).all()
    assert not torch.equal(w.detach(), torch.ones_like(w))


# Argument checking. Every bad argument is LARGER than or the same size as
# what the kernels would read, so even an unguarded launch stays in bounds.

def _bwd_args(d=64):
    b, h, hkv, s = 2, 4, 2, 128
    q, k, v, d_o = _inputs(b, h, hkv, s, d)
    ext = require_extension()
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale)
    delta = ext.attn_bwd_delta(o, d_o)
    return ext, [q, k, v, d_o, lse, delta, scale]


def _grow(t, dim, by):
    shape = list(t.shape)
    shape[dim] += by
    return torch.zeros(shape, device=t.device, dtype=t.dtype)


BAD_QKV = {
    "k_fp16": lambda a: a.__setitem__(1, a[1].to(torch.float16)),
    "v_fp32": lambda a: a.__setitem__(2, a[2].float()),
    "k_batch_plus_1": lambda a: a.__setitem__(1, _grow(a[1], 0, 1)),
    "kv_batch_plus_1": lambda a: (a.__setitem__(1, _grow(a[1], 0, 1)),
                                  a.__setitem__(2, _grow(a[2], 0, 1))),
    "v_head_dim_plus_16": lambda a: a.__setitem__(2, _grow(a[2], 3, 16)),
    "kv_head_dim_plus_16": lambda a: (a.__setitem__(1, _grow(a[1], 3, 16)),
                                      a.__setitem__(2, _grow(a[2], 3, 16))),
    "kv_longer": lambda a: (a.__setitem__(1, _grow(a[1], 2, 128)),
                            a.__setitem__(2, _grow(a[2], 2, 128))),
}
BAD_BWD = {
    "d_o_fp32": lambda a: a.__setitem__(3, a[3].float()),
    "d_o_head_dim_plus_16": lambda a: a.__setitem__(3, _grow(a[3], 3, 16)),
    "d_o_batch_plus_1": lambda a: a.__setitem__(3, _grow(a[3], 0, 1)),
    "lse_fp64": lambda a: a.__setitem__(4, a[4].double()),
    "delta_fp64": lambda a: a.__setitem__(5, a[5].double()),
    "lse_longer": lambda a: a.__setitem__(4, _grow(a[4], 2, 128)),
    "delta_more_heads": lambda a: a.__setitem__(5, _grow(a[5], 1, 1)),
    "lse_4d": lambda a: a.__setitem__(4, a[4].unsqueeze(-1)),
}


@pytest.mark.parametrize("bad", sorted(BAD_QKV))
def test_attn_fwd_rejects(bad):
    ext, args = _bwd_args()
    BAD_QKV[bad](args)
    with pytest.raises(RuntimeError):
        ext.attn_fwd(args[0], args[1], args[2], args[6])
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", sorted(BAD_QKV) + sorted(BAD_BWD))
def test_attn_bwd_rejects(bad):
    ext, args = _bwd_args()
    {**BAD_QKV, **BAD_BWD}[bad](args)
    with pytest.raises(RuntimeError):
        ext.attn_bwd(*args)
    torch.cuda.synchronize()


def test_attn_bwd_accepts_valid_arguments():
    """The checks must not reject what the wrapper passes."""
    ext, args = _bwd_args()
    dq, dk_h, dv_h = ext.attn_bwd(*args)
    assert dq.shape == args[0].shape and dk_h.shape == args[0].shape
    assert torch.isfinite(dq.float()).all()

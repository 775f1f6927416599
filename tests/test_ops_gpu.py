"""GPU numerics tests: each HIP kernel vs a plain PyTorch fp32 reference."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from metis_amd.ops import FusedAdamW, require_extension
else:  # collected but skipped on CPU
    pytest.skip("requires MI355X GPU", allow_module_level=True)


@pytest.fixture(scope="module")
def ext():
    return require_extension()


@pytest.mark.parametrize("rows,hidden", [(64, 2560), (1024, 4096), (33, 512)])
def test_layernorm_fwd_matches_fp32(ext, rows, hidden):
    torch.manual_seed(0)
    x = torch.randn(rows, hidden, device="cuda", dtype=torch.bfloat16)
    gamma = torch.randn(hidden, device="cuda", dtype=torch.float32)
    beta = torch.randn(hidden, device="cuda", dtype=torch.float32)

    y, mean, rstd = ext.layernorm_fwd(x, gamma, beta, 1e-5)

    ref = torch.nn.functional.layer_norm(
        x.float(), (hidden,), gamma, beta, 1e-5
    )
    assert torch.allclose(y.float(), ref, atol=2e-2, rtol=2e-2)
    ref_mean = x.float().mean(-1)
    assert torch.allclose(mean, ref_mean, atol=1e-3)


def test_layernorm_bwd_matches_fp32(ext):
    torch.manual_seed(1)
    rows, hidden = 256, 2048
    x = torch.randn(rows, hidden, device="cuda", dtype=torch.bfloat16)
    gamma = torch.randn(hidden, device="cuda", dtype=torch.float32)
    beta = torch.randn(hidden, device="cuda", dtype=torch.float32)
    dy = torch.randn(rows, hidden, device="cuda", dtype=torch.bfloat16)

    y, mean, rstd = ext.layernorm_fwd(x, gamma, beta, 1e-5)
    dx, dgamma, dbeta = ext.layernorm_bwd(dy, x, gamma, mean, rstd)

    xf = x.float().clone().requires_grad_(True)
    gf = gamma.clone().requires_grad_(True)
    bf = beta.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xf, (hidden,), gf, bf, 1e-5)
    ref.backward(dy.float())

    assert torch.allclose(dx.float(), xf.grad, atol=5e-2, rtol=5e-2)
    assert torch.allclose(dgamma, gf.grad, atol=0.5, rtol=2e-2)
    assert torch.allclose(dbeta, bf.grad, atol=0.5, rtol=2e-2)


def test_layernorm_autograd_module():
    from metis_amd.ops import LayerNorm

    ln = LayerNorm(1024).to("cuda")
    x = torch.randn(8, 16, 1024, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = ln(x)
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert ln.weight.grad is not None


def test_fused_adamw_gpu_matches_torch():
    torch.manual_seed(2)
    w = torch.nn.Parameter(torch.randn(4096, device="cuda", dtype=torch.float32))
    w_ref = torch.nn.Parameter(w.detach().clone())

    mine = FusedAdamW([w], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    ref = torch.optim.AdamW([w_ref], lr=1e-2, betas=(0.9, 0.95), eps=1e-8,
                            weight_decay=0.1)
    for step in range(5):
        g = torch.randn(4096, device="cuda")
        w.grad = g.clone()
        w_ref.grad = g.clone()
        mine.step()
        ref.step()
    assert torch.allclose(w.detach(), w_ref.detach(), atol=1e-5), (
        (w.detach() - w_ref.detach()).abs().max()
    )


def test_fused_adamw_bf16_params_flat_buffer():
    torch.manual_seed(3)
    w = torch.nn.Parameter(torch.randn(1024, device="cuda", dtype=torch.bfloat16))
    opt = FusedAdamW([w], lr=1e-2, weight_decay=0.0)
    assert opt._model_flat is not None
    before = w.detach().clone()
    w.grad = torch.randn_like(w)
    opt.step()
    assert not torch.equal(before, w.detach())
    # bf16 copy must track the fp32 master
    assert torch.allclose(
        w.detach().float(), opt.master[:1024], atol=1e-2, rtol=1e-2
    )


def test_model_step_gpu():
    from metis_amd.models.gpt import GPTModel, GPTModelSpec
    from metis_amd.ops import FusedAdamW

    spec = GPTModelSpec("t", hidden_size=256, num_layers=2, num_heads=4,
                        vocab_size=2048, seq_length=128)
    model = GPTModel(spec, dtype=torch.bfloat16).to("cuda")
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    tokens = torch.randint(0, 2048, (2, 128), device="cuda")
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = model(tokens, labels=torch.roll(tokens, -1, 1))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


def test_fused_cross_entropy_matches_fp32():
    from metis_amd.ops.cross_entropy import cross_entropy

    torch.manual_seed(5)
    n, v = 512, 51200
    logits = torch.randn(n, v, device="cuda", dtype=torch.bfloat16,
                         requires_grad=True)
    labels = torch.randint(0, v, (n,), device="cuda")

    loss = cross_entropy(logits, labels)
    loss.backward()

    lf = logits.detach().float().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lf, labels)
    ref.backward()

    assert abs(float(loss) - float(ref)) / float(ref) < 2e-3
    err = (logits.grad.float() - lf.grad).abs().max()
    assert err < 1e-4, err


def test_relayout_kernels_match_eager():
    from metis_amd.ops.relayout import heads_merge, qkv_split_transpose

    torch.manual_seed(6)
    b, s, nq, nkv, d = 2, 128, 8, 2, 64
    qkv = torch.randn(b, s, (nq + 2 * nkv) * d, device="cuda",
                      dtype=torch.bfloat16, requires_grad=True)
    q, k, v = qkv_split_transpose(qkv, nq, nkv, d)

    rq, rk, rv = qkv.split([nq * d, nkv * d, nkv * d], -1)
    assert torch.equal(q, rq.view(b, s, nq, d).transpose(1, 2).contiguous())
    assert torch.equal(k, rk.view(b, s, nkv, d).transpose(1, 2).contiguous())
    assert torch.equal(v, rv.view(b, s, nkv, d).transpose(1, 2).contiguous())

    # backward: gradients land back in the fused layout exactly
    gq, gk, gv = torch.randn_like(q), torch.randn_like(k), torch.randn_like(v)
    torch.autograd.backward([q, k, v], [gq, gk, gv])
    ref = torch.cat([
        gq.transpose(1, 2).reshape(b, s, -1),
        gk.transpose(1, 2).reshape(b, s, -1),
        gv.transpose(1, 2).reshape(b, s, -1),
    ], dim=-1)
    assert torch.equal(qkv.grad, ref)

    x = torch.randn(b, nq, s, d, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    y = heads_merge(x)
    assert torch.equal(y, x.transpose(1, 2).reshape(b, s, -1))
    gy = torch.randn_like(y)
    y.backward(gy)
    assert torch.equal(x.grad, gy.view(b, s, nq, d).transpose(1, 2).contiguous())


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("METIS_EXPERIMENTAL") != "1",
                    reason="fused qkv+rope kernel pending GPU validation")
def test_qkv_rope_split_gpu_matches_composition():
    import metis_amd._hip_ops as ext
    from metis_amd.ops.norms import rope_tables

    torch.manual_seed(0)
    B, S, nq, nkv, d = 2, 128, 8, 2, 64
    qkv = torch.randn(B, S, (nq + 2 * nkv) * d, device="cuda",
                      dtype=torch.bfloat16)
    cos_t, sin_t = rope_tables(S, d, 500000.0, qkv.device)
    q1, k1, v1 = ext.qkv_rope_split(qkv, nq, nkv, d, cos_t, sin_t)
    q0, k0, v0 = ext.qkv_split_transpose(qkv, nq, nkv, d)
    q0 = ext.rope_apply(q0, cos_t, sin_t, False)
    k0 = ext.rope_apply(k0, cos_t, sin_t, False)
    assert torch.allclose(q1.float(), q0.float(), atol=2e-2)
    assert torch.allclose(k1.float(), k0.float(), atol=2e-2)
    assert torch.equal(v1, v0)

    # backward gather inverts: dqkv of (dq,dk,dv) rotated back
    dq, dk, dv = torch.randn_like(q1), torch.randn_like(k1), torch.randn_like(v1)
    dqkv = ext.qkv_rope_split_bwd(dq, dk, dv, d, cos_t, sin_t)
    dq0 = ext.rope_apply(dq, cos_t, sin_t, True)
    dk0 = ext.rope_apply(dk, cos_t, sin_t, True)
    ref = ext.qkv_split_transpose_bwd(dq0, dk0, dv, d)
    assert torch.allclose(dqkv.float(), ref.float(), atol=2e-2)


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("METIS_EXPERIMENTAL") != "1",
                    reason="vocab-parallel CE kernels pending GPU validation")
def test_ce_row_kernels_match_torch():
    import metis_amd._hip_ops as ext

    torch.manual_seed(0)
    x = torch.randn(512, 6400, device="cuda", dtype=torch.bfloat16) * 4
    m = ext.ce_row_max(x)
    assert torch.allclose(m, x.float().max(dim=1).values, atol=1e-6)
    se = ext.ce_row_sumexp(x, m)
    ref = torch.exp(x.float() - m[:, None]).sum(dim=1)
    assert torch.allclose(se, ref, rtol=1e-3)

    # bwd reuse with shifted labels: -1 (unowned) must add no onehot
    labels = torch.randint(0, 6400, (512,), device="cuda")
    labels[::2] = -1
    lse = m + torch.log(se)
    scale = torch.tensor([0.5 / 512], device="cuda")
    d = ext.cross_entropy_bwd(x, labels, lse, scale)
    soft = torch.softmax(x.float(), dim=1)
    oh = torch.zeros_like(soft)
    owned = labels >= 0
    oh[owned] = torch.nn.functional.one_hot(labels[owned], 6400).float()
    ref_d = (soft - oh) * float(scale)
    assert torch.allclose(d.float(), ref_d, atol=5e-3)


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("METIS_EXPERIMENTAL") != "1",
                    reason="fp8 GEMM path pending GPU validation")
def test_fp8_matmul_matches_bf16_within_quant_tolerance():
    from metis_amd.ops.fp8 import fp8_matmul

    torch.manual_seed(0)
    x = torch.randn(512, 1024, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(2048, 1024, device="cuda", dtype=torch.bfloat16) * 0.05
    y = fp8_matmul(x, w)
    ref = x.float() @ w.float().t()
    # per-tensor e4m3 quantization error; K=1024 averaging keeps it small
    err = (y.float() - ref).abs().mean() / ref.abs().mean()
    assert err < 0.05, float(err)


@pytest.mark.gpu
def test_attn_decode_matches_sdpa():
    # default path since round 2 (decode_attention flips it on unless
    # METIS_DECODE_KERNEL=0): always numerics-tested
    import math

    import metis_amd._hip_ops as ext

    torch.manual_seed(0)
    for D, hkv in ((64, 8), (80, 8), (128, 2)):
        B, H, S = 4, 8, 777
        q = torch.randn(B, H, 1, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(B, hkv, S, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(B, hkv, S, D, device="cuda", dtype=torch.bfloat16)
        out = ext.attn_decode(q, k, v, 1.0 / math.sqrt(D))
        rep = H // hkv
        ref = torch.nn.functional.scaled_dot_product_attention(
            q.float(), k.float().repeat_interleave(rep, dim=1),
            v.float().repeat_interleave(rep, dim=1))
        assert torch.allclose(out.float(), ref, atol=2e-2), (D, hkv)


# attn_decode argument checking. Every bad tensor is the same size as or
# LARGER than what the kernel would read, so even an unguarded launch
# stays in bounds.

def _decode_args(hkv=2):
    B, H, S, D = 2, 4, 128, 64
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(*shape, generator=g).to("cuda", torch.bfloat16)
               for shape in ((B, H, 1, D), (B, hkv, S, D), (B, hkv, S, D)))
    return [q, k, v]


def _grown(t, dim, by):
    shape = list(t.shape)
    shape[dim] += by
    return torch.zeros(shape, device=t.device, dtype=t.dtype)


BAD_DECODE = {
    "k_fp16": lambda a: a.__setitem__(1, a[1].to(torch.float16)),
    "v_fp32": lambda a: a.__setitem__(2, a[2].float()),
    "v_head_dim_plus_16": lambda a: a.__setitem__(2, _grown(a[2], 3, 16)),
    "v_batch_plus_1": lambda a: a.__setitem__(2, _grown(a[2], 0, 1)),
    "kv_batch_plus_1": lambda a: (a.__setitem__(1, _grown(a[1], 0, 1)),
                                  a.__setitem__(2, _grown(a[2], 0, 1))),
    # H = 4 is not a multiple of Hkv = 3; v matches k
    "kv_heads_3": lambda a: (a.__setitem__(1, _grown(a[1], 1, 1)),
                             a.__setitem__(2, _grown(a[2], 1, 1))),
}


@pytest.mark.parametrize("bad", sorted(BAD_DECODE))
def test_attn_decode_rejects(ext, bad):
    args = _decode_args()
    BAD_DECODE[bad](args)
    with pytest.raises(RuntimeError):
        ext.attn_decode(*args, 0.125)
    torch.cuda.synchronize()


def test_attn_decode_accepts_valid_arguments(ext):
    """The checks must not reject what decode_attention passes: contiguous
    k/v and a transposed view of a [B, S, Hkv, D] cache give the same
    answer, which matches SDPA as in test_attn_decode_matches_sdpa."""
    q, k, v = _decode_args()
    out = ext.attn_decode(q, k, v, 0.125)
    kt = k.transpose(1, 2).contiguous().transpose(1, 2)
    vt = v.transpose(1, 2).contiguous().transpose(1, 2)
    assert not kt.is_contiguous() and not vt.is_contiguous()
    out_t = ext.attn_decode(q, kt, vt, 0.125)
    rep = q.size(1) // k.size(1)
    ref = torch.nn.functional.scaled_dot_product_attention(
        q.float(), k.float().repeat_interleave(rep, dim=1),
        v.float().repeat_interleave(rep, dim=1))
    assert torch.allclose(out.float(), ref, atol=2e-2)
    assert torch.equal(out, out_t)

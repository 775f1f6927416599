"""GPU conformance of cross_entropy.hip, adamw.hip, the LayerNorm/RMSNorm
forward kernels, rope.hip and swiglu.hip.

Every output is compared with a float64 reference of the documented
formula under the project's blockwise criterion

    max|got - ref| <= 2 * max|base - ref| + ulp * max|ref|     per block

with `base` the same formula in eager torch at the output's precision
(tests/elementwise_conformance.py: blocks, ulp, references, baselines).
test_elementwise_conformance_cpu.py shows on an fp32 emulation of the
kernels that the criterion passes the correct arithmetic and rejects the
mistakes that matter. Shapes are the smallest that reach each code path:
a partial last stride of the 256-thread block, fewer chunks than threads,
the grid-stride loops (more rows than the 2048-block grid, more elements
than one trip of the flat kernels). The worst ratios are printed (-s) and
recorded in docs/KERNELS.md.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import elementwise_conformance as ec
    from metis_amd.ops import FusedAdamW, require_extension
    from metis_amd.ops.cross_entropy import cross_entropy
    from metis_amd.ops.norms import apply_rope, rope_tables, swiglu
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
EPS = 1e-5


@pytest.fixture(scope="module")
def ext():
    return require_extension()


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _report(name, ratio):
    print(f"RATIO {name}: {ratio:.3f}")
    return ratio


# --- cross entropy --------------------------------------------------------
CE_SHAPES = [(n, v) for v in (8, 2040, 2048, 2056, 6152) for n in (1, 5)]
CE_SHAPES += [(2051, 264), (8, 51200)]
CE_FAMILIES = ("randn", "x8", "off1000")


def _ce_check(ext, x, labels, gs, what):
    ref = ec.ce_reference(x, labels, gs)
    base = ec.ce_baseline(x, labels, gs)
    loss, lse = ext.cross_entropy_fwd(x, labels)
    scale = torch.tensor([gs], device="cuda", dtype=torch.float32)
    d = ext.cross_entropy_bwd(x, labels, lse, scale)
    assert loss.dtype == lse.dtype == torch.float32 and d.dtype == BF16
    ok = (labels >= 0) & (labels < x.size(1))    # NaN rows: checked by caller
    r = (_report(f"ce loss {what}",
                 ec.row_ratio(loss[ok], base[0][ok], ref[0][ok])),
         _report(f"ce lse {what}", ec.row_ratio(lse, base[1], ref[1])),
         _report(f"ce dlogits {what}",
                 ec.ce_dlogits_ratio(d, base[2], ref[2], labels)))
    assert max(r) <= 1.0, (what, r)
    return loss, lse, d


@pytest.mark.parametrize("family", CE_FAMILIES)
@pytest.mark.parametrize("n,v", CE_SHAPES)
def test_ce_kernels(ext, n, v, family):
    # one row takes every pinned column in turn; more rows spread them
    seeds = range(len(ec.ce_pinned_labels(v))) if n == 1 else (0,)
    for seed in seeds:
        x, labels = _cuda(*ec.ce_input(n, v, family, seed))
        gs = 1.0 / n if seed == 0 else 0.37
        loss, lse, d = _ce_check(ext, x, labels, gs, f"N{n} V{v} {family}")
        if seed == 0:
            loss2, lse2 = ext.cross_entropy_fwd(x, labels)
            sc = torch.tensor([gs], device="cuda")
            assert torch.equal(loss, loss2) and torch.equal(lse, lse2)
            assert torch.equal(d, ext.cross_entropy_bwd(x, labels, lse, sc))
            if n > 1:       # a row run alone gives the same bits
                r = n - 1
                l1, s1 = ext.cross_entropy_fwd(x[r:r + 1], labels[r:r + 1])
                d1 = ext.cross_entropy_bwd(x[r:r + 1], labels[r:r + 1], s1, sc)
                assert torch.equal(l1, loss[r:r + 1])
                assert torch.equal(s1, lse[r:r + 1])
                assert torch.equal(d1, d[r:r + 1])


@pytest.mark.parametrize("n,v", [(5, 2056), (2051, 264), (8, 51200)])
@pytest.mark.parametrize("grad_out", (1.0, -2.5))
def test_ce_wrapper_mean_and_grad_out(n, v, grad_out):
    x, labels = _cuda(*ec.ce_input(n, v, "randn"))
    xr = x.clone().requires_grad_(True)
    loss = cross_entropy(xr, labels)
    (loss * grad_out).backward()
    ref = ec.ce_reference(x, labels, grad_out / n)
    base = ec.ce_baseline(x, labels, grad_out / n)
    ref_mean = ref[0].mean().reshape(1)
    base_mean = base[0].mean().reshape(1)
    r = (_report("ce mean loss", ec.row_ratio(loss.detach().reshape(1),
                                             base_mean, ref_mean)),
         _report("ce wrapper dlogits",
                 ec.ce_dlogits_ratio(xr.grad, base[2], ref[2], labels)))
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("n,v", [(3, 8), (3, 2040), (4, 2056), (6, 6152),
                                 (2051, 264)])
def test_ce_exact_row_max(ext, n, v):
    cols = (ec.ce_pinned_labels(v) + [v - 3])
    x, labels = _cuda(*ec.ce_exact_case(n, v, cols[-min(n, len(cols)):]))
    loss, lse = ext.cross_entropy_fwd(x, labels)
    assert torch.equal(lse.double(), x.double().max(-1).values)
    assert torch.equal(loss, torch.zeros_like(loss))


def test_ce_out_of_range_labels(ext):
    """Label V on row 0 and -1 on row 1 of a 3-row input: both stay inside
    the buffer even if dereferenced. lse is written as usual, the loss of
    those rows is NaN, the backward adds no one-hot."""
    n, v = 3, 264
    x, _ = _cuda(*ec.ce_input(n, v, "randn"))
    labels = torch.tensor([v, -1, 5], device="cuda")
    loss, lse, d = _ce_check(ext, x, labels, 0.5, "out-of-range labels")
    assert torch.isnan(loss[:2]).all() and torch.isfinite(loss[2])
    assert torch.isfinite(lse).all()
    assert float(d[:2].float().min()) >= 0.0
    assert float(d[2, 5]) < 0.0


@pytest.mark.skipif(os.environ.get("METIS_EXPERIMENTAL") != "1",
                    reason="vocab-parallel CE kernels pending GPU validation")
@pytest.mark.parametrize("n,v", CE_SHAPES)
def test_ce_row_kernels(ext, n, v):
    x, _ = _cuda(*ec.ce_input(n, v, "x8"))
    m = ext.ce_row_max(x)
    assert torch.equal(m.double(), x.double().max(-1).values)
    se = ext.ce_row_sumexp(x, m)
    ref = torch.exp(x.double() - m.double()[:, None]).sum(-1)
    base = torch.exp(x.float() - m[:, None]).sum(-1)
    assert ec.row_ratio(se, base, ref) <= 1.0


# --- LayerNorm / RMSNorm forward ------------------------------------------
NORM_SHAPES = [(r, h) for h in (8, 512, 2040, 2560, 4104, 8192)
               for r in (1, 33)] + [(2051, 8), (2051, 512)]


def _ln_check(ext, x, gamma, beta, eps, what):
    ref = ec.ln_reference(x, gamma, beta, eps)
    base = ec.ln_baseline(x, gamma, beta, eps)
    y, mean, rstd = ext.layernorm_fwd(x, gamma, beta, eps)
    assert y.dtype == BF16 and mean.dtype == rstd.dtype == torch.float32
    r = (_report(f"ln y {what}", ec.block_ratio(y, base[0], ref[0],
                                                ec.COL_BLOCK, ec.ULP_BF16)),
         _report(f"ln mean {what}", ec.row_ratio(mean, base[1], ref[1])),
         _report(f"ln rstd {what}", ec.row_ratio(rstd, base[2], ref[2])))
    assert max(r) <= 1.0, (what, r)


@pytest.mark.parametrize("family", ("randn", "x100", "x1e-3", "const3"))
@pytest.mark.parametrize("rows,h", NORM_SHAPES)
def test_layernorm_fwd(ext, rows, h, family):
    x, gamma, beta = _cuda(ec.norm_input(rows, h, family), *ec.norm_params(h))
    _ln_check(ext, x, gamma, beta, EPS, f"{rows}x{h} {family}")


@pytest.mark.parametrize("family", ("off10", "off100", "off1000"))
@pytest.mark.parametrize("rows,h", [(33, 512), (33, 2560)])
def test_layernorm_fwd_offset_rows(ext, rows, h, family):
    """offset + randn: E[x^2] - mean^2 in fp32 loses (offset/std)^2 ulps of
    the variance; the shifted sums do not."""
    x, gamma, beta = _cuda(ec.norm_input(rows, h, family), *ec.norm_params(h))
    _ln_check(ext, x, gamma, beta, EPS, f"{rows}x{h} {family}")


@pytest.mark.parametrize("family", ("randn", "x100", "x1e-3"))
@pytest.mark.parametrize("rows,h", NORM_SHAPES)
def test_rmsnorm_fwd(ext, rows, h, family):
    x, gamma = _cuda(ec.norm_input(rows, h, family), ec.norm_params(h)[0])
    ref, base = ec.rms_reference(x, gamma, EPS), ec.rms_baseline(x, gamma, EPS)
    y, rstd = ext.rmsnorm_fwd(x, gamma, EPS)
    what = f"{rows}x{h} {family}"
    r = (_report(f"rms y {what}", ec.block_ratio(y, base[0], ref[0],
                                                 ec.COL_BLOCK, ec.ULP_BF16)),
         _report(f"rms rstd {what}", ec.row_ratio(rstd, base[1], ref[1])))
    assert max(r) <= 1.0, (what, r)


@pytest.mark.parametrize("rows,h", [(3, 8), (5, 512), (2, 2040), (3, 8192),
                                    (2051, 512)])
def test_norm_exact_sums(ext, rows, h):
    """+-2 rows, eps = 0: every sum is an exact integer, so mean = 0,
    rstd = 0.5 and y = +-gamma + beta bitwise; integer rows at a power-of-
    two H: the mean equals the float64 mean bitwise."""
    x, gamma, beta = _cuda(*ec.norm_exact_case(rows, h))
    y, mean, rstd = ext.layernorm_fwd(x, gamma, beta, 0.0)
    assert torch.equal(mean, torch.zeros_like(mean))
    assert torch.equal(rstd, torch.full_like(rstd, 0.5))
    assert torch.equal(y.double(), ec.ln_reference(x, gamma, beta, 0.0)[0])
    y, rstd = ext.rmsnorm_fwd(x, gamma, 0.0)
    assert torch.equal(rstd, torch.full_like(rstd, 0.5))
    assert torch.equal(y.double(), ec.rms_reference(x, gamma, 0.0)[0])
    if h & (h - 1) == 0:
        xi = ec.norm_integer_case(rows, h).cuda()
        mean = ext.layernorm_fwd(xi, gamma, beta, EPS)[1]
        assert torch.equal(mean.double(), xi.double().mean(-1))


# --- RoPE -----------------------------------------------------------------
ROPE_SHAPES = [(2, 3, s, d) for d in (8, 64, 80, 128) for s in (1, 77, 128)]
ROPE_SHAPES.append((2, 8, 4100, 64))      # rows*D/8 > 524288: grid stride


def _rope_inputs(shape, pos_offset):
    g = torch.Generator().manual_seed(sum(shape) + pos_offset)
    x = torch.randn(*shape, generator=g).to(BF16).cuda()
    dy = torch.randn(*shape, generator=g).to(BF16).cuda()
    return x, dy


@pytest.mark.parametrize("pos_offset", (0, 37))
@pytest.mark.parametrize("shape", ROPE_SHAPES)
def test_rope_fwd_bwd(ext, shape, pos_offset):
    s, d = shape[2], shape[3]
    x, dy = _rope_inputs(shape, pos_offset)
    cos_t, sin_t = rope_tables(pos_offset + s, d, 500000.0, x.device)
    ref = ec.rope_reference(x, cos_t, sin_t, pos_offset, dy)
    base = ec.rope_baseline(x, cos_t, sin_t, pos_offset, dy)

    xr = x.clone().requires_grad_(True)
    y = apply_rope(xr, 500000.0, pos_offset)
    y.backward(dy)
    what = f"{shape} +{pos_offset}"
    r = (_report(f"rope y {what}", ec.rope_ratio(y.detach(), base[0], ref[0])),
         _report(f"rope dx {what}", ec.rope_ratio(xr.grad, base[1], ref[1])))
    assert max(r) <= 1.0, (what, r)

    # the raw entry point on the sliced tables gives the same bits
    c, sn = cos_t[pos_offset:].contiguous(), sin_t[pos_offset:].contiguous()
    assert torch.equal(ext.rope_apply(x, c, sn, False), y.detach())
    assert torch.equal(ext.rope_apply(dy, c, sn, True), xr.grad)


@pytest.mark.parametrize("d", (8, 64, 80, 128))
def test_rope_decode_row_and_long_table(ext, d):
    pos, s = 37, 77
    x, _ = _rope_inputs((2, 3, s, d), 0)
    full = apply_rope(x)
    one = apply_rope(x[:, :, pos:pos + 1].contiguous(), pos_offset=pos)
    assert torch.equal(one, full[:, :, pos:pos + 1])
    # a table longer than S is accepted and gives the same bits
    cos_l, sin_l = rope_tables(s + 11, d, 500000.0, x.device)
    assert torch.equal(ext.rope_apply(x, cos_l, sin_l, False), full)


# --- SwiGLU ---------------------------------------------------------------
@pytest.mark.parametrize("family", ("randn", "x20", "saturating"))
@pytest.mark.parametrize("n", (8, 4096, 4194304 + 296))
def test_swiglu_fwd_bwd(ext, n, family):
    a, b, dy = _cuda(*ec.swiglu_input(n, family))
    ref, base = ec.swiglu_reference(a, b, dy), ec.swiglu_baseline(a, b, dy)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = swiglu(ar, br)
    y.backward(dy)
    got = (y.detach(), ar.grad, br.grad)
    r = [_report(f"swiglu {name} n{n} {family}",
                 ec.flat_ratio(g, bs, rf, ec.ULP_BF16))
         for name, g, bs, rf in zip(("y", "da", "db"), got, base, ref)]
    assert max(r) <= 1.0, r
    if family == "saturating":
        k = min(n, 64) // len(ec.SATURATING) * len(ec.SATURATING)
        for g, rf in zip(got, ref):
            assert torch.isfinite(g.float()).all()
            assert torch.equal(g[:k].float(), rf[:k].to(BF16).float())


# --- AdamW ----------------------------------------------------------------
ADAMW_GRID = [(gs, wd, b2, lr, scale)
              for gs in (1.0, 0.125) for wd in (0.0, 0.1)
              for b2, lr in ((0.95, 1e-2), (0.999, 1e-3))
              for scale in (1.0, 1e-3)]
ADAMW_N = (4, 1028, 2097152 + 1028)


@pytest.mark.parametrize("with_model", (False, True))
@pytest.mark.parametrize("grad_dtype", (torch.float32, BF16))
@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_step(ext, n, grad_dtype, with_model):
    """master, m and v after every one of 10 steps (1, 2 and 10 among
    them); ref and base restart each step from the kernel's own state. The
    bf16 model copy is master.to(bfloat16) bitwise."""
    worst = 0.0
    for gs, wd, b2, lr, scale in ADAMW_GRID:
        master, grads = ec.adamw_case(n, scale, grad_dtype, 10)
        master = master.cuda()
        m, v = torch.zeros_like(master), torch.zeros_like(master)
        model = (torch.zeros(n, device="cuda", dtype=BF16) if with_model
                 else torch.Tensor())
        for step, g in enumerate(grads, 1):
            g = g.cuda()
            h = ec.adamw_hyper(lr, 0.9, b2, 1e-8, wd, gs, step)
            ref = ec.adamw_reference(master, m, v, g, h)
            base = ec.adamw_baseline(master, m, v, g, h)
            ext.adamw_step(master, model, g, m, v, lr, 0.9, b2, 1e-8, wd,
                           step, gs)
            r = max(ec.flat_ratio(a, bs, rf, ec.ULP_FP32)
                    for a, bs, rf in zip((master, m, v), base, ref))
            assert r <= 1.0, (gs, wd, b2, lr, scale, step, r)
            worst = max(worst, r)
            if with_model:
                assert torch.equal(model, master.to(BF16))
    _report(f"adamw master/m/v n{n} {grad_dtype} model={with_model}", worst)


def test_adamw_exact_moments(ext):
    n, steps = 1028, 3
    master = torch.zeros(n, device="cuda")
    m, v = torch.zeros_like(master), torch.zeros_like(master)
    m64, v64 = m.double(), v.double()
    for step, g in enumerate(ec.adamw_exact_case(n, steps), 1):
        g = g.cuda()
        h = ec.adamw_hyper(1e-3, 0.5, 0.5, 1e-8, 0.0, 1.0, step)
        _, m64, v64 = ec.adamw_reference(master, m64, v64, g, h)
        ext.adamw_step(master, torch.Tensor(), g, m, v, 1e-3, 0.5, 0.5, 1e-8,
                       0.0, step, 1.0)
        assert torch.equal(m.double(), m64) and torch.equal(v.double(), v64)


@pytest.mark.parametrize("param_dtype", (BF16, torch.float32))
def test_fused_adamw_three_parameters(param_dtype):
    """Three parameters, 1030 + 77 + 6 = 1113 elements (not a multiple of
    4): the pad stays 0, every parameter equals the bf16 (or fp32) of its
    master slice, and master/m/v follow the reference."""
    g = torch.Generator().manual_seed(11)
    shapes = [(103, 10), (77,), (2, 3)]
    params = [torch.nn.Parameter(torch.randn(*s, generator=g)
                                 .to(param_dtype).cuda()) for s in shapes]
    lr, b2, wd = 1e-2, 0.95, 0.1
    opt = FusedAdamW(params, lr=lr, betas=(0.9, b2), eps=1e-8, weight_decay=wd)
    total = sum(p.numel() for p in params)
    assert total % 4 and opt.master.numel() == (total + 3) // 4 * 4
    for step in range(1, 4):
        grads = [torch.randn(*s, generator=g).to(param_dtype).cuda()
                 for s in shapes]
        for p, gr in zip(params, grads):
            p.grad = gr
        flat = torch.zeros_like(opt.master)
        flat[:total] = torch.cat([gr.reshape(-1).float() for gr in grads])
        before = (opt.master.clone(), opt.m.clone(), opt.v.clone())
        h = ec.adamw_hyper(lr, 0.9, b2, 1e-8, wd, 0.5, step)
        ref = ec.adamw_reference(*before, flat, h)
        base = ec.adamw_baseline(*before, flat, h)
        opt.step(grad_scale=0.5)
        r = max(ec.flat_ratio(a, bs, rf, ec.ULP_FP32)
                for a, bs, rf in zip((opt.master, opt.m, opt.v), base, ref))
        assert _report("FusedAdamW master/m/v", r) <= 1.0
        for t in (opt.master, opt.m, opt.v):
            assert torch.equal(t[total:], torch.zeros_like(t[total:]))
        if param_dtype == BF16:
            assert torch.equal(opt._model_flat[total:],
                               torch.zeros_like(opt._model_flat[total:]))
        for p, (off, cnt) in zip(params, opt._slices):
            want = opt.master[off:off + cnt].to(param_dtype).view_as(p)
            assert torch.equal(p.detach(), want)


# --- argument checks ------------------------------------------------------
# Every bad tensor is the same size as or LARGER than what the kernel would
# read, so even an unguarded launch stays in bounds.

def _ce_args():
    x, labels = _cuda(*ec.ce_input(4, 264, "randn"))
    lse = torch.zeros(4, device="cuda")
    return {"logits": x, "labels": labels, "lse": lse,
            "grad_scale": torch.ones(1, device="cuda")}


BAD_CE = {
    "logits_fp16": lambda a: a.update(logits=a["logits"].to(torch.float16)),
    "logits_fp32": lambda a: a.update(logits=a["logits"].float()),
    "labels_int32": lambda a: a.update(
        labels=torch.zeros(8, device="cuda", dtype=torch.int32)),
    "labels_cpu": lambda a: a.update(labels=a["labels"].cpu()),
    "labels_longer": lambda a: a.update(
        labels=torch.zeros(5, device="cuda", dtype=torch.long)),
    "vocab_not_multiple_of_8": lambda a: a.update(
        logits=torch.zeros(4, 268, device="cuda", dtype=BF16)),
}
BAD_CE_BWD = dict(BAD_CE, **{
    "lse_cpu": lambda a: a.update(lse=a["lse"].cpu()),
    "lse_longer": lambda a: a.update(lse=torch.zeros(5, device="cuda")),
    "lse_fp64": lambda a: a.update(lse=a["lse"].double()),
    "lse_strided": lambda a: a.update(lse=torch.zeros(8, device="cuda")[::2]),
    "grad_scale_two_elements": lambda a: a.update(
        grad_scale=torch.ones(2, device="cuda")),
    "grad_scale_cpu": lambda a: a.update(grad_scale=torch.ones(1)),
    "grad_scale_fp64": lambda a: a.update(
        grad_scale=a["grad_scale"].double()),
})


@pytest.mark.parametrize("bad", sorted(BAD_CE))
def test_cross_entropy_fwd_rejects(ext, bad):
    a = _ce_args()
    BAD_CE[bad](a)
    with pytest.raises(RuntimeError):
        ext.cross_entropy_fwd(a["logits"], a["labels"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", sorted(BAD_CE_BWD))
def test_cross_entropy_bwd_rejects(ext, bad):
    a = _ce_args()
    BAD_CE_BWD[bad](a)
    with pytest.raises(RuntimeError):
        ext.cross_entropy_bwd(a["logits"], a["labels"], a["lse"],
                              a["grad_scale"])
    torch.cuda.synchronize()


def _swiglu_args():
    return dict(zip(("a", "b", "dy"), _cuda(*ec.swiglu_input(4096, "randn"))))


BAD_SWIGLU = {
    "dy_fp32": lambda a: a.update(dy=a["dy"].float()),
    "a_fp16": lambda a: a.update(a=a["a"].to(torch.float16)),
    "b_fp32": lambda a: a.update(b=a["b"].float()),
    "dy_longer": lambda a: a.update(
        dy=torch.zeros(4104, device="cuda", dtype=BF16)),
    "b_longer": lambda a: a.update(
        b=torch.zeros(4104, device="cuda", dtype=BF16)),
    "dy_cpu": lambda a: a.update(dy=a["dy"].cpu()),
    "a_cpu": lambda a: a.update(a=a["a"].cpu()),
    "size_not_multiple_of_8": lambda a: a.update(
        {k: torch.zeros(4100, device="cuda", dtype=BF16) for k in a}),
    "b_cpu": lambda a: a.update(b=a["b"].cpu()),
}


@pytest.mark.parametrize("bad", sorted(BAD_SWIGLU))
def test_swiglu_bwd_rejects(ext, bad):
    a = _swiglu_args()
    BAD_SWIGLU[bad](a)
    with pytest.raises(RuntimeError):
        ext.swiglu_bwd(a["dy"], a["a"], a["b"])
    torch.cuda.synchronize()


BAD_NORM_PARAM = {"longer": lambda: torch.ones(520, device="cuda"),
                  "cpu": lambda: torch.ones(512)}


@pytest.mark.parametrize("bad", sorted(BAD_NORM_PARAM))
@pytest.mark.parametrize("which", ("gamma", "beta"))
def test_layernorm_fwd_rejects_bad_parameter(ext, which, bad):
    x = ec.norm_input(4, 512, "randn").cuda()
    p = {"gamma": torch.ones(512, device="cuda"),
         "beta": torch.zeros(512, device="cuda")}
    p[which] = BAD_NORM_PARAM[bad]()
    with pytest.raises(RuntimeError):
        ext.layernorm_fwd(x, p["gamma"], p["beta"], EPS)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", sorted(BAD_NORM_PARAM))
def test_rmsnorm_fwd_rejects_bad_gamma(ext, bad):
    x = ec.norm_input(4, 512, "randn").cuda()
    with pytest.raises(RuntimeError):
        ext.rmsnorm_fwd(x, BAD_NORM_PARAM[bad](), EPS)
    torch.cuda.synchronize()


def _rope_args():
    x, _ = _rope_inputs((1, 2, 16, 64), 0)
    cos_t, sin_t = rope_tables(16, 64, 500000.0, x.device)
    return {"x": x, "cos": cos_t, "sin": sin_t}


BAD_ROPE = {
    # more rows / more columns than cos: never smaller than what is read
    "sin_more_rows": lambda a: a.update(
        sin=torch.zeros(24, 32, device="cuda")),
    "sin_more_columns": lambda a: a.update(
        sin=torch.zeros(16, 40, device="cuda")),
    "cos_cpu": lambda a: a.update(cos=a["cos"].cpu()),
    "sin_cpu": lambda a: a.update(sin=a["sin"].cpu()),
    "cos_column_slice": lambda a: a.update(
        cos=torch.zeros(16, 64, device="cuda")[:, :32]),
    "sin_column_slice": lambda a: a.update(
        sin=torch.zeros(16, 64, device="cuda")[:, :32]),
    "sin_fp64": lambda a: a.update(sin=a["sin"].double()),
    "cos_fp64": lambda a: a.update(cos=a["cos"].double()),
}


@pytest.mark.parametrize("bad", sorted(BAD_ROPE))
def test_rope_apply_rejects(ext, bad):
    a = _rope_args()
    BAD_ROPE[bad](a)
    with pytest.raises(RuntimeError):
        ext.rope_apply(a["x"], a["cos"], a["sin"], False)
    torch.cuda.synchronize()


def _adamw_args():
    n = 1028
    z = lambda dt=torch.float32: torch.zeros(n, device="cuda", dtype=dt)  # noqa: E731
    return {"master": z(), "model": z(BF16), "grad": z(), "m": z(), "v": z()}


def _strided(dtype=torch.float32):
    return torch.zeros(2056, device="cuda", dtype=dtype)[::2]


BAD_ADAMW = {
    "model_fp16": lambda a: a.update(model=a["model"].to(torch.float16)),
    "model_fp32": lambda a: a.update(model=a["model"].float()),
    "model_longer": lambda a: a.update(
        model=torch.zeros(1032, device="cuda", dtype=BF16)),
    "model_strided": lambda a: a.update(model=_strided(BF16)),
    "m_strided": lambda a: a.update(m=_strided()),
    "v_strided": lambda a: a.update(v=_strided()),
    "grad_strided": lambda a: a.update(grad=_strided()),
    "m_cpu": lambda a: a.update(m=a["m"].cpu()),
    "v_cpu": lambda a: a.update(v=a["v"].cpu()),
    "grad_cpu": lambda a: a.update(grad=a["grad"].cpu()),
    "grad_fp16": lambda a: a.update(grad=a["grad"].to(torch.float16)),
    "m_fp64": lambda a: a.update(m=a["m"].double()),
    "v_fp64": lambda a: a.update(v=a["v"].double()),
    "model_cpu": lambda a: a.update(model=a["model"].cpu()),
    "master_strided": lambda a: a.update(master=_strided()),
}


@pytest.mark.parametrize("bad", sorted(BAD_ADAMW))
def test_adamw_step_rejects(ext, bad):
    a = _adamw_args()
    BAD_ADAMW[bad](a)
    with pytest.raises(RuntimeError):
        ext.adamw_step(a["master"], a["model"], a["grad"], a["m"], a["v"],
                       1e-3, 0.9, 0.95, 1e-8, 0.1, 1, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(a["master"], torch.zeros_like(a["master"]))

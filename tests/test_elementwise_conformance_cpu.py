"""CPU check of the elementwise conformance criterion itself.

For every kernel the fp32 emulation of its arithmetic (in its own
summation order) has to sit under the bound on every input family of
test_elementwise_conformance_gpu.py, and every named mutant has to be
rejected. The worst ratios of the correct emulation are printed (-s) and
quoted in docs/KERNELS.md as the CPU prediction.

Mutants that PASS the assertions of the older tests (test_ops_gpu.py,
test_norms_gpu.py), shown below next to their rejection:
  CE    bwd_no_softmax     max|dlogits - ref| < 1e-4 at N = 512
  RoPE  bwd_forward_sign   ||grad|| == ||dy|| to 2e-2
"""

import pytest
import torch

import elementwise_conformance as ec

BF16 = torch.bfloat16
WORST = {}


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{name}: ratio to bound {ratio:.3f}")
    return ratio


# --- cross entropy --------------------------------------------------------
CE_SHAPES = [(1, 8), (5, 8), (1, 2040), (5, 2040), (5, 2048), (1, 2056),
             (5, 2056), (5, 6152), (2051, 264), (8, 51200)]
CE_FAMILIES = ("randn", "x8", "off1000")


def _ce_ratios(n, v, family, gs, mutant=None, seed=0):
    x, labels = ec.ce_input(n, v, family, seed)
    ref = ec.ce_reference(x, labels, gs)
    base = ec.ce_baseline(x, labels, gs)
    got = ec.ce_emulate(x, labels, gs, mutant)
    return (ec.row_ratio(got[0], base[0], ref[0]),
            ec.row_ratio(got[1], base[1], ref[1]),
            ec.ce_dlogits_ratio(got[2], base[2], ref[2], labels))


@pytest.mark.parametrize("family", CE_FAMILIES)
@pytest.mark.parametrize("n,v", CE_SHAPES)
def test_ce_emulation_under_bound(n, v, family):
    for gs in (1.0 / n, 0.37):
        loss, lse, d = _ce_ratios(n, v, family, gs)
        _record("ce loss", loss)
        _record("ce lse", lse)
        _record("ce dlogits", d)
        assert max(loss, lse, d) <= 1.0, (loss, lse, d)


@pytest.mark.parametrize("mutant,n,v", [
    ("bwd_no_softmax", 5, 2056),
    ("skip_last_partial_stride", 5, 2056),
    ("skip_last_partial_stride", 5, 2040),
    ("onehot_off_by_one", 5, 2056),
    ("ignore_grad_scale", 5, 2056),
    ("max_full_strides_only", 5, 2040),   # no full stride: m stays -1e30
])
def test_ce_mutants_rejected(mutant, n, v):
    for family in CE_FAMILIES:
        assert max(_ce_ratios(n, v, family, 0.2, mutant)) > 1.0, family


def test_ce_softmax_dropped_passes_old_bound_but_not_the_criterion():
    """The old test's only backward assertion, at its N = 512: a kernel
    writing zero for every non-target column passes it."""
    n, v = 512, 2056
    x, labels = ec.ce_input(n, v, "randn")
    ref = ec.ce_reference(x, labels, 1.0 / n)[2]
    bad = ec.ce_emulate(x, labels, 1.0 / n, "bwd_no_softmax")[2]
    assert float((bad.double() - ref).abs().max()) < 1e-4     # old bound
    assert _ce_ratios(n, v, "randn", 1.0 / n, "bwd_no_softmax")[2] > 1.0


@pytest.mark.parametrize("n,v", [(3, 8), (3, 2040), (4, 2056), (6, 6152)])
def test_ce_exact_row_max(n, v):
    cols = ec.ce_pinned_labels(v) + [v - 3]
    x, labels = ec.ce_exact_case(n, v, cols[-n:])
    loss, lse, _ = ec.ce_emulate(x, labels, 1.0)
    assert torch.equal(lse.double(), x.double().max(-1).values)
    assert torch.equal(loss, torch.zeros(n))
    assert torch.equal(ec.ce_emulate_row_max(x).double(),
                       x.double().max(-1).values)
    for mutant in ("max_full_strides_only", "skip_last_partial_stride"):
        bad = ec.ce_emulate(x, labels, 1.0, mutant)[1]
        assert not torch.equal(bad.double(), x.double().max(-1).values)


def test_ce_out_of_range_labels():
    x, _ = ec.ce_input(3, 264, "randn")
    labels = torch.tensor([264, -1, 5])
    loss, lse, d = ec.ce_emulate(x, labels, 0.5)
    ref = ec.ce_reference(x, labels, 0.5)
    assert torch.isnan(loss[:2]).all() and torch.isfinite(loss[2])
    assert torch.isnan(ref[0][:2]).all()
    assert torch.isfinite(lse).all()
    assert float(d[:2].float().min()) >= 0.0      # no one-hot on rows 0, 1


# --- norms ----------------------------------------------------------------
NORM_SHAPES = [(1, 8), (33, 8), (2051, 8), (33, 512), (2051, 512), (1, 2040),
               (33, 2560), (33, 4104), (1, 8192), (33, 8192)]
EPS = 1e-5


def _ln_ratios(rows, h, family, mutant=None):
    x = ec.norm_input(rows, h, family)
    gamma, beta = ec.norm_params(h)
    ref = ec.ln_reference(x, gamma, beta, EPS)
    base = ec.ln_baseline(x, gamma, beta, EPS)
    got = ec.ln_emulate(x, gamma, beta, EPS, mutant)
    return (ec.block_ratio(got[0], base[0], ref[0], ec.COL_BLOCK, ec.ULP_BF16),
            ec.row_ratio(got[1], base[1], ref[1]),
            ec.row_ratio(got[2], base[2], ref[2]))


@pytest.mark.parametrize("family", ("randn", "x100", "x1e-3", "const3"))
@pytest.mark.parametrize("rows,h", NORM_SHAPES)
def test_ln_emulation_under_bound(rows, h, family):
    y, mean, rstd = _ln_ratios(rows, h, family)
    _record("ln y", y), _record("ln mean", mean), _record("ln rstd", rstd)
    assert max(y, mean, rstd) <= 1.0, (y, mean, rstd)


@pytest.mark.parametrize("family", ("off10", "off100", "off1000"))
@pytest.mark.parametrize("rows,h", [(33, 512), (33, 2560)])
def test_ln_offset_rows(rows, h, family):
    y, mean, rstd = _ln_ratios(rows, h, family)
    _record("ln y (offset)", y), _record("ln mean (offset)", mean)
    _record("ln rstd (offset)", rstd)
    assert max(y, mean, rstd) <= 1.0, (y, mean, rstd)
    # the kernel as it was: E[x^2] - mean^2 in fp32
    assert _ln_ratios(rows, h, family, "one_pass_variance")[2] > 1.0


@pytest.mark.parametrize("mutant", ("biased_by_one", "no_beta"))
def test_ln_mutants_rejected(mutant):
    for rows, h in ((33, 512), (33, 2560)):
        assert max(_ln_ratios(rows, h, "randn", mutant)) > 1.0


@pytest.mark.parametrize("family", ("randn", "x100", "x1e-3"))
@pytest.mark.parametrize("rows,h", NORM_SHAPES)
def test_rms_emulation_under_bound(rows, h, family):
    x = ec.norm_input(rows, h, family)
    gamma, _ = ec.norm_params(h)
    ref, base = ec.rms_reference(x, gamma, EPS), ec.rms_baseline(x, gamma, EPS)
    got = ec.rms_emulate(x, gamma, EPS)
    y = _record("rms y", ec.block_ratio(got[0], base[0], ref[0],
                                        ec.COL_BLOCK, ec.ULP_BF16))
    rstd = _record("rms rstd", ec.row_ratio(got[1], base[1], ref[1]))
    assert max(y, rstd) <= 1.0
    if h % (ec.BLOCK * ec.VEC):
        bad = ec.rms_emulate(x, gamma, EPS, "skip_last_partial_stride")
        assert ec.row_ratio(bad[1], base[1], ref[1]) > 1.0


@pytest.mark.parametrize("rows,h", [(3, 8), (5, 512), (2, 2040), (3, 8192)])
def test_norm_exact_sums(rows, h):
    x, gamma, beta = ec.norm_exact_case(rows, h)
    y, mean, rstd = ec.ln_emulate(x, gamma, beta, 0.0)
    assert torch.equal(mean, torch.zeros(rows))
    assert torch.equal(rstd, torch.full((rows,), 0.5))
    assert torch.equal(y.double(), ec.ln_reference(x, gamma, beta, 0.0)[0])
    y, rstd = ec.rms_emulate(x, gamma, 0.0)
    assert torch.equal(rstd, torch.full((rows,), 0.5))
    assert torch.equal(y.double(), ec.rms_reference(x, gamma, 0.0)[0])
    if h & (h - 1) == 0:
        xi = ec.norm_integer_case(rows, h)
        mean = ec.ln_emulate(xi, gamma, beta, EPS)[1]
        assert torch.equal(mean.double(), xi.double().mean(-1))


# --- RoPE -----------------------------------------------------------------
ROPE_SHAPES = [(2, 3, 1, 8), (1, 2, 77, 64), (2, 2, 128, 80), (1, 2, 77, 128)]


def _rope_case(shape, pos_offset):
    g = torch.Generator().manual_seed(sum(shape) + pos_offset)
    x = torch.randn(*shape, generator=g).to(BF16)
    dy = torch.randn(*shape, generator=g).to(BF16)
    cos_t, sin_t = ec.rope_tables_fp32(pos_offset + shape[2], shape[3])
    return x, dy, cos_t, sin_t


def _rope_ratios(shape, pos_offset, mutant=None):
    x, dy, cos_t, sin_t = _rope_case(shape, pos_offset)
    ref = ec.rope_reference(x, cos_t, sin_t, pos_offset, dy)
    base = ec.rope_baseline(x, cos_t, sin_t, pos_offset, dy)
    y = ec.rope_emulate(x, cos_t, sin_t, pos_offset, False, mutant)
    dx = ec.rope_emulate(dy, cos_t, sin_t, pos_offset, True, mutant)
    return (ec.rope_ratio(y, base[0], ref[0]),
            ec.rope_ratio(dx, base[1], ref[1]))


@pytest.mark.parametrize("pos_offset", (0, 37))
@pytest.mark.parametrize("shape", ROPE_SHAPES)
def test_rope_emulation_under_bound(shape, pos_offset):
    y, dx = _rope_ratios(shape, pos_offset)
    _record("rope y", y), _record("rope dx", dx)
    assert max(y, dx) <= 1.0


@pytest.mark.parametrize("mutant", ec.ROPE_MUTANTS)
def test_rope_mutants_rejected(mutant):
    for shape in ROPE_SHAPES[1:]:
        assert max(_rope_ratios(shape, 37, mutant)) > 1.0, shape


def test_rope_forward_sign_backward_passes_old_norm_test():
    shape = (1, 2, 128, 64)
    x, dy, cos_t, sin_t = _rope_case(shape, 0)
    bad = ec.rope_emulate(dy, cos_t, sin_t, 0, True, "bwd_forward_sign")
    gn, dn = bad.float().pow(2).sum(), dy.float().pow(2).sum()
    assert torch.allclose(gn, dn, rtol=2e-2)                   # old test
    assert _rope_ratios(shape, 0, "bwd_forward_sign")[1] > 1.0


# --- SwiGLU ---------------------------------------------------------------
def _swiglu_ratios(n, family, mutant=None):
    a, b, dy = ec.swiglu_input(n, family)
    ref, base = ec.swiglu_reference(a, b, dy), ec.swiglu_baseline(a, b, dy)
    got = ec.swiglu_emulate(a, b, dy, mutant)
    return tuple(ec.flat_ratio(g, bs, r, ec.ULP_BF16)
                 for g, bs, r in zip(got, base, ref))


@pytest.mark.parametrize("family", ("randn", "x20", "saturating"))
@pytest.mark.parametrize("n", (8, 4096, 6144 + 296))
def test_swiglu_emulation_under_bound(n, family):
    y, da, db = _swiglu_ratios(n, family)
    _record("swiglu y", y), _record("swiglu da", da), _record("swiglu db", db)
    assert max(y, da, db) <= 1.0


def test_swiglu_mutants_rejected():
    for family in ("randn", "x20"):
        assert _swiglu_ratios(4096, family, "da_without_x_term")[1] > 1.0
        assert _swiglu_ratios(4096, family, "db_uses_s")[2] > 1.0


def test_swiglu_saturated_values_equal_reference_bf16():
    a, b, dy = ec.swiglu_input(64, "saturating")
    got = ec.swiglu_emulate(a, b, dy)
    ref = ec.swiglu_reference(a, b, dy)
    k = 60
    for g, r in zip(got, ref):
        assert torch.isfinite(g.float()).all()
        assert torch.equal(g[:k].float(), r[:k].to(BF16).float())


# --- AdamW ----------------------------------------------------------------
ADAMW_GRID = [(gs, wd, b2, lr, scale)
              for gs in (1.0, 0.125) for wd in (0.0, 0.1)
              for b2, lr in ((0.95, 1e-2), (0.999, 1e-3))
              for scale in (1.0, 1e-3)]


def _adamw_run(n, grad_dtype, gs, wd, b2, lr, scale, steps, mutant=None):
    """Worst ratio over master/m/v and the steps; the emulation's own state
    is carried from step to step, ref and base restart from it."""
    master, grads = ec.adamw_case(n, scale, grad_dtype, steps)
    m, v = torch.zeros(n), torch.zeros(n)
    worst, model_ok = 0.0, True
    for step, g in enumerate(grads, 1):
        h = ec.adamw_hyper(lr, 0.9, b2, 1e-8, wd, gs, step)
        ref = ec.adamw_reference(master, m, v, g, h)
        base = ec.adamw_baseline(master, m, v, g, h)
        got = ec.adamw_emulate(master, m, v, g, h, mutant)
        worst = max([worst] + [ec.flat_ratio(a, b, r, ec.ULP_FP32)
                               for a, b, r in zip(got, base, ref)])
        model_ok &= torch.equal(got[3], got[0].to(BF16))
        master, m, v = got[:3]
    return worst, model_ok


@pytest.mark.parametrize("grad_dtype", (torch.float32, BF16))
@pytest.mark.parametrize("n", (4, 1028))
def test_adamw_emulation_under_bound(n, grad_dtype):
    for cfg in ADAMW_GRID:
        worst, model_ok = _adamw_run(n, grad_dtype, *cfg, steps=10)
        _record("adamw master/m/v", worst)
        assert worst <= 1.0 and model_ok, cfg


@pytest.mark.parametrize("mutant", ("ignore_grad_scale",
                                    "coupled_weight_decay",
                                    "no_bias_correction"))
def test_adamw_mutants_rejected(mutant):
    worst, _ = _adamw_run(1028, torch.float32, 0.125, 0.1, 0.999, 1e-3, 1.0,
                          steps=2, mutant=mutant)
    assert worst > 1.0


def test_adamw_truncated_model_rejected():
    _, model_ok = _adamw_run(1028, torch.float32, 1.0, 0.1, 0.95, 1e-2, 1.0,
                             steps=1, mutant="model_truncated")
    assert not model_ok


def test_adamw_stride_tail_rejected():
    n = ec.ADAMW_STRIDE + 1028
    worst, _ = _adamw_run(n, torch.float32, 1.0, 0.1, 0.95, 1e-2, 1.0,
                          steps=1, mutant="stride_tail_not_updated")
    assert worst > 1.0
    worst, _ = _adamw_run(n, torch.float32, 1.0, 0.1, 0.95, 1e-2, 1.0, steps=1)
    assert worst <= 1.0


def test_adamw_exact_moments():
    n, steps = 1028, 3
    master = torch.zeros(n)
    m, v = torch.zeros(n), torch.zeros(n)
    m64, v64 = m.double(), v.double()
    for step, g in enumerate(ec.adamw_exact_case(n, steps), 1):
        h = ec.adamw_hyper(1e-3, 0.5, 0.5, 1e-8, 0.0, 1.0, step)
        _, m64, v64 = ec.adamw_reference(master, m64, v64, g, h)
        master, m, v, _ = ec.adamw_emulate(master, m, v, g, h)
        assert torch.equal(m.double(), m64) and torch.equal(v.double(), v64)


def test_bias_c2_gap_is_what_the_docs_say():
    assert 1.2e-5 < ec.bias_c2_gap(0.999, 1) < 1.4e-5


def test_print_worst_ratios():
    """Last in the file: the figures quoted in docs/KERNELS.md."""
    for name in sorted(WORST):
        print(f"CPU emulation worst ratio  {name:24s} {WORST[name]:.3f}")

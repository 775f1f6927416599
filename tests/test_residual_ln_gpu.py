"""GPU tests of the fused bias + residual + LayerNorm forward
(bias_residual_layernorm_fwd, bias_residual_add; ln_row.h) and of the norm
backward with the residual gradient folded in (layernorm_bwd_add; the ADD
instantiation of norm_bwd.h).

Forward. x = bf16(residual + bf16(y + bias)) keeps the roundings of the
two aten adds it replaces, and the row body sums the statistics in the
order of layernorm_fwd, so x, z, mean and rstd are compared BITWISE with
`residual + (y + bias)` in aten followed by ext.layernorm_fwd. Shapes: H of
1 to 4 chunks per thread with full and partial last strides, 1 to 257
rows, and 4100 rows (more rows than any grid has workgroups).

Backward. g = bf16(dres + bf16(dx)) bitwise against dres + layernorm_bwd's
dx; dgamma and dbeta bitwise layernorm_bwd's (the two launch the same
grid); colsum against the float64 column sum of the returned g under the
any-order fp32 sum bound rows * 2^-24 * sum|g|; and an exact case.

The exact case takes norm_bwd_conformance.exact_case with integer dres
that are multiples of 512 (+-512, +-1024): |dx| stays below 16 there, so
bf16(dres + dx) is an even integer of magnitude 496..1040 and the fp32
sum of up to 12293 of them (< 2^24) is exact in any order. (Small integer
dres would not do: dx carries fractions of 1/H, and g then has more bits
than an fp32 sum over thousands of rows keeps.) colsum then equals the
float64 sum bitwise at every shape, which is what sees a dropped or
doubled row or slab in the long trips.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import elementwise_conformance as ec
    import norm_bwd_conformance as nb
    from metis_amd.ops import require_extension
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
EPS = 1e-5
FWD_HIDDEN = (8, 512, 768, 2048, 2560, 4096, 8192)
ROWS = (1, 3, 33, 257)
FWD_SHAPES = [(r, h) for h in FWD_HIDDEN for r in ROWS] + [(4100, 2560)]
FWD_KINDS = ("randn", "x100", "off100")

# the shapes of test_norm_bwd_conformance_gpu.py: SHAPES and its long trips
BWD_HIDDEN = (8, 512, 768, 2560, 4096, 8192)
LONG = [(12293, 8), (12293, 512), (12293, 2560), (6147, 4096)]
BWD_SHAPES = [(r, h) for h in BWD_HIDDEN for r in ROWS] + LONG
SUM_BOUND_MAX_ROWS = 257


@pytest.fixture(scope="module")
def ext():
    return require_extension()


def _fwd_input(rows, h, kind):
    """(y, bias, residual, gamma, beta): randn; y and residual x 100;
    residual rows offset by 100 at std 1."""
    g = torch.Generator("cuda").manual_seed(rows * 8209 + h)
    kw = dict(generator=g, device="cuda")
    y, res = torch.randn(rows, h, **kw), torch.randn(rows, h, **kw)
    bias = torch.randn(h, **kw)
    if kind == "x100":
        y, res = y * 100, res * 100
    elif kind == "off100":
        res = res + 100
    gamma, beta = (t.cuda() for t in ec.norm_params(h))
    return y.to(BF16), bias.to(BF16), res.to(BF16), gamma, beta


@pytest.mark.parametrize("rows,h", FWD_SHAPES)
def test_bias_residual_layernorm_fwd_bitwise(ext, rows, h):
    for kind in FWD_KINDS:
        y, bias, res, gamma, beta = _fwd_input(rows, h, kind)
        x_ref = res + (y + bias)
        z_ref, mean_ref, rstd_ref = ext.layernorm_fwd(x_ref, gamma, beta, EPS)
        x, z, mean, rstd = ext.bias_residual_layernorm_fwd(
            y, bias, res, gamma, beta, EPS)
        assert x.dtype == z.dtype == BF16 and x.shape == z.shape == y.shape
        assert mean.dtype == rstd.dtype == torch.float32
        assert mean.shape == rstd.shape == (rows,)
        for name, got, ref in (("x", x, x_ref), ("z", z, z_ref),
                               ("mean", mean, mean_ref),
                               ("rstd", rstd, rstd_ref)):
            assert torch.equal(got, ref), (name, rows, h, kind)
        assert torch.equal(ext.bias_residual_add(y, bias, res), x_ref), kind


def test_forward_accepts_3d(ext):
    y, bias, res, gamma, beta = _fwd_input(6, 768, "randn")
    flat = ext.bias_residual_layernorm_fwd(y, bias, res, gamma, beta, EPS)
    got = ext.bias_residual_layernorm_fwd(
        y.view(2, 3, 768), bias, res.view(2, 3, 768), gamma.to(BF16).float(),
        beta, EPS)
    flat16 = ext.bias_residual_layernorm_fwd(
        y, bias, res, gamma.to(BF16), beta, EPS)
    assert got[0].shape == (2, 3, 768) and got[2].shape == (6,)
    assert torch.equal(got[0].view(6, 768), flat[0])
    assert torch.equal(got[1].view(6, 768), flat16[1])
    assert torch.equal(
        ext.bias_residual_add(y.view(2, 3, 768), bias, res.view(2, 3, 768)),
        flat[0].view(2, 3, 768))


# --- launcher rejections --------------------------------------------------
# Every bad tensor is on the device and at least as large in bytes as what
# an unguarded kernel would read, so a launch that slipped through would
# stay in bounds.
R_, H_ = 4, 512


def _z(*shape, dtype=BF16):
    return torch.zeros(*shape, device="cuda", dtype=dtype)


def _fwd_args():
    y, bias, res, gamma, beta = _fwd_input(R_, H_, "randn")
    return {"y": y, "bias": bias, "residual": res, "gamma": gamma,
            "beta": beta}


BAD_FWD = {
    "y_fp32": lambda a: a.update(y=a["y"].float()),
    "residual_fp16": lambda a: a.update(residual=a["residual"].half()),
    "bias_fp32": lambda a: a.update(bias=a["bias"].float()),
    "bias_short": lambda a: a.update(bias=_z(2 * H_)[:H_ - 8]),
    "bias_longer": lambda a: a.update(bias=_z(H_ + 8)),
    "residual_more_rows": lambda a: a.update(residual=_z(R_ + 1, H_)),
    "residual_other_row_length": lambda a: a.update(
        residual=_z(R_ // 2, 2 * H_)),
    "hidden_8200": lambda a: a.update(
        y=_z(R_, 8200), residual=_z(R_, 8200), bias=_z(8200),
        gamma=_z(8200, dtype=torch.float32),
        beta=_z(8200, dtype=torch.float32)),
    "hidden_not_multiple_of_8": lambda a: a.update(
        y=_z(R_, H_ + 4), residual=_z(R_, H_ + 4), bias=_z(H_ + 4),
        gamma=_z(H_ + 4, dtype=torch.float32),
        beta=_z(H_ + 4, dtype=torch.float32)),
    "y_strided": lambda a: a.update(y=_z(R_, 2 * H_)[:, ::2]),
    "residual_strided": lambda a: a.update(residual=_z(R_, 2 * H_)[:, ::2]),
    "bias_cpu": lambda a: a.update(bias=a["bias"].cpu()),
}
BAD_FWD_LN = dict(BAD_FWD, **{
    "gamma_longer": lambda a: a.update(gamma=_z(H_ + 8, dtype=torch.float32)),
    "beta_cpu": lambda a: a.update(beta=a["beta"].cpu()),
})


@pytest.mark.parametrize("bad", sorted(BAD_FWD_LN))
def test_bias_residual_layernorm_fwd_rejects(ext, bad):
    a = _fwd_args()
    BAD_FWD_LN[bad](a)
    with pytest.raises(RuntimeError):
        ext.bias_residual_layernorm_fwd(a["y"], a["bias"], a["residual"],
                                        a["gamma"], a["beta"], EPS)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", sorted(BAD_FWD))
def test_bias_residual_add_rejects(ext, bad):
    a = _fwd_args()
    BAD_FWD[bad](a)
    with pytest.raises(RuntimeError):
        ext.bias_residual_add(a["y"], a["bias"], a["residual"])
    torch.cuda.synchronize()


def test_layernorm_fwd_rejects_hidden_above_8192(ext):
    with pytest.raises(RuntimeError):
        ext.layernorm_fwd(_z(R_, 8200), _z(8200, dtype=torch.float32),
                          _z(8200, dtype=torch.float32), EPS)
    torch.cuda.synchronize()


# --- backward -------------------------------------------------------------
def _dres(rows, h, seed=0):
    g = torch.Generator("cuda").manual_seed(seed + rows * 131 + h)
    return torch.randn(rows, h, generator=g, device="cuda").to(BF16)


def _colsum_ratio(colsum, g):
    rows = g.size(0)
    gd = g.double()
    bound = rows * 2.0 ** -24 * gd.abs().sum(0)
    return nb.sum_ratio(colsum, gd.sum(0), bound)


@pytest.mark.parametrize("rows,h", BWD_SHAPES)
def test_layernorm_bwd_add(ext, rows, h):
    for kind in nb.KINDS:
        dy, x, gamma, mean, rstd = nb.bwd_input(rows, h, kind, False,
                                                device="cuda")
        dres = _dres(rows, h)
        dx, dgamma, dbeta = ext.layernorm_bwd(dy, x, gamma, mean, rstd)
        g, dgamma_a, dbeta_a, colsum = ext.layernorm_bwd_add(
            dy, dres, x, gamma, mean, rstd, True)
        what = (rows, h, kind)
        assert g.dtype == BF16 and g.shape == x.shape
        assert colsum.dtype == torch.float32 and colsum.shape == (h,)
        assert torch.equal(g, dres + dx), what
        assert torch.equal(dgamma_a, dgamma), what
        assert torch.equal(dbeta_a, dbeta), what
        if rows <= SUM_BOUND_MAX_ROWS:
            ratio = _colsum_ratio(colsum, g)
            print(f"RATIO ln add colsum {rows}x{h} {kind}: {ratio:.3f}")
            assert ratio <= 1.0, what

        if kind != "dy_xhat_off":
            continue
        again = ext.layernorm_bwd_add(dy, dres, x, gamma, mean, rstd, True)
        for a, b in zip((g, dgamma_a, dbeta_a, colsum), again):
            assert torch.equal(a, b), what       # a repeated run: same bits
        no_sum = ext.layernorm_bwd_add(dy, dres, x, gamma, mean, rstd, False)
        assert no_sum[3].numel() == 0
        assert torch.equal(no_sum[0], g) and torch.equal(no_sum[1], dgamma)


@pytest.mark.parametrize(
    "rows,h,shifted",
    [(r, h, False) for r, h in BWD_SHAPES]
    + [(33, 512, True), (12293, 2560, True), (257, 8192, True)])
def test_layernorm_bwd_add_exact(ext, rows, h, shifted):
    """colsum equals the float64 column sum bitwise (module docstring);
    shifted: x in {-1, 3} with mean = 1 passed in."""
    dy, x, gamma, mean, rstd = nb.exact_case(rows, h, shifted, device="cuda")
    gen = torch.Generator("cuda").manual_seed(rows + h)
    k = torch.randint(0, 4, (rows, h), generator=gen, device="cuda")
    dres = (512.0 * torch.tensor([-2.0, -1.0, 1.0, 2.0], device="cuda")[k])
    dres = dres.to(BF16)
    dx, dgamma, dbeta = ext.layernorm_bwd(dy, x, gamma, mean, rstd)
    assert float(dx.float().abs().max()) < 16.0
    g, dgamma_a, dbeta_a, colsum = ext.layernorm_bwd_add(
        dy, dres, x, gamma, mean, rstd, True)
    assert torch.equal(g, dres + dx)
    assert float(g.float().abs().min()) >= 496.0
    assert torch.equal(dgamma_a, dgamma) and torch.equal(dbeta_a, dbeta)
    assert torch.equal(colsum.double(), g.double().sum(0))


BAD_DRES = {
    "dres_fp32": lambda d: d.float(),
    "dres_more_rows": lambda d: _z(d.size(0) + 1, d.size(1)),
    "dres_other_row_length": lambda d: _z(2 * d.size(0), d.size(1) // 2),
    "dres_strided": lambda d: _z(d.size(0), 2 * d.size(1))[:, ::2],
    "dres_cpu": lambda d: d.cpu(),
}


@pytest.mark.parametrize("bad", sorted(BAD_DRES))
def test_layernorm_bwd_add_rejects(ext, bad):
    dy, x, gamma, mean, rstd = nb.bwd_input(8, 512, "randn", False,
                                            device="cuda")
    dres = BAD_DRES[bad](_dres(8, 512))
    with pytest.raises(RuntimeError):
        ext.layernorm_bwd_add(dy, dres, x, gamma, mean, rstd, True)
    torch.cuda.synchronize()


def test_layernorm_bwd_add_rejects_what_layernorm_bwd_rejects(ext):
    dy, x, gamma, mean, rstd = nb.bwd_input(8, 512, "randn", False,
                                            device="cuda")
    dres = _dres(8, 512)
    for bad in (dict(rstd=rstd.double()), dict(mean=_z(9, dtype=torch.float32)),
                dict(gamma=_z(520, dtype=torch.float32)), dict(x=x.float())):
        a = dict(dy=dy, x=x, gamma=gamma, mean=mean, rstd=rstd)
        a.update(bad)
        with pytest.raises(RuntimeError):
            ext.layernorm_bwd_add(a["dy"], dres, a["x"], a["gamma"],
                                  a["mean"], a["rstd"], True)
    torch.cuda.synchronize()

"""One GPTBlock forward + backward with the fused bias / residual /
LayerNorm passes (METIS_FUSED_RESIDUAL unset) against the eager composition
(METIS_FUSED_RESIDUAL=0), on the default training path.

Bitwise equal in every case: the block output, fc2.weight.grad and
fc2.bias.grad (nothing in front of them changed its arithmetic).

Everything else in the backward lies downstream of dh, the GeLU backward.
The test finds out which of two cases holds, from h, da and aten's dh taken
out of the eager run, and prints it:

  dh bitwise aten's      the input gradient and every other weight and
                         LayerNorm gradient are bitwise equal too. The two
                         bias gradients that are now fp32 column sums in
                         another order, proj.bias.grad and fc1.bias.grad,
                         get, per column,
                           |got - base| <= ulp_bf16(max(|got|, |base|))
                                           + 2 * rows * 2^-24 * sum|term|
                         with `term` the rows of the summed gradient (both
                         sides round an fp32 sum of the same bf16 terms,
                         each within rows * 2^-24 * sum|term| of the exact
                         sum; two fp32 values that close round to bf16
                         values at most that far apart plus one ulp)
  dh not bitwise         (the case that holds on an MI355X: 36 of 524288
                         and 60 of 655360 dh values differ from aten's;
                         worst ratio below 0.613, qkv.weight at H = 640)
                         all of those take the project
                         criterion per 256 columns against a float64 copy
                         of the block, with the eager run as baseline:
                           max|got - ref| <= 2 max|base - ref|
                                             + 2^-8 max|ref|

The fused block also runs once under torch.utils.checkpoint (non-reentrant)
and must give the bits of the plain fused run.
"""

import copy

import pytest
import torch
import torch.utils.checkpoint

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import elementwise_conformance as ec
    from metis_amd.models.gpt import GPTBlock, GPTModelSpec
    from metis_amd.ops import require_extension
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
B, S = 2, 128
CONFIGS = [(512, 4), (640, 8)]       # (H, heads): D = 128 and D = 80
ALWAYS_BITWISE = ("fc2.weight", "fc2.bias")
REORDERED_BIAS = ("proj.bias", "fc1.bias")


def _make(h, heads):
    torch.manual_seed(h)
    spec = GPTModelSpec("t", h, 1, heads, 1024, S)
    block = GPTBlock(spec, 1, BF16).cuda()
    with torch.no_grad():                    # biases and norms off their init
        for name, p in block.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(B, S, h, device="cuda").to(BF16)
    dout = torch.randn(B, S, h, device="cuda").to(BF16)
    return block, x, dout


def _run(block, x, dout, checkpoint=False):
    """(out, dx, {name: grad})."""
    block.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    if checkpoint:
        out = torch.utils.checkpoint.checkpoint(block, xi, None, False,
                                                use_reentrant=False)
    else:
        out = block(xi, None)
    out.backward(dout.to(out.dtype))
    grads = {n: p.grad.clone() for n, p in block.named_parameters()}
    return out.detach(), xi.grad.clone(), grads


def _eager_with_taps(block, x, dout):
    """The eager run, keeping h with its gradient (aten's dh), da, and the
    gradient of proj's output (the rows proj.bias.grad sums)."""
    taps = {}

    def keep(name):
        def hook(_mod, _inp, out):
            out.retain_grad()
            taps[name] = out
        return hook

    def keep_input(_mod, inp):
        inp[0].retain_grad()
        taps["a"] = inp[0]

    handles = [block.fc1.register_forward_hook(keep("h")),
               block.proj.register_forward_hook(keep("proj_out")),
               block.fc2.register_forward_pre_hook(keep_input)]
    try:
        res = _run(block, x, dout)
    finally:
        for hd in handles:
            hd.remove()
    return res, taps


def _ulp_bf16(v):
    return torch.ldexp(torch.ones_like(v),
                       torch.floor(torch.log2(v.clamp_min(2.0 ** -126))).int()
                       - 7)


@pytest.mark.parametrize("h,heads", CONFIGS)
def test_fused_block_matches_eager(monkeypatch, h, heads):
    ext = require_extension()
    block, x, dout = _make(h, heads)

    monkeypatch.setenv("METIS_FUSED_RESIDUAL", "0")
    (out0, dx0, g0), taps = _eager_with_taps(block, x, dout)
    monkeypatch.setenv("METIS_FUSED_RESIDUAL", "1")
    out1, dx1, g1 = _run(block, x, dout)

    assert torch.equal(out1, out0)
    for name in ALWAYS_BITWISE:
        assert torch.equal(g1[name], g0[name]), name

    hh, da = taps["h"].detach(), taps["a"].grad
    dh_aten = taps["h"].grad
    dh = ext.gelu_tanh_bwd_bgrad(hh.contiguous(), da.contiguous())[0]
    dh_bitwise = torch.equal(dh, dh_aten)
    print(f"CASE H={h}: dh bitwise aten's: {dh_bitwise} "
          f"({int((dh != dh_aten).sum())} of {dh.numel()} differ)")
    rest = [n for n in g0 if n not in ALWAYS_BITWISE + REORDERED_BIAS]

    if dh_bitwise:
        assert torch.equal(dx1, dx0)
        for name in rest:
            assert torch.equal(g1[name], g0[name]), name
        terms = {"proj.bias": taps["proj_out"].grad, "fc1.bias": dh_aten}
        for name in REORDERED_BIAS:
            t = terms[name].double().reshape(-1, g0[name].numel())
            got, base = g1[name].double(), g0[name].double()
            tol = (_ulp_bf16(torch.maximum(got.abs(), base.abs()))
                   + 2 * t.size(0) * 2.0 ** -24 * t.abs().sum(0))
            assert bool(((got - base).abs() <= tol).all()), name
        return

    ref_block = copy.deepcopy(block).double()
    monkeypatch.setenv("METIS_FUSED_RESIDUAL", "0")
    _, dxr, gr = _run(ref_block, x.double(), dout.double())
    worst = {}
    for name, got, base, ref in (
            [("dx", dx1, dx0, dxr)]
            + [(n, g1[n], g0[n], gr[n]) for n in rest + list(REORDERED_BIAS)]):
        cols = got.size(-1)
        worst[name] = ec.block_ratio(got.reshape(-1, cols),
                                     base.reshape(-1, cols),
                                     ref.reshape(-1, cols),
                                     ec.COL_BLOCK, ec.ULP_BF16)
        print(f"RATIO fused block H={h} {name}: {worst[name]:.3f}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("h,heads", CONFIGS)
def test_fused_block_under_checkpoint(monkeypatch, h, heads):
    monkeypatch.setenv("METIS_FUSED_RESIDUAL", "1")
    block, x, dout = _make(h, heads)
    out, dx, g = _run(block, x, dout)
    out_c, dx_c, g_c = _run(block, x, dout, checkpoint=True)
    assert torch.equal(out_c, out) and torch.equal(dx_c, dx)
    for name in g:
        assert torch.equal(g_c[name], g[name]), name


def test_fused_path_is_taken(monkeypatch):
    """The fused Functions are in the graph by default and absent with
    METIS_FUSED_RESIDUAL=0."""
    block, x, _ = _make(512, 4)
    xi = x.clone().requires_grad_(True)
    monkeypatch.setenv("METIS_FUSED_RESIDUAL", "1")
    assert "BiasResidualAdd" in type(block(xi, None).grad_fn).__name__
    monkeypatch.setenv("METIS_FUSED_RESIDUAL", "0")
    assert "BiasResidualAdd" not in type(block(xi, None).grad_fn).__name__

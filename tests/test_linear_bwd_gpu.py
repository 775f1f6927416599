"""Linear backward GEMMs: the three hipBLASLt entries of lt_gemm.cpp
(lt_linear_dgrad_tn, lt_linear_dgrad, lt_linear_wgrad) and the table-routed
``metis_amd.ops.linear.linear``.

Shapes (dy [M,N], w [N,K], x [M,K]): M in {8, 136, 1032}, N and K in
{8, 264, 2568}, a subset of the product in which every size stands in every
position, plus M = 4104 so that the weight gradient's contraction crosses
many K tiles.

* Exact: x, w, dy are integers in -4..4, so every product and every fp32
  partial sum is exact (|sum| <= 16 * 4104 < 2^24) in any summation order;
  dx and dw must equal the float64 product rounded to bf16, bitwise. This is
  what sees a wrong transposition, a swapped operand or a wrong leading
  dimension.
* Criterion: on randn inputs, per (row, 256 columns),
  max|got - ref| <= 2 max|base - ref| + 2^-8 max|ref| with ref the float64
  product and base the aten bf16 matmul.
* Staleness of the transposed weight copy: after weight.data.add_, after
  FusedAdamW.step (all-bf16 flat buffer, and bf16 + fp32 parameters) and
  after load_state_dict (module and optimizer) the next forward/backward
  gives the dx of the new weight, bitwise; a repeated backward of one
  forward does not rebuild the copy (counted, not timed).
* Argument checks raise before any launch.

The tests build their own tables; none reads the committed one.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from elementwise_conformance import COL_BLOCK, ULP_BF16, block_ratio
    from metis_amd.models.gpt import ColumnParallelLinear
    from metis_amd.ops import FusedAdamW, require_extension
    from metis_amd.ops import linear as L
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
SHAPES = [(8, 8, 264), (8, 264, 2568), (136, 2568, 8), (136, 264, 264),
          (1032, 8, 2568), (1032, 2568, 264), (1032, 264, 8),
          (4104, 264, 264)]


@pytest.fixture(scope="module")
def ext():
    return require_extension()


def _ints(gen, *shape):
    return torch.randint(-4, 5, shape, device="cuda", generator=gen).to(BF16)


_CASES = {}


def case(M, N, K):
    """Integer and randn operands of one shape with their float64 and aten
    results, computed once per module."""
    key = (M, N, K)
    if key not in _CASES:
        g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
        c = {}
        for kind in ("int", "randn"):
            if kind == "int":
                dy, w, x = _ints(g, M, N), _ints(g, N, K), _ints(g, M, K)
            else:
                dy, w, x = (torch.randn(*s, device="cuda", generator=g).to(BF16)
                            for s in ((M, N), (N, K), (M, K)))
            c[kind] = dict(
                dy=dy, w=w, x=x,
                dx_ref=dy.double() @ w.double(),
                dw_ref=dy.double().t() @ x.double(),
                dx_base=dy @ w, dw_base=dy.t() @ x)
        _CASES[key] = c
    return _CASES[key]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16),
                                              b.contiguous().view(torch.int16))


def table(*entries):
    return L.GemmTable(0, "test", {
        (op, M, N, K): (route, algo) for op, M, N, K, route, algo in entries})


def entries_under_test(ext, c):
    """name -> (dx or None, dw or None) callables for every entry/algorithm
    form: heuristic (-1) and an explicit index."""
    dy, w, x = c["dy"], c["w"], c["x"]
    M, N = dy.shape
    K = w.size(1)
    dgrad_algo = ext.lt_heuristic_algo("dgrad", M, N, K)
    wgrad_algo = ext.lt_heuristic_algo("wgrad", M, N, K)
    return {
        "dgrad_tn": ("dx", lambda: ext.lt_linear_dgrad_tn(
            dy, ext.transpose_bf16(w))),
        "dgrad": ("dx", lambda: ext.lt_linear_dgrad(dy, w, -1)),
        "dgrad_explicit": ("dx", lambda: ext.lt_linear_dgrad(dy, w, dgrad_algo)),
        "wgrad": ("dw", lambda: ext.lt_linear_wgrad(dy, x, -1)),
        "wgrad_explicit": ("dw", lambda: ext.lt_linear_wgrad(dy, x, wgrad_algo)),
    }


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_entries_exact(ext, M, N, K):
    c = case(M, N, K)["int"]
    for name, (out, fn) in entries_under_test(ext, c).items():
        assert same_bits(fn(), c[out + "_ref"].to(BF16)), name


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_entries_criterion(ext, M, N, K):
    c = case(M, N, K)["randn"]
    for name, (out, fn) in entries_under_test(ext, c).items():
        ratio = block_ratio(fn(), c[out + "_base"], c[out + "_ref"],
                            COL_BLOCK, ULP_BF16)
        print(f"{name} M={M} N={N} K={K} ratio={ratio:.3f}")
        assert ratio <= 1.0, name


ROUTES = [("aten", "aten"), ("lt", "lt"), ("lt_tn", "lt"), ("lt_tn", "aten")]


@pytest.mark.parametrize("dgrad_route,wgrad_route", ROUTES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_routes(ext, M, N, K, dgrad_route, wgrad_route):
    """linear() per route: forward bitwise F.linear; integer dx, dw and the
    bias gradient exact; randn within the criterion. The input is 3-d, as
    in the model."""
    t = table(("dgrad", M, N, K, dgrad_route, -1),
              ("wgrad", M, N, K, wgrad_route, -1))
    for kind in ("int", "randn"):
        c = case(M, N, K)[kind]
        x = c["x"].view(1, M, K).clone().requires_grad_()
        w = c["w"].clone().requires_grad_()
        b = torch.zeros(N, device="cuda", dtype=BF16, requires_grad=True)
        with L.use_table(t):
            y = L.linear(x, w, b)
            y.backward(c["dy"].view(1, M, N))
        assert same_bits(y, F.linear(x.detach(), w.detach(), b.detach()))
        assert same_bits(b.grad, c["dy"].sum(0, keepdim=True).view(N))
        assert x.grad.shape == x.shape and w.grad.shape == w.shape
        if kind == "int":
            assert same_bits(x.grad.view(M, K), c["dx_ref"].to(BF16))
            assert same_bits(w.grad, c["dw_ref"].to(BF16))
        else:
            assert block_ratio(x.grad.view(M, K), c["dx_base"], c["dx_ref"],
                               COL_BLOCK, ULP_BF16) <= 1.0
            assert block_ratio(w.grad, c["dw_base"], c["dw_ref"],
                               COL_BLOCK, ULP_BF16) <= 1.0


def test_linear_miss_is_aten_bitwise(ext):
    """A shape without an entry makes autograd's own calls."""
    M, N, K = 136, 264, 264
    c = case(M, N, K)["randn"]
    grads = []
    for fn in (L.linear, F.linear):
        x = c["x"].clone().requires_grad_()
        w = c["w"].clone().requires_grad_()
        b = torch.ones(N, device="cuda", dtype=BF16, requires_grad=True)
        with L.use_table(table(("dgrad", M + 8, N, K, "lt_tn", -1))):
            fn(x, w, b).backward(c["dy"])
        grads.append((x.grad, w.grad, b.grad))
    for a, b in zip(*grads):
        assert same_bits(a, b)


# --- staleness of the transposed copy ---------------------------------------
SM, SN, SK = 136, 264, 520


def _tn_table():
    return table(("dgrad", SM, SN, SK, "lt_tn", -1))


def _dx(layer, x, dy):
    x = x.clone().requires_grad_()
    with L.use_table(_tn_table()):
        layer(x, None).backward(dy)
    return x.grad


def _fresh_dx(ext, layer, dy):
    return ext.lt_linear_dgrad_tn(dy, layer.weight.detach().t().contiguous())


@pytest.fixture()
def layer_x_dy():
    g = torch.Generator(device="cuda").manual_seed(5)
    layer = ColumnParallelLinear(SK, SN, 1, BF16).cuda()
    with torch.no_grad():
        layer.weight.copy_(_ints(g, SN, SK))
    return layer, _ints(g, SM, SK), _ints(g, SM, SN)


def test_stale_after_data_add(ext, layer_x_dy):
    layer, x, dy = layer_x_dy
    before = _dx(layer, x, dy)
    assert same_bits(before, (dy.double() @ layer.weight.double()).to(BF16))
    layer.weight.data.add_(1.0)          # no version bump, no epoch bump
    after = _dx(layer, x, dy)
    assert same_bits(after, (dy.double() @ layer.weight.double()).to(BF16))
    assert not same_bits(after, before)


@pytest.mark.parametrize("mixed", [False, True])
def test_stale_after_fused_adamw_step(ext, layer_x_dy, mixed):
    """All-bf16 parameters live in one flat buffer that adamw_step writes
    behind autograd's back; with an fp32 parameter the step copies into each
    parameter instead."""
    layer, x, dy = layer_x_dy
    extra = torch.nn.Parameter(torch.ones(
        8, device="cuda", dtype=torch.float32 if mixed else BF16))
    opt = FusedAdamW(list(layer.parameters()) + [extra], lr=0.5)
    before = _dx(layer, x, dy)            # after the re-bind to the flat buffer
    assert same_bits(before, _fresh_dx(ext, layer, dy))
    for p in opt.params:
        p.grad = torch.ones_like(p)
    opt.step()
    after = _dx(layer, x, dy)
    assert same_bits(after, _fresh_dx(ext, layer, dy))
    assert not same_bits(after, before)


def test_stale_after_load_state_dict(ext, layer_x_dy):
    layer, x, dy = layer_x_dy
    opt = FusedAdamW(layer.parameters(), lr=0.5)
    before = _dx(layer, x, dy)
    state = {k: v.clone() for k, v in layer.state_dict().items()}
    state["weight"] = state["weight"] + 2.0
    layer.load_state_dict(state)
    after = _dx(layer, x, dy)
    assert same_bits(after, (dy.double() @ layer.weight.double()).to(BF16))
    assert not same_bits(after, before)
    # the optimizer's load advances the epoch: the copy is rebuilt even
    # though neither the version nor the pointer of the weight moved
    x2 = x.clone().requires_grad_()
    with L.use_table(_tn_table()):
        y = layer(x2, None)
        y.backward(dy, retain_graph=True)
        n = L.transpose_refreshes
        opt.load_state_dict(opt.state_dict())
        y.backward(dy)
    assert L.transpose_refreshes == n + 1


def test_copy_not_rebuilt_when_nothing_changed(ext, layer_x_dy):
    layer, x, dy = layer_x_dy
    x = x.clone().requires_grad_()
    with L.use_table(_tn_table()):
        y = layer(x, None)
        n = L.transpose_refreshes
        y.backward(dy, retain_graph=True)
        assert L.transpose_refreshes == n + 1
        first, x.grad = x.grad, None
        y.backward(dy)
        assert L.transpose_refreshes == n + 1
    assert same_bits(first, x.grad)
    # and the aten route never builds one
    x.grad = None
    n = L.transpose_refreshes
    with L.use_table(table()):
        layer(x, None).backward(dy)
    assert L.transpose_refreshes == n


# --- argument checks --------------------------------------------------------
def test_argument_checks(ext):
    z = lambda *s, dtype=BF16: torch.zeros(*s, device="cuda", dtype=dtype)
    with pytest.raises(RuntimeError, match="inner sizes"):
        ext.lt_linear_dgrad_tn(z(16, 24), z(8, 32))
    with pytest.raises(RuntimeError, match="inner sizes"):
        ext.lt_linear_dgrad(z(16, 24), z(32, 8), -1)
    with pytest.raises(RuntimeError, match="inner sizes"):
        ext.lt_linear_wgrad(z(16, 24), z(24, 8), -1)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.lt_linear_dgrad(z(16, 24), z(24, 8, dtype=torch.float32), -1)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.lt_linear_wgrad(z(16, 24, dtype=torch.float32), z(16, 8), -1)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.lt_linear_dgrad(z(16, 48)[:, ::2], z(24, 8), -1)
    with pytest.raises(RuntimeError, match="2-d"):
        ext.lt_linear_wgrad(z(2, 8, 24), z(16, 8), -1)
    with pytest.raises(RuntimeError, match="aligned"):
        ext.lt_linear_dgrad(z(16 * 24 + 1)[1:].view(16, 24), z(24, 8), -1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.lt_linear_dgrad(torch.zeros(16, 24, dtype=BF16), z(24, 8), -1)


def test_rejected_algorithm_raises(ext):
    c = case(136, 264, 264)["int"]
    with pytest.raises(RuntimeError, match="not supported"):
        ext.lt_linear_dgrad(c["dy"], c["w"], 2 ** 30)
    with pytest.raises(RuntimeError, match="not supported"):
        ext.lt_linear_wgrad(c["dy"], c["x"], 2 ** 30)
    # an index of the TN layout is not one of the NN layout
    tn = set(ext.lt_supported_algos("dgrad_tn", 136, 264, 264))
    nn = set(ext.lt_supported_algos("dgrad", 136, 264, 264))
    only_tn = sorted(tn - nn)
    assert only_tn
    with pytest.raises(RuntimeError, match="not supported"):
        ext.lt_linear_dgrad(c["dy"], c["w"], only_tn[0])

"""Weight gradient on transposed activations: the four hipBLASLt entries of
lt_gemm.cpp (lt_linear_wgrad_dyt, _xt, _xt_nn, _tn), the routes of
``metis_amd.ops.linear.linear`` that use them (``lt_dyt``, ``lt_xt``,
``lt_xt_nn``, ``lt_dyt_xt``) and ``transpose_bf16_out`` at tall shapes.

Shapes (dy [M,N], x [M,K], dw [N,K]): every size is 8 (one 16-byte chunk), an
odd multiple of 8 past one tile (264, 520), or past many tiles (2568); the
last shape contracts over M = 1032, no multiple of 256, so a k-loop has
several tiles and a tail.

* Exact: dy and x are integers in -4..4, so every product and every fp32
  partial sum is exact (|sum| <= 16 * 1032 < 2^24) in any summation order;
  dw must equal the float64 product rounded to bf16, bitwise, with the
  heuristic algorithm and with the first 8 indices lt_supported_algos lists
  for the layout (the cap only bounds the test's time).
* Criterion: on randn inputs, per (row, 256 columns),
  max|got - ref| <= 2 max|base - ref| + 2^-8 max|ref| with ref the float64
  product and base the bf16 eager ``dy.t() @ x``.
* Repeatability: three calls give the same bits.
* A table miss and METIS_LT_BWD=0 give ``dy.t() @ x`` bitwise.
* Scratch reuse: the transposed activation lives in a reused buffer; layers
  of different shapes back to back and a repeated backward give the bits of
  fresh runs.
* Argument checks raise before any launch.

The tests build their own tables; none reads the committed one.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from elementwise_conformance import COL_BLOCK, ULP_BF16, block_ratio
    from metis_amd.ops import require_extension
    from metis_amd.ops import linear as L
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
SHAPES = [(8, 8, 264), (8, 264, 2568), (136, 2568, 8), (136, 264, 264),
          (1032, 264, 520)]
MAX_ALGOS = 8

# route of linear() -> (problem name of lt_gemm.cpp, entry point)
ROUTES = {"lt_dyt": "wgrad_dyt", "lt_xt": "wgrad_xt",
          "lt_xt_nn": "wgrad_xt_nn", "lt_dyt_xt": "wgrad_tn"}


@pytest.fixture(scope="module")
def ext():
    return require_extension()


def _ints(gen, *shape):
    return torch.randint(-4, 5, shape, device="cuda", generator=gen).to(BF16)


_CASES = {}


def case(M, N, K):
    """Integer and randn operands of one shape, their transposes and the
    float64 and eager results, computed once per module."""
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
                dy=dy, w=w, x=x, dyt=dy.t().contiguous(),
                xt=x.t().contiguous(),
                dw_ref=dy.double().t() @ x.double(), dw_base=dy.t() @ x)
        _CASES[key] = c
    return _CASES[key]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16),
                                              b.contiguous().view(torch.int16))


def table(*entries):
    return L.GemmTable(0, "test", {
        (op, M, N, K): (route, algo) for op, M, N, K, route, algo in entries})


def entry(ext, c, problem, algo):
    """dw [N,K] through one entry point on pre-transposed operands."""
    if problem == "wgrad_dyt":
        return ext.lt_linear_wgrad_dyt(c["dyt"], c["x"], algo)
    if problem == "wgrad_xt":
        return ext.lt_linear_wgrad_xt(c["dy"], c["xt"], algo)
    if problem == "wgrad_xt_nn":
        dwt = ext.lt_linear_wgrad_xt_nn(c["dy"], c["xt"], algo)
        assert dwt.shape == (c["x"].size(1), c["dy"].size(1))
        return dwt.t().contiguous()
    return ext.lt_linear_wgrad_tn(c["dyt"], c["xt"], algo)


def algos(ext, problem, M, N, K):
    """-1, the heuristic's index and the first MAX_ALGOS supported ones."""
    listed = [int(a) for a in ext.lt_supported_algos(problem, M, N, K)]
    heur = int(ext.lt_heuristic_algo(problem, M, N, K))
    return [-1, heur] + listed[:MAX_ALGOS]


@pytest.mark.parametrize("problem", sorted(ROUTES.values()))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_entries_exact(ext, M, N, K, problem):
    c = case(M, N, K)["int"]
    want = c["dw_ref"].to(BF16)
    tried = algos(ext, problem, M, N, K)
    assert len(tried) > 2, "no supported algorithm listed"
    for algo in tried:
        assert same_bits(entry(ext, c, problem, algo), want), algo


@pytest.mark.parametrize("problem", sorted(ROUTES.values()))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_entries_criterion_and_repeatable(ext, M, N, K, problem):
    c = case(M, N, K)["randn"]
    for algo in algos(ext, problem, M, N, K):
        outs = [entry(ext, c, problem, algo) for _ in range(3)]
        assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]), algo
        ratio = block_ratio(outs[0], c["dw_base"], c["dw_ref"], COL_BLOCK,
                            ULP_BF16)
        print(f"{problem} algo={algo} M={M} N={N} K={K} ratio={ratio:.3f}")
        assert ratio <= 1.0, algo


def _backward(c, t, M, N, K):
    """One forward and backward of linear() under table ``t``; the input is
    3-d, as in the model."""
    x = c["x"].view(1, M, K).clone().requires_grad_()
    w = c["w"].clone().requires_grad_()
    b = torch.zeros(N, device="cuda", dtype=BF16, requires_grad=True)
    with L.use_table(t):
        y = L.linear(x, w, b)
        y.backward(c["dy"].view(1, M, N))
    return y, x, w, b


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_routes(ext, M, N, K, route):
    """linear() per wgrad route, with the heuristic and with an explicit
    index: forward bitwise F.linear; integer dw, dx and the bias gradient
    exact; randn within the criterion and the same bits over three calls."""
    explicit = int(ext.lt_supported_algos(ROUTES[route], M, N, K)[0])
    for algo in (-1, explicit):
        t = table(("wgrad", M, N, K, route, algo))
        for kind in ("int", "randn"):
            c = case(M, N, K)[kind]
            y, x, w, b = _backward(c, t, M, N, K)
            assert same_bits(y, F.linear(x.detach(), w.detach(), b.detach()))
            assert same_bits(b.grad, c["dy"].sum(0, keepdim=True).view(N))
            assert same_bits(x.grad.view(M, K), c["dy"] @ c["w"])
            assert w.grad.shape == w.shape
            if kind == "int":
                assert same_bits(w.grad, c["dw_ref"].to(BF16))
            else:
                assert block_ratio(w.grad, c["dw_base"], c["dw_ref"],
                                   COL_BLOCK, ULP_BF16) <= 1.0
                for _ in range(2):
                    assert same_bits(_backward(c, t, M, N, K)[2].grad, w.grad)


def test_linear_miss_and_switch_are_aten_bitwise(ext, monkeypatch):
    """A shape without an entry, and METIS_LT_BWD=0 with an entry, make
    autograd's own calls."""
    M, N, K = 136, 264, 264
    c = case(M, N, K)["randn"]
    want = c["dy"].t() @ c["x"]
    miss = table(("wgrad", M + 8, N, K, "lt_xt", -1))
    assert same_bits(_backward(c, miss, M, N, K)[2].grad, want)
    hit = table(("wgrad", M, N, K, "lt_xt", -1))
    monkeypatch.setenv("METIS_LT_BWD", "0")
    y, x, w, b = _backward(c, hit, M, N, K)
    assert type(y.grad_fn).__name__ != "_LinearBackward"
    assert same_bits(w.grad, want)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_scratch_reuse(ext, route):
    """Two layers of different shapes back to back, then a second backward
    of the first layer's graph: each dw has the bits of a run on its own, so
    no call read a transposed activation another call left behind."""
    A, B = (1032, 264, 520), (136, 2568, 8)
    ca, cb = case(*A)["randn"], case(*B)["randn"]
    t = table(("wgrad", *A, route, -1), ("wgrad", *B, route, -1))
    fresh_a = _backward(ca, t, *A)[2].grad
    L._scratch.clear()
    fresh_b = _backward(cb, t, *B)[2].grad
    L._scratch.clear()

    xa = ca["x"].clone().requires_grad_()
    wa = ca["w"].clone().requires_grad_()
    with L.use_table(t):
        ya = L.linear(xa, wa)
        ya.backward(ca["dy"], retain_graph=True)
        first, wa.grad = wa.grad, None
        second_layer = _backward(cb, t, *B)[2].grad
        ya.backward(ca["dy"])
    assert same_bits(first, fresh_a)
    assert same_bits(second_layer, fresh_b)
    assert same_bits(wa.grad, fresh_a)
    # one buffer per operand that the route transposes, sized by the largest
    assert len(L._scratch) == (2 if route == "lt_dyt_xt" else 1)


def test_argument_checks(ext):
    z = lambda *s, dtype=BF16: torch.zeros(*s, device="cuda", dtype=dtype)
    # (entry, good first operand, good second operand) at M 16, N 24, K 8
    entries = [(ext.lt_linear_wgrad_dyt, (24, 16), (16, 8), ((24, 32), (16, 8))),
               (ext.lt_linear_wgrad_xt, (16, 24), (8, 16), ((16, 24), (8, 32))),
               (ext.lt_linear_wgrad_xt_nn, (16, 24), (8, 16),
                ((32, 24), (8, 16))),
               (ext.lt_linear_wgrad_tn, (24, 16), (8, 16), ((24, 16), (8, 32)))]
    for fn, sa, sb, (bad_a, bad_b) in entries:
        assert fn(z(*sa), z(*sb), -1).shape in ((24, 8), (8, 24))
        with pytest.raises(RuntimeError, match="inner sizes"):
            fn(z(*bad_a), z(*bad_b), -1)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(z(sa[0], 2 * sa[1])[:, ::2], z(*sb), -1)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(z(*sa), z(sb[1], sb[0]).t(), -1)
        with pytest.raises(RuntimeError, match="bf16"):
            fn(z(*sa, dtype=torch.float32), z(*sb), -1)
        with pytest.raises(RuntimeError, match="bf16"):
            fn(z(*sa), z(*sb, dtype=torch.float32), -1)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(torch.zeros(*sa, dtype=BF16), z(*sb), -1)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(z(*sa), torch.zeros(*sb, dtype=BF16), -1)
        with pytest.raises(RuntimeError, match="2-d"):
            fn(z(1, *sa), z(*sb), -1)
        with pytest.raises(RuntimeError, match="aligned"):
            fn(z(sa[0] * sa[1] + 1)[1:].view(*sa), z(*sb), -1)
        with pytest.raises(RuntimeError, match="not supported"):
            fn(z(*sa), z(*sb), 2 ** 30)
    with pytest.raises(RuntimeError, match="unknown op"):
        ext.lt_supported_algos("wgrad_nt", 16, 24, 8)


def _pattern(R, C):
    """Every element names its own position (mod 2^16): a misplaced chunk or
    a stale one from another matrix cannot match."""
    i = torch.arange(R * C, device="cuda", dtype=torch.int32)
    return (i * 7 + 3).to(torch.int16).view(R, C).view(BF16)


@pytest.mark.parametrize("R,C", [(1032, 264), (4104, 8), (8, 4104)])
def test_transpose_tall(ext, R, C):
    w = _pattern(R, C)
    want = w.t().contiguous()
    out = torch.empty(C, R, device="cuda", dtype=BF16)
    ext.transpose_bf16_out(w, out)
    assert same_bits(out, want)
    # into the head of a buffer that held a larger matrix's transpose
    big = _pattern(R + 64, C + 8)
    buf = torch.empty(big.numel(), device="cuda", dtype=BF16)
    ext.transpose_bf16_out(big, buf.view(C + 8, R + 64))
    tail = buf[R * C:].clone()
    ext.transpose_bf16_out(w, buf[:R * C].view(C, R))
    assert same_bits(buf[:R * C].view(C, R), want)
    assert same_bits(buf[R * C:], tail)      # and nothing past its own end

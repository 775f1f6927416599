"""GPU tests of the fp8 weight-only decode linear (w8_linear.hip), its
Python routing (ops/w8.py) and the quantised serving path.

Exact-integer test: data on which every term and every partial sum is an
exact fp32 integer and every result is exact in bf16 (the preconditions
are asserted, on the float64 reference), so the kernel must be BITWISE
equal to the reference whatever its summation order: any indexing, tail
or number-format slip changes at least one output.

Random data: the project's criterion (tests/attn_conformance.py), per
(row m, 64-column block):
    max|got - ref| <= 2 * max|base - ref| + 2**-8 * max|ref|
with ref the formula in float64 and base the same formula in bf16 eager
on the device. tests/w8_support.py holds cases, reference and criterion.
"""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from metis_amd.ops import require_extension
else:  # collected but skipped on CPU
    pytest.skip("requires MI355X GPU", allow_module_level=True)

import w8_support as ws
from metis_amd.models.llama import LlamaModel, LLAMA_SPECS
from metis_amd.ops.w8 import W8Linear, quantize_weight_e4m3, w8_linear
from metis_amd.runtime import generate as gen
from metis_amd.runtime.quantize import quantize_for_decode

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    return require_extension()


def _dev(*ts):
    return [t.to(DEV) for t in ts]


# --- exact integers: bitwise ------------------------------------------------
@pytest.mark.parametrize("M", ws.MS)
@pytest.mark.parametrize("K,N", ws.INT_SHAPES)
def test_exact_integer_bitwise(ext, K, N, M):
    ws.check_integer_preconditions(M, K, N)
    x, w8, scale, bias, ref = ws.integer_case(M, K, N)
    xd, wd, sd, bd = _dev(x, w8, scale, bias)
    want = ref.to(torch.bfloat16)
    for ns in ws.split_values(K):
        y = ext.w8_linear(xd, wd, sd, bd, ns)
        assert y.shape == (M, N) and y.dtype == torch.bfloat16
        bad = (y.cpu().view(torch.int16) != want.view(torch.int16))
        assert not bad.any(), (
            f"num_splits={ns}: {int(bad.sum())} wrong, first at "
            f"{bad.nonzero()[0].tolist()}")
    y = ext.w8_linear(xd, wd, sd, None, 0)          # bias is optional
    assert torch.equal(y.cpu().double(), ref - bias.double())


# --- random data: the criterion ---------------------------------------------
def _criterion(fn, M, K, N, variant):
    x, w8, scale, bias = ws.random_case(M, K, N, variant)
    xd, wd, sd, bd = _dev(x, w8, scale, bias)
    ref = ws.reference_fp64(xd, wd, sd, bd)
    base = ws.baseline_bf16(xd, wd, sd, bd)
    return ws.worst_ratio(fn(xd, wd, sd, bd), base, ref)


@pytest.mark.parametrize("M", ws.RANDOM_MS)
@pytest.mark.parametrize("K,N", ws.RANDOM_SHAPES)
def test_random_criterion(ext, K, N, M):
    worst = {}
    for ns in ws.split_values(K):
        r = _criterion(lambda x, w, s, b: ext.w8_linear(x, w, s, b, ns),
                       M, K, N, "plain")
        worst[ns] = round(r, 3)
    print(f"K={K} N={N} M={M}: worst ratio per num_splits {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("variant", ["x8", "row100"])
@pytest.mark.parametrize("K,N", ws.RANDOM_SHAPES)
def test_random_criterion_scaled_inputs(ext, K, N, variant):
    r = _criterion(lambda x, w, s, b: ext.w8_linear(x, w, s, b), 4, K, N,
                   variant)
    print(f"K={K} N={N} {variant}: worst ratio {r:.3f}")
    assert r <= 1.0, r


# --- batch invariance, determinism ------------------------------------------
@pytest.mark.parametrize("M", [2, 5, 16])
@pytest.mark.parametrize("K,N", [(768, 250), (8192, 2048)])
def test_batch_invariance_bitwise(ext, K, N, M):
    x, w8, scale, bias = _dev(*ws.random_case(16, K, N, "plain"))
    x = x[:M].contiguous()
    full = ext.w8_linear(x, w8, scale, bias)
    for m in range(M):
        alone = ext.w8_linear(x[m:m + 1].contiguous(), w8, scale, bias)
        assert torch.equal(full[m], alone[0]), m
        poisoned = torch.full_like(x, float("nan"))
        poisoned[m] = x[m]
        assert torch.equal(ext.w8_linear(poisoned, w8, scale, bias)[m],
                           full[m]), m


def test_repeated_call_bitwise_equal(ext):
    x, w8, scale, bias = _dev(*ws.random_case(4, 8192, 2048, "plain"))
    for ns in (0, 1, 3):
        a = ext.w8_linear(x, w8, scale, bias, ns)
        b = ext.w8_linear(x, w8, scale, bias, ns)
        assert torch.equal(a, b), ns


# --- never reads past M, N, K -----------------------------------------------
@pytest.mark.parametrize("M,K,N", [(3, 80, 17), (13, 2560, 33),
                                   (16, 1040, 64), (5, 14336, 250)])
def test_nan_guard_around_every_operand(ext, M, K, N):
    """x is the first M rows of a larger NaN-filled buffer; w8 and scale
    are contiguous slices at the start of larger NaN-filled allocations: a
    read past row M-1 of x, or past the end of w8 / scale, poisons the
    output."""
    x, w8, scale, bias = ws.random_case(M, K, N, "plain")
    xbuf = torch.full((M + 16, K), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    xbuf[:M] = x.to(DEV)
    wbuf = torch.full((N + 64, K), float("nan"), device=DEV,
                      dtype=torch.float32).to(torch.float8_e4m3fn)
    assert torch.isnan(wbuf[N:].float()).all()
    wbuf.view(torch.uint8)[:N] = w8.to(DEV).view(torch.uint8)
    sbuf = torch.full((N + 64,), float("nan"), device=DEV)
    sbuf[:N] = scale.to(DEV)
    bbuf = torch.full((N + 64,), float("nan"), device=DEV,
                      dtype=torch.bfloat16)
    bbuf[:N] = bias.to(DEV)
    xv, wv, sv, bv = xbuf[:M], wbuf[:N], sbuf[:N], bbuf[:N]
    assert xv.is_contiguous() and wv.is_contiguous()
    clean = ext.w8_linear(*_dev(x, w8, scale, bias))
    for ns in ws.split_values(K):
        y = ext.w8_linear(xv, wv, sv, bv, ns)
        assert torch.isfinite(y).all(), ns
        if ns == 0:
            assert torch.equal(y, clean)


# --- launcher rejections ----------------------------------------------------
def test_launcher_rejections_leave_the_device_usable(ext):
    x, w8, scale, bias = _dev(*ws.random_case(4, 768, 250, "plain"))
    good = ext.w8_linear(x, w8, scale, bias)
    bf = torch.bfloat16
    bad_calls = {
        "M=0": lambda: ext.w8_linear(x[:0], w8, scale, bias),
        "M=17": lambda: ext.w8_linear(x.new_zeros(17, 768), w8, scale, bias),
        "x fp32": lambda: ext.w8_linear(x.float(), w8, scale, bias),
        "w8 bf16": lambda: ext.w8_linear(x, w8.to(bf), scale, bias),
        "w8 fnuz": lambda: ext.w8_linear(
            x, w8.view(torch.float8_e4m3fnuz), scale, bias),
        "K%16": lambda: ext.w8_linear(
            x[:, :760].contiguous(), w8[:, :760].contiguous(), scale, bias),
        "K mismatch": lambda: ext.w8_linear(
            x[:, :512].contiguous(), w8, scale, bias),
        "x strided": lambda: ext.w8_linear(x[:, ::2], w8[:, :384].contiguous(),
                                           scale, bias),
        "w8 strided": lambda: ext.w8_linear(x[:, :384].contiguous(),
                                            w8[:, ::2], scale, bias),
        "scale short": lambda: ext.w8_linear(x, w8, scale[:-1], bias),
        "scale bf16": lambda: ext.w8_linear(x, w8, scale.to(bf), bias),
        "bias short": lambda: ext.w8_linear(x, w8, scale, bias[:-1]),
        "bias fp32": lambda: ext.w8_linear(x, w8, scale, bias.float()),
        "scale on cpu": lambda: ext.w8_linear(x, w8, scale.cpu(), bias),
        "w8 on cpu": lambda: ext.w8_linear(x, w8.cpu(), scale, bias),
        "splits<0": lambda: ext.w8_linear(x, w8, scale, bias, -1),
        "splits>K/16": lambda: ext.w8_linear(x, w8, scale, bias, 49),
    }
    for name, call in bad_calls.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name} was accepted")
        assert torch.equal(ext.w8_linear(x, w8, scale, bias), good), name
    assert ext.w8_linear(x, w8, scale, bias, 48).shape == (4, 250)


# --- wrapper routing --------------------------------------------------------
class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


@pytest.fixture
def spy(ext, monkeypatch):
    s = _Spy(ext.w8_linear)
    monkeypatch.setattr(ext, "w8_linear", s)
    monkeypatch.delenv("METIS_W8_KERNEL", raising=False)
    return s


def test_wrapper_routing(spy, monkeypatch):
    K, N = 768, 250
    for M, calls in ((16, 1), (17, 1), (64, 1)):
        r = _criterion(w8_linear, M, K, N, "plain")
        print(f"wrapper M={M}: worst ratio {r:.3f}")
        assert r <= 1.0, (M, r)
        assert spy.calls == calls, M         # only M <= 16 runs the kernel

    x, w8, scale, bias = _dev(*ws.random_case(8, K, N, "plain"))
    y = w8_linear(x.reshape(8, 1, K), w8, scale, bias)
    assert y.shape == (8, 1, N) and spy.calls == 2
    assert torch.equal(y[:, 0], spy.fn(x, w8, scale, bias))
    odd = torch.zeros(8 * K + 8, device=DEV, dtype=torch.bfloat16)
    odd[3:3 + 8 * K] = x.reshape(-1)         # 6-byte offset: misaligned view
    y2 = w8_linear(odd[3:3 + 8 * K].view(8, K), w8, scale, bias)
    assert torch.equal(y2, y[:, 0]) and spy.calls == 3

    monkeypatch.setenv("METIS_W8_KERNEL", "0")
    r = _criterion(w8_linear, 8, K, N, "plain")
    assert r <= 1.0 and spy.calls == 3       # eager arm, kernel not called


# --- end to end -------------------------------------------------------------
PROMPTS = ((5, 9, 3), (7, 11, 13))


def _prefill_and_one_step(model, device, monkeypatch):
    """Three requests through ContinuousBatcher: one prefill each, then ONE
    ragged decode step with the fed tokens pinned, so every arm decodes the
    same inputs. Returns the step's logits [3, vocab] in fp32 on the CPU."""
    g = torch.Generator().manual_seed(11)
    vocab = model.spec.vocab_size
    prompts = [torch.randint(0, vocab, (n,), generator=g).tolist()
               for n in PROMPTS[0]]
    fed = iter(PROMPTS[1])
    monkeypatch.setattr(
        gen, "_sample",
        lambda last, *a, **kw: torch.tensor([[next(fed)]], device=last.device))
    with torch.no_grad():
        cb = gen.ContinuousBatcher(model, capacity=32, max_batch=3,
                                   device=device)
        for p in prompts:
            cb.submit(p, 4, temperature=0.0)
        cb.step()
    return torch.stack([cb._last_logits[s] for s in range(3)]).float().cpu()


def test_quantised_llama_end_to_end(spy, monkeypatch):
    torch.manual_seed(0)
    spec = LLAMA_SPECS["llama-tiny"]
    original = LlamaModel(spec, dtype=torch.bfloat16).eval()
    qmodel = quantize_for_decode(copy.deepcopy(original))
    twin = copy.deepcopy(original).float()          # fp32, dequantised, CPU
    mods = dict(twin.named_modules())
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if isinstance(m, W8Linear):
                mods[name].weight.copy_(m.w8.float() * m.scale[:, None])
    qmodel = qmodel.to(DEV)
    assert qmodel.head.w8.dtype == torch.float8_e4m3fn

    kern = _prefill_and_one_step(qmodel, DEV, monkeypatch)
    # 4 linears per block + head, for 3 prefills (M = 5, 9, 3) + 1 decode
    assert spy.calls == 4 * (4 * spec.num_layers + 1)
    monkeypatch.setenv("METIS_W8_KERNEL", "0")
    eager = _prefill_and_one_step(qmodel, DEV, monkeypatch)
    assert spy.calls == 4 * (4 * spec.num_layers + 1)
    ref = _prefill_and_one_step(twin, None, monkeypatch)

    assert torch.isfinite(kern).all()
    err_k = (kern - ref).abs().amax(1)
    err_e = (eager - ref).abs().amax(1)
    bound = 2 * err_e + 2.0 ** -8 * ref.abs().amax(1)
    print(f"per-row logit err vs fp32 dequantised twin: kernel "
          f"{err_k.tolist()}, eager arm {err_e.tolist()}, "
          f"bound {bound.tolist()}")
    assert (err_k <= bound).all()

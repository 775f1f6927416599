"""References, yardsticks, criterion and kernel emulations for the cross
entropy, AdamW, LayerNorm/RMSNorm forward, RoPE and SwiGLU kernel tests.

Plain test support (not a conftest): imported by
test_elementwise_conformance_cpu.py and test_elementwise_conformance_gpu.py.
References and baselines run on whatever device the inputs live on; the
emulations are CPU fp32.

Per operation:
  *_reference   the documented formula in float64
  *_baseline    the same formula at the output's precision in eager torch:
                bf16 tensors for bf16 outputs, fp32 for fp32 outputs (lse,
                per-row loss, mean, rstd, AdamW master/m/v)
  *_emulate     the kernel's arithmetic in fp32 in the kernel's own order
                (256-thread stride partials, 64-lane butterfly, 4 wave
                totals), __expf/__logf/rsqrtf stood in by fp32 exp/log/
                1/sqrt, with named mutants the criterion has to reject

Criterion (the project's own; attn_conformance.blockwise_ratio and
w8_support.worst_ratio are the same rule on [B,H,S,D] 16-row blocks and on
64-column blocks, block shapes that fit none of these outputs, so the rule
is restated here for a free block length):

    per block   max|got - ref| <= 2 * max|base - ref| + ulp * max|ref|
    ulp = 2**-8 for bf16 outputs, 2**-23 for fp32 outputs

Blocks: CE dlogits one per (row, 256 columns) with the target column in a
block of its own; norm y one per (row, 256 columns); RoPE one per (row,
half); SwiGLU and AdamW one per 2048 contiguous elements. The per-row fp32
outputs (lse, loss, mean, rstd) take one block per 256 consecutive rows:
one element's fp32 baseline can be exact by chance, which would turn the
rule into "within one ulp" for that row, a demand no other summation
order meets; over a block the baseline's error is a property of the
method.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

ULP_BF16 = 2.0 ** -8
ULP_FP32 = 2.0 ** -23
BLOCK = 256            # threads per workgroup of every kernel here
VEC = 8                # bf16 per lane per step
COL_BLOCK = 256
FLAT_BLOCK = 2048
ROW_BLOCK = 256
BF16 = torch.bfloat16


# --- criterion ------------------------------------------------------------
def _block_max(e: torch.Tensor, block: int) -> torch.Tensor:
    """max|e| over blocks of `block` along the last dim (zero padded)."""
    e = e.abs()
    pad = -e.size(-1) % block
    if pad:
        e = torch.cat([e, e.new_zeros(*e.shape[:-1], pad)], dim=-1)
    return e.reshape(*e.shape[:-1], -1, block).amax(-1)


def _ratio(eg, eb, r, ulp) -> float:
    bound = 2.0 * eb + ulp * r
    ratio = torch.where(eg == 0, torch.zeros_like(eg), eg / bound)
    ratio = torch.where(torch.isfinite(ratio), ratio,
                        torch.full_like(ratio, float("inf")))
    return float(ratio.max()) if ratio.numel() else 0.0


def block_ratio(got, base, ref, block: int, ulp: float) -> float:
    """Worst block of max|got-ref| / (2*max|base-ref| + ulp*max|ref|) with
    blocks of `block` along the last dim; <= 1 passes. A non-finite value
    in got gives inf; a block whose bound is zero passes only with zero
    error."""
    ref = ref.double()
    return _ratio(_block_max(got.double() - ref, block),
                  _block_max(base.double() - ref, block),
                  _block_max(ref, block), ulp)


def flat_ratio(got, base, ref, ulp: float, block: int = FLAT_BLOCK) -> float:
    return block_ratio(got.reshape(-1), base.reshape(-1), ref.reshape(-1),
                       block, ulp)


def row_ratio(got, base, ref) -> float:
    """Per-row fp32 outputs: one block per 256 consecutive rows."""
    return flat_ratio(got, base, ref, ULP_FP32, ROW_BLOCK)


def ce_dlogits_ratio(got, base, ref, labels) -> float:
    """(row, 256-column) blocks with the target column taken out into a
    block of its own, so the one-hot cannot hide the softmax term."""
    ref = ref.double()
    eg, eb, r = (got.double() - ref).abs(), (base.double() - ref).abs(), ref.abs()
    n, v = ref.shape
    valid = (labels >= 0) & (labels < v)
    rows = torch.arange(n, device=ref.device)[valid]
    cols = labels[valid]
    tgt = _ratio(eg[rows, cols], eb[rows, cols], r[rows, cols], ULP_BF16)
    eg, eb, r = eg.clone(), eb.clone(), r.clone()
    for t in (eg, eb, r):
        t[rows, cols] = 0
    rest = _ratio(_block_max(eg, COL_BLOCK), _block_max(eb, COL_BLOCK),
                  _block_max(r, COL_BLOCK), ULP_BF16)
    return max(tgt, rest)


# --- the kernels' block reduction, emulated -------------------------------
def _butterfly(p: torch.Tensor, op) -> torch.Tensor:
    """[..., 64] lane values -> lane 0 of the xor-butterfly (32, 16, .. 1)."""
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = op(p, p[..., lanes ^ off])
    return p[..., 0]


def block_reduce(partial: torch.Tensor, op=torch.add) -> torch.Tensor:
    """[rows, 256] per-thread fp32 partials -> [rows], in the order of
    common.h: butterfly inside each of the 4 waves, then the 4 wave totals
    through a butterfly of which only (t0 op t2) op (t1 op t3) matters."""
    w = _butterfly(partial.reshape(partial.size(0), 4, 64), op)
    return op(op(w[:, 0], w[:, 2]), op(w[:, 1], w[:, 3]))


def stride_partials(x: torch.Tensor, fn, init: float, op=torch.add,
                    full_strides_only=False, skip_tail=False) -> torch.Tensor:
    """Per-thread partials [rows, 256] of `fn(x)` over a row of L = 8*lv
    elements: thread t takes the 8-element chunks t, t+256, ... in turn and
    folds their elements in order. The two flags drop the last, partial
    stride (mutants)."""
    rows, length = x.shape
    lv = length // VEC
    acc = torch.full((rows, BLOCK), init, dtype=torch.float32)
    drop_tail = full_strides_only or skip_tail
    for j in range(0, lv, BLOCK):
        cnt = min(BLOCK, lv - j)
        if cnt < BLOCK and drop_tail:
            break
        chunk = fn(x[:, j * VEC:(j + cnt) * VEC].float()).reshape(rows, cnt, VEC)
        for k in range(VEC):
            acc[:, :cnt] = op(acc[:, :cnt], chunk[:, :, k])
    return acc


# --- cross entropy --------------------------------------------------------
def _valid(labels, v):
    return (labels >= 0) & (labels < v)


def ce_reference(logits, labels, grad_scale: float):
    """(loss [N], lse [N], dlogits [N,V]) in float64. A label outside
    [0, V) gives loss NaN and no one-hot (docs/KERNELS.md)."""
    x = logits.double()
    v = x.size(1)
    ok = _valid(labels, v)
    lse = torch.logsumexp(x, dim=-1)
    tl = x.gather(1, labels.clamp(0, v - 1)[:, None]).squeeze(1)
    loss = torch.where(ok, lse - tl, torch.full_like(lse, float("nan")))
    d = torch.exp(x - lse[:, None])
    rows = torch.arange(x.size(0), device=x.device)[ok]
    d[rows, labels[ok]] -= 1.0
    return loss, lse, d * float(grad_scale)


def ce_baseline(logits, labels, grad_scale: float):
    """loss and lse from fp32 eager torch; dlogits from bf16 tensors:
    (softmax(bf16) - onehot) * bf16(grad_scale)."""
    xf = logits.float()
    v = xf.size(1)
    ok = _valid(labels, v)
    lse = torch.logsumexp(xf, dim=-1)
    loss = F.cross_entropy(xf, labels.clamp(0, v - 1), reduction="none")
    loss = torch.where(ok, loss, torch.full_like(loss, float("nan")))
    d = torch.softmax(logits.to(BF16), dim=-1)
    rows = torch.arange(xf.size(0), device=xf.device)[ok]
    d[rows, labels[ok]] -= 1.0
    return loss, lse, d * torch.tensor(grad_scale, dtype=BF16, device=d.device)


CE_MUTANTS = ("bwd_no_softmax", "skip_last_partial_stride",
              "onehot_off_by_one", "ignore_grad_scale",
              "max_full_strides_only")


def ce_emulate_row_max(logits, mutant=None) -> torch.Tensor:
    """Row max as ce_fwd_kernel / row_max_kernel take it (idle threads keep
    -1e30)."""
    part = stride_partials(
        logits, lambda t: t, -1e30, torch.maximum,
        full_strides_only=mutant == "max_full_strides_only",
        skip_tail=mutant == "skip_last_partial_stride")
    return block_reduce(part, torch.maximum)


def ce_emulate(logits, labels, grad_scale: float, mutant=None):
    """(loss, lse, dlogits) of cross_entropy.hip in fp32, CPU."""
    assert mutant is None or mutant in CE_MUTANTS
    x = logits.float()
    n, v = x.shape
    skip = mutant == "skip_last_partial_stride"
    m = ce_emulate_row_max(logits, mutant)
    part = stride_partials(x, lambda t: torch.exp(t - m[:, None]), 0.0,
                           skip_tail=skip)
    ls = torch.log(block_reduce(part))
    lse = m + ls
    ok = _valid(labels, v)
    tl = x.gather(1, labels.clamp(0, v - 1)[:, None]).squeeze(1)
    loss = torch.where(ok, (m - tl) + ls, torch.full_like(ls, float("nan")))

    gs = torch.tensor(1.0 if mutant == "ignore_grad_scale" else grad_scale,
                      dtype=torch.float32)
    p = torch.exp(x - lse[:, None])
    if mutant == "bwd_no_softmax":
        p = torch.zeros_like(p)
    tgt = labels + 1 if mutant == "onehot_off_by_one" else labels
    okt = _valid(tgt, v)
    p[torch.arange(n)[okt], tgt[okt]] -= 1.0
    d = (p * gs).to(BF16)
    if skip:
        full = (v // VEC) // BLOCK * BLOCK * VEC
        d[:, full:] = 0          # never written
    return loss, lse, d


def ce_pinned_labels(v: int):
    """Columns 0, 7, 8, V-1 and, from V = 2056 on, 2047 and 2048: the first
    and last element of a 16-byte chunk and of a 256-thread stride."""
    cols = [0, 7 % v, 8 % v, v - 1]
    if v >= 2056:
        cols += [2047, 2048]
    return cols


def ce_input(n: int, v: int, family: str, seed=0):
    """(logits bf16 [N,V], labels [N]) on the CPU. Families: randn, x8
    (peaked), off1000 (large common offset). Row i is pinned to column
    ce_pinned_labels(V)[(i + seed) % len]."""
    g = torch.Generator().manual_seed(seed * 65537 + n * 131 + v)
    x = torch.randn(n, v, generator=g)
    if family == "x8":
        x = x * 8
    elif family == "off1000":
        x = x + 1000
    else:
        assert family == "randn", family
    cols = ce_pinned_labels(v)
    labels = torch.tensor([cols[(i + seed) % len(cols)] for i in range(n)])
    return x.to(BF16), labels


def ce_exact_case(n: int, v: int, max_cols):
    """Integer logits in -60..-20 with one entry of +100 per row at
    max_cols[row % len]: the other terms add less than half an ulp to the
    1.0 of the maximum, so every partial sum is exact, lse equals the row
    max bitwise and the loss at the maximum is exactly 0. A maximum that
    the max pass misses leaves exp(100 - m') = inf behind."""
    g = torch.Generator().manual_seed(v * 31 + n)
    x = torch.randint(-60, -19, (n, v), generator=g).float()
    labels = torch.tensor([max_cols[i % len(max_cols)] for i in range(n)])
    x[torch.arange(n), labels] = 100.0
    return x.to(BF16), labels


# --- LayerNorm / RMSNorm forward ------------------------------------------
def ln_reference(x, gamma, beta, eps):
    """(y, mean, rstd) in float64."""
    xd = x.double()
    mean = xd.mean(-1)
    var = (xd - mean[:, None]).pow(2).mean(-1)
    rstd = torch.rsqrt(var + eps)
    y = (xd - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    return y, mean, rstd


def ln_baseline(x, gamma, beta, eps):
    """y from F.layer_norm on bf16 tensors; mean and rstd fp32 two-pass."""
    h = x.size(-1)
    y = F.layer_norm(x.to(BF16), (h,), gamma.to(BF16), beta.to(BF16), eps)
    xf = x.float()
    mean = xf.mean(-1)
    var = (xf - mean[:, None]).pow(2).mean(-1)
    return y, mean, torch.rsqrt(var + eps)


def rms_reference(x, gamma, eps):
    xd = x.double()
    rstd = torch.rsqrt(xd.pow(2).mean(-1) + eps)
    return xd * rstd[:, None] * gamma.double(), rstd


def rms_baseline(x, gamma, eps):
    xb = x.to(BF16)
    y = xb * torch.rsqrt(xb.pow(2).mean(-1, keepdim=True) + eps) * gamma.to(BF16)
    return y, torch.rsqrt(x.float().pow(2).mean(-1) + eps)


LN_MUTANTS = ("one_pass_variance", "biased_by_one", "no_beta")
RMS_MUTANTS = ("skip_last_partial_stride",)


def ln_emulate(x, gamma, beta, eps, mutant=None):
    """(y, mean, rstd) of ln_fwd_kernel in fp32, CPU: the mean from the
    plain sum, the variance from the sums of d = x - K and d*d with K the
    mean of the row's first 8 elements on the bf16 grid of the largest of
    them. Mutant one_pass_variance is the
    kernel before the fix: K = 0, no clamp."""
    assert mutant is None or mutant in LN_MUTANTS
    xf = x.float()
    rows, h = xf.shape
    one_pass = mutant == "one_pass_variance"
    shift = torch.zeros(rows)
    if not one_pass:
        for k in range(VEC):
            shift = shift + xf[:, k]
        shift = shift * torch.tensor(1.0 / VEC)
        # rounded to the bf16 grid of the largest of the 8: add and
        # subtract 1.5 * 2^23 grid units, as the kernel does
        _, e = torch.frexp(xf[:, :VEC].abs().amax(-1))
        big = torch.ldexp(torch.tensor(98304.0), e - 1)
        big = torch.where(xf[:, :VEC].abs().amax(-1) > 0, big,
                          torch.zeros_like(big))
        shift = (shift + big) - big
    s = block_reduce(stride_partials(xf, lambda t: t, 0.0))
    ds = block_reduce(stride_partials(xf, lambda t: t - shift[:, None], 0.0))
    dss = block_reduce(stride_partials(
        xf, lambda t: (t - shift[:, None]) * (t - shift[:, None]), 0.0))
    inv_n = torch.tensor(1.0, dtype=torch.float32) / h
    if mutant == "biased_by_one":
        inv_n = torch.tensor(1.0, dtype=torch.float32) / (h - 1)
    mean = s * inv_n
    dmean = ds * inv_n
    var = dss * inv_n - dmean * dmean
    if not one_pass:
        var = var.clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    y = (xf - mean[:, None]) * rstd[:, None] * gamma.float()
    if mutant != "no_beta":
        y = y + beta.float()
    return y.to(BF16), mean, rstd


def rms_emulate(x, gamma, eps, mutant=None):
    assert mutant is None or mutant in RMS_MUTANTS
    xf = x.float()
    ss = block_reduce(stride_partials(
        xf, lambda t: t * t, 0.0,
        skip_tail=mutant == "skip_last_partial_stride"))
    rstd = 1.0 / torch.sqrt(ss / x.size(-1)
                            + torch.tensor(eps, dtype=torch.float32))
    return (xf * rstd[:, None] * gamma.float()).to(BF16), rstd


def norm_input(rows, h, family, seed=0):
    """bf16 [rows, H] on the CPU. Families: randn, x100, x1e-3, const3,
    off10 / off100 / off1000 (offset + randn, std 1)."""
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 8209 + h)
    x = torch.randn(rows, h, generator=g)
    if family == "x100":
        x = x * 100
    elif family == "x1e-3":
        x = x * 1e-3
    elif family == "const3":
        x = torch.full_like(x, 3.0)
    elif family.startswith("off"):
        x = x + float(family[3:])
    else:
        assert family == "randn", family
    return x.to(BF16)


def norm_params(h, seed=0):
    g = torch.Generator().manual_seed(seed + h)
    return torch.randn(h, generator=g), torch.randn(h, generator=g)


def norm_exact_case(rows, h):
    """x = +-2 with as many of each sign per row (also among the first 8),
    integer gamma and beta, eps = 0: mean = 0, every sum is an exact fp32
    integer in any order, var = 4, rstd = 0.5 and y = +-gamma + beta
    exactly."""
    g = torch.Generator().manual_seed(rows * 7 + h)
    x = torch.empty(rows, h)
    for r in range(rows):
        head = torch.tensor([2.0, -2.0] * 4)[torch.randperm(8, generator=g)]
        tail = torch.tensor([2.0, -2.0] * ((h - 8) // 2))
        x[r] = torch.cat([head, tail[torch.randperm(h - 8, generator=g)]])
    gamma = torch.randint(-3, 4, (h,), generator=g).float()
    beta = torch.randint(-3, 4, (h,), generator=g).float()
    return x.to(BF16), gamma, beta


def norm_integer_case(rows, h):
    """Integers in -8..8, H a power of two: 1/H is exact, so the fp32 mean
    of the shifted sums equals the float64 mean bitwise."""
    assert h & (h - 1) == 0
    g = torch.Generator().manual_seed(rows * 13 + h)
    return torch.randint(-8, 9, (rows, h), generator=g).to(BF16)


# --- RoPE -----------------------------------------------------------------
def rope_tables_fp32(length, d, base=500000.0):
    """[length, D/2] fp32 cos/sin, the expression of ops.norms.rope_tables
    on the CPU."""
    inv = 1.0 / (base ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    freqs = torch.outer(torch.arange(length, dtype=torch.float32), inv)
    return freqs.cos(), freqs.sin()


def _rotate(x, c, s, sign=1.0):
    d = x.size(-1)
    x1, x2 = x[..., : d // 2], x[..., d // 2:]
    return torch.cat((x1 * c - x2 * (sign * s), x2 * c + x1 * (sign * s)), -1)


def _rope_run(x, cos_t, sin_t, pos_offset, dy, dtype):
    s = x.size(2)
    c = cos_t[pos_offset:pos_offset + s].to(dtype)
    sn = sin_t[pos_offset:pos_offset + s].to(dtype)
    x_ = x.detach().to(dtype).requires_grad_(dy is not None)
    y = _rotate(x_, c, sn)
    if dy is None:
        return y.detach(), None
    (dx,) = torch.autograd.grad(y, x_, dy.to(dtype))
    return y.detach(), dx


def rope_reference(x, cos_t, sin_t, pos_offset=0, dy=None):
    """(y, dx) in float64 from the fp32 tables the kernel is given; dx is
    float64 AUTOGRAD of the forward, None without dy."""
    return _rope_run(x, cos_t, sin_t, pos_offset, dy, torch.float64)


def rope_baseline(x, cos_t, sin_t, pos_offset=0, dy=None):
    """The same in bf16 tensors (tables rounded to bf16, as _rope_ref)."""
    return _rope_run(x, cos_t, sin_t, pos_offset, dy, BF16)


ROPE_MUTANTS = ("bwd_forward_sign", "no_pos_offset", "adjacent_pairs")


def rope_emulate(x, cos_t, sin_t, pos_offset=0, backward=False, mutant=None):
    """rope_kernel in fp32, CPU: products and their difference in fp32, one
    rounding to bf16."""
    assert mutant is None or mutant in ROPE_MUTANTS
    s, d = x.size(2), x.size(3)
    off = 0 if mutant == "no_pos_offset" else pos_offset
    c, sn = cos_t[off:off + s].float(), sin_t[off:off + s].float()
    sign = -1.0 if backward and mutant != "bwd_forward_sign" else 1.0
    xf = x.float()
    if mutant == "adjacent_pairs":
        xe, xo = xf[..., 0::2], xf[..., 1::2]
        y = torch.empty_like(xf)
        y[..., 0::2] = xe * c - xo * (sign * sn)
        y[..., 1::2] = xo * c + xe * (sign * sn)
        return y.to(BF16)
    return _rotate(xf, c, sn, sign).to(BF16)


def rope_ratio(got, base, ref) -> float:
    """One block per (row, half)."""
    return block_ratio(got, base, ref, got.size(-1) // 2, ULP_BF16)


# --- SwiGLU ---------------------------------------------------------------
SATURATING = (100.0, -100.0, 88.0, -88.0, 0.0, -0.0)


def _swiglu_run(a, b, dy, dtype):
    a_ = a.detach().to(dtype).requires_grad_(True)
    b_ = b.detach().to(dtype).requires_grad_(True)
    y = F.silu(a_) * b_
    da, db = torch.autograd.grad(y, (a_, b_), dy.to(dtype))
    return y.detach(), da, db


def swiglu_reference(a, b, dy):
    """(y, da, db) in float64: y = a*sigmoid(a)*b."""
    return _swiglu_run(a, b, dy, torch.float64)


def swiglu_baseline(a, b, dy):
    return _swiglu_run(a, b, dy, BF16)


SWIGLU_MUTANTS = ("da_without_x_term", "db_uses_s")


def swiglu_emulate(a, b, dy, mutant=None):
    assert mutant is None or mutant in SWIGLU_MUTANTS
    x, bb, g = a.float(), b.float(), dy.float()
    s = 1.0 / (1.0 + torch.exp(-x))
    y = x * s * bb
    dsilu = s if mutant == "da_without_x_term" else s * (1.0 + x * (1.0 - s))
    da = g * bb * dsilu
    db = g * (s if mutant == "db_uses_s" else x * s)
    return y.to(BF16), da.to(BF16), db.to(BF16)


def swiglu_input(n, family, seed=0):
    """(a, b, dy) bf16 on the CPU. Families: randn, x20, saturating (a
    cycles through +-100, +-88, +-0.0; b and dy are 1 there, so the
    expected values carry no rounding of their own)."""
    g = torch.Generator().manual_seed(seed * 7919 + n)
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g)
    dy = torch.randn(n, generator=g)
    if family == "x20":
        a = a * 20
    elif family == "saturating":
        sat = torch.tensor(SATURATING)
        k = min(n, 64) // len(SATURATING) * len(SATURATING)
        a[:k] = sat.repeat(k // len(SATURATING))
        b[:k] = 1.0
        dy[:k] = 1.0
    else:
        assert family == "randn", family
    return a.to(BF16), b.to(BF16), dy.to(BF16)


# --- AdamW ----------------------------------------------------------------
def adamw_hyper(lr, beta1, beta2, eps, weight_decay, grad_scale, step):
    """The hyperparameters as the kernel receives them: each rounded to
    fp32; the bias corrections 1/(1 - beta^t) in float64 from the ROUNDED
    betas."""
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    h = dict(lr=f(lr), b1=f(beta1), b2=f(beta2), eps=f(eps),
             wd=f(weight_decay), gs=f(grad_scale))
    h["c1"] = 1.0 / (1.0 - h["b1"] ** step)
    h["c2"] = 1.0 / (1.0 - h["b2"] ** step)
    return h


ADAMW_MUTANTS = ("ignore_grad_scale", "coupled_weight_decay",
                 "no_bias_correction", "model_truncated",
                 "stride_tail_not_updated")
ADAMW_STRIDE = 2048 * BLOCK * 4     # elements per grid-stride trip


def _adamw(master, m, v, grad, h, dtype, mutant=None):
    """One step of the documented update at `dtype`; returns new
    (master, m, v)."""
    t = lambda k: torch.tensor(h[k], dtype=dtype, device=master.device)  # noqa: E731
    one = torch.tensor(1.0, dtype=dtype, device=master.device)
    p, m, v = master.to(dtype), m.to(dtype), v.to(dtype)
    g = grad.to(dtype)
    if mutant != "ignore_grad_scale":
        g = g * t("gs")
    wd = t("wd")
    if mutant == "coupled_weight_decay":
        g = g + wd * p
        wd = torch.zeros_like(wd)
    m = t("b1") * m + (one - t("b1")) * g
    v = t("b2") * v + (one - t("b2")) * g * g
    c1, c2 = (one, one) if mutant == "no_bias_correction" else (t("c1"), t("c2"))
    p = p - t("lr") * ((m * c1) / (torch.sqrt(v * c2) + t("eps")) + wd * p)
    return p, m, v


def adamw_reference(master, m, v, grad, h):
    return _adamw(master, m, v, grad, h, torch.float64)


def adamw_baseline(master, m, v, grad, h):
    return _adamw(master, m, v, grad, h, torch.float32)


def adamw_emulate(master, m, v, grad, h, mutant=None):
    """adamw_kernel in fp32, CPU: (master, m, v, model bf16). It IS the
    fp32 formula element by element; the mutants are what differs."""
    assert mutant is None or mutant in ADAMW_MUTANTS
    p, mm, vv = _adamw(master, m, v, grad, h, torch.float32, mutant)
    if mutant == "stride_tail_not_updated":
        p[ADAMW_STRIDE:] = master[ADAMW_STRIDE:]
        mm[ADAMW_STRIDE:] = m[ADAMW_STRIDE:]
        vv[ADAMW_STRIDE:] = v[ADAMW_STRIDE:]
    if mutant == "model_truncated":
        model = (p.view(torch.int32) & -65536).view(torch.float32).to(BF16)
    else:
        model = p.to(BF16)
    return p, mm, vv, model


def adamw_case(n, scale, grad_dtype, steps, seed=0):
    """(master fp32 [n], [grad per step]) on the CPU; parameters are
    randn * scale, gradients randn (bf16-rounded for the bf16 branch)."""
    g = torch.Generator().manual_seed(seed * 104729 + n)
    master = torch.randn(n, generator=g) * scale
    grads = [torch.randn(n, generator=g).to(grad_dtype) for _ in range(steps)]
    return master, grads


def adamw_exact_case(n, steps):
    """Integer gradients in -4..4 with beta1 = beta2 = 0.5: every m and v
    is a small dyadic rational, exact in fp32 for the first few steps."""
    g = torch.Generator().manual_seed(n)
    return [torch.randint(-4, 5, (n,), generator=g).float()
            for _ in range(steps)]


def bias_c2_gap(beta2=0.999, step=1) -> float:
    """Relative difference of 1/(1-beta2^t) between the fp32-rounded beta
    (what the kernel receives) and the Python double (torch.optim.AdamW):
    documented in docs/KERNELS.md, not tested against."""
    b32 = float(torch.tensor(beta2, dtype=torch.float32))
    return abs((1 - beta2 ** step) / (1 - b32 ** step) - 1.0)


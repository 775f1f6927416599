"""References, baselines, inputs and the kernel emulation for the
LayerNorm / RMSNorm backward tests (norm_bwd.h, rms_bwd_kernel).

Plain test support (not a conftest), a sibling of
elementwise_conformance.py, whose criterion (block_ratio, ULP_BF16) it
uses: imported by test_norm_bwd_conformance_cpu.py and
test_norm_bwd_conformance_gpu.py. References and baselines run on the
device of their inputs; the emulation is CPU fp32.

  statistics   mean and rstd in float64, rounded to fp32: they are INPUTS
               of the backward, so every party (kernel, reference,
               baseline, emulation) is given the same fp32 values
  reference    the formulas in the header of norm_bwd.h in float64
  baseline     the same formulas on bf16 eager tensors (dx only)
  emulate      norm_bwd_kernel + norm_bwd_reduce_kernel in fp32 in their
               own order: 8 columns per lane folded in turn, a 64-lane
               butterfly, the wave totals added in wave order; one
               dgamma/dbeta slab per workgroup, row groups taken by
               blockIdx stride (the grid is a parameter); the reduce
               kernel's 64 slab lanes, (p0 + p1) + (p2 + p3) inside a wave
               and the 16 waves in order

dx criterion: the project's rule per (row, 256 columns), ulp = 2^-8.
dgamma/dbeta on random data: the worst-case bound of an fp32 sum of
`rows` terms in ANY order, per column (sum_bound); twice an fp32 baseline
is not usable, two fp32 sums in different orders differ by more than that.
"""

from __future__ import annotations

import torch

import elementwise_conformance as ec

BF16 = torch.bfloat16
VEC = 8
WAVE = 64
R4_MAX_THREADS = 384        # up to 6 waves: 4 rows per iteration, else 2
MAX_SLABS = 1024
RED_LANES = 64              # slab lanes of norm_bwd_reduce_kernel
KINDS = ("randn", "dy_off", "dy_xhat_off", "dy_off_x_off")
MEAN_KINDS = KINDS[2:]      # both row means O(1)


def rows_per_iter(h: int) -> int:
    threads = (h // VEC + WAVE - 1) // WAVE * WAVE
    return 4 if threads <= R4_MAX_THREADS else 2


# --- inputs ---------------------------------------------------------------
def stats(x, rms: bool, eps=1e-5):
    """(mean fp32 or None, rstd fp32) from float64."""
    xd = x.double()
    if rms:
        return None, torch.rsqrt(xd.pow(2).mean(-1) + eps).float()
    mean = xd.mean(-1)
    var = (xd - mean[:, None]).pow(2).mean(-1)
    return mean.float(), torch.rsqrt(var + eps).float()


def bwd_input(rows, h, kind, rms: bool, seed=0, device="cpu"):
    """(dy bf16, x bf16, gamma fp32, mean, rstd), drawn on `device`.

    randn          dy, x ~ N(0, 1): both row means are O(1/sqrt(H))
    dy_off         dy = randn + 2: mean(dy*g) is O(1)
    dy_xhat_off    dy = randn + 2*xhat + 2: both means O(1)
    dy_off_x_off   dy_off with x offset by +10 (LayerNorm) / +0.5 (RMSNorm)
    gamma = 1 + 0.5 * randn."""
    assert kind in KINDS, kind
    g = torch.Generator(device).manual_seed(seed * 1000003 + rows * 8209 + h)
    x = torch.randn(rows, h, generator=g, device=device)
    dy = torch.randn(rows, h, generator=g, device=device)
    gamma = 1.0 + 0.5 * torch.randn(h, generator=g, device=device)
    if kind == "dy_off_x_off":
        x = x + (0.5 if rms else 10.0)
    x = x.to(BF16)
    mean, rstd = stats(x, rms)
    if kind in ("dy_off", "dy_off_x_off"):
        dy = dy + 2.0
    elif kind == "dy_xhat_off":
        mu = 0.0 if rms else mean[:, None]
        dy = dy + 2.0 * (x.float() - mu) * rstd[:, None] + 2.0
    return dy.to(BF16), x, gamma, mean, rstd


def exact_case(rows, h, shifted=False, seed=0, device="cpu"):
    """(dy, x, gamma, mean, rstd): x = +-2 (shifted: -1 / 3 with mean 1),
    the passed-in mean = 0 (1) and rstd = 0.5, so xhat = +-1; integer dy in
    -4..4; gamma in {0.5, 1, 2}. Every product and every sum in any order
    is exact in fp32, 1/H is exact at a power-of-two H."""
    g = torch.Generator(device).manual_seed(seed + rows * 31 + h)
    kw = dict(generator=g, device=device)
    sign = torch.randint(0, 2, (rows, h), **kw).float() * 2 - 1
    x = 2.0 * sign + (1.0 if shifted else 0.0)
    dy = torch.randint(-4, 5, (rows, h), **kw).float()
    gamma = torch.ldexp(torch.ones(h, device=device),
                        torch.randint(-1, 2, (h,), **kw))
    mean = torch.full((rows,), 1.0 if shifted else 0.0, device=device)
    return (dy.to(BF16), x.to(BF16), gamma, mean,
            torch.full((rows,), 0.5, device=device))


# --- reference and baseline ------------------------------------------------
def _formula(dy, x, gamma, mean, rstd, dtype, want_params=True):
    dy, x, g = dy.to(dtype), x.to(dtype), gamma.to(dtype)
    rs = rstd.to(dtype)[:, None]
    if mean is None:
        xhat = x * rs
        dyg = dy * g
        dx = rs * dyg - rs * xhat * (dyg * xhat).mean(-1, keepdim=True)
    else:
        xhat = (x - mean.to(dtype)[:, None]) * rs
        dyg = dy * g
        dx = rs * (dyg - dyg.mean(-1, keepdim=True)
                   - xhat * (dyg * xhat).mean(-1, keepdim=True))
    if not want_params:
        return dx
    return dx, (dy * xhat).sum(0), (None if mean is None else dy.sum(0))


def reference(dy, x, gamma, mean, rstd):
    """(dx, dgamma, dbeta or None) in float64; mean None selects RMSNorm."""
    return _formula(dy, x, gamma, mean, rstd, torch.float64)


def baseline_dx(dy, x, gamma, mean, rstd):
    return _formula(dy, x, gamma, mean, rstd, BF16, want_params=False)


def dx_ratio(got, base, ref) -> float:
    return ec.block_ratio(got, base, ref, ec.COL_BLOCK, ec.ULP_BF16)


def sum_bound(dy, x, mean, rstd):
    """Per-column bounds (dgamma, dbeta) of an fp32 sum over the rows in
    any order: (rows - 1) * 2^-24 * sum|term| to first order, written with
    `rows`; dgamma's terms carry three more roundings (x - mean, * rstd,
    dy * xhat), hence rows + 4 with one to spare."""
    rows = dy.size(0)
    mu = 0.0 if mean is None else mean.double()[:, None]
    xhat = (x.double() - mu) * rstd.double()[:, None]
    u = 2.0 ** -24
    return ((rows + 4) * u * (dy.double() * xhat).abs().sum(0),
            rows * u * dy.double().abs().sum(0))


def sum_ratio(got, ref, bound) -> float:
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


# --- emulation ------------------------------------------------------------
DX_MUTANTS = ("no_mean_dyg", "no_mean_dyg_xhat", "last_wave_missing",
              "prev_group_sums", "divisor_h_minus_1")
PARAM_MUTANTS = ("dbeta_from_dyg", "last_group_dropped", "slab_off_by_one")


def _lanes(t, nw):
    """[rows, H] -> [rows, nw, 64, 8], lanes past the row zero."""
    rows, h = t.shape
    pad = nw * WAVE * VEC - h
    if pad:
        t = torch.cat([t, t.new_zeros(rows, pad)], -1)
    return t.reshape(rows, nw, WAVE, VEC)


def _row_sum(t, nw, drop_last_wave=False):
    p = _lanes(t, nw)
    acc = torch.zeros(p.shape[:-1])
    for k in range(VEC):
        acc = acc + p[..., k]
    w = ec._butterfly(acc, torch.add)                 # [rows, nw]
    tot = torch.zeros(t.size(0))
    for i in range(nw - 1 if drop_last_wave else nw):
        tot = tot + w[:, i]
    return tot


def _slabs(term, grid, r, drop_last_group=False):
    """[rows, H] per-row terms -> [grid, H]: workgroup b adds the rows of
    the groups b, b + grid, ... in turn."""
    rows, h = term.shape
    groups = (rows + r - 1) // r
    if drop_last_group:
        term = term.clone()
        term[(groups - 1) * r:] = 0
    iters = (groups + grid - 1) // grid
    pad = iters * grid * r - rows
    if pad:
        term = torch.cat([term, term.new_zeros(pad, h)], 0)
    term = term.reshape(iters, grid, r, h)
    acc = torch.zeros(grid, h)
    for it in range(iters):
        for j in range(r):
            acc = acc + term[it, :, j]
    return acc


def _reduce(slabs, nslabs):
    """norm_bwd_reduce_kernel: slab lane sy adds slabs sy, sy + 64, ...;
    thread = sy * 16 + column, so a wave holds 4 slab lanes, folded as
    (p0 + p1) + (p2 + p3); then the 16 waves in order."""
    h = slabs.size(1)
    part = torch.zeros(RED_LANES, h)
    for s in range(nslabs):
        part[s % RED_LANES] = part[s % RED_LANES] + slabs[s]
    p = part.reshape(16, 4, h)
    w = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])
    out = torch.zeros(h)
    for i in range(16):
        out = out + w[i]
    return out


def emulate(dy, x, gamma, mean, rstd, grid=None, mutant=None):
    """(dx bf16, dgamma, dbeta or None) of the streaming kernel and its
    reduce in fp32, CPU. `grid` is the number of workgroups (default: one
    per row group, capped at MAX_SLABS)."""
    assert mutant is None or mutant in DX_MUTANTS + PARAM_MUTANTS
    rms = mean is None
    rows, h = x.shape
    nw = (h // VEC + WAVE - 1) // WAVE
    r = rows_per_iter(h)
    groups = (rows + r - 1) // r
    grid = min(groups, MAX_SLABS) if grid is None else min(grid, groups)

    dyf, g, rs = dy.float(), gamma.float(), rstd.float()[:, None]
    xhat = (x.float() * rs) if rms else (x.float() - mean.float()[:, None]) * rs
    dyg = dyf * g
    last = mutant == "last_wave_missing"
    s1 = torch.zeros(rows) if rms else _row_sum(dyg, nw, last)
    s2 = _row_sum(dyg * xhat, nw, last)
    if mutant == "prev_group_sums":
        s1, s2 = torch.roll(s1, r), torch.roll(s2, r)
    div = h - 1 if mutant == "divisor_h_minus_1" else h
    inv_n = torch.tensor(1.0, dtype=torch.float32) / div
    s1, s2 = (s1 * inv_n)[:, None], (s2 * inv_n)[:, None]
    if mutant == "no_mean_dyg":
        s1 = torch.zeros_like(s1)
    if mutant == "no_mean_dyg_xhat":
        s2 = torch.zeros_like(s2)
    dx = rs * dyg - rs * xhat * s2 if rms else rs * (dyg - s1 - xhat * s2)

    drop = mutant == "last_group_dropped"
    nsl = grid - 1 if mutant == "slab_off_by_one" else grid
    dgamma = _reduce(_slabs(dyf * xhat, grid, r, drop), nsl)
    dbeta = None
    if not rms:
        term = dyg if mutant == "dbeta_from_dyg" else dyf
        dbeta = _reduce(_slabs(term, grid, r, drop), nsl)
    return dx.to(BF16), dgamma, dbeta


def emulate_wide(dy, x, gamma, rstd, grid=128):
    """rms_bwd_kernel (H > 8192) in fp32, CPU: 256-thread stride partials
    and block_reduce_sum for the row sum, one row at a time per workgroup,
    rows by blockIdx stride."""
    rows, h = x.shape
    grid = min(grid, rows)
    dyf, g, rs = dy.float(), gamma.float(), rstd.float()[:, None]
    part = torch.zeros(rows, ec.BLOCK)
    hv = h // VEC
    xf = x.float()
    for j in range(0, hv, ec.BLOCK):
        cnt = min(ec.BLOCK, hv - j)
        sl = slice(j * VEC, (j + cnt) * VEC)
        t = (dyf[:, sl] * g[sl] * xf[:, sl] * rs).reshape(rows, cnt, VEC)
        for k in range(VEC):
            part[:, :cnt] = part[:, :cnt] + t[:, :, k]
    s2 = (ec.block_reduce(part) / h)[:, None]
    xhat = xf * rs
    dx = rs * (dyf * g) - rs * xhat * s2
    return dx.to(BF16), _reduce(_slabs(dyf * xhat, grid, 1), grid)


def old_allclose(dx, ref) -> bool:
    """The dx assertion of test_norm_bwd_shapes_gpu.py."""
    return torch.allclose(dx.float(), ref.float(), atol=5e-2, rtol=5e-2)

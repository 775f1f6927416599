"""Reference, baseline, inputs and the kernel emulation for the tests of
gelu_tanh_bwd_bgrad (gelu.hip).

Plain test support (not a conftest), a sibling of norm_bwd_conformance.py,
whose slab and reduce emulation and sum criterion it uses; imported by
test_gelu_bgrad_cpu.py and test_gelu_bgrad_gpu.py.

  reference   dh = da * gelu'(h) in float64, with
              gelu'(h) = 0.5 (1 + t) + 0.5 h (1 - t^2) u',
              u = sqrt(2/pi) (h + 0.044715 h^3), t = tanh(u)
  baseline    the same formula on bf16 eager tensors
  emulate     the kernel in fp32 on the CPU: the exp form of the derivative,
              one rounding of dh to bf16, column sums of the ROUNDED dh in
              the kernel's order (row groups of 4 by blockIdx.y stride into
              one slab per row range, then norm_bwd_reduce_kernel's order)

dh criterion: the project's rule per (row, 256 columns), ulp = 2^-8.
dbias: against the float64 column sum of the dh that was returned, under
the bound of an fp32 sum of `rows` terms in any order, rows * 2^-24 *
sum|dh| per column.
"""

from __future__ import annotations

import math

import torch

import elementwise_conformance as ec
import norm_bwd_conformance as nb

BF16 = torch.bfloat16
R = 4                       # rows in flight per thread
MAX_SLABS = 1024
KBETA = math.sqrt(2.0 / math.pi)
KAPPA = 0.044715
KINDS = ("randn", "x8", "zero_crossing")
MUTANTS = ("last_group_dropped", "slab_off_by_one", "dbias_from_unrounded")


def gelu_input(rows, n, kind, seed=0, device="cpu"):
    """(h, da) bf16. randn; h x 8 (both tails saturate); h within 0.02 of
    -0.7518, where gelu' changes sign and dh is a difference of two terms
    of size 0.2 |da|."""
    assert kind in KINDS, kind
    g = torch.Generator(device).manual_seed(seed * 1000003 + rows * 8209 + n)
    h = torch.randn(rows, n, generator=g, device=device)
    da = torch.randn(rows, n, generator=g, device=device)
    if kind == "x8":
        h = h * 8
    elif kind == "zero_crossing":
        h = -0.7518 + 0.02 * h
    return h.to(BF16), da.to(BF16)


def exact_case(rows, n, seed=0, device="cpu"):
    """(h, da, dh expected): h in {0, +20, -20} at random, integer da in
    -4..4. gelu' is exactly 0.5, 1 and 0 there, so dh = da/2, da and +-0,
    and every column sum of dh is exact in fp32 in any order."""
    g = torch.Generator(device).manual_seed(seed + rows * 31 + n)
    kw = dict(generator=g, device=device)
    k = torch.randint(0, 3, (rows, n), **kw)
    h = torch.tensor([0.0, 20.0, -20.0], device=device)[k]
    da = torch.randint(-4, 5, (rows, n), **kw).float()
    factor = torch.tensor([0.5, 1.0, 0.0], device=device)[k]
    return h.to(BF16), da.to(BF16), (da * factor).to(BF16)


def _formula(h, da, dtype):
    h, da = h.to(dtype), da.to(dtype)
    h2 = h * h
    u = KBETA * (h + KAPPA * h2 * h)
    t = torch.tanh(u)
    du = KBETA * (1.0 + 3.0 * KAPPA * h2)
    return da * (0.5 * (1.0 + t) + 0.5 * h * (1.0 - t * t) * du)


def reference(h, da):
    return _formula(h, da, torch.float64)


def baseline(h, da):
    return _formula(h, da, BF16)


def dh_ratio(got, base, ref) -> float:
    return ec.block_ratio(got, base, ref, ec.COL_BLOCK, ec.ULP_BF16)


def dbias_ratio(dbias, dh) -> float:
    """dbias against the float64 column sum of the returned dh."""
    d = dh.double()
    bound = dh.size(0) * 2.0 ** -24 * d.abs().sum(0)
    return nb.sum_ratio(dbias, d.sum(0), bound)


def row_ranges(rows, n, resident=1024):
    """Slabs the launcher takes with `resident` workgroups on the chip."""
    strips = (n // 8 + 255) // 256
    want = max(1, resident // strips)
    return min(want, MAX_SLABS, (rows + R - 1) // R)


def emulate(h, da, ranges=None, mutant=None):
    """(dh bf16, dbias fp32) of gelu_bwd_bgrad_kernel and the slab reduce in
    fp32, CPU."""
    assert mutant is None or mutant in MUTANTS
    rows, n = h.shape
    ranges = row_ranges(rows, n) if ranges is None else ranges
    hf, af = h.float(), da.float()
    h2 = hf * hf
    u = KBETA * (hf + KAPPA * h2 * hf)
    e = torch.exp(-2.0 * u.abs())
    r = 1.0 / (1.0 + e)
    t = torch.copysign((1.0 - e) * r, u)
    sech2 = 4.0 * e * r * r
    du = KBETA * (1.0 + 3.0 * KAPPA * h2)
    v = af * (0.5 * (1.0 + t) + 0.5 * hf * sech2 * du)
    dh = v.to(BF16)
    term = v if mutant == "dbias_from_unrounded" else dh.float()
    slabs = nb._slabs(term, ranges, R, mutant == "last_group_dropped")
    nsl = ranges - 1 if mutant == "slab_off_by_one" else ranges
    return dh, nb._reduce(slabs, nsl)


def aten_distance(got, h, da):
    """(count of differing bf16 values, max distance in bf16 ulps) between
    `got` and aten's gelu_backward on the same inputs."""
    aten = torch.ops.aten.gelu_backward(da, h, approximate="tanh")
    a = got.view(torch.int16).int()
    b = aten.view(torch.int16).int()
    # order-preserving map of the sign-magnitude bf16 bits
    a = torch.where(a < 0, -(a & 0x7FFF), a)
    b = torch.where(b < 0, -(b & 0x7FFF), b)
    d = (a - b).abs()
    return int((d != 0).sum()), int(d.max())

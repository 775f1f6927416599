"""The criterion of test_gelu_bgrad_gpu.py, shown on the CPU: it passes an
fp32 emulation of gelu_bwd_bgrad_kernel and its slab reduce
(gelu_bgrad_conformance.emulate) and rejects three mutants of it.

  last_group_dropped     the last row group adds nothing to dbias
  slab_off_by_one        the reduce leaves the last slab out
  dbias_from_unrounded   dbias sums the fp32 dh instead of the bf16 it wrote

The first two are caught by the exact case (three-valued h, integer da),
where dbias must equal the float64 sum bitwise. The third cannot be: dh is
exactly representable there, rounded and unrounded agree. It is caught by
the sum bound on random data, where the roundings of `rows` values, about
sqrt(rows) * 2^-9 |dh| in a column, exceed rows * 2^-24 * sum|dh|.
"""

import pytest
import torch

import gelu_bgrad_conformance as gb

SHAPES = [(r, n) for n in (8, 520, 2048) for r in (1, 3, 33, 257)]
SHAPES += [(33, 10240), (2053, 512)]


@pytest.mark.parametrize("rows,n", SHAPES)
def test_criterion_passes_emulation(rows, n):
    for kind in gb.KINDS:
        h, da = gb.gelu_input(rows, n, kind)
        dh, dbias = gb.emulate(h, da)
        assert gb.dh_ratio(dh, gb.baseline(h, da), gb.reference(h, da)) <= 1.0
        assert gb.dbias_ratio(dbias, dh) <= 1.0


def test_zero_crossing_inputs_straddle_the_sign_change():
    h, da = gb.gelu_input(33, 2048, "zero_crossing")
    ones = torch.ones_like(da)
    d = gb.reference(h, ones)
    assert float(d.min()) < 0.0 < float(d.max())
    assert float(d.abs().max()) < 0.05


@pytest.mark.parametrize("rows,n", SHAPES)
def test_exact_case_emulation(rows, n):
    h, da, want = gb.exact_case(rows, n)
    dh, dbias = gb.emulate(h, da)
    assert torch.equal(dh.float(), want.float())     # +-0 compare equal
    assert torch.equal(dbias.double(), dh.double().sum(0))


@pytest.mark.parametrize("mutant", ("last_group_dropped", "slab_off_by_one"))
@pytest.mark.parametrize("rows,n,ranges", [(33, 520, None), (257, 2048, None),
                                           (2053, 512, 7), (2053, 512, 200)])
def test_exact_case_rejects_dropped_rows_and_slabs(rows, n, ranges, mutant):
    h, da, _ = gb.exact_case(rows, n)
    dh, dbias = gb.emulate(h, da, ranges, mutant)
    assert not torch.equal(dbias.double(), dh.double().sum(0))


@pytest.mark.parametrize("rows,n", [(33, 520), (257, 2048)])
def test_sum_bound_rejects_dbias_from_unrounded(rows, n):
    h, da = gb.gelu_input(rows, n, "randn")
    dh, dbias = gb.emulate(h, da, mutant="dbias_from_unrounded")
    assert gb.dbias_ratio(dbias, dh) > 1.0
    h, da, _ = gb.exact_case(rows, n)       # blind here, as said above
    dh, dbias = gb.emulate(h, da, mutant="dbias_from_unrounded")
    assert torch.equal(dbias.double(), dh.double().sum(0))

"""CPU check of the norm backward criterion and inputs themselves.

The fp32 emulation of norm_bwd_kernel + norm_bwd_reduce_kernel (in their
own summation order, norm_bwd_conformance.emulate) has to sit well under
the bound, and every named mutant has to be rejected, on the inputs of
test_norm_bwd_conformance_gpu.py. The worst ratios of the correct
emulation are printed (-s) and quoted in docs/KERNELS.md as the CPU
prediction.

Why the inputs matter: on randn data the two row means of dx are
O(1/sqrt(H)). A dx without the mean(dy*g) term passes the older
assertion (allclose 5e-2 in test_norm_bwd_shapes_gpu.py) at H = 8192 and
scores 0.71 of the per-block bound there; row sums that miss a wave score
0.63. With dy = randn + 2*xhat + 2 both means are O(1) and every mutant
is at 2.2 times the bound or more at every H. The fourth kind (dy =
randn + 2, x offset) makes mean(dy*g*xhat) O(1) for RMSNorm only: for
LayerNorm the offset cancels in xhat, so there the mutants of that term
are rejected by a smaller margin (1.08 at H = 8192) and the 2.2 is
asserted on the third kind.
"""

import pytest
import torch

import norm_bwd_conformance as nb

HIDDEN = (8, 512, 2560, 8192)
ROWS = 33
WORST = {}


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{name}: ratio to bound {ratio:.3f}")
    return ratio


def _case(h, kind, rms, rows=ROWS):
    args = nb.bwd_input(rows, h, kind, rms)
    return args, nb.reference(*args), nb.baseline_dx(*args)


def _mutants(h, rms):
    out = ["no_mean_dyg_xhat", "prev_group_sums"]
    if not rms:
        out.append("no_mean_dyg")
    if h >= 512:
        out.append("last_wave_missing")
    return out


@pytest.mark.parametrize("rms", (False, True), ids=("ln", "rms"))
@pytest.mark.parametrize("kind", nb.KINDS)
@pytest.mark.parametrize("h", HIDDEN)
def test_emulation_under_bound(h, kind, rms):
    args, ref, base = _case(h, kind, rms)
    dx, dgamma, dbeta = nb.emulate(*args, grid=3)     # 3 iterations at least
    name = "rms" if rms else "ln"
    r = _record(f"{name} dx {kind}", nb.dx_ratio(dx, base, ref[0]))
    assert r < 0.5
    if kind in nb.MEAN_KINDS:
        assert r <= 0.33
    bg, bb = nb.sum_bound(args[0], args[1], args[3], args[4])
    assert _record(f"{name} dgamma {kind}", nb.sum_ratio(dgamma, ref[1], bg)) < 0.5
    if not rms:
        assert _record(f"{name} dbeta {kind}", nb.sum_ratio(dbeta, ref[2], bb)) < 0.5


@pytest.mark.parametrize("rms", (False, True), ids=("ln", "rms"))
@pytest.mark.parametrize("h", HIDDEN)
def test_dx_mutants_rejected(h, rms):
    for kind in nb.MEAN_KINDS:
        args, ref, base = _case(h, kind, rms)
        for mutant in _mutants(h, rms):
            r = nb.dx_ratio(nb.emulate(*args, mutant=mutant)[0], base, ref[0])
            print(f"{'rms' if rms else 'ln'} H={h} {kind} {mutant}: {r:.2f}")
            assert r > 1.0, (kind, mutant, r)
            if kind == "dy_xhat_off" or rms:
                assert r >= 2.2, (kind, mutant, r)


@pytest.mark.parametrize("rms", (False, True), ids=("ln", "rms"))
def test_divisor_mutant_rejected_at_h8(rms):
    for kind in nb.KINDS:
        args, ref, base = _case(8, kind, rms)
        bad = nb.emulate(*args, mutant="divisor_h_minus_1")[0]
        assert nb.dx_ratio(bad, base, ref[0]) >= 2.2, kind


def test_randn_hides_the_mean_terms():
    """The reason for the input kinds: at H = 8192 on randn data the dx
    without mean(dy*g) passes the old allclose AND the per-block criterion,
    as do row sums that miss a wave."""
    args, ref, base = _case(8192, "randn", rms=False)
    bad = nb.emulate(*args, mutant="no_mean_dyg")[0]
    assert nb.old_allclose(bad, ref[0])
    assert nb.dx_ratio(bad, base, ref[0]) < 1.0
    bad = nb.emulate(*args, mutant="last_wave_missing")[0]
    assert nb.dx_ratio(bad, base, ref[0]) < 1.0
    # ... and with both means O(1) neither survives either check
    args, ref, base = _case(8192, "dy_xhat_off", rms=False)
    for mutant in ("no_mean_dyg", "last_wave_missing"):
        bad = nb.emulate(*args, mutant=mutant)[0]
        assert not nb.old_allclose(bad, ref[0])
        assert nb.dx_ratio(bad, base, ref[0]) >= 2.2


@pytest.mark.parametrize("rows,h,grid", [(33, 512, 3), (257, 2560, 7),
                                         (33, 4096, 1024), (13, 8, 2)])
def test_param_sums_reject_a_dropped_row(rows, h, grid):
    """One row group left out moves a column by far more than the bound of
    an fp32 sum in any order; so does a slab left out by the reduce."""
    for rms in (False, True):
        args = nb.bwd_input(rows, h, "randn", rms)
        ref = nb.reference(*args)
        bg, bb = nb.sum_bound(args[0], args[1], args[3], args[4])
        for mutant in ("last_group_dropped", "slab_off_by_one"):
            _, dgamma, dbeta = nb.emulate(*args, grid=grid, mutant=mutant)
            assert nb.sum_ratio(dgamma, ref[1], bg) > 100, mutant
            if not rms:
                assert nb.sum_ratio(dbeta, ref[2], bb) > 100, mutant
    args = nb.bwd_input(rows, h, "randn", False)
    ref = nb.reference(*args)
    _, bb = nb.sum_bound(args[0], args[1], args[3], args[4])
    dbeta = nb.emulate(*args, grid=grid, mutant="dbeta_from_dyg")[2]
    assert nb.sum_ratio(dbeta, ref[2], bb) > 100


EXACT = [(1, 8, 1), (3, 8, 2), (33, 512, 3), (257, 768, 5), (33, 2560, 4),
         (33, 4096, 1024), (5, 8192, 2), (1229, 8, 100)]


@pytest.mark.parametrize("shifted", (False, True))
@pytest.mark.parametrize("rows,h,grid", EXACT)
def test_exact_integer_case(rows, h, grid, shifted):
    """Every product and sum exact: dgamma and dbeta equal float64 bitwise,
    dx equals the bf16 of the float64 result at a power-of-two H; the three
    accumulation mutants do not."""
    for rms in (False, True):
        dy, x, gamma, mean, rstd = nb.exact_case(rows, h, shifted and not rms)
        args = (dy, x, gamma, None if rms else mean, rstd)
        ref = nb.reference(*args)
        dx, dgamma, dbeta = nb.emulate(*args, grid=grid)
        assert torch.equal(dgamma.double(), ref[1])
        if not rms:
            assert torch.equal(dbeta.double(), ref[2])
        if h & (h - 1) == 0:
            assert torch.equal(dx, ref[0].to(nb.BF16))
        if rows * h < 64:
            continue        # a handful of small integers may cancel
        for mutant in ("last_group_dropped", "slab_off_by_one"):
            if mutant == "slab_off_by_one" and min(grid, -(-rows // nb.rows_per_iter(h))) < 2:
                continue
            bad = nb.emulate(*args, grid=grid, mutant=mutant)
            assert not torch.equal(bad[1].double(), ref[1]), mutant
        if not rms:
            bad = nb.emulate(*args, grid=grid, mutant="dbeta_from_dyg")
            assert not torch.equal(bad[2].double(), ref[2])


@pytest.mark.parametrize("rows,h", [(3, 8200), (130, 8200), (3, 16384)])
def test_wide_emulation_under_bound(rows, h):
    for kind in nb.KINDS:
        args = nb.bwd_input(rows, h, kind, True)
        ref, base = nb.reference(*args), nb.baseline_dx(*args)
        dx, dgamma = nb.emulate_wide(args[0], args[1], args[2], args[4])
        assert _record(f"rms wide dx {kind}", nb.dx_ratio(dx, base, ref[0])) < 0.5
        bg, _ = nb.sum_bound(args[0], args[1], None, args[4])
        assert _record(f"rms wide dgamma {kind}",
                       nb.sum_ratio(dgamma, ref[1], bg)) < 0.5
    dy, x, gamma, _, rstd = nb.exact_case(rows, h)
    ref = nb.reference(dy, x, gamma, None, rstd)
    dx, dgamma = nb.emulate_wide(dy, x, gamma, rstd)
    assert torch.equal(dgamma.double(), ref[1])
    if h & (h - 1) == 0:
        assert torch.equal(dx, ref[0].to(nb.BF16))

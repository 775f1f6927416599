"""CPU check of the dense decode criterion and inputs themselves.

The fp32 emulation of attn_decode_kernel (decode_conformance.emulate)
has to sit under half the bound at every sequence length of
test_decode_conformance_gpu.py, and the named mutants have to be
rejected; the exact cases have to hold for the emulation and fail for
the mutants. The worst ratios are printed (-s) and quoted in
docs/KERNELS.md.

The older test (test_ops_gpu.py, atol = 2e-2 at S = 777, max|o| ~ 0.2)
passes a kernel that drops the last key or the S % 4 tail; shown below
next to the rejection.

On the `shifted` kind the bf16 baseline rounds scores near 1e3 to
multiples of 4 or 8, so its own error is of the size of the output and the
bound is wide: that kind checks that a running maximum far from the
-1e30 start merges cleanly, it does not resolve a dropped key.
"""

import pytest
import torch

import decode_conformance as dc

B = 3
HEAD_DIMS = (64, 80, 96, 128)
SEQ = (1, 2, 3, 4, 5, 63, 65, 777, 1025)
WORST = {}


def _record(name, r):
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"{name}: ratio to bound {r:.3f}")
    return r


def _case(h, hkv, s, d, kind):
    q, k, v = dc.decode_input(B, h, hkv, s, d, kind)
    sc = dc.default_scale(d)
    return (q, k, v, sc), dc.reference(q, k, v, sc), dc.baseline(q, k, v, sc)


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("d,h,hkv", [(d, 8, 2) for d in HEAD_DIMS]
                         + [(64, 8, 8), (80, 8, 1), (96, 6, 2)])
def test_emulation_under_bound(d, h, hkv, kind):
    for s in SEQ:
        args, ref, base = _case(h, hkv, s, d, kind)
        r = _record(f"decode {kind}", dc.ratio(dc.emulate(*args), base, ref))
        assert r < 0.5, (s, r)


@pytest.mark.parametrize("d,h,hkv", [(64, 8, 2), (80, 8, 2), (96, 6, 2),
                                     (128, 8, 2)])
def test_mutants_rejected(d, h, hkv):
    for s in (5, 63, 65):
        args, ref, base = _case(h, hkv, s, d, "randn")
        for mutant in dc.MUTANTS:
            r = dc.ratio(dc.emulate(*args, mutant=mutant), base, ref)
            print(f"D{d} H{h}/{hkv} S{s} {mutant}: {r:.2f}")
            assert r >= 6.0, (s, mutant, r)


def test_old_tolerance_passes_a_dropped_key():
    """At the old test's shape (S = 777, D = 128, Hkv = 2) a kernel without
    the last key, or without the S % 4 tail, is inside atol = 2e-2; the
    per-row criterion has both at 6 times the bound or more."""
    args, ref, base = _case(8, 2, 777, 128, "randn")
    for mutant in ("last_key_dropped", "tail_dropped"):
        bad = dc.emulate(*args, mutant=mutant)
        assert torch.allclose(bad.double(), ref, atol=2e-2)        # old
        assert dc.ratio(bad, base, ref) >= 6.0


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_exact_cases(d):
    h, hkv = 6, 2
    kvh = torch.arange(h) // (h // hkv)
    for s in SEQ:
        for row in dc.dominant_rows(s):
            q, k, v = dc.dominant_case(B, h, hkv, s, d, row)
            out = dc.emulate(q, k, v, dc.default_scale(d))
            assert torch.equal(out[:, :, 0], v[:, kvh, row]), (s, row)
        q, k, v = dc.uniform_case(B, h, hkv, s, d, constant=1.5)
        out = dc.emulate(q, k, v, dc.default_scale(d))
        assert torch.equal(out, torch.full_like(out, 1.5)), s
    for s in (1, 2, 4, 64, 1024):
        q, k, v = dc.uniform_case(B, h, hkv, s, d)
        want = v.double().mean(2)[:, kvh].to(dc.BF16)
        assert torch.equal(dc.emulate(q, k, v, 0.125)[:, :, 0], want), s
        if s >= 64:
            for mutant in ("last_key_dropped", "wave_dropped",
                           "wrong_kv_head"):
                bad = dc.emulate(q, k, v, 0.125, mutant)[:, :, 0]
                assert not torch.equal(bad, want), (s, mutant)
    # the dominant key in the dropped tail / wave / on the other kv head
    s = 65
    q, k, v = dc.dominant_case(B, h, hkv, s, d, s - 1)
    for mutant in ("last_key_dropped", "tail_dropped", "wrong_kv_head"):
        bad = dc.emulate(q, k, v, dc.default_scale(d), mutant)
        assert not torch.equal(bad[:, :, 0], v[:, kvh, s - 1]), mutant
    q, k, v = dc.dominant_case(B, h, hkv, s, d, 34)            # wave 2
    bad = dc.emulate(q, k, v, dc.default_scale(d), "wave_dropped")
    assert not torch.equal(bad[:, :, 0], v[:, kvh, 34])

"""CPU tests of the attention comparators (tests/attn_conformance.py).

The flash kernels' arithmetic is emulated in fp32 (scores and softmax in
fp32, P and dS rounded to bf16 before their second matmul, per-q-head bf16
dK/dV summed over the GQA group, bf16 outputs). Two things are shown:

  * the clean emulation passes every comparator with room to spare (worst
    ratio < 0.5), so factor 2 is not tight for a correct kernel;
  * each of a list of realistic kernel defects is rejected by at least one
    comparator, including the two that the older global max-abs criteria
    (|o - ref| < 3e-2, grad err < 0.06 of the global max) let through.
"""

import math

import pytest
import torch

from attn_conformance import (LSE_ATOL, assert_blockwise_close,
                              assert_lse_close, baseline_bf16,
                              blockwise_ratio, causal_mask, lse_error,
                              reference_fp64)
from metis_amd.ops.attention import HEAD_DIMS, _head_dim_supported

B, H, HKV = 2, 4, 2
SHAPES = [(s, d) for s in (128, 384) for d in (64, 128)]


def _bf16(x):
    return x.to(torch.bfloat16).float()


def emulate(q, k, v, d_o, scale, mask, kv_map=None):
    """fp32 emulation of attention.hip / attention_bwd.hip. Returns bf16
    o, fp32 lse, bf16 dq and the per-q-head bf16 dk_h, dv_h [B,H,S,D]."""
    h, hkv = q.size(1), k.size(1)
    if kv_map is None:
        kv_map = [i // (h // hkv) for i in range(h)]
    qf, dof = q.float(), d_o.float()
    kf, vf = k.float()[:, kv_map], v.float()[:, kv_map]

    s = (qf @ kf.transpose(-1, -2)) * scale
    s = s.masked_fill(mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o = ((_bf16(p) @ vf) / l).to(torch.bfloat16)
    lse = (m + torch.log(l)).squeeze(-1)

    delta = (o.float() * dof).sum(-1, keepdim=True)
    pb = torch.exp(s - lse.unsqueeze(-1))
    ds = _bf16(scale * pb * (dof @ vf.transpose(-1, -2) - delta))
    dq = (ds @ kf).to(torch.bfloat16)
    dk_h = (ds.transpose(-1, -2) @ qf).to(torch.bfloat16)
    dv_h = (_bf16(pb).transpose(-1, -2) @ dof).to(torch.bfloat16)
    return o, lse, dq, dk_h, dv_h


def reduce_gqa(x_h, hkv):
    """The wrapper's group reduction: fp32 sum of the bf16 per-head grads."""
    b, h, s, d = x_h.shape
    return x_h.view(b, hkv, h // hkv, s, d).sum(2, dtype=torch.float32).to(
        torch.bfloat16)


class Case:
    """Inputs, fp64 reference and bf16 baseline of one shape, computed once."""

    def __init__(self, s, d):
        gen = torch.Generator().manual_seed(1000 * s + d)
        rn = lambda *shape: torch.randn(*shape, generator=gen).to(torch.bfloat16)
        self.s, self.d = s, d
        self.scale = 1.0 / math.sqrt(d)
        self.q, self.k, self.v = rn(B, H, s, d), rn(B, HKV, s, d), rn(B, HKV, s, d)
        self.d_o = rn(B, H, s, d)
        self.ref = dict(zip(("o", "lse", "dq", "dk", "dv"), reference_fp64(
            self.q, self.k, self.v, self.scale, self.d_o)))
        self.base = dict(zip(("o", "dq", "dk", "dv"), baseline_bf16(
            self.q, self.k, self.v, self.scale, self.d_o)))

    def run(self, mask=None, kv_map=None):
        if mask is None:
            mask = causal_mask(self.s)
        o, lse, dq, dk_h, dv_h = emulate(self.q, self.k, self.v, self.d_o,
                                         self.scale, mask, kv_map)
        return {"o": o, "lse": lse, "dq": dq, "dk": reduce_gqa(dk_h, HKV),
                "dv": reduce_gqa(dv_h, HKV), "dk_h": dk_h}

    def ratios(self, out):
        """Every comparator's figure for one result; > 1 means rejected."""
        r = {n: blockwise_ratio(out[n], self.base[n], self.ref[n])[0]
             for n in ("o", "dq", "dk", "dv")}
        r["lse"] = lse_error(out["lse"], self.ref["lse"]) / LSE_ATOL
        return r

    def old_figures(self, out):
        """What the global max-abs checks of test_attn_bwd_gpu.py look at:
        o must stay under 3e-2, each gradient under 0.06."""
        f = {"o": float((out["o"].double() - self.ref["o"]).abs().max())}
        for n in ("dq", "dk", "dv"):
            err = (out[n].double() - self.ref[n]).abs().max()
            f[n] = float(err / self.ref[n].abs().max().clamp(min=1.0))
        return f


_cases = {}


def case(s, d):
    if (s, d) not in _cases:
        _cases[(s, d)] = Case(s, d)
    return _cases[(s, d)]


@pytest.mark.parametrize("s,d", SHAPES)
def test_clean_emulation_has_headroom(s, d):
    c = case(s, d)
    out = c.run()
    for n in ("o", "dq", "dk", "dv"):
        ratio = assert_blockwise_close(out[n], c.base[n], c.ref[n], what=n)
        print(f"S={s} D={d} {n}: worst ratio {ratio:.3f}")
        assert ratio < 0.5, (n, ratio)
    err = assert_lse_close(out["lse"], c.ref["lse"])
    print(f"S={s} D={d} lse: max err {err:.2e}")


def _mask_one_key_past_diagonal(s):
    """Row S-16 also sees key S-15: a wrong `kvcol > qrow` compare."""
    mask = causal_mask(s)
    mask[s - 16, s - 15] = False
    return mask


def _mask_last_block_skips_tile(s):
    """The last 16-row block skips the 16 keys before its diagonal block:
    an early kv_end / rb_active cut-off."""
    mask = causal_mask(s)
    mask[s - 16:, s - 32:s - 16] = True
    return mask


@pytest.mark.parametrize("s,d", SHAPES)
@pytest.mark.parametrize("make_mask", [_mask_one_key_past_diagonal,
                                       _mask_last_block_skips_tile])
def test_mask_defects_rejected(make_mask, s, d):
    c = case(s, d)
    r = c.ratios(c.run(mask=make_mask(s)))
    print(f"{make_mask.__name__} S={s} D={d}: {r}")
    assert max(r.values()) > 1.0, r


@pytest.mark.parametrize("make_mask,s,d,quantities", [
    (_mask_one_key_past_diagonal, 384, 64, ("o", "dq", "dk", "dv")),
    (_mask_last_block_skips_tile, 384, 64, ("dk", "dv")),
    (_mask_last_block_skips_tile, 384, 128, ("dq",)),
])
def test_mask_defects_pass_old_criteria(make_mask, s, d, quantities):
    """Why the suite changed: the global max-abs bounds accept these
    defects on the quantities named (the new comparators reject every one of
    them, see test_mask_defects_rejected)."""
    c = case(s, d)
    out = c.run(mask=make_mask(s))
    old, new = c.old_figures(out), c.ratios(out)
    print(f"{make_mask.__name__} S={s} D={d}: old figures {old}")
    for n in quantities:
        assert old[n] < (3e-2 if n == "o" else 0.06), (n, old)
        assert new[n] > 1.0, (n, new)


@pytest.mark.parametrize("s,d", SHAPES)
def test_one_output_element_scaled_rejected(s, d):
    c = case(s, d)
    out = c.run()
    # the largest element of a late row: 1.25x moves it by a quarter of the
    # block's own scale
    row = out["o"][1, 2, s - 5]
    out["o"][1, 2, s - 5, int(row.abs().argmax())] *= 1.25
    r = c.ratios(out)
    assert r["o"] > 1.0, r


@pytest.mark.parametrize("s,d", SHAPES)
def test_wrong_kv_head_mapping_rejected(s, d):
    c = case(s, d)
    r = c.ratios(c.run(kv_map=[i % HKV for i in range(H)]))
    assert min(r[n] for n in ("o", "dq", "dk", "dv")) > 1.0, r


@pytest.mark.parametrize("s,d", SHAPES)
def test_zeroed_d_tail_rejected(s, d):
    """What a wrong dchunks tail would do: the last 16 columns come back 0."""
    c = case(s, d)
    out = c.run()
    for n in ("o", "dq", "dk", "dv"):
        out[n][..., -16:] = 0
    r = c.ratios(out)
    assert min(r[n] for n in ("o", "dq", "dk", "dv")) > 1.0, r


@pytest.mark.parametrize("s,d", SHAPES)
def test_dk_from_one_q_head_rejected(s, d):
    c = case(s, d)
    out = c.run()
    out["dk"] = out["dk_h"][:, ::H // HKV].contiguous()
    r = c.ratios(out)
    assert r["dk"] > 1.0, r


def test_lse_bound_rejects_one_dropped_key():
    """A row of 384 keys with one key removed: a key of average weight
    (1/384) and the median-weight key of each randn row must both move LSE
    by well over LSE_ATOL."""
    c = case(384, 64)
    s = 384
    g = H // HKV
    scores = (c.q.double() @ c.k.double().repeat_interleave(g, 1)
              .transpose(-1, -2)) * c.scale              # [B, H, S, S]
    last = scores[:, :, s - 1]                            # the 384-key row
    full = torch.logsumexp(last, -1, keepdim=True)
    # LSE of the row without key j, for every j
    dropped = full + torch.log1p(-torch.exp(last - full))
    shift = (full - dropped).abs()
    print(f"smallest LSE shift from one dropped key: {float(shift.min()):.2e}"
          f", median {float(shift.median()):.2e}, bound {LSE_ATOL:g}")
    assert -math.log1p(-1.0 / s) > 10 * LSE_ATOL
    assert float(shift.median(-1).values.min()) > 10 * LSE_ATOL

    # and through the comparator itself: drop the median-weight key
    out = c.run()
    j = int(last[0, 0].argsort()[s // 2])
    out["lse"][0, 0, s - 1] = float(dropped[0, 0, j])
    with pytest.raises(AssertionError):
        assert_lse_close(out["lse"], c.ref["lse"])


def test_comparator_reports_worst_block():
    c = case(128, 64)
    out = c.run()
    out["o"][1, 3, 37, 5] += 0.5
    ratio, where, e_got, e_base = blockwise_ratio(out["o"], c.base["o"],
                                                  c.ref["o"])
    assert where == (1, 3, 37 // 16) and ratio > 1.0 and e_got > e_base
    with pytest.raises(AssertionError, match=r"\(1, 3, 2\)"):
        assert_blockwise_close(out["o"], c.base["o"], c.ref["o"], what="o")
    out["o"][0, 0, 0, 0] = float("nan")
    assert blockwise_ratio(out["o"], c.base["o"], c.ref["o"])[0] == float("inf")


def test_head_dim_predicate_matches_instantiations():
    """flash_attention must route every head dim the kernels are not
    instantiated for to SDPA instead of into a TORCH_CHECK(false)."""
    assert HEAD_DIMS == (64, 80, 96, 128)
    accepted = [d for d in range(16, 129, 16) if _head_dim_supported(d)]
    assert accepted == [64, 80, 96, 128]
    assert not _head_dim_supported(72) and not _head_dim_supported(256)

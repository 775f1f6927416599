"""Reference, baseline, inputs and the kernel emulation for the dense
decode attention tests (decode.hip, attn_decode).

Plain test support (not a conftest), a sibling of
elementwise_conformance.py, whose criterion it uses: imported by
test_decode_conformance_cpu.py and test_decode_conformance_gpu.py.

  reference   softmax(q k^T scale) v in float64 with the GQA head map
              h -> h // (H / Hkv)
  baseline    the same on bf16 eager tensors
  emulate     attn_decode_kernel in fp32, CPU: lane l holds elements l,
              l + 64 of a row, a 64-lane butterfly for the dot product,
              wave w walks the keys w, w + 4, ... with an online softmax
              (m = -1e30, l = 0 to start), and wave 0 merges the four
              (m, l, acc) triples in wave order

Criterion: the project's rule per (batch, head) row of D outputs,
ulp = 2^-8.
"""

from __future__ import annotations

import math

import torch

import elementwise_conformance as ec

BF16 = torch.bfloat16
NWAVE = 4
WAVE = 64
KINDS = ("randn", "peaked", "shifted")
MUTANTS = ("last_key_dropped", "wave_dropped", "tail_dropped",
           "wrong_kv_head")


def decode_input(b, h, hkv, s, d, kind, seed=0):
    """(q [B,H,1,D], k, v [B,Hkv,S,D]) bf16 on the CPU.

    randn     all three N(0, 1)
    peaked    q * 4: a few keys carry the weight, the running maximum
              moves and the accumulator is rescaled
    shifted   q = |randn|, k = randn - c with c = 1e4 / (0.8 D): every
              score sits near -1e4 * scale, far from the -1e30 start"""
    assert kind in KINDS, kind
    g = torch.Generator().manual_seed(seed * 7919 + s * 131 + d * 17 + h + hkv)
    q = torch.randn(b, h, 1, d, generator=g)
    k = torch.randn(b, hkv, s, d, generator=g)
    v = torch.randn(b, hkv, s, d, generator=g)
    if kind == "peaked":
        q = q * 4
    elif kind == "shifted":
        q = q.abs()
        k = k - 1e4 / (0.8 * d)
    return q.to(BF16), k.to(BF16), v.to(BF16)


def _run(q, k, v, scale, dtype):
    rep = q.size(1) // k.size(1)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    k = k.repeat_interleave(rep, dim=1)
    v = v.repeat_interleave(rep, dim=1)
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    return p @ v


def reference(q, k, v, scale):
    return _run(q, k, v, scale, torch.float64)


def baseline(q, k, v, scale):
    return _run(q, k, v, scale, BF16)


def ratio(got, base, ref) -> float:
    """One block per (batch, head)."""
    return ec.block_ratio(got, base, ref, got.size(-1), ec.ULP_BF16)


def emulate(q, k, v, scale, mutant=None):
    assert mutant is None or mutant in MUTANTS
    b, h, _, d = q.shape
    hkv, s = k.size(1), k.size(2)
    grp = h // hkv
    heads = torch.arange(h)
    kvh = heads % hkv if mutant == "wrong_kv_head" else heads // grp
    kf, vf = k.float()[:, kvh], v.float()[:, kvh]          # [B, H, S, D]
    qf = q.float()
    if mutant == "last_key_dropped":
        s -= 1
    elif mutant == "tail_dropped":
        s -= s % NWAVE
    vpl = (d + WAVE - 1) // WAVE
    pad = vpl * WAVE - d

    def lanes(t):               # [..., D] -> [..., vpl, 64], zero padded
        if pad:
            t = torch.cat([t, t.new_zeros(*t.shape[:-1], pad)], -1)
        return t.reshape(*t.shape[:-1], vpl, WAVE)

    scale = torch.tensor(scale, dtype=torch.float32)
    ql = lanes(qf[:, :, 0])                                  # [B, H, vpl, 64]
    m = torch.full((b, h, NWAVE), -1e30)
    l = torch.zeros(b, h, NWAVE)
    acc = torch.zeros(b, h, NWAVE, d)
    for r0 in range(0, s, NWAVE):
        n = min(NWAVE, s - r0)          # waves 0..n-1 have a key this trip
        kl = lanes(kf[:, :, r0:r0 + n])                      # [B,H,n,vpl,64]
        part = torch.zeros(b, h, n, WAVE)
        for i in range(vpl):
            part = part + ql[:, :, None, i] * kl[:, :, :, i]
        dot = ec._butterfly(part, torch.add) * scale
        m_new = torch.maximum(m[:, :, :n], dot)
        alpha = torch.exp(m[:, :, :n] - m_new)
        p = torch.exp(dot - m_new)
        l[:, :, :n] = l[:, :, :n] * alpha + p
        acc[:, :, :n] = (acc[:, :, :n] * alpha[..., None]
                         + p[..., None] * vf[:, :, r0:r0 + n])
        m[:, :, :n] = m_new
    gm = torch.full((b, h), -1e30)
    for w in range(NWAVE):
        gm = torch.maximum(gm, m[:, :, w])
    gl = torch.zeros(b, h)
    gacc = torch.zeros(b, h, d)
    for w in range(NWAVE):
        if mutant == "wave_dropped" and w == 2:
            continue
        aw = torch.exp(m[:, :, w] - gm)
        gl = gl + l[:, :, w] * aw
        gacc = gacc + acc[:, :, w] * aw[..., None]
    return (gacc * (1.0 / gl)[..., None]).to(BF16)[:, :, None]


def default_scale(d):
    return 1.0 / math.sqrt(d)


def dominant_case(b, h, hkv, s, d, row):
    """Key `row` of every (batch, kv head) is 4 * sign(q-ish) in every
    element and q = +-4 with the same signs, the other keys are 0: the
    scaled score of that key is 16 D / sqrt(D) >= 128 above the rest, whose
    weights exp(-128) are below half an ulp of 1 in every sum, so the
    output equals v[row] bitwise. All q heads share the signs, so any GQA
    map is served."""
    g = torch.Generator().manual_seed(s * 53 + d + row)
    sign = torch.randint(0, 2, (d,), generator=g).float() * 2 - 1
    q = (4.0 * sign).expand(b, h, 1, d).contiguous()
    k = torch.zeros(b, hkv, s, d)
    k[:, :, row] = 4.0 * sign
    v = torch.randn(b, hkv, s, d, generator=g)
    return q.to(BF16), k.to(BF16), v.to(BF16)


def dominant_rows(s):
    """Row 0, row S-1 and one row in each of the four waves' residues."""
    rows = {0, s - 1}
    for w in range(NWAVE):
        r = (s // 2) // NWAVE * NWAVE + w
        if r < s:
            rows.add(r)
    return sorted(rows)


def uniform_case(b, h, hkv, s, d, constant=None):
    """k = 0: every weight is exactly 1/S-to-be. v is the constant 1.5, or
    small integers in -4..4 whose sum is exact in fp32."""
    g = torch.Generator().manual_seed(s * 71 + d)
    q = torch.randn(b, h, 1, d, generator=g)
    k = torch.zeros(b, hkv, s, d)
    if constant is not None:
        v = torch.full((b, hkv, s, d), constant)
    else:
        v = torch.randint(-4, 5, (b, hkv, s, d), generator=g).float()
    return q.to(BF16), k.to(BF16), v.to(BF16)

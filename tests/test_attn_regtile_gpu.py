"""GPU test: exact one-hot attention through the register-resident P / dS tiles.

The attention kernels feed the accumulator of their first MFMA product
straight into the second, with a permuted k order the other operand has to
follow (attn_tile.h AccFrag / tr16_frag_acc; lane simulation in
test_attn_regtile_cpu.py). A k-order mismatch pairs P with the wrong V, K or
Q rows, which random data only shows statistically. Here every row i attends
to exactly one key t(i) <= i, all values are small integers, and every
output is known exactly:

  * the first 18 dims of k carry a +-16 two-dims-per-bit code of the key
    index, the same dims of q the code of the row's target: a matching bit
    adds 512 to the score, a differing one takes 512 off. All other dims of q
    and k, and all of v and dO, are integers in -2..2, so any other key under
    the mask scores at least 1024 - 8 (D - 18) >= 144 lower, checked in
    float64 to be >= 120: fp32 exp gives exactly 0, P is one-hot, l = 1.
  * forward: o[i] = v[t(i)] and lse[i] = the target score, bitwise.
  * backward with that lse and delta[i] = dP[i][t(i)] - g_i, g_i in
    {+-1, +-2}: dS is g_i at the target and 0 elsewhere, so
    dq[i] = g_i k[t(i)], dv[j] = sum_{t(i)=j} dO[i], dk[j] = sum g_i q[i],
    integers of magnitude <= 256 (fan-in <= 8), bitwise in bf16.

The map t is built so that, for the tile geometry of each kernel, the targets
reach every (16-row subtile, lane group, register) position both in the
diagonal tile and in earlier tiles; that is asserted on the CPU.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from metis_amd.ops import require_extension
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

B, H = 2, 2
SEQS = (128, 384)
DIMS = (64, 80, 96, 128)
BITS = 9                  # key index bits, two dims each
MAX_FAN_IN = 8
SCALE = 1.0


def target_map(h, s):
    """t(i) <= i for head h. Rows with i % 3 == i // 128 attend to themselves
    (the diagonal tile, every position: the residue class moves with the
    tile). The other rows of the first 128 draw a key at or before
    themselves; later ones walk a head-dependent permutation of the 128
    in-tile positions, in a random EARLIER 128-row tile."""
    rng = np.random.default_rng(1234 + h)
    perm = rng.permutation(128)
    t = np.zeros(s, dtype=np.int64)
    far = 0
    for i in range(s):
        if i % 3 == (i // 128) % 3:
            t[i] = i
        elif i < 128:
            t[i] = rng.integers(max(0, i - 40), i + 1)
        else:
            t[i] = 128 * rng.integers(0, i // 128) + perm[far % 128]
            far += 1
    return t


def key_code(idx):
    """[n, 2 * BITS]: bit b of idx -> (+16, -16) if set, else (-16, +16)."""
    bits = (idx[:, None] >> np.arange(BITS)[None, :]) & 1
    sign = 2.0 * bits - 1.0
    return np.stack([16.0 * sign, -16.0 * sign], axis=-1).reshape(len(idx), -1)


@functools.lru_cache(maxsize=None)
def case(s, d):
    """Inputs and float64 expectations for one (S, D), built once."""
    rng = np.random.default_rng(100 * d + s)
    q = rng.integers(-2, 3, (B, H, s, d)).astype(np.float64)
    k = rng.integers(-2, 3, (B, H, s, d)).astype(np.float64)
    v = rng.integers(-2, 3, (B, H, s, d)).astype(np.float64)
    d_o = rng.integers(-2, 3, (B, H, s, d)).astype(np.float64)
    g = rng.choice([-2.0, -1.0, 1.0, 2.0], (B, H, s))
    t = np.stack([target_map(h, s) for h in range(H)])          # [H, S]
    for h in range(H):
        k[:, h, :, :2 * BITS] = key_code(np.arange(s))
        q[:, h, :, :2 * BITS] = key_code(t[h])

    rows = np.arange(s)
    lse = np.zeros((B, H, s))
    delta = np.zeros((B, H, s))
    o = np.zeros_like(q)
    dq = np.zeros_like(q)
    dk = np.zeros_like(q)
    dv = np.zeros_like(q)
    for b in range(B):
        for h in range(H):
            score = q[b, h] @ k[b, h].T
            best = score[rows, t[h]]
            others = np.where(rows[None, :] <= rows[:, None], score, -np.inf)
            others[rows, t[h]] = -np.inf
            assert (best - others.max(axis=1) >= 120).all()
            lse[b, h] = best
            o[b, h] = v[b, h, t[h]]
            dp = d_o[b, h] @ v[b, h].T
            delta[b, h] = dp[rows, t[h]] - g[b, h]
            dq[b, h] = g[b, h][:, None] * k[b, h, t[h]]
            np.add.at(dv[b, h], t[h], d_o[b, h])
            np.add.at(dk[b, h], t[h], g[b, h][:, None] * q[b, h])
    assert max(np.abs(x).max() for x in (dq, dk, dv)) <= 256

    def dev(x, dtype=torch.bfloat16):
        y = torch.from_numpy(x).to(dtype)
        assert torch.equal(y.double(), torch.from_numpy(x))     # exact
        return y.cuda()

    f32 = torch.float32
    return dict(q=dev(q), k=dev(k), v=dev(v), d_o=dev(d_o), lse=dev(lse, f32),
                delta=dev(delta, f32), o=dev(o), dq=dev(dq), dk=dev(dk),
                dv=dev(dv))


def packed(*heads):
    """[B, H, S, D] tensors side by side as column blocks of [B, S, n H D]."""
    return torch.cat([x.transpose(1, 2).reshape(x.size(0), x.size(2), -1)
                      for x in heads], dim=-1).contiguous()


@pytest.fixture(scope="module")
def ext():
    return require_extension()


@pytest.mark.parametrize("s", (384,))
def test_targets_cover_every_tile_position(s):
    """Register positions: the key within the KV tile for fwd (128 keys at
    D <= 80, else 64) and dQ (64); the q row within the 64-row q tile for
    dKV, against the 64-key (128 at D = 64) block of the key."""
    for h in range(H):
        t = target_map(h, s)
        i = np.arange(s)
        assert (t <= i).all()
        assert np.bincount(t, minlength=s).max() <= MAX_FAN_IN
        for tile in (64, 128):          # fwd, dQ: key position in its tile
            diag = i // tile == t // tile
            assert set(t[diag] % tile) == set(range(tile))
            assert set(t[~diag] % tile) == set(range(tile))
        for block in (64, 128):         # dKV: q position in its 64-row tile
            diag = i // block == t // block
            assert set(i[diag] % 64) == set(range(64))
            assert set(i[~diag] % 64) == set(range(64))
        # every lane column on both sides
        assert set(zip(t % 16, i % 16)) >= {(a, a) for a in range(16)}


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("s", SEQS)
def test_one_hot_forward_exact(ext, s, d):
    c = case(s, d)
    o, lse = ext.attn_fwd(c["q"], c["k"], c["v"], SCALE)
    assert torch.equal(lse, c["lse"]), "lse"
    assert torch.equal(o, c["o"]), "o"
    o_p, lse_p = ext.attn_fwd_packed(packed(c["q"], c["k"], c["v"]), H, H, d,
                                     SCALE)
    assert torch.equal(lse_p, c["lse"]), "packed lse"
    assert torch.equal(o_p, packed(c["o"])), "packed o"


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("s", SEQS)
def test_one_hot_backward_exact(ext, s, d):
    c = case(s, d)
    dq, dk, dv = ext.attn_bwd(c["q"], c["k"], c["v"], c["d_o"], c["lse"],
                              c["delta"], SCALE)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.equal(got, c[name]), name
    dqkv = ext.attn_bwd_packed(packed(c["q"], c["k"], c["v"]), packed(c["d_o"]),
                               c["lse"], c["delta"], H, H, d, SCALE)
    assert torch.equal(dqkv, packed(c["dq"], c["dk"], c["dv"])), "packed dqkv"

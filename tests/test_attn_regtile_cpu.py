"""CPU lane simulation of the register-resident P / dS tiles of the attention
kernels (attn_tile.h: AccFrag, tr16_frag_acc), in the style of
scripts/gemm8_sim.py.

The lane maps of v_mfma_f32_16x16x32_bf16 (docs/KERNELS.md): lane
(c = l & 15, g = l >> 4) holds A[c][8g + i], B[8g + i][c] and C[4g + r][c].
An accumulator tile can therefore be the operand of a following product that
sums over its ROW index, with the k order permuted: element i of lane group g
is row 16 (i >> 2) + 4g + (i & 3) of the 32-row strip. The other operand has
to follow that order; its ds_read_b64_tr_b16 reads take the 4-row blocks at
rows 4g and 16 + 4g, not 8g and 8g + 4.

Each of the three operand chains of the kernels must equal the plain matrix
product on asymmetric integer data, and the natural-order tr16 rule paired
with the accumulator fragment (the mutant) must not.
"""

import numpy as np
import pytest

ROWS, D, PAD = 64, 48, 8          # natural LDS image [ROWS][D + PAD]
CHUNK, COL0 = 32, 16              # second 32-row strip, second 16-col d tile


def mfma_16x16x32(a_frag, b_frag, c):
    """a_frag, b_frag: [64 lanes][8]; c: [64 lanes][4], accumulated into."""
    a = np.zeros((16, 32))
    b = np.zeros((32, 16))
    for lane in range(64):
        col, g = lane & 15, lane >> 4
        a[col, 8 * g:8 * g + 8] = a_frag[lane]
        b[8 * g:8 * g + 8, col] = b_frag[lane]
    d = a @ b
    for lane in range(64):
        col, g = lane & 15, lane >> 4
        c[lane] += d[4 * g:4 * g + 4, col]
    return c


def lds_frag(img, row0, d0):
    """Plain fragment read: lane (c, g) takes img[row0 + c][d0 + 8g .. + 8]."""
    return np.array([img[row0 + (lane & 15), d0 + 8 * (lane >> 4):][:8]
                     for lane in range(64)])


def ds_read_tr16_b64(img, addr):
    """addr[lane] = (row, col) of the 4 elements the lane points at. Per
    16-lane group the 16 x 4 elements form a [4 rows][16 cols] block (lane p
    supplies row p >> 2, columns 4 (p & 3) ..); lane p receives column p."""
    out = np.zeros((64, 4))
    for grp in range(4):
        block = np.zeros((4, 16))
        for p in range(16):
            row, col = addr[16 * grp + p]
            block[p >> 2, 4 * (p & 3):4 * (p & 3) + 4] = img[row, col:col + 4]
        for p in range(16):
            out[16 * grp + p] = block[:, p]
    return out


def tr16_rows(img, row_lo, row_hi, col0):
    """attn_tile.h tr16_rows: row_lo / row_hi are functions of the lane group."""
    halves = []
    for rows in (row_lo, row_hi):
        addr = [(rows(lane >> 4) + ((lane & 15) >> 2), col0 + 4 * (lane & 3))
                for lane in range(64)]
        halves.append(ds_read_tr16_b64(img, addr))
    return np.concatenate(halves, axis=1)


def tr16_frag(img, chunk, col0):        # natural k order
    return tr16_rows(img, lambda g: chunk + 8 * g, lambda g: chunk + 8 * g + 4,
                     col0)


def tr16_frag_acc(img, chunk, col0):    # accumulator k order
    return tr16_rows(img, lambda g: chunk + 4 * g, lambda g: chunk + 16 + 4 * g,
                     col0)


def acc_frag(x_lo, x_hi):
    """AccFrag: the two accumulator tiles of a 32-row strip, lane by lane."""
    return np.concatenate([x_lo, x_hi], axis=1)


def first_product(img_rows, own, strip):
    """The two 16-row accumulator tiles of img_rows[strip .. +32] @ own^T
    (own: [16][D] fragments in registers, B operand), summed over D."""
    tiles = []
    for j in range(2):
        c = np.zeros((64, 4))
        for d0 in range(0, D, 32):
            a = np.zeros((64, 8))
            b = np.zeros((64, 8))
            for lane in range(64):
                col, g = lane & 15, lane >> 4
                if d0 + 8 * g < D:      # the kernels' zero D tail
                    a[lane] = img_rows[strip + 16 * j + col, d0 + 8 * g:][:8]
                    b[lane] = own[col, d0 + 8 * g:][:8]
            mfma_16x16x32(a, b, c)
        tiles.append(c)
    return tiles


def c_tile(c):
    out = np.zeros((16, 16))
    for lane in range(64):
        out[4 * (lane >> 4):4 * (lane >> 4) + 4, lane & 15] = c[lane]
    return out


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    img = np.zeros((ROWS, D + PAD))
    img[:, :D] = rng.integers(-2, 3, (ROWS, D))     # Q (dKV), K (dQ, fwd)
    other = np.zeros((ROWS, D + PAD))
    other[:, :D] = rng.integers(-2, 3, (ROWS, D))   # dO (dKV), V (fwd)
    own = rng.integers(-2, 3, (16, D)).astype(float)
    return img, other, own


def test_data_is_asymmetric(data):
    img, other, own = data
    x = img[CHUNK:CHUNK + 32, :D] @ own.T
    assert not np.array_equal(x[:16], x[16:])
    assert not np.array_equal(x[:16], x[:16].T)
    assert np.abs(x).max() <= 256          # exact in bf16


def test_tiles_as_a_operand(data):
    """dKV: dV += P^T dO and dK += dS^T Q; dQ: dQ += dS K. X = rows @ own^T,
    result[own][d] = sum over rows of X[row][own] * other[row][d]."""
    img, other, own = data
    x_lo, x_hi = first_product(img, own, CHUNK)
    x = img[CHUNK:CHUNK + 32, :D] @ own.T
    assert np.array_equal(np.vstack([c_tile(x_lo), c_tile(x_hi)]), x)
    for second in (other, img):     # P^T dO reads the other image, dS^T Q / dS K its own
        want = x.T @ second[CHUNK:CHUNK + 32, COL0:COL0 + 16]
        got = mfma_16x16x32(acc_frag(x_lo, x_hi),
                            tr16_frag_acc(second, CHUNK, COL0), np.zeros((64, 4)))
        assert np.array_equal(c_tile(got), want)
        mutant = mfma_16x16x32(acc_frag(x_lo, x_hi),
                               tr16_frag(second, CHUNK, COL0), np.zeros((64, 4)))
        assert not np.array_equal(c_tile(mutant), want)
        assert (c_tile(mutant) != want).mean() > 0.5


def test_tiles_as_b_operand(data):
    """fwd: O^T += V^T P^T with S^T = K Q^T; result[d][q], q on the lane."""
    img, other, own = data
    x_lo, x_hi = first_product(img, own, CHUNK)
    x = img[CHUNK:CHUNK + 32, :D] @ own.T
    want = other[CHUNK:CHUNK + 32, COL0:COL0 + 16].T @ x
    got = mfma_16x16x32(tr16_frag_acc(other, CHUNK, COL0), acc_frag(x_lo, x_hi),
                        np.zeros((64, 4)))
    assert np.array_equal(c_tile(got), want)
    mutant = mfma_16x16x32(tr16_frag(other, CHUNK, COL0), acc_frag(x_lo, x_hi),
                           np.zeros((64, 4)))
    assert (c_tile(mutant) != want).mean() > 0.5


def test_natural_rule_still_matches_natural_fragments(data):
    """The rule the kernels had: a natural-order A fragment read back from a
    [16][32] tile against tr16_frag."""
    img, other, own = data
    x = img[CHUNK:CHUNK + 32, :D] @ own.T           # [32][16]
    want = x.T @ other[CHUNK:CHUNK + 32, COL0:COL0 + 16]
    got = mfma_16x16x32(lds_frag(x.T.copy(), 0, 0), tr16_frag(other, CHUNK, COL0),
                        np.zeros((64, 4)))
    assert np.array_equal(c_tile(got), want)

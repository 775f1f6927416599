"""transpose_bf16 (transpose.hip): bitwise against w.t().contiguous().

Index-pattern data (element (r, c) holds a value that depends on r and c,
distinct within any 64 x 64 tile and across tile boundaries) so that a chunk
written to the wrong row, column or tile shows. Shapes: one 16-byte chunk
(8 x 8), a partial tile in the columns only (8 x 520), partial tiles at both
edges (72 x 136), more row tiles than one with a single column tile
(264 x 64) and many tiles with both edges partial (1032 x 2568). The _out
form writes into a buffer pre-filled with NaN, so an element it leaves out
shows as well. A size that is no multiple of 8, an fp32 tensor and a
non-contiguous view are rejected by the launcher.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from metis_amd.ops import require_extension
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
SHAPES = [(8, 8), (8, 520), (72, 136), (264, 64), (1032, 2568)]


@pytest.fixture(scope="module")
def ext():
    return require_extension()


def index_pattern(r, c):
    """bf16 [r, c] whose bit pattern is (row * 131 + col * 7) mod 2^15: every
    value a finite or at least comparable-by-bits positive bf16, neighbours
    in both directions distinct."""
    rows = torch.arange(r, device="cuda", dtype=torch.int64)[:, None]
    cols = torch.arange(c, device="cuda", dtype=torch.int64)[None, :]
    bits = ((rows * 131 + cols * 7) % 0x7F80).to(torch.int16)
    return bits.view(BF16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16),
                                              b.contiguous().view(torch.int16))


@pytest.mark.parametrize("r,c", SHAPES)
def test_transpose_bitwise(ext, r, c):
    w = index_pattern(r, c)
    assert same_bits(ext.transpose_bf16(w), w.t().contiguous())


@pytest.mark.parametrize("r,c", SHAPES)
def test_transpose_out_overwrites_all(ext, r, c):
    w = index_pattern(r, c)
    wt = torch.full((c, r), float("nan"), device="cuda", dtype=BF16)
    ext.transpose_bf16_out(w, wt)
    assert same_bits(wt, w.t().contiguous())


def test_transpose_rejects(ext):
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ext.transpose_bf16(torch.zeros(12, 16, device="cuda", dtype=BF16))
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ext.transpose_bf16(torch.zeros(16, 20, device="cuda", dtype=BF16))
    with pytest.raises(RuntimeError, match="bf16"):
        ext.transpose_bf16(torch.zeros(16, 16, device="cuda"))
    view = torch.zeros(16, 32, device="cuda", dtype=BF16)[:, ::2]
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.transpose_bf16(view)
    w = torch.zeros(16, 24, device="cuda", dtype=BF16)
    with pytest.raises(RuntimeError, match="wt must be"):
        ext.transpose_bf16_out(w, torch.zeros(16, 24, device="cuda", dtype=BF16))

"""GPU conformance of the head relayout kernels (relayout.hip):
qkv_split_transpose, qkv_split_transpose_bwd, heads_merge, heads_unmerge.

Pure data movement, so every comparison is bitwise against eager
split / view / transpose, on data that names its source: element i holds
the low 16 bits of i, and in a second pass the high 16 bits, viewed as
bf16. Together the two passes tell every source element of a tensor
apart; a misplaced 16-byte chunk cannot land on equal data. The patterns
include NaNs, which are unequal to themselves under torch.equal, so the
comparison goes through .view(torch.int16).

Shapes: every head dim the models use (D / 8 = 8, 10, 12, 16 chunks per
row: 10 and 12 exercise the i % dv walk off the power-of-two path), MHA,
GQA and MQA head counts including odd ones, one batch and three, S = 1, 7
and 130, and one case per kernel of more than 2048 * 256 = 524288 chunks,
where the grid-stride loop makes a second trip.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from metis_amd.ops import require_extension
    from metis_amd.ops.relayout import heads_merge, qkv_split_transpose
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
HEAD_DIMS = (64, 80, 96, 128)
HEADS = ((4, 4), (8, 2), (6, 2), (5, 1))
SMALL = [(b, s) for b in (1, 3) for s in (1, 7, 130)]
BIG = (2, 3300, 8, 2, 80)     # merge: 2 * 3300 * 8 * 10 = 528000 chunks
ONE_TRIP_CHUNKS = 2048 * 256


@pytest.fixture(scope="module")
def ext():
    return require_extension()


def _pattern(shape, part):
    """bf16 tensor whose element i carries bits 16*part .. 16*part+15 of i."""
    n = 1
    for v in shape:
        n *= v
    bits = (torch.arange(n, device="cuda") >> (16 * part)) & 0xFFFF
    bits = (bits + 32768) % 65536 - 32768
    return bits.to(torch.int16).view(BF16).view(*shape)


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == BF16
    return torch.equal(a.contiguous().view(torch.int16),
                       b.contiguous().view(torch.int16))


def _split_eager(qkv, nq, nkv, d):
    b, s, _ = qkv.shape
    q, k, v = qkv.split([nq * d, nkv * d, nkv * d], -1)
    return (q.view(b, s, nq, d).transpose(1, 2),
            k.view(b, s, nkv, d).transpose(1, 2),
            v.view(b, s, nkv, d).transpose(1, 2))


def _gather_eager(dq, dk, dv):
    b, _, s, _ = dq.shape
    return torch.cat([t.transpose(1, 2).reshape(b, s, -1)
                      for t in (dq, dk, dv)], dim=-1)


def _check_all(ext, b, s, nq, nkv, d):
    ht = nq + 2 * nkv
    for part in (0, 1):
        qkv = _pattern((b, s, ht * d), part)
        got = ext.qkv_split_transpose(qkv, nq, nkv, d)
        for g, w in zip(got, _split_eager(qkv, nq, nkv, d)):
            assert g.is_contiguous() and _same(g, w)
        # backward of the split on its own patterns, and the round trip
        assert _same(ext.qkv_split_transpose_bwd(*got, d), qkv)
        # each operand numbered apart, so a chunk taken from the wrong one
        # of dq/dk/dv differs
        dq = _pattern((b, nq, s, d), part)
        dk = _pattern((b, nkv, s, d), part).flip(1).contiguous()
        dv = _pattern((b, nkv, s, d), part).flip(2).contiguous()
        dqkv = ext.qkv_split_transpose_bwd(dq, dk, dv, d)
        assert _same(dqkv, _gather_eager(dq, dk, dv))
        for g, w in zip(ext.qkv_split_transpose(dqkv, nq, nkv, d),
                        (dq, dk, dv)):
            assert _same(g, w)

        x = _pattern((b, nq, s, d), part)
        y = ext.heads_merge(x)
        assert _same(y, x.transpose(1, 2).reshape(b, s, nq * d))
        assert _same(ext.heads_unmerge(y, nq), x)
        yy = _pattern((b, s, nq * d), part)
        xx = ext.heads_unmerge(yy, nq)
        assert _same(xx, yy.view(b, s, nq, d).transpose(1, 2))
        assert _same(ext.heads_merge(xx), yy)


@pytest.mark.parametrize("nq,nkv", HEADS)
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_relayout_kernels(ext, d, nq, nkv):
    for b, s in SMALL:
        _check_all(ext, b, s, nq, nkv, d)


def test_relayout_kernels_second_grid_trip(ext):
    b, s, nq, nkv, d = BIG
    assert b * s * nq * d // 8 > ONE_TRIP_CHUNKS        # merge / unmerge
    _check_all(ext, b, s, nq, nkv, d)


@pytest.mark.parametrize("b,s,nq,nkv,d", [(3, 7, 6, 2, 80), (1, 130, 5, 1, 96),
                                          (2, 130, 8, 2, 64)])
def test_relayout_autograd_wrappers(b, s, nq, nkv, d):
    """ops/relayout.py: forward and backward through autograd, with
    gradients that arrive as non-contiguous views."""
    qkv = _pattern((b, s, (nq + 2 * nkv) * d), 0).requires_grad_(True)
    q, k, v = qkv_split_transpose(qkv, nq, nkv, d)
    for g, w in zip((q, k, v), _split_eager(qkv.detach(), nq, nkv, d)):
        assert _same(g.detach(), w)
    gq = _pattern((b, s, nq, d), 0).transpose(1, 2)
    gk = _pattern((b, s, nkv, d), 0).flip(0).transpose(1, 2)
    gv = _pattern((b, s, nkv, d), 0).flip(1).transpose(1, 2)
    assert not gq.is_contiguous() or s == 1
    torch.autograd.backward([q, k, v], [gq, gk, gv])
    assert _same(qkv.grad, _gather_eager(gq, gk, gv))

    x = _pattern((b, nq, s, d), 0).requires_grad_(True)
    y = heads_merge(x)
    assert _same(y.detach(), x.detach().transpose(1, 2).reshape(b, s, nq * d))
    gy = _pattern((s, b, nq * d), 0).transpose(0, 1)
    y.backward(gy)
    assert _same(x.grad, gy.reshape(b, s, nq, d).transpose(1, 2))


# --- argument checks ------------------------------------------------------
# Every bad tensor is on the device and at least as large in bytes as what
# the unguarded kernel would read.
def _z(*shape, dtype=BF16):
    return torch.zeros(*shape, device="cuda", dtype=dtype)


B_, S_, NQ_, NKV_, D_ = 2, 16, 4, 2, 64


def _bwd_args():
    return {"dq": _z(B_, NQ_, S_, D_), "dk": _z(B_, NKV_, S_, D_),
            "dv": _z(B_, NKV_, S_, D_), "d": D_}


BAD_SPLIT_BWD = {
    "dq_fp32": lambda a: a.update(dq=a["dq"].float()),
    "dk_fp16": lambda a: a.update(dk=a["dk"].to(torch.float16)),
    "dv_fp32": lambda a: a.update(dv=a["dv"].float()),
    "dk_longer_sequence": lambda a: a.update(dk=_z(B_, NKV_, S_ + 1, D_),
                                             dv=_z(B_, NKV_, S_ + 1, D_)),
    "dv_more_heads": lambda a: a.update(dv=_z(B_, NKV_ + 1, S_, D_)),
    "dk_more_batches": lambda a: a.update(dk=_z(B_ + 1, NKV_, S_, D_),
                                          dv=_z(B_ + 1, NKV_, S_, D_)),
    "dk_wider_head": lambda a: a.update(dk=_z(B_, NKV_, S_, D_ + 8),
                                        dv=_z(B_, NKV_, S_, D_ + 8)),
    "head_dim_halved": lambda a: a.update(d=D_ // 2),
    "head_dim_not_multiple_of_8": lambda a: a.update(
        dq=_z(B_, NQ_, S_, 60), dk=_z(B_, NKV_, S_, 60),
        dv=_z(B_, NKV_, S_, 60), d=60),
    "dq_3d": lambda a: a.update(dq=_z(B_ * NQ_, S_, D_)),
}


@pytest.mark.parametrize("bad", sorted(BAD_SPLIT_BWD))
def test_qkv_split_transpose_bwd_rejects(ext, bad):
    a = _bwd_args()
    BAD_SPLIT_BWD[bad](a)
    with pytest.raises(RuntimeError):
        ext.qkv_split_transpose_bwd(a["dq"], a["dk"], a["dv"], a["d"])
    torch.cuda.synchronize()


BAD_UNMERGE = {
    "y_fp32": lambda: (_z(B_, S_, NQ_ * D_, dtype=torch.float32), NQ_),
    "y_fp16": lambda: (_z(B_, S_, NQ_ * D_, dtype=torch.float16), NQ_),
    "y_2d": lambda: (_z(B_ * S_, NQ_ * D_), NQ_),
    "y_4d": lambda: (_z(B_, S_, NQ_, D_), NQ_),
    "heads_do_not_divide": lambda: (_z(B_, S_, NQ_ * D_), 5),
    "head_dim_not_multiple_of_8": lambda: (_z(B_, S_, NQ_ * 60), NQ_),
    "heads_zero": lambda: (_z(B_, S_, NQ_ * D_), 0),
}


@pytest.mark.parametrize("bad", sorted(BAD_UNMERGE))
def test_heads_unmerge_rejects(ext, bad):
    y, h = BAD_UNMERGE[bad]()
    with pytest.raises(RuntimeError):
        ext.heads_unmerge(y, h)
    torch.cuda.synchronize()

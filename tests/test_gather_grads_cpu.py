"""FusedAdamW.gather_grads fills the flat fp32 buffer with one converting
copy per parameter; the result must equal the earlier two-step expression
(fp32 temporary, then copy) bit for bit."""

import torch

from metis_amd.ops import FusedAdamW


def test_gather_grads_equals_float_then_copy():
    torch.manual_seed(0)
    params = [
        torch.nn.Parameter(torch.randn(7, 5).to(torch.bfloat16)),
        torch.nn.Parameter(torch.randn(11)),                       # fp32
        torch.nn.Parameter(torch.randn(3, 2, 4).to(torch.bfloat16)),
        torch.nn.Parameter(torch.randn(6).to(torch.bfloat16)),     # grad None
        torch.nn.Parameter(torch.randn(9, 3)),
    ]
    opt = FusedAdamW(params, lr=1e-3)
    for i, p in enumerate(params):
        if i != 3:
            p.grad = torch.randn(p.shape).to(p.dtype)
    # non-contiguous gradient: reshape(-1) has to copy it
    params[4].grad = torch.randn(3, 9).t()
    assert not params[4].grad.is_contiguous()
    # stale contents must not survive where grad is None
    opt.grad_flat.fill_(123.0)

    want = torch.zeros_like(opt.grad_flat)
    off = 0
    for p in params:
        n = p.numel()
        if p.grad is not None:
            want[off:off + n].copy_(p.grad.reshape(-1).float())
        off += n

    got = opt.gather_grads()
    assert got is opt.grad_flat and got.dtype == torch.float32
    assert torch.equal(got[:off], want[:off])
    assert torch.equal(got[70:76], torch.zeros(6))     # the grad=None slot

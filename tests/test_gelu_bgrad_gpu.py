"""GPU conformance of gelu_tanh_bwd_bgrad (gelu.hip): the tanh GeLU
backward that also returns the column sums of the dh it writes.

dh is compared with the float64 formula under the project's blockwise
criterion per (row, 256 columns),

    max|got - ref| <= 2 * max|base - ref| + 2^-8 * max|ref|

with `base` the same formula on bf16 eager tensors, on randn, on h x 8 and
on h within 0.02 of the sign change of gelu' (-0.7518). dbias is compared
with the float64 column sum of the RETURNED dh under the any-order fp32
sum bound rows * 2^-24 * sum|dh|. Exact case (h in {0, +20, -20}, integer
da): dh = da/2, da and +-0 bitwise and dbias equals float64 bitwise, which
is what sees a dropped or doubled row or slab in 12293 rows.

Shapes: N of one lane (8), a partial second wave (520), one full strip
(2048), five strips (10240), with 1 row, fewer rows than an iteration and
partial last iterations; 12293 x 512 has more row groups than slabs.

The distance to aten's gelu_backward (count of differing bf16 values and
the largest distance in bf16 ulps) is printed, not asserted. The worst
ratios are printed (-s) and recorded in docs/KERNELS.md;
test_gelu_bgrad_cpu.py shows that the criterion passes an fp32 emulation of
the kernel and rejects its mutants.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gelu_bgrad_conformance as gb
    from metis_amd.ops import require_extension
else:
    pytest.skip("requires MI355X GPU", allow_module_level=True)

BF16 = torch.bfloat16
SHAPES = [(r, n) for n in (8, 520, 2048, 10240) for r in (1, 3, 33, 257)]
SHAPES.append((12293, 512))


@pytest.fixture(scope="module")
def ext():
    return require_extension()


@pytest.mark.parametrize("rows,n", SHAPES)
def test_gelu_bwd_bgrad(ext, rows, n):
    for kind in gb.KINDS:
        h, da = gb.gelu_input(rows, n, kind, device="cuda")
        dh, dbias = ext.gelu_tanh_bwd_bgrad(h, da)
        assert dh.dtype == BF16 and dh.shape == h.shape
        assert dbias.dtype == torch.float32 and dbias.shape == (n,)
        what = f"{rows}x{n} {kind}"
        r_dh = gb.dh_ratio(dh, gb.baseline(h, da), gb.reference(h, da))
        r_db = gb.dbias_ratio(dbias, dh)
        count, ulps = gb.aten_distance(dh, h, da)
        print(f"RATIO gelu dh {what}: {r_dh:.3f}")
        print(f"RATIO gelu dbias {what}: {r_db:.3f}")
        print(f"ATEN gelu dh {what}: {count} of {dh.numel()} differ, "
              f"max {ulps} ulp")
        assert r_dh <= 1.0 and r_db <= 1.0, (what, r_dh, r_db)
        if kind == "randn":
            again = ext.gelu_tanh_bwd_bgrad(h, da)   # repeated: same bits
            assert torch.equal(again[0], dh) and torch.equal(again[1], dbias)


@pytest.mark.parametrize("rows,n", SHAPES)
def test_gelu_bwd_bgrad_exact(ext, rows, n):
    h, da, want = gb.exact_case(rows, n, device="cuda")
    dh, dbias = ext.gelu_tanh_bwd_bgrad(h, da)
    assert torch.equal(dh.float(), want.float())     # +-0 compare equal
    assert torch.equal(dbias.double(), dh.double().sum(0))


def test_gelu_bwd_bgrad_accepts_3d(ext):
    h, da = gb.gelu_input(6, 520, "randn", device="cuda")
    flat = ext.gelu_tanh_bwd_bgrad(h, da)
    got = ext.gelu_tanh_bwd_bgrad(h.view(2, 3, 520), da.view(2, 3, 520))
    assert got[0].shape == (2, 3, 520) and got[1].shape == (520,)
    assert torch.equal(got[0].view(6, 520), flat[0])
    assert torch.equal(got[1], flat[1])


def _z(*shape, dtype=BF16):
    return torch.zeros(*shape, device="cuda", dtype=dtype)


BAD = {
    "h_fp32": lambda a: a.update(h=a["h"].float()),
    "da_fp16": lambda a: a.update(da=a["da"].half()),
    "da_more_rows": lambda a: a.update(da=_z(9, 512)),
    "da_other_row_length": lambda a: a.update(da=_z(16, 256)),
    "h_strided": lambda a: a.update(h=_z(8, 1024)[:, ::2]),
    "da_strided": lambda a: a.update(da=_z(8, 1024)[:, ::2]),
    "da_cpu": lambda a: a.update(da=a["da"].cpu()),
    "n_not_multiple_of_8": lambda a: a.update(h=_z(8, 516), da=_z(8, 516)),
}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_gelu_bwd_bgrad_rejects(ext, bad):
    h, da = gb.gelu_input(8, 512, "randn", device="cuda")
    a = {"h": h, "da": da}
    BAD[bad](a)
    with pytest.raises(RuntimeError):
        ext.gelu_tanh_bwd_bgrad(a["h"], a["da"])
    torch.cuda.synchronize()

"""The backward-GEMM algorithm table of metis_amd.ops.linear, without a GPU:
parsing, the fall-back to the aten route on a version or device mismatch, on
a malformed file and on a miss, and linear() against F.linear on fp32 CPU
tensors. The tests build their own small tables and never read the committed
one.
"""

import json
import logging

import pytest
import torch
import torch.nn.functional as F

from metis_amd.ops import linear as L

GOOD = {
    "hipblaslt_version": 100200,
    "device": "AMD Instinct MI355X",
    "entries": [
        {"op": "dgrad", "M": 32768, "N": 2560, "K": 10240, "route": "lt_tn",
         "algo": -1, "best_us": 1.0, "default_us": 2.0, "aten_us": 3.0},
        {"op": "dgrad", "M": 32768, "N": 2560, "K": 2560, "route": "aten",
         "algo": -1},
        {"op": "wgrad", "M": 32768, "N": 2560, "K": 10240, "route": "lt",
         "algo": 4711},
    ],
}


def write(tmp_path, obj):
    p = tmp_path / "table.json"
    p.write_text(obj if isinstance(obj, str) else json.dumps(obj))
    return str(p)


def test_parse_and_lookup(tmp_path):
    t = L.load_table(write(tmp_path, GOOD))
    assert t.matches(100200, "AMD Instinct MI355X")
    assert t.lookup("dgrad", 32768, 2560, 10240) == ("lt_tn", -1)
    assert t.lookup("dgrad", 32768, 2560, 2560) == ("aten", -1)
    assert t.lookup("wgrad", 32768, 2560, 10240) == ("lt", 4711)
    assert len(t.entries) == 3


def test_miss_is_aten(tmp_path):
    t = L.load_table(write(tmp_path, GOOD))
    assert t.lookup("wgrad", 32768, 2560, 2560) == ("aten", -1)
    assert t.lookup("dgrad", 32760, 2560, 10240) == ("aten", -1)
    assert t.lookup("dgrad", 32768, 10240, 2560) == ("aten", -1)


@pytest.mark.parametrize("version,device", [
    (100201, "AMD Instinct MI355X"), (100200, "AMD Instinct MI300X")])
def test_mismatch_falls_back_everywhere(tmp_path, caplog, version, device):
    t = L.load_table(write(tmp_path, GOOD))
    with caplog.at_level(logging.WARNING, logger=L.__name__):
        r = L.resolve_table(t, version, device)
    assert not r.entries
    for e in GOOD["entries"]:
        assert r.lookup(e["op"], e["M"], e["N"], e["K"]) == ("aten", -1)
    assert len([m for m in caplog.records if m.levelno == logging.WARNING]) == 1
    assert L.resolve_table(t, 100200, "AMD Instinct MI355X") is t


def _with(i, **kw):
    obj = json.loads(json.dumps(GOOD))
    obj["entries"][i].update(kw)
    return obj


MALFORMED = [
    "{ not json",
    "[]",
    {"device": "x", "entries": []},
    {"hipblaslt_version": "1", "device": "x", "entries": []},
    {"hipblaslt_version": 1, "device": "x", "entries": {}},
    _with(0, op="fwd"),
    _with(0, route="fastest"),
    _with(2, route="lt_tn"),            # the TN route is a dgrad route only
    _with(1, M=0),
    _with(1, N="2560"),
    _with(2, algo=-2),
    _with(2, algo=1.5),
    _with(1, K=10240, N=2560, route="lt"),   # duplicate key of entry 0
]


@pytest.mark.parametrize("obj", MALFORMED)
def test_malformed_falls_back_everywhere(tmp_path, caplog, obj):
    """One bad entry voids the whole table, not only itself."""
    with caplog.at_level(logging.WARNING, logger=L.__name__):
        t = L.load_table(write(tmp_path, obj))
    assert not t.entries
    assert t.lookup("dgrad", 32768, 2560, 10240) == ("aten", -1)
    assert len([m for m in caplog.records if m.levelno == logging.WARNING]) == 1


def test_missing_file_falls_back(tmp_path):
    assert not L.load_table(str(tmp_path / "absent.json")).entries


def _grads(fn, x, w, b, dy):
    x = x.clone().requires_grad_()
    w = w.clone().requires_grad_()
    b = None if b is None else b.clone().requires_grad_()
    y = fn(x, w, b)
    y.backward(dy)
    return y, x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(3, 5, 24), (7, 24)])
def test_linear_is_f_linear_on_cpu(shape, bias):
    """With no table linear() is F.linear, forward and backward, bitwise."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g)
    w = torch.randn(40, 24, generator=g)
    b = torch.randn(40, generator=g) if bias else None
    dy = torch.randn(*shape[:-1], 40, generator=g)
    with L.use_table(L.GemmTable.empty()):
        got = _grads(L.linear, x, w, b, dy)
    ref = _grads(F.linear, x, w, b, dy)
    for a, r in zip(got, ref):
        assert (a is None and r is None) or torch.equal(a, r)


def test_linear_bias_without_grad_on_cpu():
    """The fused block passes a detached bias: no gradient is returned."""
    x = torch.randn(4, 24, requires_grad=True)
    w = torch.randn(40, 24, requires_grad=True)
    b = torch.randn(40)
    L.linear(x, w, b).sum().backward()
    assert b.grad is None and x.grad is not None and w.grad is not None


def test_env_switch_restores_f_linear(monkeypatch):
    monkeypatch.setenv("METIS_LT_BWD", "0")
    x = torch.randn(4, 24, requires_grad=True)
    w = torch.randn(40, 24, requires_grad=True)
    y = L.linear(x, w)
    assert type(y.grad_fn).__name__ != "_LinearBackward"
    monkeypatch.setenv("METIS_LT_BWD", "1")
    assert type(L.linear(x, w).grad_fn).__name__ == "_LinearBackward"

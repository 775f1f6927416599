"""The weight-gradient routes on transposed activations in the algorithm
table of metis_amd.ops.linear, without a GPU: the strict parser takes them
for ``wgrad`` only, and one malformed entry still voids the whole table.
"""

import json
import logging

import pytest

from metis_amd.ops import linear as L

NEW_ROUTES = ("lt_dyt", "lt_xt", "lt_xt_nn", "lt_dyt_xt")


def _table(op, route, algo=-1, **extra):
    return {
        "hipblaslt_version": 100000,
        "device": "gfx950-256cu",
        "entries": [
            {"op": "dgrad", "M": 32768, "N": 2560, "K": 10240,
             "route": "lt_tn", "algo": -1},
            dict({"op": op, "M": 32768, "N": 10240, "K": 2560,
                  "route": route, "algo": algo}, **extra),
        ],
    }


def _load(tmp_path, obj):
    p = tmp_path / "table.json"
    p.write_text(json.dumps(obj))
    return L.load_table(str(p))


def test_routes_are_listed():
    assert set(NEW_ROUTES) <= set(L.ROUTES["wgrad"])
    assert not set(NEW_ROUTES) & set(L.ROUTES["dgrad"])
    assert {"aten", "lt"} <= set(L.ROUTES["wgrad"])


@pytest.mark.parametrize("algo", [-1, 617780])
@pytest.mark.parametrize("route", NEW_ROUTES)
def test_wgrad_accepts(tmp_path, route, algo):
    t = _load(tmp_path, _table("wgrad", route, algo, lt_xt_us=1500.0))
    assert len(t.entries) == 2
    assert t.lookup("wgrad", 32768, 10240, 2560) == (route, algo)
    assert t.lookup("dgrad", 32768, 2560, 10240) == ("lt_tn", -1)
    # the other op at the same shape, and the same op elsewhere, miss
    assert t.lookup("dgrad", 32768, 10240, 2560) == ("aten", -1)
    assert t.lookup("wgrad", 32768, 2560, 10240) == ("aten", -1)


@pytest.mark.parametrize("route", NEW_ROUTES)
def test_dgrad_rejects_and_voids_the_table(tmp_path, caplog, route):
    with caplog.at_level(logging.WARNING, logger=L.__name__):
        t = _load(tmp_path, _table("dgrad", route))
    assert not t.entries
    assert t.lookup("dgrad", 32768, 2560, 10240) == ("aten", -1)
    assert len([m for m in caplog.records if m.levelno == logging.WARNING]) == 1


@pytest.mark.parametrize("bad", [
    {"route": "lt_yt"}, {"algo": -2}, {"algo": 1.5}, {"algo": True},
    {"M": 0}, {"K": "2560"}, {"op": "wgrad_xt"}])
def test_malformed_new_route_entry_voids_the_table(tmp_path, caplog, bad):
    """A good lt_xt entry with one bad field: the good dgrad entry beside
    it is not applied either."""
    obj = _table("wgrad", "lt_xt")
    obj["entries"][1].update(bad)
    with caplog.at_level(logging.WARNING, logger=L.__name__):
        t = _load(tmp_path, obj)
    assert not t.entries
    assert t.lookup("dgrad", 32768, 2560, 10240) == ("aten", -1)
    assert len([m for m in caplog.records if m.levelno == logging.WARNING]) == 1


def test_committed_table_parses():
    """The committed file is well formed and every wgrad route in it is one
    linear() can dispatch."""
    with open(L.TABLE_PATH) as f:
        t = L.GemmTable.parse(json.load(f))
    assert t.entries
    for (op, *_), (route, _) in t.entries.items():
        assert route in L.ROUTES[op]

"""Which kernels a convolution / ConvBNReLU call launches (tests/golden/conv_routes.json, recorded by
tests/golden/make_golden_conv_routes.py): numeric goldens pass just as well when a call silently falls to the library, so
here the ordered launch trace, the library calls and -- under deterministic mode -- the bytes of the results are held."""
import json
import os

import pytest

import make_golden_conv_routes as G
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "conv_routes.json")) as _f:
    FIXTURE = json.load(_f)["cases"]


def _plain(v):
    """what json makes of a record (tuples -> lists)"""
    return json.loads(json.dumps(v))


def test_fixture_covers_the_cases():
    assert sorted(FIXTURE) == sorted(G.CASES)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_unstable_only_with_a_library_call(name):
    want = FIXTURE[name]
    assert not want.get("unstable") or want["det_library"]
    assert ("aten_only" in want) == (name in G.ATEN_ONLY)
    if "aten_only" in want:
        assert not (want["trace"] or want["library"] or want["det_trace"] or want["det_library"] or "raises" in want)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_route(dev, monkeypatch, name):
    from refign_amd import _lib
    want = FIXTURE[name]
    tracer = G.Tracer(_lib.call)
    monkeypatch.setattr(_lib, "call", tracer)
    plain = _plain(G.record(name, dev, tracer, False))
    det = _plain(G.record(name, dev, tracer, True))
    assert plain["trace"] == want["trace"]
    assert plain["library"] == want["library"]
    assert det["trace"] == want["det_trace"]
    assert det["library"] == want["det_library"]
    assert plain.get("raises") == want.get("raises") and det.get("raises") == want.get("raises")
    if "raises" not in want:
        if want.get("unstable") or "aten_only" in want:          # held by the traces; the generator's docstring says which and why
            assert det["hashes"]["out_meta"] == want["hashes"]["out_meta"]
            assert "aten_only" in want or sorted(det["hashes"]) == sorted(want["hashes"])
        else:
            assert det["hashes"] == want["hashes"]

"""The host helpers of ``hostops.py`` that need no GPU: the parameter key and the cache built on it, the gradient normaliser,
and the boolean opt-ins as the classifier reads them."""
import types

import pytest
import torch
import torch.nn as nn

from ed_gated_gcn_amd import hostops
from ed_gated_gcn_amd.classifier import GatedGCNEventDetector
from ed_gated_gcn_amd.csr import tensor_version


def test_param_key_names_pointer_version_and_device():
    a, b = torch.zeros(3), torch.zeros(2, 2)
    key = hostops.param_key(a, None, b)
    assert key == ((a.data_ptr(), a._version, a.device), None, (b.data_ptr(), b._version, b.device))
    assert hostops.param_key() == ()
    a.add_(1.0)                                        # an in-place update moves the version, not the pointer
    after = hostops.param_key(a, None, b)
    assert after != key and after[0][0] == key[0][0] and after[0][1] == key[0][1] + 1 and after[1:] == key[1:]
    p = nn.Parameter(torch.zeros(3))
    before = hostops.param_key(p)
    p.data = torch.zeros(3)                            # a re-assigned .data moves the pointer
    assert hostops.param_key(p)[0][0] != before[0][0]
    with torch.inference_mode():
        t = torch.zeros(3)
    assert tensor_version(t) is None
    assert hostops.param_key(t) == ((t.data_ptr(), None, t.device),) == hostops.param_key(t)   # compares equal to itself: no rebuild


def test_cached_rebuilds_on_a_new_key_only():
    owner, w, built = nn.Linear(2, 2), torch.zeros(3), []

    def build():
        built.append(len(built))
        return "value %d" % built[-1]
    assert not hasattr(owner, "_kept")
    assert hostops.cached(owner, "_kept", hostops.param_key(w), build) == "value 0"
    assert owner._kept == (hostops.param_key(w), "value 0")                 # (key, value) under the attribute
    assert hostops.cached(owner, "_kept", hostops.param_key(w), build) == "value 0" and built == [0]
    w.mul_(2.0)
    assert hostops.cached(owner, "_kept", hostops.param_key(w), build) == "value 1" and built == [0, 1]
    assert owner._kept == (hostops.param_key(w), "value 1")
    owner._none = None                                                      # an attribute that holds None counts as empty
    assert hostops.cached(owner, "_none", 7, build) == "value 2" and owner._none == (7, "value 2")


def test_cached_slots_sit_side_by_side():
    owner, w, built = types.SimpleNamespace(), torch.zeros(3), []

    def build(tag):
        built.append(tag)
        return tag
    key = hostops.param_key(w)
    assert not hasattr(owner, "_slots")
    assert hostops.cached(owner, "_slots", key, lambda: build("a0"), slot="a") == "a0"
    assert hostops.cached(owner, "_slots", key, lambda: build("b0"), slot=("b", True)) == "b0"
    assert owner._slots == {"a": (key, "a0"), ("b", True): (key, "b0")}
    assert hostops.cached(owner, "_slots", key, lambda: build("a1"), slot="a") == "a0" and built == ["a0", "b0"]
    w.add_(1.0)
    key2 = hostops.param_key(w)
    assert hostops.cached(owner, "_slots", key2, lambda: build("a1"), slot="a") == "a1"     # one slot rebuilds, the other keeps its
    assert owner._slots == {"a": (key2, "a1"), ("b", True): (key, "b0")}                  # own key until it is asked for


def test_f32_rows():
    assert hostops.f32_rows(None) is None and hostops.f32_rows(None, (2, 3)) is None
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    assert hostops.f32_rows(t) is t                                          # contiguous float32: handed on as it lies
    r = hostops.f32_rows(t, (3, 2))
    assert r.data_ptr() == t.data_ptr() and r.shape == (3, 2)                # ... a view of it under another shape
    h = t.to(torch.bfloat16)
    c = hostops.f32_rows(h)
    assert c.dtype == torch.float32 and c.is_contiguous() and c.data_ptr() != h.data_ptr() and torch.equal(c, t)
    s = torch.arange(12, dtype=torch.float32).reshape(2, 6)[:, ::2]          # strided
    c = hostops.f32_rows(s)
    assert c.is_contiguous() and c.data_ptr() != s.data_ptr() and torch.equal(c, s)
    e = torch.ones(()).expand(2, 3)                                          # an expanded scalar, as a loss hands it back
    c = hostops.f32_rows(e, (6, 1))
    assert c.is_contiguous() and c.shape == (6, 1) and torch.equal(c, torch.ones(6, 1))


@pytest.mark.parametrize("name", ["head_backward", "gate_backward", "hip_lstm", "hip_lstm_backward", "pool_layers"])
def test_classifier_opt_ins(monkeypatch, name):
    env = "GGCN_" + name.upper()

    def option(**opt):
        m = GatedGCNEventDetector(nn.Identity(), types.SimpleNamespace(dropout=0.0, polarities_dim=5, **opt))
        v = getattr(m, name)
        assert type(v) is bool
        return v
    monkeypatch.delenv(env, raising=False)
    assert option() is False                                                 # neither
    assert option(**{"ggcn_" + name: True}) is True                          # the attribute
    assert option(**{"ggcn_" + name: 0}) is False
    monkeypatch.setenv(env, "1")
    assert option() is True                                                  # the environment
    assert option(**{"ggcn_" + name: False}) is True
    monkeypatch.setenv(env, "0")
    assert option() is False
    assert option(**{"ggcn_" + name: True}) is True
    assert hostops._opted_in(None, name) is False

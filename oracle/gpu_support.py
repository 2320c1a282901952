"""WHAT THE GPU TESTS SHARE THAT TOUCHES THE LIBRARY (test infrastructure, NOT product code).

The ``dev`` / ``pkg`` fixtures (a test file imports them: ``from oracle.gpu_support import dev, pkg  # noqa: F401``; module
scope, so every test module gets its own instance), the call counter and the call recorder on the loaded library's entries, the
keep factors of ``ggcn_dropout_mask``, the f16mx8 range flag, the layer builder and the classifier batches.  The gates themselves
are in ``oracle/gates.py``.
"""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pkg():
    import ed_gated_gcn_amd as p
    p.load_library()  # fails loudly if the HIP library was not built
    return p


def _library():
    from ed_gated_gcn_amd import _capi
    return _capi.load_library()


def count_calls(monkeypatch, names, prec_arg=None, lib=None):
    """Wrap the entries ``names`` of the loaded library (or of ``lib``) with a counter; returns the dict of counts.  ``prec_arg``
    maps an entry that serves several arithmetics to the index of its ``precision`` argument: its calls are also counted under
    "entry/precision" (every precision the package names starts at 0)."""
    prec_arg = prec_arg or {}
    lib = _library() if lib is None else lib
    calls = {n: 0 for n in names}
    if prec_arg:
        from ed_gated_gcn_amd import _capi
        prec_names = {v: k for k, v in _capi.PREC.items()}
        calls.update({"%s/%s" % (n, p): 0 for n in prec_arg for p in _capi.PREC})
    for n in names:
        fn = getattr(lib, n)

        def wrap(*a, _fn=fn, _n=n):
            calls[_n] += 1
            if _n in prec_arg:
                key = "%s/%s" % (_n, prec_names.get(int(a[prec_arg[_n]]), "?"))
                calls[key] = calls.get(key, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, n, wrap)
    return calls


def call_log(monkeypatch, names, lib=None):
    """``[(entry, [arguments])]`` of every call of an entry of ``names`` from here on, pointers as integers (NULL: None)."""
    lib = _library() if lib is None else lib
    calls = []
    for n in names:
        fn = getattr(lib, n)

        def wrap(*a, _fn=fn, _n=n):
            calls.append((_n, [v.value if isinstance(v, ctypes.c_void_p) else v for v in a]))
            return _fn(*a)
        monkeypatch.setattr(lib, n, wrap)
    return calls


def drop_mask(pkg, dev, rows, F, p, seed, stream):
    """float32 [rows,F] keep factors of one stream as ``ggcn_dropout_mask`` writes them."""
    from ed_gated_gcn_amd import _capi
    m = torch.empty(rows, F, dtype=torch.float32, device=dev)
    _capi.check(pkg.load_library().ggcn_dropout_mask(rows, F, float(p), int(seed), stream, _capi.ptr(m), _capi.stream_of(dev)),
                "ggcn_dropout_mask")
    return m


def range_bits(pkg, dev):
    """The raw f16mx8 range bits of every translation unit, read into a zeroed word and cleared."""
    from ed_gated_gcn_amd import _capi
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.check(pkg.load_library().ggcn_range_flag(_capi.ptr(flag), 1, _capi.stream_of(dev)), "ggcn_range_flag")
    return int(flag.item())


def clean_range_flag(pkg, dev):
    """The body of an autouse ``clean_flag`` fixture (``yield from``): the test starts and ends with the range flag clear and with
    ``range_guard`` having forgotten what it saw, so neither a later forward nor the interpreter's exit reports the test's probes."""
    from ed_gated_gcn_amd import range_guard
    range_bits(pkg, dev)
    range_guard.reset(dev)
    yield
    range_bits(pkg, dev)
    range_guard.reset(dev)


def make_layer(pkg, dev, w, b=None, opt=None, expect_defaults=None, **options):
    """A ``GraphConvolution`` on ``dev`` holding ``w`` [K,F] and ``b`` [F] (tensors or arrays; ``b=None``: no bias), built from
    ``opt``.  ``expect_defaults`` {attribute: value} is asserted on the fresh layer (the off-by-default statements), then every
    option is set as an attribute that must already exist (a typo cannot silently set nothing); an option given as None is left
    at its default."""
    w, b = torch.as_tensor(w), (None if b is None else torch.as_tensor(b))
    m = pkg.GraphConvolution(w.shape[0], w.shape[1], opt=opt, bias=b is not None).to(dev)
    for k, v in (expect_defaults or {}).items():
        got = getattr(m, k)
        assert got == v and type(got) is type(v), "%s is %r by default, not %r" % (k, got, v)
    for k, v in options.items():
        assert hasattr(m, k), k
        if v is not None:
            setattr(m, k, v)
    with torch.no_grad():
        m.weight.copy_(w)
        if b is not None:
            m.bias.copy_(b)
    return m


def ace_batch(rng, B, ORI_ML, BERT_ML, vocab=None, weights=None):
    """A classifier batch in the shape of data_utils.py:749-766 on CPU tensors: dependency trees of 5..ORI_ML words (the first
    graph full), word <- word-piece transform, token ids all 0 or drawn below ``vocab``; ``weights=(lo, hi)`` makes the graph
    real-valued with edge weights in [lo, hi)."""
    from ed_gated_gcn_amd import synth
    sent_len = rng.integers(5, ORI_ML + 1, size=B)
    sent_len[0] = ORI_ML
    bert_len = np.minimum(sent_len + rng.integers(2, 10, size=B), BERT_ML)
    adj = synth.dependency_batch(B, ORI_ML, 3.5, seed=12, lengths=sent_len).astype(np.float32)
    if weights is not None:
        adj = adj * rng.uniform(weights[0], weights[1], size=adj.shape).astype(np.float32)
    transform = np.zeros((B, ORI_ML, BERT_ML), dtype=np.float32)
    for b in range(B):
        for tkn in range(int(sent_len[b])):
            transform[b, tkn, 1 + min(tkn, BERT_ML - 2)] = 1.0
    ids = np.zeros((B, BERT_ML), dtype=np.int64) if vocab is None else rng.integers(0, vocab, size=(B, BERT_ML))
    return {
        "sentence_length": torch.from_numpy(sent_len), "cls_text_sep_length": torch.from_numpy(bert_len),
        "cls_text_sep_indices": torch.from_numpy(ids),
        "cls_text_sep_segments_ids": torch.zeros(B, BERT_ML, dtype=torch.long),
        "transform": torch.from_numpy(transform),
        "anchor_index": torch.from_numpy(np.array([int(rng.integers(0, n)) for n in sent_len])),
        "dist_to_target": torch.from_numpy(rng.integers(0, 6, size=(B, ORI_ML))),
        "dependency_graph": torch.from_numpy(adj),
    }


def classifier_batch(dev, ORI_ML=31, BERT_ML=65):
    """``(inputs on dev, number of classes)``: 8 sentences with BERT-vocabulary token ids for the classifiers under autocast."""
    inputs = ace_batch(np.random.default_rng(3), 8, ORI_ML, BERT_ML, vocab=30522)
    return {k: v.to(dev) for k, v in inputs.items()}, 34

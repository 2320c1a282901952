"""Host side of the inference BiLSTM (``ggcn_bilstm_recurrence``, ``recurrent.bilstm``): the float64 statement against float64
``nn.LSTM`` (gate order, reverse direction), the entry on all three sides of the ABI, its refusals with the exact
``ggcn_last_error`` text (every check comes before a launch: the pointers handed in are never dereferenced, so no GPU is needed),
the raises of ``bilstm``, the truth table of ``takes_hip_lstm`` and the classifier's opt-in ``hip_lstm``."""
import ctypes
import re
import types

import pytest
import torch

import ed_gated_gcn_amd as pkg
from ed_gated_gcn_amd import _capi, recurrent
from oracle.host_support import ROOT, header as _header, msg as _msg

import bilstm_ref as br

EINVAL, EUNSUPPORTED = 1, 3
ENTRY = "ggcn_bilstm_recurrence"
P = ctypes.c_void_p(1 << 20)   # non-null, 16-byte aligned, never dereferenced


# ---------------------------------------------------------------- the statement
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", [(1, 1, 4), (3, 5, 64), (2, 33, 64)], ids=lambda s: "x".join(map(str, s)))
def test_statement_equals_float64_lstm(shape, bias):
    B, T, I = shape
    lstm = br.make_lstm(I, bias=bias, seed=sum(shape)).double()
    x = br.make_x(B, T, I, seed=T).double()
    with torch.no_grad():
        ref = lstm(x)[0]
    got = br.bilstm_ref(x, lstm)
    assert got.shape == ref.shape == (B, T, 2 * br.HD) and got.dtype == torch.float64
    assert float((got - ref).abs().max()) <= 1e-12
    assert float((br.lstm64(x, lstm) - ref).abs().max()) == 0.0          # the yardstick helper is that module


def test_the_statement_is_sensitive_to_gate_order_and_direction():
    lstm = br.make_lstm(16, seed=5).double()
    x = br.make_x(2, 6, 16).double()
    with torch.no_grad():
        ref = lstm(x)[0]
    wih, whh_f, whh_r, bias_f, bias_r = br.operands64(lstm)
    G = x @ wih.t()
    assert float((br.recurrence64(G, whh_f, whh_r, bias_f, bias_r) - ref).abs().max()) <= 1e-12
    assert float((br.recurrence64(G, whh_r, whh_f, bias_f, bias_r) - ref).abs().max()) > 1e-3     # directions swapped
    perm = torch.cat([torch.arange(128), torch.arange(256, 384), torch.arange(128, 256), torch.arange(384, 512)])   # i, g, f, o
    Gp = torch.cat([G[..., :512][..., perm], G[..., 512:]], dim=-1)
    assert float((br.recurrence64(Gp, whh_f[perm], whh_r, bias_f[perm], bias_r)[..., :128] - ref[..., :128]).abs().max()) > 1e-3


# ---------------------------------------------------------------- the ABI
def test_declared_bound_exported_and_without_a_float_argument():
    lib = ctypes.CDLL(pkg.lib_path())
    header = _header()
    assert "int %s(" % ENTRY in header and ENTRY in _capi.PROTOTYPES and hasattr(lib, ENTRY)
    res, args = _capi.PROTOTYPES[ENTRY]
    vp, i64, i32 = _capi.c_vp, _capi.c_i64, _capi.c_i32
    assert res is i32 and args == [vp, i64, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]
    decl = header[header.index("int %s(" % ENTRY):]
    decl = decl[:decl.index(";")]
    assert "float " not in decl.replace("float *", ""), "the entry takes a float by value"
    assert decl.count(",") + 1 == len(args)
    assert _capi.ABI_VERSION == 14 and pkg.load_library().ggcn_abi_version() == 14


def test_tile_constant_follows_the_header():
    with open(ROOT + "/include/ggcn.h") as f:
        tile = int(re.search(r"#define\s+GGCN_BILSTM_TILE\s+(\d+)", f.read()).group(1))
    assert recurrent.TILE == _capi.BILSTM_TILE == tile and recurrent.HIDDEN == 128
    assert pkg.bilstm is recurrent.bilstm and pkg.takes_hip_lstm is recurrent.takes_hip_lstm
    assert "bilstm" in pkg.__all__ and "takes_hip_lstm" in pkg.__all__


# ---------------------------------------------------------------- the refusals
def _call(lib, **kw):
    a = dict(G=P, ldg=1024, wf=P, wr=P, bf=P, br=P, Y=P, ldy=256, B=3, T=5, hd=128)
    a.update(kw)
    return lib.ggcn_bilstm_recurrence(*[a[k] for k in ("G", "ldg", "wf", "wr", "bf", "br", "Y", "ldy", "B", "T", "hd")], None)


OFF = ctypes.c_void_p((1 << 20) + 4)
LEADING = "leading dimension too small"
UNBUILT = "(the kernel is built for hd = 128, bert_amir5.py:551)"


@pytest.mark.parametrize("kw, code, text", [
    (dict(G=None), EINVAL, "null pointer"), (dict(wf=None), EINVAL, "null pointer"), (dict(wr=None), EINVAL, "null pointer"),
    (dict(Y=None), EINVAL, "null pointer"),
    (dict(B=0), EINVAL, "B=0 T=5 must be positive"), (dict(B=-1), EINVAL, "B=-1 T=5 must be positive"),
    (dict(T=0), EINVAL, "B=3 T=0 must be positive"), (dict(T=-7), EINVAL, "B=3 T=-7 must be positive"),
    (dict(hd=64, ldg=512, ldy=128), EUNSUPPORTED, "hd=64 " + UNBUILT), (dict(hd=256, ldg=2048, ldy=512), EUNSUPPORTED, "hd=256 " + UNBUILT),
    (dict(hd=0), EUNSUPPORTED, "hd=0 " + UNBUILT),
    (dict(ldg=1023), EINVAL, LEADING), (dict(ldy=255), EINVAL, LEADING),
    (dict(B=1 << 16, T=1 << 15), EUNSUPPORTED, "B*T=2147483648 rows (at most 2^31 - 1)"),
    (dict(wf=OFF), EINVAL, "Whh_f and Whh_r must be 16-byte aligned"), (dict(wr=OFF), EINVAL, "Whh_f and Whh_r must be 16-byte aligned"),
    (dict(G=None, B=0, hd=5), EINVAL, "null pointer"),                      # the order of the checks: pointers first
    (dict(B=0, hd=5), EINVAL, "B=0 T=5 must be positive"),
])
def test_the_entry_refuses_before_it_launches(kw, code, text):
    lib = pkg.load_library()
    assert _msg(lib, _call(lib, **kw), code, ENTRY) == "%s: %s" % (ENTRY, text)


# ---------------------------------------------------------------- bilstm's raises and the predicate
def _lstm(**kw):
    a = dict(input_size=8, hidden_size=128, bidirectional=True, batch_first=True, num_layers=1)
    a.update(kw)
    return torch.nn.LSTM(**a).requires_grad_(False)


SHAPE = "lstm must be one bidirectional batch_first layer without projection, got num_layers=%d bidirectional=%s batch_first=%s proj_size=%d"
RAISES = [
    ("not a tensor", lambda: ([[1.0]], _lstm()), TypeError, "x must be a 3-d tensor"),
    ("2-d", lambda: (torch.zeros(3, 8), _lstm()), TypeError, "x must be a 3-d tensor"),
    ("float64 x", lambda: (torch.zeros(2, 3, 8, dtype=torch.float64), _lstm()), RuntimeError, "x must be float32, got torch.float64"),
    ("bf16 x", lambda: (torch.zeros(2, 3, 8, dtype=torch.bfloat16), _lstm()), RuntimeError, "x must be float32, got torch.bfloat16"),
    ("not an LSTM", lambda: (torch.zeros(2, 3, 8), torch.nn.GRU(8, 128)), RuntimeError, "lstm must be a torch.nn.LSTM, got GRU"),
    ("two layers", lambda: (torch.zeros(2, 3, 8), _lstm(num_layers=2)), RuntimeError, SHAPE % (2, True, True, 0)),
    ("one direction", lambda: (torch.zeros(2, 3, 8), _lstm(bidirectional=False)), RuntimeError, SHAPE % (1, False, True, 0)),
    ("time first", lambda: (torch.zeros(2, 3, 8), _lstm(batch_first=False)), RuntimeError, SHAPE % (1, True, False, 0)),
    ("projected", lambda: (torch.zeros(2, 3, 8), _lstm(proj_size=32)), RuntimeError, SHAPE % (1, True, True, 32)),
    ("hidden 64", lambda: (torch.zeros(2, 3, 8), _lstm(hidden_size=64)), RuntimeError, "lstm.hidden_size must be 128, got 64"),
    ("float64 module", lambda: (torch.zeros(2, 3, 8), _lstm().double()), RuntimeError, "lstm.weight_ih_l0 must be float32, got torch.float64"),
    ("width", lambda: (torch.zeros(2, 3, 9), _lstm()), RuntimeError, "x (2, 3, 9) does not match lstm.input_size 8"),
    ("x wants grad", lambda: (torch.zeros(2, 3, 8, requires_grad=True), _lstm()), RuntimeError, "bilstm is forward only"),
    ("a parameter wants grad", lambda: (torch.zeros(2, 3, 8), _lstm().requires_grad_(True)), RuntimeError, "bilstm is forward only"),
    ("cpu", lambda: (torch.zeros(2, 3, 8), _lstm()), RuntimeError, "x is on cpu: the HIP path has no CPU fallback"),
    ("cpu, empty", lambda: (torch.zeros(0, 3, 8), _lstm()), RuntimeError, "x is on cpu: the HIP path has no CPU fallback"),
]


@pytest.mark.parametrize("what, make, exc, text", RAISES, ids=[r[0] for r in RAISES])
def test_bilstm_raises(what, make, exc, text):
    x, lstm = make()
    with pytest.raises(exc, match=re.escape(text)):
        pkg.bilstm(x, lstm)
    assert pkg.takes_hip_lstm(x, lstm) is False


def test_no_grad_turns_the_gradient_raise_into_the_cpu_raise():
    x, lstm = torch.zeros(2, 3, 8, requires_grad=True), _lstm().requires_grad_(True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.bilstm(x, lstm)


def _fake_gpu(t):
    """A stand-in for a GPU tensor: what ``takes_hip_lstm`` asks of ``x`` and of a parameter, answered by ``t`` with ``is_cuda``."""
    class Fake(torch.Tensor):
        is_cuda = True
        device = torch.device("cuda:0")
    return t.as_subclass(Fake)


def test_takes_hip_lstm_truth_table():
    def on_gpu(lstm):
        for n in recurrent.PARAMS:
            if getattr(lstm, n, None) is not None:
                lstm._parameters[n] = _fake_gpu(lstm._parameters[n])
        return lstm
    x = _fake_gpu(torch.zeros(2, 3, 8))
    assert pkg.takes_hip_lstm(x, on_gpu(_lstm())) is True
    assert pkg.takes_hip_lstm(x, on_gpu(_lstm(bias=False))) is True
    assert pkg.takes_hip_lstm(x, _lstm()) is False                                   # the module is on another device
    assert pkg.takes_hip_lstm(torch.zeros(2, 3, 8), on_gpu(_lstm())) is False        # x on the CPU
    assert pkg.takes_hip_lstm(_fake_gpu(torch.zeros(2, 3, 8, dtype=torch.bfloat16)), on_gpu(_lstm())) is False
    assert pkg.takes_hip_lstm(_fake_gpu(torch.zeros(2, 3, 8, dtype=torch.float16)), on_gpu(_lstm())) is False
    assert pkg.takes_hip_lstm(_fake_gpu(torch.zeros(3, 8)), on_gpu(_lstm())) is False
    assert pkg.takes_hip_lstm(_fake_gpu(torch.zeros(2, 3, 9)), on_gpu(_lstm())) is False
    for kw in (dict(num_layers=2), dict(bidirectional=False), dict(batch_first=False), dict(proj_size=32), dict(hidden_size=64)):
        assert pkg.takes_hip_lstm(x, on_gpu(_lstm(**kw))) is False, kw
    assert pkg.takes_hip_lstm(x, torch.nn.GRU(8, 128)) is False and pkg.takes_hip_lstm(None, _lstm()) is False
    # a gradient wanted: grad enabled and x or a parameter requires it
    wants = on_gpu(_lstm())
    wants._parameters["weight_hh_l0_reverse"].requires_grad_(True)
    assert pkg.takes_hip_lstm(x, wants) is False
    assert pkg.takes_hip_lstm(_fake_gpu(torch.zeros(2, 3, 8)).requires_grad_(True), on_gpu(_lstm())) is False
    with torch.no_grad():
        assert pkg.takes_hip_lstm(x, wants) is True
        assert pkg.takes_hip_lstm(_fake_gpu(torch.zeros(2, 3, 8)).requires_grad_(True), on_gpu(_lstm())) is True
    assert not hasattr(wants, "_ggcn_lstm"), "the predicate has no side effect"


# ---------------------------------------------------------------- the classifier's option
def _classifier(cls, **opt):
    return cls(torch.nn.Identity(), types.SimpleNamespace(dropout=0.0, polarities_dim=5, **opt))


@pytest.mark.parametrize("cls_name", ["GatedGCNEventDetector", "GatedGCNEventDetector54", "GCNEventDetectorNoGate"])
def test_option_is_off_by_default_and_read_from_opt_and_environment(monkeypatch, cls_name):
    cls = getattr(pkg, cls_name)
    for k in ("GGCN_HIP_LSTM", "GGCN_GATE_BACKWARD", "GGCN_HEAD_BACKWARD"):
        monkeypatch.delenv(k, raising=False)
    assert _classifier(cls).hip_lstm is False
    assert _classifier(cls, ggcn_hip_lstm=True).hip_lstm is True
    assert _classifier(cls, ggcn_hip_lstm=False).hip_lstm is False
    on = _classifier(cls, ggcn_hip_lstm=True)
    assert on.gate_backward is False and on.head_backward is False, "the options are independent"
    assert _classifier(cls, ggcn_gate_backward=True, ggcn_head_backward=True).hip_lstm is False
    monkeypatch.setenv("GGCN_HIP_LSTM", "1")
    assert _classifier(cls).hip_lstm is True and _classifier(cls).gate_backward is False
    monkeypatch.setenv("GGCN_HIP_LSTM", "0")
    assert _classifier(cls).hip_lstm is False
    assert sorted(on.state_dict()) == sorted(_classifier(cls).state_dict()), "the option adds nothing to the state_dict"
    assert takes_none_on_cpu(on)


def takes_none_on_cpu(model):
    """On CPU tensors the predicate is False, so the classifier's line :610 stays ``nn.LSTM`` whatever the option says."""
    return pkg.takes_hip_lstm(torch.zeros(2, 3, model.lstm.input_size), model.lstm) is False

"""Per-sample sequence lengths on the CPU: the any-shape forward body (ttrnn_core.h rnn_fwd_body) with lengths, and the
UNCHANGED reverse-time body (rnn_bwd_body) on the frozen records it leaves — through the serial host executor
(tests/hostemu/hostemu_varlen.cpp).  This is the proof, where no GPU exists, of the design the variable-length entry points
rest on (include/ttrnn.h, TTRNN_HAS_VARLEN): a forward that writes, for t >= len_b,
    LSTM (i, g, f, o) = (0, 0, 1, 0) with c_t = c_{len-1}        GRU (r, z, n, hn) = (0, 1, 0, 0)
makes every reverse kernel produce exact-zero gate gradients there and pass dc / dh through, so that no reverse kernel has to
know about lengths; the gradient of hT enters through the seeded d_out.

Expected results: the oracle run per sample on x[b:b+1, :len_b], losses summed (autograd for the gradients).
Tolerances (the project's own, tests/test_w2.py): forward / states 1e-5 absolute; gradients 1e-4 * max(1e-3, max|ref|).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from golden_io import Case
from oracle import ttrnn_oracle as O
from test_hostemu import _p, _tt_from_sd
from ttrnn_hip._lib import RnnDesc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "hostemu", "libttrnn_hostemu_varlen.so")

B, T = 5, 7
LENGTHS = [7, 1, 4, 7, 2]


@pytest.fixture(scope="module")
def emu():
    srcs = [os.path.join(HERE, "hostemu", "hostemu_varlen.cpp"), os.path.join(HERE, "hostemu", "hostemu.cpp"),
            os.path.join(ROOT, "tensorized-rnn_amd", "csrc", "ttrnn_core.h")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "tensorized-rnn_amd", "csrc"), "-o", SO, srcs[0]])
    lib = ctypes.CDLL(SO)
    lib.hostemu_packed_elems.restype = ctypes.c_int64
    return lib


def _data(lstm):
    """Layer 0 of the tiny TT fixtures (in = 28, H = 64, d = 2, r = 3) on seeded inputs, initial states and loss weights."""
    case = Case("g8_var_ttlstm_tiny" if lstm else "g8_var_ttgru_tiny")
    H = case.meta["hidden_size"]
    g = torch.Generator().manual_seed(4242)
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(case=case, H=H, I=case.meta["input_size"], x=r(B, T, case.meta["input_size"]), h0=0.5 * r(B, H),
             c0=0.5 * r(B, H) if lstm else None, w_out=r(B, T, H), w_h=r(B, H), w_c=r(B, H) if lstm else None)
    return d


_REF = {}


def _reference(lstm):
    """Oracle per sample on the truncated input; gate gradients through a probe: the input weights as a dense matrix with an
    identity block appended, fed [x_t, delta_t] with delta = 0 — d loss / d delta IS the gradient w.r.t. the pre-activations
    of the input TTLinear (d_gates_in).  Computed once per cell kind, never modified."""
    if lstm in _REF:
        return _REF[lstm]
    d = _data(lstm)
    H, I, G = d["H"], d["I"], 4 if lstm else 3
    layers, leaves = O.layers_from_state_dict(d["case"].state_dict(), 1, requires_grad=False)
    w_in, w_hid = layers[0]
    assert w_in[0] == "tt"
    dense_in = O.ttlinear(w_in[1], None, torch.eye(I))                   # [I][G H]: row j = W_in e_j
    w_probe = ("dense", torch.cat([dense_in.t(), torch.eye(G * H)], dim=1), w_in[2])
    out = torch.zeros(B, T, H)
    hT, cT = torch.zeros(B, H), torch.zeros(B, H)
    dgin = torch.zeros(B, T, G * H)
    dx = torch.zeros(B, T, I)
    dh0, dc0 = torch.zeros(B, H), torch.zeros(B, H)
    for b, n in enumerate(LENGTHS):
        xb = d["x"][b:b + 1, :n].clone().requires_grad_(True)
        delta = torch.zeros(1, n, G * H, requires_grad=True)
        h0 = d["h0"][b:b + 1].clone().requires_grad_(True)
        xa = torch.cat([xb, delta], dim=2)
        if lstm:
            c0 = d["c0"][b:b + 1].clone().requires_grad_(True)
            o, (h, c) = O.lstm_forward([(w_probe, w_hid)], xa, (h0, c0))
            loss = (o * d["w_out"][b:b + 1, :n]).sum() + (h * d["w_h"][b:b + 1]).sum() + (c * d["w_c"][b:b + 1]).sum()
        else:
            o, h = O.gru_forward([(w_probe, w_hid)], xa, h0)
            loss = (o * d["w_out"][b:b + 1, :n]).sum() + (h * d["w_h"][b:b + 1]).sum()
        loss.backward()
        out[b, :n] = o.detach()[0]
        hT[b] = h.detach()[0]
        dgin[b, :n] = delta.grad[0]
        dx[b, :n] = xb.grad[0]
        dh0[b] = h0.grad[0]
        if lstm:
            cT[b] = c.detach()[0]
            dc0[b] = c0.grad[0]
    ref = dict(out=out.numpy(), hT=hT.numpy(), cT=cT.numpy(), dgin=dgin.numpy(), dx=dx.numpy(), dh0=dh0.numpy(),
               dc0=dc0.numpy())
    for v in ref.values():
        v.setflags(write=False)
    _REF[lstm] = ref
    return ref


def _close(got, ref, what):
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    assert err <= 1e-5, "%s: max abs error %g" % (what, err)


def _gclose(got, ref, what):
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    bound = 1e-4 * max(1e-3, float(np.abs(ref).max()))
    assert err <= bound, "%s: max abs error %g > %g" % (what, err, bound)


def _run(emu, lstm, nb, with_reserve=True, poison_x=None):
    d = _data(lstm)
    H, G = d["H"], 4 if lstm else 3
    case = d["case"]
    w_in, _ = _tt_from_sd(emu, case, "cell0.input_weights.")
    w_hid, _ = _tt_from_sd(emu, case, "cell0.hidden_weights.")
    desc = RnnDesc()
    desc.cell, desc.dtype, desc.batch, desc.seq_len = (0 if lstm else 1), 0, B, T
    desc.input_size, desc.hidden_size = w_in.in_f, H
    desc.has_bias_in, desc.has_bias_hid = int(w_in.bias is not None), int(w_hid.bias is not None)
    desc.in_w, desc.hid_w = w_in.desc, w_hid.desc
    x = np.ascontiguousarray(d["x"].numpy())
    if poison_x is not None:
        for b, n in enumerate(LENGTHS):
            x[b, n:] = poison_x
    h0 = np.ascontiguousarray(d["h0"].numpy())
    c0 = np.ascontiguousarray(d["c0"].numpy()) if lstm else None
    lens = np.array(LENGTHS, dtype=np.int32)
    # every output buffer starts as NaN: whatever the body leaves unwritten shows
    out = np.full((B, T, H), np.nan, dtype=np.float32)
    hT = np.full((B, H), np.nan, dtype=np.float32)
    cT = np.full((B, H), np.nan, dtype=np.float32)
    reserve = np.full(B * T * (5 if lstm else 4) * H, np.nan, dtype=np.float32) if with_reserve else None
    rc = emu.hostemu_rnn_forward_varlen(ctypes.byref(desc), _p(lens), _p(x), _p(h0), _p(c0), _p(w_in.packed), _p(w_in.bias),
                                        _p(w_hid.packed), _p(w_hid.bias), _p(out), _p(hT), _p(cT), _p(reserve), nb, 40)
    assert rc == 0
    return dict(d=d, desc=desc, w_in=w_in, w_hid=w_hid, x=x, h0=h0, c0=c0, out=out, hT=hT, cT=cT, reserve=reserve, H=H, G=G)


@pytest.mark.parametrize("nb", [2, 5])
@pytest.mark.parametrize("lstm", [True, False], ids=["lstm", "gru"])
def test_varlen_forward_body(emu, lstm, nb):
    r = _run(emu, lstm, nb)
    ref = _reference(lstm)
    H = r["H"]
    _close(r["out"], ref["out"], "out")
    _close(r["hT"], ref["hT"], "hT")
    if lstm:
        _close(r["cT"], ref["cT"], "cT")
    gates = r["reserve"][:B * T * H * 4].reshape(B, T, H, 4)
    cells = r["reserve"][B * T * H * 4:].reshape(B, T, H) if lstm else None
    assert not np.isnan(r["reserve"]).any()
    frozen = np.array([0, 0, 1, 0] if lstm else [0, 1, 0, 0], dtype=np.float32)
    for b, n in enumerate(LENGTHS):
        assert np.array_equal(r["out"][b, n:], np.zeros((T - n, H), dtype=np.float32)), "padded rows of sample %d" % b
        assert np.array_equal(gates[b, n:], np.broadcast_to(frozen, (T - n, H, 4))), "frozen records of sample %d" % b
        if lstm:       # c_t = c_{len-1}: the sample's final cell state
            assert np.array_equal(cells[b, n:], np.broadcast_to(r["cT"][b], (T - n, H))), "frozen cells of sample %d" % b


@pytest.mark.parametrize("lstm", [True, False], ids=["lstm", "gru"])
def test_varlen_forward_ignores_padded_inputs_and_tiling(emu, lstm):
    """Input rows at t >= len never influence a result (bit for bit), nor does the tiling of the batch, nor the reserve."""
    a = _run(emu, lstm, 2)
    for other in (_run(emu, lstm, 2, poison_x=1e30), _run(emu, lstm, 5), _run(emu, lstm, 3, with_reserve=False)):
        for k in ("out", "hT") + (("cT",) if lstm else ()):
            assert np.array_equal(a[k], other[k]), k


@pytest.mark.parametrize("nb", [2, 5])
@pytest.mark.parametrize("lstm", [True, False], ids=["lstm", "gru"])
def test_unchanged_reverse_body_on_frozen_records(emu, lstm, nb):
    r = _run(emu, lstm, nb)
    ref = _reference(lstm)
    d, H, G = r["d"], r["H"], r["G"]
    # d_out_seeded[b][t] = (t < len ? d_out[b][t] : 0) + (t == len - 1 ? d_hT[b] : 0); d_hT = NULL afterwards; d_cT as it is
    seeded = np.zeros((B, T, H), dtype=np.float32)
    for b, n in enumerate(LENGTHS):
        seeded[b, :n] = d["w_out"].numpy()[b, :n]
        seeded[b, n - 1] += d["w_h"].numpy()[b]
    d_cT = np.ascontiguousarray(d["w_c"].numpy()) if lstm else None
    dg_in = np.full((B, T, G * H), np.nan, dtype=np.float32)
    dg_hid = dg_in if lstm else np.full((B, T, G * H), np.nan, dtype=np.float32)
    d_h0 = np.full((B, H), np.nan, dtype=np.float32)
    d_c0 = np.full((B, H), np.nan, dtype=np.float32)
    rc = emu.hostemu_rnn_backward(ctypes.byref(r["desc"]), _p(r["out"]), _p(r["h0"]), _p(r["c0"]), _p(r["w_hid"].packed),
                                  _p(r["reserve"]), _p(seeded), _p(None), _p(d_cT), _p(dg_in), _p(dg_hid), _p(d_h0),
                                  _p(d_c0), nb, 33)
    assert rc == 0
    for b, n in enumerate(LENGTHS):
        assert np.array_equal(dg_in[b, n:], np.zeros((T - n, G * H), dtype=np.float32)), "gate gradients past len, sample %d" % b
        assert np.array_equal(dg_hid[b, n:], np.zeros((T - n, G * H), dtype=np.float32)), "hidden gate gradients past len, %d" % b
    _gclose(dg_in, ref["dgin"], "d_gates_in")
    _gclose(d_h0, ref["dh0"], "d_h0")
    if lstm:
        _gclose(d_c0, ref["dc0"], "d_c0")
    # the input gradient is the unchanged TTLinear backward over all B*T rows: exact zeros on the padded ones
    dx, _, _ = r["w_in"].backward(r["x"].reshape(B * T, -1), dg_in.reshape(B * T, -1))
    dx = dx.reshape(B, T, -1)
    _gclose(dx, ref["dx"], "d_x")
    for b, n in enumerate(LENGTHS):
        assert np.array_equal(dx[b, n:], np.zeros_like(dx[b, n:])), "x gradient past len, sample %d" % b


@pytest.mark.parametrize("name", ["g11_varlen_spk_lstm", "g11_varlen_spk_gru"])
def test_per_sample_oracle_harness_vs_reference(name):
    """tests/varlen_ref.py (the expected results of every variable-length test) against the reference's own numbers: the
    reference run per sample on the truncated inputs of the encoder layer (tests/golden/gen_golden_varlen.py)."""
    from varlen_ref import grad_bound, oracle_varlen
    case = Case(name)
    lstm = case.meta["kind"] == "ttlstm"
    t = case.tensor
    assert case.meta["lengths"] == [12, 1, 7, 12, 3] and list(case.arr["lengths"]) == case.meta["lengths"]
    r = oracle_varlen(case.meta["kind"], case.state_dict(), 1, t("x"), case.meta["lengths"], t("h0"), t("c0"), t("w_out"),
                      t("w_h"), t("w_c"))
    for k in ("out", "hT") + (("cT",) if lstm else ()):
        _close(r[k].numpy(), case.arr[k], k)
    for b, n in enumerate(case.meta["lengths"]):
        assert not case.arr["out"][b, n:].any() and not case.arr["grad_x"][b, n:].any()
    for k in ("grad_x", "grad_h0") + (("grad_c0",) if lstm else ()):
        assert float((r[k] - t(k)).abs().max()) <= grad_bound(t(k)), k
    grads = case.grads()
    assert grads and set(grads) <= set(r["grads"])
    for k, g in grads.items():
        assert float((r["grads"][k] - g).abs().max()) <= grad_bound(g), k

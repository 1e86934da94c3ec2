"""Route TTRNN_ROUTE_DENSE_STEP on the GPU (csrc/ttrnn_fast_dense.hip): the dense (nn.Linear) LSTM / GRU layers as one MFMA GEMM
launch per time step, through the module API (tensorized_rnn.lstm.LSTM / gru.GRU) and the C ABI.

Bounds.  Fixtures: DESIGN.md section 2's rule (forward 1e-5 abs, gradients 1e-4 of the tensor's maximum).  Seeded cases, per
tensor, against a float64 evaluation of the oracle:  max(4 x the error of the any-shape route (force_generic = 1) on the same
input, 2^-19 x max|reference|) — measured against the route the layers ran on before, not against the code under test.
"""
import contextlib
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_io import Case
from test_gpu_parity import _check_forward, _check_gradients_golden, _loaded_module, _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_STEP = "dense_step"


def dev():
    return torch.device("cuda:0")


def _model(kind, inp, H, L, bias):
    from tensorized_rnn.gru import GRU
    from tensorized_rnn.lstm import LSTM
    return (LSTM if kind == "lstm" else GRU)(inp, H, L, dev(), bias=bias)


def _assert_route(model, B, T):
    from ttrnn_hip import functional as F
    for l in range(model.num_layers):
        spec = getattr(model, "cell%d" % l)._layer_spec()
        assert F.rnn_route(spec, B, T) == DENSE_STEP and F.rnn_backward_route(spec, B, T) == DENSE_STEP


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g11_dense_lstm", "g11_dense_gru"])
def test_fixtures(name):
    case = Case(name)
    m = _loaded_module(case)
    _assert_route(m, case.meta["B"], case.meta["T"])
    with torch.no_grad():
        _check_forward(case, _run(case, m), 1e-5)
    _check_gradients_golden(name)


# ---- seeded cases against the float64 oracle ----------------------------------------------------------------------------------------
def _reference(kind, sd, L, x, h0, c0, loss_w):
    from oracle import ttrnn_oracle as O
    layers, leaves = O.layers_from_state_dict(sd, L, requires_grad=True, dtype=torch.float64)
    t = {"x": x.double().requires_grad_(True)}
    if h0 is not None:
        t["h0"] = h0.double().requires_grad_(True)
    if c0 is not None:
        t["c0"] = c0.double().requires_grad_(True)
    if kind == "lstm":
        out, (h, c) = O.lstm_forward(layers, t["x"], None if h0 is None else (t["h0"], t["c0"]))
    else:
        out, h = O.gru_forward(layers, t["x"], t.get("h0"))
        c = None
    _loss(out, h, c, loss_w, torch.float64, "cpu").backward()
    res = {"out": out.detach(), "hT": h.detach()}
    if c is not None:
        res["cT"] = c.detach()
    for k, v in t.items():
        res["d_" + k] = v.grad
    for k, v in leaves.items():
        res["grad/" + k] = v.grad
    return res


def _loss(out, h, c, w, dtype, device):
    wo, wh, wc = (None if v is None else v.to(device=device, dtype=dtype) for v in w)
    loss = 0.0
    if wo is not None:
        loss = loss + (out * wo).sum()
    if wh is not None:
        loss = loss + (h * wh).sum()
    if wc is not None and c is not None:
        loss = loss + (c * wc).sum()
    return loss


def _product(model, kind, x, h0, c0, loss_w, need_out=True):
    model.zero_grad(set_to_none=True)
    t = {"x": x.to(dev()).requires_grad_(True)}
    if h0 is not None:
        t["h0"] = h0.to(dev()).requires_grad_(True)
    if c0 is not None:
        t["c0"] = c0.to(dev()).requires_grad_(True)
    if kind == "lstm":
        out, (h, c) = model(t["x"], None if h0 is None else (t["h0"], t["c0"]))
    else:
        out, h = model(t["x"], t.get("h0"))
        c = None
    _loss(out, h, c, loss_w, torch.float32, dev()).backward()
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "hT": h.detach().cpu()}
    if c is not None:
        res["cT"] = c.detach().cpu()
    for k, v in t.items():
        res["d_" + k] = v.grad.cpu()
    for k, p in model.named_parameters():
        res["grad/" + k] = p.grad.cpu()
    return res


def _errors(got, ref):
    return {k: float((got[k].double() - ref[k]).abs().max()) for k in ref}


def _check_case(kind, inp, H, B, T, L=1, bias=True, init=True, x_scale=1.0, w_scale=1.0, h0_scale=0.5, loss="all", seed=0):
    import ttrnn_hip
    torch.manual_seed(1000 + seed + inp + H + B + T)
    model = _model(kind, inp, H, L, bias)
    if w_scale != 1.0:
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "bias" not in n:
                    p.mul_(w_scale)
    _assert_route(model, B, T)
    x = torch.randn(B, T, inp) * x_scale
    h0 = torch.randn(B, H) * h0_scale if init else None
    c0 = torch.randn(B, H) * 0.5 if (init and kind == "lstm") else None
    wo, wh, wc = torch.randn(B, T, H), torch.randn(B, H), torch.randn(B, H)
    if loss == "hT":
        wo = wc = None
    elif loss == "cT":
        wo = wh = None
    elif loss == "decades":          # d_out spread over ten decades across the samples
        wo = wo * (10.0 ** torch.linspace(-5, 5, B)).view(B, 1, 1)
    loss_w = (wo, wh, wc)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = _reference(kind, sd, L, x, h0, c0, loss_w)
    new = _errors(_product(model, kind, x, h0, c0, loss_w), ref)
    with ttrnn_hip.option("force_generic", 1):
        old = _errors(_product(model, kind, x, h0, c0, loss_w), ref)
    bad = []
    for k in sorted(ref):
        scale = float(ref[k].abs().max())
        bound = max(4.0 * old[k], 2.0 ** -19 * scale)
        print("%-34s max|ref| %.3e  dense_step %.3e  any-shape %.3e  bound %.3e" % (k, scale, new[k], old[k], bound))
        if not new[k] <= bound:
            bad.append((k, new[k], bound))
    assert not bad, bad


SEEDED = [
    # kind, in, H, B, T, layers, bias, initial states
    ("lstm", 28, 128, 3, 9, 1, True, True),
    ("gru", 28, 128, 3, 9, 1, True, True),
    ("lstm", 1, 256, 33, 2, 1, True, False),
    ("gru", 1, 192, 70, 1, 1, False, True),
    ("lstm", 40, 192, 70, 9, 1, False, True),       # B T = 630 < 4 H: the hidden matrix's gradient off the dense-gradient tail
    ("gru", 40, 256, 1, 9, 1, True, False),
    ("lstm", 128, 128, 33, 2, 1, True, True),       # in = H
    ("gru", 192, 192, 3, 2, 1, True, True),
    ("gru", 1, 160, 1, 1, 1, True, True),           # one sample, one step; 3 H / 32 odd
    ("lstm", 40, 128, 70, 9, 2, True, True),        # two layers; B T = 630 >= 4 H: the dense-gradient tail
    ("gru", 28, 128, 33, 9, 2, True, False),        # two layers, B T = 297 < 4 H
]


@pytest.mark.parametrize("kind,inp,H,B,T,L,bias,init", SEEDED)
def test_seeded_against_float64(kind, inp, H, B, T, L, bias, init):
    _check_case(kind, inp, H, B, T, L, bias, init)


RANGES = [
    ("lstm", dict(x_scale=1e-4)), ("lstm", dict(x_scale=1e4)), ("gru", dict(x_scale=1e-4)), ("gru", dict(x_scale=1e4)),
    ("lstm", dict(w_scale=1e-3)), ("lstm", dict(w_scale=1e2)), ("gru", dict(w_scale=1e-3)), ("gru", dict(w_scale=1e2)),
    ("gru", dict(h0_scale=1e3)),
    ("lstm", dict(loss="decades")), ("gru", dict(loss="decades")),
    ("lstm", dict(loss="hT")), ("gru", dict(loss="hT")), ("lstm", dict(loss="cT")),
]


@pytest.mark.parametrize("kind,knobs", RANGES, ids=["%s-%s" % (k, "-".join("%s=%s" % kv for kv in sorted(d.items()))) for k, d in RANGES])
def test_operand_ranges(kind, knobs):
    _check_case(kind, 28, 128, 35, 5, seed=7, **knobs)


def test_inference_without_outputs():
    """out == NULL (need_outputs=False under no_grad): the final state equals the one of the call that stores the outputs."""
    for kind in ("lstm", "gru"):
        torch.manual_seed(3)
        model = _model(kind, 28, 128, 1, True)
        x = torch.randn(35, 5, 28, device=dev())
        h0 = torch.randn(35, 128, device=dev())
        init = (h0, h0 * 0.5) if kind == "lstm" else h0
        with torch.no_grad():
            full = model(x, init)
            none = model(x, init, need_outputs=False)
        assert none[0] is None
        a, b = (full[1], none[1]) if kind == "gru" else (torch.cat(full[1]), torch.cat(none[1]))
        assert torch.equal(a, b)


# ---- calls with lengths: the forward keeps the any-shape kernel, the REVERSE of such a call runs on k_dense_bwd --------------------
@pytest.mark.parametrize("dout", [True, False], ids=["out_term", "states_only"])
@pytest.mark.parametrize("kind,inp,H,L", [("lstm", 28, 128, 1), ("gru", 28, 160, 1), ("lstm", 40, 128, 2), ("gru", 1, 128, 2)])
def test_training_step_with_lengths(kind, inp, H, L, dout):
    """ttrnn_rnn_backward_ex cannot see lengths (include/ttrnn.h: no reverse kernel knows about them), so the reverse-time part
    of a training call with lengths takes this route on the frozen records the any-shape forward left: exact-zero gate
    gradients on the padded steps, dc / dh passed through.  The checks of tests/test_varlen.py::test_training_step: parity
    with every sample run alone on its own length (the oracle), exact zeros on the padded rows, at that file's tolerances
    (forward 1e-5 abs, gradients 1e-4 * max(1e-3, max|ref|)); B = 35 crosses the 32-row batch tile."""
    from ttrnn_hip import functional as F
    from varlen_ref import grad_bound, oracle_varlen
    B, T = 35, 9
    lens = [9, 1, 5, 8, 2] * 7
    torch.manual_seed(73 + H + inp)
    m = _model(kind, inp, H, L, True)
    lstm = kind == "lstm"
    for l in range(L):
        spec = getattr(m, "cell%d" % l)._layer_spec()
        assert F.rnn_route(spec, B, T, varlen=True) == "valu" and F.rnn_backward_route(spec, B, T) == DENSE_STEP
    g = torch.Generator().manual_seed(79)
    x = torch.randn(B, T, inp, generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.5
    c0 = torch.randn(B, H, generator=g) * 0.5 if lstm else None
    w = torch.randn(B, T, H, generator=g) if dout else None
    wh, wc = torch.randn(B, H, generator=g), (torch.randn(B, H, generator=g) if lstm else None)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = oracle_varlen(kind, sd, L, x, lens, h0, c0, w, wh, wc)
    xg, hg = x.to(dev()).requires_grad_(True), h0.to(dev()).requires_grad_(True)
    cg = c0.to(dev()).requires_grad_(True) if lstm else None
    if lstm:
        out, (hT, cT) = m(xg, (hg, cg), lengths=lens)
    else:
        out, hT = m(xg, hg, lengths=lens)
        cT = None
    ls = (hT * wh.to(dev())).sum()
    if lstm:
        ls = ls + (cT * wc.to(dev())).sum()
    if dout:
        ls = ls + (out * w.to(dev())).sum()
    ls.backward()
    torch.cuda.synchronize()
    assert float((out.detach().cpu() - ref["out"]).abs().max()) <= 1e-5 and float((hT.detach().cpu() - ref["hT"]).abs().max()) <= 1e-5
    got = {n: p.grad.cpu() for n, p in m.named_parameters()}
    expect = {n: ref["grads"][n] for n in got}
    got.update(x=xg.grad.cpu(), h0=hg.grad.cpu())
    expect.update(x=ref["grad_x"], h0=ref["grad_h0"])
    if lstm:
        got["c0"], expect["c0"] = cg.grad.cpu(), ref["grad_c0"]
    for n, r in expect.items():
        assert torch.isfinite(got[n]).all(), n
        err = float((got[n].double() - r.double()).abs().max())
        assert err <= grad_bound(r), (n, err, grad_bound(r))
    for b, n in enumerate(lens):
        assert not got["x"][b, n:].any(), "x gradient on the padded rows of sample %d" % b
        assert not out[b, n:].any()


# ---- the C ABI: bitwise properties and graph capture --------------------------------------------------------------------------------
class _Abi(object):
    """One dense layer driven through ttrnn_rnn_forward / ttrnn_rnn_backward_ex with caller-owned buffers."""

    def __init__(self, kind, inp, H, seed=0):
        from ttrnn_hip import _lib
        from ttrnn_hip.functional import RnnLayerSpec, TTSpec
        self.lib = _lib.load()
        self.kind, self.inp, self.H, self.G = kind, inp, H, 4 if kind == "lstm" else 3
        g = torch.Generator().manual_seed(seed)
        GH = self.G * H
        self.w_in = (torch.randn(GH, inp, generator=g) / max(inp, 1) ** 0.5).to(dev())
        self.w_hid = (torch.randn(GH, H, generator=g) / H ** 0.5).to(dev())
        self.b_in = torch.randn(GH, generator=g).to(dev()) * 0.1
        self.b_hid = torch.randn(GH, generator=g).to(dev()) * 0.1
        self.spec = RnnLayerSpec(kind, inp, H, TTSpec([inp], [GH], [1, 1]), TTSpec([H], [GH], [1, 1]), True, True)
        self.p_in = self.spec.in_spec.pack([self.w_in.view(1, GH, inp, 1)])
        self.p_hid = self.spec.hid_spec.pack([self.w_hid.view(1, GH, H, 1)])

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    def _ws(self, nbytes, nan):
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev())
        ws.fill_(0xFF if nan else 0)                 # 0xFFFFFFFF / 0xFFFF: NaN as fp32 and as bf16
        return ws

    def forward(self, x, h0=None, c0=None, train=True, want_out=True, nan_ws=False):
        lib, H = self.lib, self.H
        B, T, _ = x.shape
        d = self.spec.desc(B, T, 0)
        assert lib.ttrnn_rnn_forward_route(ctypes.byref(d)) == 5 and lib.ttrnn_rnn_backward_route(ctypes.byref(d), 0) == 5
        r = dict(d=d, x=x, h0=h0, c0=c0)
        r["out"] = torch.full((B, T, H), float("nan"), device=dev()) if want_out else None
        r["hT"] = torch.full((B, H), float("nan"), device=dev())
        r["cT"] = torch.full((B, H), float("nan"), device=dev()) if self.kind == "lstm" else None
        r["reserve"] = torch.full((lib.ttrnn_rnn_reserve_bytes(ctypes.byref(d)) // 4,), float("nan"), device=dev()) if train else None
        wsb = lib.ttrnn_rnn_workspace(ctypes.byref(d))
        ws = self._ws(wsb, nan_ws)
        st = lib.ttrnn_rnn_forward(ctypes.byref(d), self._p(x), self._p(h0), self._p(c0), self._p(self.p_in), self._p(self.b_in),
                                   self._p(self.p_hid), self._p(self.b_hid), self._p(r["out"]), self._p(r["hT"]), self._p(r["cT"]),
                                   self._p(r["reserve"]), self._p(ws), wsb, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st
        r["ws"] = ws
        return r

    def backward(self, f, d_out, d_hT, d_cT=None, nan_ws=False):
        lib, H, G = self.lib, self.H, self.G
        B, T, _ = f["x"].shape
        d = f["d"]
        r = {}
        r["dg_in"] = torch.full((B, T, G * H), float("nan"), device=dev())
        r["dg_hid"] = torch.full((B, T, G * H), float("nan"), device=dev()) if self.kind == "gru" else r["dg_in"]
        r["d_h0"] = torch.full((B, H), float("nan"), device=dev())
        r["d_c0"] = torch.full((B, H), float("nan"), device=dev()) if self.kind == "lstm" else None
        wsb = lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 0)
        ws = self._ws(wsb, nan_ws)
        st = lib.ttrnn_rnn_backward_ex(ctypes.byref(d), self._p(f["out"]), self._p(f["h0"]), self._p(f["c0"]), self._p(self.p_hid),
                                       self._p(f["reserve"]), self._p(d_out), self._p(d_hT), self._p(d_cT), self._p(r["dg_in"]),
                                       self._p(r["dg_hid"]), self._p(r["d_h0"]), self._p(r["d_c0"]), None, None, None, self._p(ws), wsb,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, st
        r["ws"] = ws
        return r


def _same(a, b, keys):
    for k in keys:
        if a[k] is None:
            assert b[k] is None
            continue
        assert torch.equal(a[k], b[k]), k         # NaN anywhere fails too: every element was written


FWD_KEYS = ("out", "hT", "cT", "reserve")
BWD_KEYS = ("dg_in", "dg_hid", "d_h0", "d_c0")


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_bitwise_properties(kind):
    A = _Abi(kind, 28, 160, seed=11)
    B, T, H = 70, 6, 160
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, 28, generator=g).to(dev())
    h0 = torch.randn(B, H, generator=g).to(dev())
    c0 = torch.randn(B, H, generator=g).to(dev()) if kind == "lstm" else None
    d_out, d_hT = torch.randn(B, T, H, generator=g).to(dev()), torch.randn(B, H, generator=g).to(dev())
    d_cT = torch.randn(B, H, generator=g).to(dev()) if kind == "lstm" else None
    f1 = A.forward(x, h0, c0)
    b1 = A.backward(f1, d_out, d_hT, d_cT)
    torch.cuda.synchronize()
    assert all(torch.isfinite(f1[k]).all() for k in FWD_KEYS if f1[k] is not None)
    assert all(torch.isfinite(b1[k]).all() for k in BWD_KEYS if b1[k] is not None)
    # two runs; a run on a NaN-filled workspace
    f2 = A.forward(x, h0, c0, nan_ws=True)
    b2 = A.backward(f2, d_out, d_hT, d_cT, nan_ws=True)
    _same(f1, f2, FWD_KEYS)
    _same(b1, b2, BWD_KEYS)
    # the batch whole and in two halves (37 + 33: both across the 32-row tile)
    for lo, hi in ((0, 37), (37, 70)):
        s = slice(lo, hi)
        fh = A.forward(x[s].contiguous(), h0[s].contiguous(), None if c0 is None else c0[s].contiguous())
        bh = A.backward(fh, d_out[s].contiguous(), d_hT[s].contiguous(), None if d_cT is None else d_cT[s].contiguous())
        for k in ("out", "hT", "cT"):
            if f1[k] is not None:
                assert torch.equal(f1[k][s], fh[k]), k
        for k in BWD_KEYS:
            if b1[k] is not None:
                assert torch.equal(b1[k][s], bh[k]), k
    # T steps against two runs chained through (hT, cT)
    fa = A.forward(x[:, :4].contiguous(), h0, c0)
    fb = A.forward(x[:, 4:].contiguous(), fa["hT"], fa["cT"])
    assert torch.equal(torch.cat([fa["out"], fb["out"]], dim=1), f1["out"])
    assert torch.equal(fb["hT"], f1["hT"])
    if kind == "lstm":
        assert torch.equal(fb["cT"], f1["cT"])
    # inference without outputs and without a reserve: the same final state
    fi = A.forward(x, h0, c0, train=False, want_out=False, nan_ws=True)
    assert torch.equal(fi["hT"], f1["hT"])
    if kind == "lstm":
        assert torch.equal(fi["cT"], f1["cT"])


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_graph_capture_replays_the_eager_call(kind):
    A = _Abi(kind, 40, 128, seed=13)
    B, T, H = 33, 9, 128
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, T, 40, generator=g).to(dev())
    h0 = torch.randn(B, H, generator=g).to(dev())
    c0 = torch.randn(B, H, generator=g).to(dev()) if kind == "lstm" else None
    d_out, d_hT = torch.randn(B, T, H, generator=g).to(dev()), torch.randn(B, H, generator=g).to(dev())
    fe = A.forward(x, h0, c0)
    be = A.backward(fe, d_out, d_hT)
    torch.cuda.synchronize()
    xs = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fc = A.forward(xs, h0, c0)
            bc = A.backward(fc, d_out, d_hT)
    torch.cuda.current_stream().wait_stream(side)
    for k in FWD_KEYS + BWD_KEYS:
        t = fc.get(k) if k in FWD_KEYS else bc.get(k)
        if t is not None:
            t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _same(fe, fc, FWD_KEYS)
    _same(be, bc, BWD_KEYS)
    # a replay on new input values computes what the eager call computes on them
    x2 = torch.randn(B, T, 40, generator=g).to(dev())
    xs.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    f2 = A.forward(x2, h0, c0)
    b2 = A.backward(f2, d_out, d_hT)
    torch.cuda.synchronize()
    _same(f2, fc, FWD_KEYS)
    _same(b2, bc, BWD_KEYS)


# ---- harness ------------------------------------------------------------------------------------------------------------------------
def _run_example(args):
    env = dict(os.environ)
    p = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    assert p.returncode == 0, text
    return text


def _finite_loss(text):
    import re
    vals = [float(v) for v in re.findall(r"loss[^0-9\-]*(-?[0-9]+\.[0-9]+(?:e-?[0-9]+)?)", text, flags=re.I)]
    assert vals and all(np.isfinite(v) for v in vals), text


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_benchmarking_dense_runs(train):
    """--train prints the loss of the last timed step; eval (a no_grad forward: there is no loss) prints the largest
    log-probability of the last timed forward, which must be finite and <= 0."""
    import re
    text = _run_example(["examples/benchmarking.py", "--dense", "--hidden_size", "128", "--batch_size", "8", "--seq_len", "12",
                         "--in_size", "28", "--emb_size", "10", "-n", "2"] + (["--train"] if train else []))
    assert "forward dense_step, reverse dense_step" in text, text
    if train:
        _finite_loss(text)
    else:
        vals = [float(v) for v in re.findall(r"max log-probability: (\S+)", text)]
        assert len(vals) == 1 and np.isfinite(vals[0]) and vals[0] <= 0.0, text


def test_speaker_step_dense_runs():
    text = _run_example(["examples/speaker_step.py", "--dense", "--speakers", "4", "--utterances", "3", "--frames", "10",
                         "--hidden_size", "128", "--n_layers", "2", "-n", "2"])
    assert "forward dense_step, reverse dense_step" in text, text
    _finite_loss(text)

"""Per-sample sequence lengths on the GPU (include/ttrnn.h TTRNN_HAS_VARLEN; LSTM.forward / GRU.forward `lengths=`): the three
forward kernels that take lengths — the encoder-shape kernels (ttrnn_fast_w2.hip), the runtime-shape kernel (k_g2_fwd) and the
any-shape kernel (rnn_fwd_body) — and every reverse-kernel family UNCHANGED on the frozen records they leave.

Expected results: the oracle per sample on x[b:b+1, :len_b], losses summed (tests/varlen_ref.py; checked against the
reference's own numbers in tests/test_varlen_host.py).  Tolerances, the project's own (tests/test_w2.py:179-185): forward and
final states 1e-5 absolute; each gradient 1e-4 * max(1e-3, max|ref|)."""
import contextlib
import ctypes
import re

import pytest
import torch

from golden_io import Case
from test_gpu_parity import _maxabs, build_module, dev
from varlen_ref import grad_bound, oracle_varlen

pytestmark = pytest.mark.gpu

ENC = dict(kind="ttlstm", input_size=40, hidden_size=768, num_layers=1, n_cores=2, tt_rank=2)
SHAPES = {
    "enc_lstm": ENC,
    "enc_gru": dict(ENC, kind="ttgru"),
    "enc_lstm_r4": dict(ENC, tt_rank=4),
    "enc_gru_d4": dict(ENC, kind="ttgru", n_cores=4),
    "cfg2": dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8),
    "gru_h256_r8": dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8),
    "cfg1": dict(kind="ttlstm", input_size=1, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4),
    "naive_h256": dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8, is_naive=True),
    "h1024_r32": dict(kind="ttlstm", input_size=1, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32),
    "stack_r16": dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=16),
    "dense_lstm": dict(kind="lstm", input_size=28, hidden_size=64, num_layers=1),
    "dense_gru": dict(kind="gru", input_size=28, hidden_size=64, num_layers=1),
}
# the option that moves the encoder shape from its own kernels to the other two forward kernels that take lengths
ROUTE_OPTS = {"fused_core": None, "runtime_mfma": ("enc_fwd_on_tier", 1), "valu": ("force_generic", 1)}


@contextlib.contextmanager
def _opt(o):
    import ttrnn_hip
    if o is None:
        yield
    else:
        with ttrnn_hip.option(*o):
            yield


def _is_lstm(meta):
    return meta["kind"] in ("ttlstm", "lstm")


def _module(name, seed=61):
    torch.manual_seed(seed)
    return build_module(SHAPES[name], dev())


def _varlen_route(m, B, T, layer=0):
    from ttrnn_hip import functional as F
    return F.rnn_route(m._all_layers[layer]._layer_spec(), B, T, varlen=True)


def _bwd_route(m, B, T, layer=0):
    from ttrnn_hip import functional as F
    return F.rnn_backward_route(m._all_layers[layer]._layer_spec(), B, T)


def _sd(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def _call(m, x, init, **kw):
    """(out, hT, cT or None) of the module, LSTM or GRU."""
    if m.kind == "lstm":
        out, (h, c) = m(x, init, **kw)
        return out, h, c
    out, h = m(x, None if init is None else init[0], **kw)
    return out, h, None


# ---- 1. routes ----------------------------------------------------------------------------------------------------------------
def test_routes():
    import ttrnn_hip
    m = _module("enc_lstm")
    assert _varlen_route(m, 6, 11) == "fused_core"
    assert _varlen_route(_module("enc_gru"), 6, 11) == "fused_core"
    with ttrnn_hip.option("enc_fwd_on_tier", 1):
        assert _varlen_route(m, 6, 11) == "runtime_mfma"
    with ttrnn_hip.option("force_generic", 1):
        assert _varlen_route(m, 6, 11) == "valu"
    # shapes whose fixed-length forward is a fused-core / merged kernel that does not take lengths: the runtime tier
    for name in ("cfg2", "gru_h256_r8", "cfg1", "naive_h256", "h1024_r32", "stack_r16"):
        assert _varlen_route(_module(name), 4, 9) == "runtime_mfma", name
    # ... always one sample per workgroup, whatever the batch (the fixed-length call pairs samples past the CU count)
    assert _varlen_route(_module("naive_h256"), 600, 9) == "runtime_mfma"
    for name in ("dense_lstm", "dense_gru"):
        assert _varlen_route(_module(name), 4, 9) == "valu", name


# ---- 2. forward ---------------------------------------------------------------------------------------------------------------
FB, FT = 6, 11
FLEN = [11, 1, 2, 6, 11, 10]          # 1, 2 (the two-deep x prefetch), T - 1 and T
_FWD_REF = {}


def _fwd_data(shape, init):
    meta = SHAPES[shape]
    g = torch.Generator().manual_seed(67)
    x = torch.randn(FB, FT, meta["input_size"], generator=g)
    h0 = torch.randn(FB, meta["hidden_size"], generator=g) * 0.5
    c0 = torch.randn(FB, meta["hidden_size"], generator=g) * 0.5
    if not init:
        return x, None, None
    return x, h0, (c0 if _is_lstm(meta) else None)


def _fwd_ref(shape, init, m):
    """Computed once per (shape, init) and shared by the three routes; never modified."""
    key = (shape, init)
    if key not in _FWD_REF:
        x, h0, c0 = _fwd_data(shape, init)
        _FWD_REF[key] = oracle_varlen(SHAPES[shape]["kind"], _sd(m), 1, x, FLEN, h0, c0)
    return _FWD_REF[key]


@pytest.mark.parametrize("init", [True, False], ids=["init", "zero_state"])
@pytest.mark.parametrize("route", ["fused_core", "runtime_mfma", "valu"])
@pytest.mark.parametrize("shape", ["enc_lstm", "enc_gru", "enc_lstm_r4", "enc_gru_d4"])
def test_forward(shape, route, init):
    m = _module(shape)          # (same seed every time: the three routes share one reference)
    lstm = m.kind == "lstm"
    ref = _fwd_ref(shape, init, m)
    x, h0, c0 = _fwd_data(shape, init)
    xd = x.to(dev())
    st = None if not init else (h0.to(dev()), c0.to(dev()) if lstm else None)
    H = SHAPES[shape]["hidden_size"]
    with torch.no_grad(), _opt(ROUTE_OPTS[route]):
        assert _varlen_route(m, FB, FT) == route
        out, hT, cT = _call(m, xd, st, lengths=FLEN)
        assert _maxabs(out, ref["out"]) <= 1e-5
        assert _maxabs(hT, ref["hT"]) <= 1e-5
        if lstm:
            assert _maxabs(cT, ref["cT"]) <= 1e-5
        for b, n in enumerate(FLEN):
            assert not out[b, n:].any(), "padded rows of sample %d" % b
            if n < FT:        # the final state is the sample's own last step, not step T - 1
                assert torch.equal(out[b, n - 1], hT[b])
        # the inference call that consumes only the final state
        _, h2, c2 = _call(m, xd, st, need_outputs=False, lengths=FLEN)
        assert torch.equal(h2, hT) and (not lstm or torch.equal(c2, cT))
        # a device tensor of lengths (no validation, no synchronisation) is the same call
        o3, h3, _ = _call(m, xd, st, lengths=torch.tensor(FLEN, dtype=torch.int64, device=dev()))
        assert torch.equal(o3, out) and torch.equal(h3, hT)
        # input rows past a sample's length never influence a result
        xp = xd.clone()
        for b, n in enumerate(FLEN):
            xp[b, n:] = 37.5 - 3.0 * b
        o4, h4, c4 = _call(m, xp, st, lengths=FLEN)
        if route == "fused_core":
            assert torch.equal(o4, out) and torch.equal(h4, hT) and (not lstm or torch.equal(c4, cT))
            # sample b is, bit for bit, the fixed-length call on that sample alone
            for b, n in enumerate(FLEN):
                sb = None if st is None else (st[0][b:b + 1], st[1][b:b + 1] if lstm else None)
                ob, hb, cb = _call(m, xd[b:b + 1, :n].contiguous(), sb)
                assert torch.equal(ob[0], out[b, :n]) and torch.equal(hb[0], hT[b]), b
                assert not lstm or torch.equal(cb[0], cT[b]), b
            # all lengths = T: the fixed-length call
            of, hf, cf = _call(m, xd, st)
            ol, hl, cl = _call(m, xd, st, lengths=[FT] * FB)
            assert torch.equal(of, ol) and torch.equal(hf, hl) and (not lstm or torch.equal(cf, cl))
        else:
            assert _maxabs(o4, out) <= 1e-5 and _maxabs(h4, hT) <= 1e-5
            assert not lstm or _maxabs(c4, cT) <= 1e-5
    assert out.shape == (FB, FT, H)


@pytest.mark.parametrize("route", ["fused_core", "runtime_mfma", "valu"])
@pytest.mark.parametrize("name", ["g11_varlen_spk_lstm", "g11_varlen_spk_gru"])
def test_forward_vs_reference_fixture(name, route):
    """the reference itself, run per sample on the truncated inputs (tests/golden/gen_golden_varlen.py)"""
    case = Case(name)
    lstm = case.meta["kind"] == "ttlstm"
    m = build_module(case.meta, dev())
    m.load_state_dict(case.state_dict(), strict=True)
    st = (case.tensor("h0").to(dev()), case.tensor("c0").to(dev()) if lstm else None)
    with torch.no_grad(), _opt(ROUTE_OPTS[route]):
        assert _varlen_route(m, case.meta["B"], case.meta["T"]) == route
        out, hT, cT = _call(m, case.tensor("x").to(dev()), st, lengths=case.meta["lengths"])
    assert _maxabs(out, case.arr["out"]) <= 1e-5 and _maxabs(hT, case.arr["hT"]) <= 1e-5
    assert not lstm or _maxabs(cT, case.arr["cT"]) <= 1e-5


@pytest.mark.parametrize("name", ["g11_varlen_spk_lstm", "g11_varlen_spk_gru"])
def test_training_step_vs_reference_fixture(name):
    case = Case(name)
    lstm = case.meta["kind"] == "ttlstm"
    m = build_module(case.meta, dev())
    m.load_state_dict(case.state_dict(), strict=True)
    t = lambda k: case.tensor(k).to(dev())
    x, h0 = t("x").requires_grad_(True), t("h0").requires_grad_(True)
    c0 = t("c0").requires_grad_(True) if lstm else None
    out, hT, cT = _call(m, x, (h0, c0), lengths=case.meta["lengths"])
    loss = (out * t("w_out")).sum() + (hT * t("w_h")).sum()          # (the padded rows of out are zeros: w_out there is inert)
    if lstm:
        loss = loss + (cT * t("w_c")).sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(case.arr["loss"])) <= 1e-4 * max(1.0, abs(float(case.arr["loss"])))
    got = {"grad_x": x.grad, "grad_h0": h0.grad}
    if lstm:
        got["grad_c0"] = c0.grad
    for k, g in got.items():
        assert _maxabs(g, case.arr[k]) <= grad_bound(case.tensor(k)), k
    for k, g in case.grads().items():
        assert _maxabs(dict(m.named_parameters())[k].grad, g) <= grad_bound(g), k


# ---- 3. co-residency ----------------------------------------------------------------------------------------------------------
def test_coresident_workgroups_retire_independently():
    """B = 300 > 256 CUs: workgroups of different lengths share a CU; each sample equals, bit for bit, the fixed-length call on
    the group of samples that share its length."""
    m = _module("enc_lstm")
    B, T = 300, 5
    g = torch.Generator().manual_seed(71)
    x = torch.randn(B, T, 40, generator=g).to(dev())
    lens = torch.randint(1, T + 1, (B,), generator=g)
    with torch.no_grad():
        assert _varlen_route(m, B, T) == "fused_core"
        out, hT, cT = _call(m, x, None, lengths=lens)
        for n in range(1, T + 1):
            idx = (lens == n).nonzero().flatten().to(dev())
            assert idx.numel() > 0
            og, hg, cg = _call(m, x[idx][:, :n].contiguous(), None)
            assert torch.equal(out[idx][:, :n], og) and torch.equal(hT[idx], hg) and torch.equal(cT[idx], cg), n
            assert not out[idx][:, n:].any()


# ---- 4. training step: one case per reverse-kernel family ---------------------------------------------------------------------
TB, TT_, TLEN = 4, 9, [9, 1, 5, 8]
# name: (shape, library option or None, reverse-kernel family per layer, batch, steps, lengths, initial states)
TRAIN = {
    "enc_lstm": ("enc_lstm", None, ["fused_core"], TB, TT_, TLEN, True),
    "enc_gru": ("enc_gru", None, ["fused_core"], TB, TT_, TLEN, True),
    "enc_lstm_tier_bwd": ("enc_lstm", ("enc_bwd_on_tier", 1), ["runtime_mfma"], TB, TT_, TLEN, True),
    "enc_gru_tier_bwd": ("enc_gru", ("enc_bwd_on_tier", 1), ["runtime_mfma"], TB, TT_, TLEN, False),
    "force_generic": ("enc_lstm", ("force_generic", 1), ["valu"], TB, TT_, TLEN, True),
    "cfg2": ("cfg2", None, ["fused_core"], TB, TT_, TLEN, True),
    "gru_h256_r8": ("gru_h256_r8", None, ["fused_core"], TB, TT_, TLEN, True),
    "cfg1": ("cfg1", None, ["fused_core"], TB, TT_, TLEN, False),
    "naive_h256": ("naive_h256", None, ["fused_core"], TB, TT_, TLEN, True),
    "h1024_r32": ("h1024_r32", None, ["merged_big"], 2, 4, [4, 2], True),
    "stack_r16": ("stack_r16", None, ["fused_core", "fused_core"], TB, TT_, TLEN, True),
}


@pytest.mark.parametrize("dout", [True, False], ids=["out_term", "states_only"])
@pytest.mark.parametrize("case", sorted(TRAIN))
def test_training_step(case, dout):
    shape, o, families, B, T, lens, init = TRAIN[case]
    meta = SHAPES[shape]
    lstm, L, H = _is_lstm(meta), meta["num_layers"], meta["hidden_size"]
    m = _module(shape, seed=73)
    g = torch.Generator().manual_seed(79)
    x = torch.randn(B, T, meta["input_size"], generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.5 if init else None
    c0 = torch.randn(B, H, generator=g) * 0.5 if (init and lstm) else None
    w = torch.randn(B, T, H, generator=g) if dout else None
    wh, wc = torch.randn(B, H, generator=g), (torch.randn(B, H, generator=g) if lstm else None)
    ref = oracle_varlen(meta["kind"], _sd(m), L, x, lens, h0, c0, w, wh, wc)

    def run():
        m.zero_grad()
        xg = x.to(dev()).requires_grad_(True)
        hg = None if h0 is None else h0.to(dev()).requires_grad_(True)
        cg = None if c0 is None else c0.to(dev()).requires_grad_(True)
        out, hT, cT = _call(m, xg, None if not init else (hg, cg), lengths=lens)
        ls = (hT * wh.to(dev())).sum()
        if lstm:
            ls = ls + (cT * wc.to(dev())).sum()
        if dout:
            ls = ls + (out * w.to(dev())).sum()
        ls.backward()
        grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
        grads["x"] = xg.grad.cpu()
        if hg is not None:
            grads["h0"] = hg.grad.cpu()
        if cg is not None:
            grads["c0"] = cg.grad.cpu()
        return out.detach().cpu(), hT.detach().cpu(), grads

    with _opt(o):
        for layer, fam in enumerate(families):
            assert _bwd_route(m, B, T, layer) == fam, (layer, fam)       # the intended reverse-kernel family really runs
            assert _varlen_route(m, B, T, layer) == ("valu" if fam == "valu" else ("fused_core" if shape.startswith("enc_") else "runtime_mfma"))
        out, hT, got = run()
        again = run()[2] if case in ("enc_lstm", "enc_gru") else None
    assert _maxabs(out, ref["out"]) <= 1e-5 and _maxabs(hT, ref["hT"]) <= 1e-5
    expect = {"x": ref["grad_x"]}
    if init:
        expect["h0"] = ref["grad_h0"]
        if lstm:
            expect["c0"] = ref["grad_c0"]
    names = [n for n, _ in m.named_parameters()]
    for n in names:
        key = re.sub(r"\.gate(\d+)\.", r".gates.\1.", n)           # (a naive set's per-gate parameters: the oracle's key)
        expect[n] = ref["grads"][key]
    assert len(expect) >= len(names) + 1
    for n, r in expect.items():
        assert torch.isfinite(got[n]).all(), n
        assert _maxabs(got[n], r) <= grad_bound(r), (n, _maxabs(got[n], r), grad_bound(r))
    for b, n in enumerate(lens):
        assert not got["x"][b, n:].any(), "x gradient on the padded rows of sample %d" % b
    if again is not None:
        # bit for bit on a second run, wherever tests/test_w2.py asserts it for the fixed-length step
        rep = [n for n in got if "input_weights" not in n] if case == "enc_lstm" else ["x", "h0"]
        for n in rep:
            assert torch.equal(got[n], again[n]), n


# ---- 5. the seed kernel through the raw C ABI ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("have", ["both", "d_out_null", "d_hT_null"])
def test_seed_dout_c_abi(have, dtype):
    from ttrnn_hip import _lib
    from ttrnn_hip.functional import _ptr, _stream
    lib = _lib.load()
    m = _module("enc_lstm")
    B, T, H = 5, 7, 768
    lens = [7, 1, 4, 7, 2]
    desc = m._all_layers[0]._layer_spec().desc(B, T, _lib.TTRNN_F32 if dtype == torch.float32 else _lib.TTRNN_BF16)
    g = torch.Generator().manual_seed(83)
    d_out = torch.randn(B, T, H, generator=g).to(dtype).to(dev()) if have != "d_out_null" else None
    d_hT = torch.randn(B, H, generator=g).to(dtype).to(dev()) if have != "d_hT_null" else None
    ld = torch.tensor(lens, dtype=torch.int32, device=dev())
    seeded = torch.full((B, T, H), float("nan"), dtype=dtype, device=dev())
    with torch.cuda.device(dev()):
        rc = lib.ttrnn_rnn_varlen_seed_dout(ctypes.byref(desc), _ptr(ld), _ptr(d_out), _ptr(d_hT), _ptr(seeded), _stream(seeded))
    assert rc == 0
    exp = torch.zeros(B, T, H, dtype=torch.float32, device=dev())
    for b, n in enumerate(lens):
        if d_out is not None:
            exp[b, :n] = d_out[b, :n].float()
        if d_hT is not None:
            exp[b, n - 1] += d_hT[b].float()
    assert torch.equal(seeded, exp.to(dtype))          # the sum is formed in fp32 and rounded once
    assert lib.ttrnn_rnn_varlen_seed_dout(ctypes.byref(desc), None, _ptr(d_out), _ptr(d_hT), _ptr(seeded), _stream(seeded)) == -2


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_reads_lengths_at_replay():
    m = _module("enc_lstm")
    B, T = 6, 11
    g = torch.Generator().manual_seed(89)
    x = torch.randn(B, T, 40, generator=g).to(dev())
    lens = torch.tensor(FLEN, dtype=torch.int32, device=dev())
    other = [3, 11, 11, 1, 7, 2]
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x, lengths=lens)                                   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, (hT, cT) = m(x, lengths=lens)
        lens.copy_(torch.tensor(other, dtype=torch.int32))       # in place: the graph holds the buffer
        graph.replay()
        torch.cuda.synchronize()
        eo, (eh, ec) = m(x, lengths=other)
    assert torch.equal(out, eo) and torch.equal(hT, eh) and torch.equal(cT, ec)
    for b, n in enumerate(other):
        assert not out[b, n:].any()


# ---- 7. host validation -------------------------------------------------------------------------------------------------------
def test_host_validation():
    m = _module("enc_lstm")
    x = torch.randn(4, 9, 40, device=dev())
    for bad in ([9, 0, 5, 8], [9, 10, 5, 8], [9, 1, 5], [9, 1, 5, 8, 2], [9.0, 1.0, 5.0, 8.0]):
        with pytest.raises(ValueError):
            m(x, lengths=bad)
    with pytest.raises(ValueError):
        m(x, lengths=torch.tensor([9, 1, 5], device=dev()))
    import io
    from tensorized_rnn.gru import TTGRU
    with contextlib.redirect_stdout(io.StringIO()):
        logged = TTGRU(40, 768, 1, dev(), n_cores=2, tt_rank=2, log_grads=True)
    with pytest.raises(ValueError):
        logged(x, lengths=[9, 1, 5, 8])
    # a prepared module given lengths takes the unprepared path
    with torch.no_grad():
        plain = m(x, lengths=[9, 1, 5, 8])[0]
        m.prepare_for_inference()
        assert torch.equal(m(x, lengths=[9, 1, 5, 8])[0], plain)

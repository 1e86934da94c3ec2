"""GPU parity tests (run with `-m gpu` on an MI355X): the product modules — drop-in
`tensorized_rnn` / `t3nsor` API over libttrnn.so — against
  (1) the golden fixtures generated from the reference itself (tests/golden/*.npz),
  (2) the CPU oracle on seeded random inputs at sizes it finishes in seconds,
  (3) size-independent properties at BASELINE.json's full sizes.
Tolerances: fp32 forward 1e-5 abs (784-step cases included; measured 1.2e-7); gradients 1e-4 of
the tensor's max magnitude; bf16 storage vs the fp32 oracle 2e-2 abs.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

from golden_io import Case, build_module, case_names

pytestmark = pytest.mark.gpu



class _RouteSwitches(object):
    """The library's kernel-route switches (include/ttrnn.h: ttrnn_set_option) behind the names of the environment
    variables that initialise them: OPT["TTRNN_NO_GEMM"] = "1"; OPT.pop("TTRNN_NO_GEMM") restores the default."""
    DEFAULTS = {"big_merge": 2}

    @staticmethod
    def _name(key):
        assert key.startswith("TTRNN_")
        return key[len("TTRNN_"):].lower()

    def __setitem__(self, key, value):
        import ttrnn_hip
        ttrnn_hip.set_option(self._name(key), int(value))

    def pop(self, key, default=None):
        import ttrnn_hip
        name = self._name(key)
        ttrnn_hip.set_option(name, self.DEFAULTS.get(name, 0))

    def update(self, mapping):
        for k, v in mapping.items():
            self[k] = v


OPT = _RouteSwitches()


def dev():
    return torch.device("cuda:0")


def _maxabs(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _loaded_module(case):
    m = build_module(case.meta, dev())
    missing = m.load_state_dict(case.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m


def _run(case, m, requires_grad=False):
    lstm = case.meta["kind"] in ("ttlstm", "lstm")
    x = case.tensor("x").to(dev())
    h0 = case.tensor("h0")
    c0 = case.tensor("c0")
    h0 = h0.to(dev()) if h0 is not None else None
    c0 = c0.to(dev()) if c0 is not None else None
    if requires_grad:
        x.requires_grad_(True)
        if h0 is not None:
            h0.requires_grad_(True)
        if c0 is not None:
            c0.requires_grad_(True)
    if lstm:
        out, (hT, cT) = m(x, None if h0 is None else (h0, c0))
    else:
        out, hT = m(x, h0)
        cT = None
    return dict(out=out, hT=hT, cT=cT, x=x, h0=h0, c0=c0)


def _check_forward(case, res, tol):
    out = res["out"].detach().cpu()
    if "out_t_index" in case.arr:
        out = out[:, torch.from_numpy(case.arr["out_t_index"]), :]
    assert _maxabs(out, case.arr["out"]) <= tol
    assert _maxabs(res["hT"].detach(), case.arr["hT"]) <= tol
    if res["cT"] is not None:
        assert _maxabs(res["cT"].detach(), case.arr["cT"]) <= tol


def test_library_loaded_and_device_visible():
    from ttrnn_hip import _lib
    lib = _lib.load()
    assert lib.ttrnn_device_available() == 1


@pytest.mark.parametrize("name", case_names("g3_ttlinear_"))
def test_ttlinear_golden(name):
    from t3nsor.layers import TTLinear
    case = Case(name)
    meta = case.meta
    with contextlib.redirect_stdout(io.StringIO()):
        lin = TTLinear(out_features=int(np.prod(meta["shape"][1])), shape=meta["shape"], bias=meta["bias"],
                       auto_shapes=False, d=len(meta["shape"][0]), tt_rank=meta["tt_rank"]).to(dev())
    lin.load_state_dict(case.state_dict(), strict=True)
    x = case.tensor("x").to(dev()).requires_grad_(True)
    y = lin(x)
    assert _maxabs(y.detach(), case.arr["y"]) <= 1e-5
    (y * case.tensor("w").to(dev())).sum().backward()

    def close(got, exp, what):
        assert _maxabs(got, exp) <= 1e-4 * max(float(np.abs(exp).max()), 1e-6) + 1e-7, what

    close(x.grad, case.arr["grad_x"], "grad_x")
    for n, p in lin.named_parameters():
        close(p.grad, case.arr["grad/" + n], n)
        assert p.grad.stride() == p.stride()


@pytest.mark.parametrize("name", case_names("g3_ttlinear_"))
def test_tt_dense_matmul_golden(name):
    """The drop-in `t3nsor.tt_dense_matmul` itself (the reference's t3nsor/ops.py:54-93: TT-matrix (M x N) @ dense (N x P) ->
    dense (M x P)) called the way TTLinear.forward calls it (layers.py:121-127: `tt_dense_matmul(weight_t, x^T)^T + bias`) on the
    reference-generated TTLinear fixtures, plus its ValueError on mismatched inner dimensions (ops.py:65-69)."""
    import t3nsor
    from t3nsor.layers import TTLinear
    case = Case(name)
    meta = case.meta
    with contextlib.redirect_stdout(io.StringIO()):
        lin = TTLinear(out_features=int(np.prod(meta["shape"][1])), shape=meta["shape"], bias=meta["bias"],
                       auto_shapes=False, d=len(meta["shape"][0]), tt_rank=meta["tt_rank"]).to(dev())
    lin.load_state_dict(case.state_dict(), strict=True)
    x = case.tensor("x").to(dev())
    with torch.no_grad():
        y = t3nsor.tt_dense_matmul(lin.weight_t, x.transpose(0, 1))
        assert tuple(y.shape) == (int(np.prod(meta["shape"][1])), x.shape[0])          # (out_features, batch): ops.py:93
        y = y.transpose(0, 1)
        if lin.bias is not None:
            y = y + lin.bias
    assert _maxabs(y, case.arr["y"]) <= 1e-5
    with pytest.raises(ValueError):                       # inner dimensions do not align
        t3nsor.tt_dense_matmul(lin.weight_t, torch.zeros(x.shape[1] + 1, 3, device=dev()))


@pytest.mark.parametrize("name", case_names("g4_cell_"))
def test_cell_step_golden(name):
    case = Case(name)
    m = _loaded_module(case)
    x, h = case.tensor("x").to(dev()), case.tensor("h").to(dev())
    with torch.no_grad():
        if case.meta["kind"] == "ttlstm":
            hy, cy = m.cell0(x, h, case.tensor("c").to(dev()))
            assert _maxabs(cy, case.arr["cy"]) <= 1e-5
        else:
            hy = m.cell0(x, h)
    assert _maxabs(hy, case.arr["hy"]) <= 1e-5


@pytest.mark.parametrize("name", case_names("g5_seq_") + case_names("g8_var_"))
def test_sequence_golden(name):
    case = Case(name)
    m = _loaded_module(case)
    with torch.no_grad():
        res = _run(case, m)
    _check_forward(case, res, 1e-5)      # <= 1e-5 abs, the 784-step sequences included


def _check_gradients_golden(name):
    case = Case(name)
    m = _loaded_module(case)
    res = _run(case, m, requires_grad=True)
    _check_forward(case, res, 1e-5)
    loss = (res["out"] * case.tensor("w_out").to(dev())).sum() + (res["hT"] * case.tensor("w_h").to(dev())).sum()
    if res["cT"] is not None:
        loss = loss + (res["cT"] * case.tensor("w_c").to(dev())).sum()
    loss.backward()

    def close(got, exp, what):
        assert got is not None, what
        assert _maxabs(got, exp) <= 1e-4 * max(float(np.abs(exp).max()), 1e-6) + 1e-7, what

    params = dict(m.named_parameters())
    for key, g in case.grads().items():
        close(params[key].grad, g.numpy(), key)
    close(res["x"].grad, case.arr["grad_x"], "grad_x")
    if "grad_h0" in case.arr:
        close(res["h0"].grad, case.arr["grad_h0"], "grad_h0")
    if "grad_c0" in case.arr:
        close(res["c0"].grad, case.arr["grad_c0"], "grad_c0")


@pytest.mark.parametrize("name", case_names("g6_bwd_") + [n for n in case_names("g8_var_") if "b1t1" not in n])
def test_gradients_golden(name):
    _check_gradients_golden(name)


# ---- (2) seeded random inputs against the oracle -----------------------------------------------------
ORACLE_CFGS = [
    ("ttlstm", 1, 256, 1, 3, 8, 6, 40),      # cfg2 shapes
    ("ttgru", 1, 256, 1, 3, 8, 5, 40),       # cfg3 shapes (fp32)
    ("ttlstm", 40, 256, 3, 3, 16, 5, 12),    # cfg4 shapes
    ("ttlstm", 1, 128, 1, 2, 4, 7, 50),      # cfg1 shapes
    ("ttgru", 28, 64, 2, 2, 3, 9, 11),       # ragged batch, tiny
    ("ttlstm", 10, 100, 1, 2, 5, 3, 7),      # non power-of-two modes
]


def _oracle_forward(kind, sd, L, x, init=None):
    from oracle import ttrnn_oracle as O
    layers, _ = O.layers_from_state_dict(sd, L, dtype=x.dtype)
    with torch.no_grad():
        if kind == "ttlstm":
            out, (h, c) = O.lstm_forward(layers, x, init)
            return out, h, c
        out, h = O.gru_forward(layers, x, init)
        return out, h, None


@pytest.mark.parametrize("kind,inp,H,L,d,r,B,T", ORACLE_CFGS)
def test_sequence_vs_oracle(kind, inp, H, L, d, r, B, T):
    torch.manual_seed(1234 + H + T)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=d, tt_rank=r)
    m = build_module(meta, dev())
    x = torch.randn(B, T, inp)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ro, rh, rc = _oracle_forward(kind, sd, L, x)
    with torch.no_grad():
        res = m(x.to(dev()))
    out = res[0]
    hT = res[1][0] if kind == "ttlstm" else res[1]
    assert _maxabs(out, ro) <= 1e-5
    assert _maxabs(hT, rh) <= 1e-5
    if kind == "ttlstm":
        assert _maxabs(res[1][1], rc) <= 1e-5


def test_bf16_storage_vs_fp32_oracle():
    """cfg3-shaped TT-GRU with bf16 storage (x / out / weights), fp32 state and accumulation; the
    reference has no bf16 path, so the check is against the fp32 oracle on bf16-rounded weights."""
    torch.manual_seed(7)
    meta = dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8)
    m = build_module(meta, dev()).to(torch.bfloat16)
    x = torch.rand(8, 64, 1).to(torch.bfloat16)
    sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items()}
    ro, rh, _ = _oracle_forward("ttgru", sd, 1, x.float())
    with torch.no_grad():
        out, hT = m(x.to(dev()))
    assert out.dtype == torch.bfloat16
    # relative to the oracle's own magnitude (a default-init TT-GRU's outputs have std ~ 0.03: an absolute 2e-2 would pass a
    # badly wrong kernel): bf16 rounding of the stored outputs is 2^-8 = 3.9e-3 of a value, everything else is fp32
    assert _maxabs(out.float(), ro) <= 1.5e-2 * float(ro.abs().max())
    assert _maxabs(hT.float(), rh) <= 1.5e-2 * float(rh.abs().max())


# ---- (3) properties at full size -------------------------------------------------------------------
def _cfg2_module():
    torch.manual_seed(1111)
    return build_module(dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), dev())


def test_full_size_batch_independence_and_prefix():
    """cfg2 at full size (B=64, T=784): samples never interact, and the first steps of a long
    sequence equal a short run (causality); hT equals the last output row; cT is finite."""
    m = _cfg2_module()
    torch.manual_seed(1111)
    x = torch.rand(64, 784, 1, device=dev())
    with torch.no_grad():
        out, (hT, cT) = m(x)
        out_a, _ = m(x[:17])
        out_b, _ = m(x[17:])
        out_p, (hp, cp) = m(x[:, :100].contiguous())
    assert torch.equal(out[:17], out_a) and torch.equal(out[17:], out_b)
    assert torch.equal(out[:, :100], out_p)
    assert torch.equal(out[:, -1], hT)
    assert torch.isfinite(out).all() and torch.isfinite(cT).all()
    # restart from the state at step 100 reproduces the tail
    with torch.no_grad():
        out_t, (ht, ct) = m(x[:, 100:].contiguous(), (hp, cp))
    assert _maxabs(out_t, out[:, 100:]) <= 1e-6
    assert _maxabs(ct, cT) <= 1e-6


def test_full_size_cfg2_subsample_vs_oracle():
    """Two samples of the full cfg2 problem against the oracle over all 784 steps."""
    m = _cfg2_module()
    torch.manual_seed(5)
    x = torch.rand(64, 784, 1)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ro, rh, rc = _oracle_forward("ttlstm", sd, 1, x[[3, 60]])
    with torch.no_grad():
        out, (hT, cT) = m(x.to(dev()))
    assert _maxabs(out[[3, 60]], ro) <= 1e-5
    assert _maxabs(cT[[3, 60]], rc) <= 1e-5


def test_full_size_cfg2_split_vs_exact_all_rows():
    """cfg2 at full size (B = 64, T = 784) in BOTH math modes: the default split mode (two fp16 pieces per fp32 operand) against the
    mode whose every product is an fp32 MFMA product on ALL 64 x 784 output rows, and both against the oracle evaluated in float64
    on a subset of the batch rows over all steps (the forward counterpart of
    tests/test_full_size_backward.py::test_cfg2_full_batch_unmasked)."""
    import ttrnn_hip
    m = _cfg2_module()
    torch.manual_seed(1111)
    x = torch.rand(64, 784, 1)
    rows = [0, 7, 31, 50, 63]
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, _, c64 = _oracle_forward("ttlstm", sd, 1, x[rows].double())
    res = {}
    for mode in ("split", "exact"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            res[mode] = m(x.to(dev()))
    d_out = _maxabs(res["split"][0], res["exact"][0])
    d_c = _maxabs(res["split"][1][1], res["exact"][1][1])
    errs = {mode: max(_maxabs(res[mode][0][rows], r64), _maxabs(res[mode][1][1][rows], c64)) for mode in res}
    print("cfg2 64 x 784: max |split - exact| out %.3g cT %.3g; vs float64 on rows %s: %s" % (d_out, d_c, rows, errs))
    assert d_out <= 1e-6 and d_c <= 2e-6
    assert errs["split"] <= 1e-6 and errs["exact"] <= 1e-6
    assert errs["split"] <= 2.0 * errs["exact"] + 1e-7


FULL_SIZE = {
    # BASELINE.json configs[2..4] at their full per-GPU size: (kind, in, H, L, d, r, B, T, storage dtype, sub-sampled
    # batch rows checked against the oracle over ALL steps, abs tol, tol relative to max |oracle|)
    "cfg3": ("ttgru", 1, 256, 1, 3, 8, 256, 784, torch.bfloat16, [0, 101, 255], 3e-3, 1.5e-2),      # measured 8.4e-4 / 4.0e-3 (one bf16 ulp)
    "cfg3_fp32": ("ttgru", 1, 256, 1, 3, 8, 256, 784, torch.float32, [0, 101, 255], 5e-6, 2e-5),   # measured 1.2e-7 / 5.6e-7
    "cfg4": ("ttlstm", 40, 256, 3, 3, 16, 512, 160, torch.float32, [0, 1, 300, 511], 5e-6, 5e-5),  # measured 1.2e-7 / 4.9e-6
    "cfg5": ("ttlstm", 1024, 1024, 1, 4, 32, 128, 1024, torch.float32, [5, 127], 5e-6, 2e-5),       # measured 5.9e-7 / 9.3e-7
}


@pytest.mark.parametrize("name", sorted(FULL_SIZE))
def test_full_size_configs_vs_oracle_and_properties(name):
    """cfg3 / cfg4 / cfg5 at the sizes bench.py times them — the kernels that only run there (cfg3: 256 workgroups of the
    bf16 fused-core GRU; cfg4: two samples per workgroup + dense-GEMM K-in over 81 920 rows; cfg5: pair kernels with the
    1 024-step tagged exchange) against the oracle on sub-sampled batch rows over ALL steps, plus the size-independent
    properties of tensorized_rnn/lstm.py:101-135: samples never interact (a different batch split reproduces the rows
    bit for bit), causality (a prefix run equals the head of the long run), hT == outputs[:, -1], restart from a
    mid-sequence state reproduces the tail."""
    kind, inp, H, L, d, r, B, T, dtype, rows, atol, rtol = FULL_SIZE[name]
    lstm = kind == "ttlstm"
    torch.manual_seed(1111)
    m = build_module(dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=d, tt_rank=r), dev()).to(dtype)
    torch.manual_seed(23)
    x = torch.rand(B, T, inp).to(dtype)
    sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items()}
    ro, rh, rc = _oracle_forward(kind, sd, L, x[rows].float())
    xd = x.to(dev())
    if name == "cfg3_fp32":      # the reference's own GRU dtype: the two-piece fused-core kernel (k_gru_fwd_f10vh, round 5)
        from ttrnn_hip import functional as F
        assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == "fused_core"
    with torch.no_grad():
        res = m(xd)
        out, hT = res[0], (res[1][0] if lstm else res[1])
        cT = res[1][1] if lstm else None
        assert out.dtype == dtype and out.shape == (B, T, H)
        err = _maxabs(out[rows].float(), ro)
        scale = float(ro.abs().max())
        print("%s: max |out - oracle| = %.3g over %d x %d steps (max |oracle| %.3g, relative %.3g)" % (
            name, err, len(rows), T, scale, err / scale))
        assert err <= atol
        if rtol is not None:
            assert err <= rtol * scale
        assert _maxabs(hT[rows].float(), rh) <= atol
        if lstm:
            assert _maxabs(cT[rows].float(), rc) <= atol
        assert torch.isfinite(out.float()).all()
        assert torch.equal(out[:, -1], hT)                                        # lstm.py:133,135
        # batch independence: another split of the batch (different workgroup <-> sample assignment; for cfg4 the second
        # part has an odd number of samples: one workgroup of the two-samples kernel runs half empty)
        cut = B // 2 - 3
        oa = m(xd[:cut])[0]
        ob = m(xd[cut:])[0]
        assert torch.equal(out[:cut], oa) and torch.equal(out[cut:], ob)
        # causality + restart (only layer-0-state semantics for L == 1: init_states is shared by all layers, lstm.py:120)
        tp = T // 3
        resp = m(xd[:, :tp].contiguous())
        assert torch.equal(out[:, :tp], resp[0])
        if L == 1:
            rest = m(xd[:, tp:].contiguous(), resp[1])
            tail_tol = 2e-2 if dtype == torch.bfloat16 else 1e-6
            assert _maxabs(rest[0].float(), out[:, tp:].float()) <= tail_tol


def test_ttlinear_linearity_full_rows():
    """TTLinear over 64*784 rows: f(a x1 + b x2) - bias = a (f(x1) - bias) + b (f(x2) - bias)."""
    from t3nsor.layers import TTLinear
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        lin = TTLinear(out_features=1024, shape=[[4, 8, 8], [8, 8, 16]], bias=True, auto_shapes=False, d=3,
                       tt_rank=8).to(dev())
    x1 = torch.randn(64 * 784, 256, device=dev())
    x2 = torch.randn(64 * 784, 256, device=dev())
    with torch.no_grad():
        b = lin.bias
        lhs = lin(0.5 * x1 - 2.0 * x2) - b
        rhs = 0.5 * (lin(x1) - b) - 2.0 * (lin(x2) - b)
    assert _maxabs(lhs, rhs) <= 1e-5


def test_empty_and_degenerate_inputs():
    m = _cfg2_module()
    with torch.no_grad():
        out, (hT, cT) = m(torch.zeros(0, 5, 1, device=dev()))
        assert out.shape == (0, 5, 256) and hT.shape == (0, 256)
        out, (hT, cT) = m(torch.rand(1, 1, 1, device=dev()))
        assert out.shape == (1, 1, 256) and torch.equal(out[:, -1], hT)
    with pytest.raises(Exception):
        m(torch.zeros(2, 3, 5, device=dev()))          # wrong input size
    with pytest.raises(Exception):
        m(torch.zeros(2, 3, 1))                          # CPU tensor: no CPU fallback


_DEGENERATE_ROUTES = {
    "fused_core_lstm": dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8),
    "fused_core_lstm_r16_stack": dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=16),
    "fused_core_gru": dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8),
    "stagewise": dict(kind="ttlstm", input_size=1, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4),
    "runtime_mfma_gru": dict(kind="ttgru", input_size=28, hidden_size=128, num_layers=2, n_cores=3, tt_rank=4),
    "merged_big": dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32),
}


@pytest.mark.parametrize("route", sorted(_DEGENERATE_ROUTES))
def test_degenerate_shapes_across_routes(route):
    """The shapes a caller can hand over without thinking (the reference's loops simply run zero or one times,
    lstm.py:123-133 / gru.py:124-134): an empty batch, a single step, a single sample — on every kernel family, forward
    against the oracle and one backward pass (finite gradients of the right shapes; single step: against the oracle too)."""
    from oracle import ttrnn_oracle as O
    torch.manual_seed(17)
    meta = _DEGENERATE_ROUTES[route]
    lstm = meta["kind"] == "ttlstm"
    m = build_module(meta, dev())
    inp, H, L = meta["input_size"], meta["hidden_size"], meta["num_layers"]
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        res = m(torch.zeros(0, 4, inp, device=dev()))
        assert res[0].shape == (0, 4, H) and (res[1][0] if lstm else res[1]).shape == (0, H)
    for B, T in ((1, 1), (3, 1), (1, 5)):
        x = torch.randn(B, T, inp)
        layers, leaves = O.layers_from_state_dict(sd, L, requires_grad=True)
        xr = x.clone().requires_grad_(True)
        ro = (O.lstm_forward(layers, xr) if lstm else O.gru_forward(layers, xr))[0]
        w = torch.randn(B, T, H)
        (ro * w).sum().backward()
        m.zero_grad()
        xg = x.to(dev()).requires_grad_(True)
        out = m(xg)[0]
        (out * w.to(dev())).sum().backward()
        assert out.shape == (B, T, H) and _maxabs(out.detach(), ro.detach()) <= 1e-5, (route, B, T)
        assert _maxabs(xg.grad, xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-6), (route, B, T)
        for name, p in m.named_parameters():
            ref = leaves[name].grad
            assert p.grad is not None and p.grad.shape == ref.shape
            assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), (route, B, T, name)


def test_stagewise_shape_takes_the_dense_gradient_route_over_many_rows():
    """The speaker encoder's --gru variant (speaker_encoder.py:69-78: 3-layer TT-GRU, H = 256, r = 16): a shape with stage-wise
    MFMA kernels but no fused-core weight-gradient kernel.  Over >= 4 * in rows its TTLinear backward now runs as dense GEMMs
    (dW = x^T dy, dx = dy W^T) with the pull-back to the cores by ttrnn_fast_proj.hip, like the shapes of the other tiers
    (before: row by row through the stage-wise kernel, 6 ms per matrix at the experiment's size): every gradient against
    the oracle, and the two routes (option no_gemm) against each other."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(31)
    meta = dict(kind="ttgru", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=16)
    m = build_module(meta, dev())
    B, T = 24, 48                                    # 1 152 rows >= 4 * 256
    x = torch.randn(B, T, 40) * 0.5
    w = torch.randn(B, T, 256)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 2, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    ro = O.gru_forward(layers, xr)[0]
    (ro * w).sum().backward()
    grads = {}
    for name, opts in (("dense", {}), ("rows", {"no_gemm": 1})):
        m.zero_grad()
        xg = x.to(dev()).requires_grad_(True)
        with contextlib.ExitStack() as st:
            for k, v in opts.items():
                st.enter_context(ttrnn_hip.option(k, v))
            out = m(xg)[0]
            (out * w.to(dev())).sum().backward()
        grads[name] = ({n: p.grad.detach().clone() for n, p in m.named_parameters()}, xg.grad.detach().clone())
        assert _maxabs(out.detach(), ro.detach()) <= 1e-5
        assert _maxabs(xg.grad, xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-6), name
        for n, g in grads[name][0].items():
            ref = leaves[n].grad
            assert _maxabs(g, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), (name, n)
    assert any(not torch.equal(grads["dense"][0][n], grads["rows"][0][n]) for n in grads["dense"][0])      # the switch works


def test_bf16_storage_gradients_vs_fp32_oracle():
    """bf16 storage through the MFMA forward + reverse-time + batched backward kernels (fp32 gate
    gradients against bf16 activations); checked against the fp32 oracle on the bf16-rounded weights."""
    from oracle import ttrnn_oracle as O
    torch.manual_seed(11)
    for kind in ("ttgru", "ttlstm"):
        meta = dict(kind=kind, input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8)
        m = build_module(meta, dev()).to(torch.bfloat16)
        x = torch.rand(6, 12, 1).to(torch.bfloat16)
        sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items()}
        layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True)
        xr = x.float().requires_grad_(True)
        if kind == "ttlstm":
            ro, (rh, rc) = O.lstm_forward(layers, xr)
        else:
            ro, rh = O.gru_forward(layers, xr)
        w = torch.randn(ro.shape)
        (ro * w).sum().backward()
        xg = x.to(dev()).requires_grad_(True)
        res = m(xg)
        (res[0].float() * w.to(dev())).sum().backward()
        assert _maxabs(res[0].float(), ro.detach()) <= 1.5e-2 * float(ro.detach().abs().max())      # (relative: see above)
        for name, p in m.named_parameters():
            ref = leaves[name].grad
            scale = max(float(ref.abs().max()), 1e-3)
            assert p.grad is not None and p.grad.dtype == torch.bfloat16
            assert _maxabs(p.grad.float(), ref) <= 6e-2 * scale, (kind, name)
        assert _maxabs(xg.grad.float(), xr.grad) <= 6e-2 * max(float(xr.grad.abs().max()), 1e-3)


def test_fast_and_generic_paths_agree():
    """The shape-specialised MFMA kernels against the any-shape kernels (TTRNN_FORCE_GENERIC=1) on the
    same module: forward and every gradient."""
    import os
    torch.manual_seed(5)
    meta = dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8)
    m = build_module(meta, dev())
    x = torch.rand(5, 20, 1, device=dev())
    w = torch.randn(5, 20, 256, device=dev())
    outs = []
    for force in ("0", "1"):
        OPT["TTRNN_FORCE_GENERIC"] = force
        try:
            m.zero_grad()
            xg = x.clone().requires_grad_(True)
            out, (h, c) = m(xg)
            ((out * w).sum() + c.sum()).backward()
            outs.append((out.detach().clone(), xg.grad.clone(), [p.grad.clone() for p in m.parameters()]))
        finally:
            OPT["TTRNN_FORCE_GENERIC"] = "0"
    assert _maxabs(outs[0][0], outs[1][0]) <= 2e-6
    assert _maxabs(outs[0][1], outs[1][1]) <= 1e-5 * max(1.0, float(outs[1][1].abs().max()))
    for a, b in zip(outs[0][2], outs[1][2]):
        assert _maxabs(a, b) <= 1e-4 * max(float(b.abs().max()), 1e-6)


def test_classifier_and_encoder_heads_vs_oracle():
    """The callers of the path: TT-RNN -> TTLinear head -> log_softmax, and
    TT-RNN -> TTLinear -> ReLU -> L2-normalise; forward and one backward against the CPU oracle."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from models import MNISTClassifier, SpeakerEncoder
    from oracle import ttrnn_oracle as O
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        clf = MNISTClassifier(1, 10, 256, 1, dev(), gru=False, n_cores=3, tt_rank=8).to(dev())
        enc = SpeakerEncoder(40, 256, 2, 256, dev(), n_cores=3, rank=16).to(dev())
    x = torch.rand(4, 30, 1)
    target = torch.tensor([1, 3, 5, 7])
    logp = clf(x.to(dev()))
    loss = torch.nn.functional.nll_loss(logp, target.to(dev()))
    loss.backward()
    sd = {k: v.detach().cpu() for k, v in clf.state_dict().items()}
    layers, leaves = O.layers_from_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("rnn.")}, 1, True)
    head = [sd["linear.parameters.%d" % k].clone().requires_grad_(True) for k in range(3)]
    hb = sd["linear.bias"].clone().requires_grad_(True)
    ro, _ = O.lstm_forward(layers, x)
    rlogp = torch.log_softmax(O.ttlinear(head, hb, ro[:, -1, :]), dim=1)
    rloss = torch.nn.functional.nll_loss(rlogp, target)
    rloss.backward()
    assert _maxabs(logp.detach(), rlogp.detach()) <= 1e-5
    assert abs(loss.item() - rloss.item()) <= 1e-5
    for k in range(3):
        g = clf.linear.weight_t.tt_cores[k].grad
        assert _maxabs(g, head[k].grad) <= 1e-4 * max(float(head[k].grad.abs().max()), 1e-6)
    for name, p in clf.rnn.named_parameters():
        ref = leaves[name].grad
        assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
    # speaker encoder forward
    u = torch.rand(6, 12, 40)
    emb = enc(u.to(dev()))
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    layers, _ = O.layers_from_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("rnn.")}, 2)
    with torch.no_grad():
        _, (rh, _) = O.lstm_forward(layers, u)
        raw = torch.relu(O.ttlinear([sd["linear.parameters.%d" % k] for k in range(3)], sd["linear.bias"], rh))
        remb = raw / torch.norm(raw, dim=1, keepdim=True)
    assert emb.shape == (6, 256)
    assert _maxabs(emb.detach(), remb) <= 1e-4


@pytest.mark.parametrize("kind,inp,H,L,r,B,T,dtype", [
    ("ttlstm", 1, 256, 1, 8, 64, 200, torch.float32),      # fused LSTM kernel, in=1 path
    ("ttgru", 1, 256, 1, 8, 96, 120, torch.float32),       # unfused kernel
    ("ttlstm", 40, 256, 2, 16, 80, 40, torch.float32),     # r=16, hoisted batched projection, 2 layers
    ("ttgru", 1, 256, 1, 8, 128, 150, torch.bfloat16),     # bf16 MFMA kernel
])
def test_repeat_runs_are_bitwise_identical(kind, inp, H, L, r, B, T, dtype):
    """Race screen for the LDS hand-offs behind raw s_barrier: forward results must not change between
    launches (no atomics on the forward path), and gradients must agree to rounding (atomic flushes)."""
    torch.manual_seed(3)
    m = build_module(dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=3, tt_rank=r), dev())
    m = m.to(dtype)
    x = torch.rand(B, T, inp, device=dev()).to(dtype)
    with torch.no_grad():
        ref = m(x)[0].clone()
        for rep in range(4):
            got = m(x)[0]
            if not torch.equal(got, ref):      # say where: a race shows as a few (b, t) rows, not as noise everywhere
                bad = (got != ref).nonzero()
                raise AssertionError("launch %d differs from the first in %d elements: b %s, t %d..%d, max |diff| %.3g" % (
                    rep + 1, len(bad), sorted(set(bad[:, 0].tolist()))[:8], int(bad[:, 1].min()), int(bad[:, 1].max()),
                    float((got - ref).abs().max())))
    grads = []
    for _ in range(2):
        m.zero_grad()
        out = m(x)[0]
        out.float().square().mean().backward()
        grads.append([p.grad.float().clone() for p in m.parameters()])
    for a, b in zip(*grads):
        assert _maxabs(a, b) <= 2e-3 * max(float(b.abs().max()), 1e-6)


@pytest.mark.parametrize("kind,inp,H,r,naive,B,T", [("ttlstm", 40, 512, 8, True, 300, 40), ("ttgru", 40, 512, 16, False, 301, 30),
                                                     ("ttlstm", 1, 256, 8, True, 64, 300), ("ttgru", 28, 256, 8, True, 70, 60)])
def test_round5_forward_kernels_repeat_bitwise(kind, inp, H, r, naive, B, T):
    """Race screen for the forward kernels of round 5 behind raw s_barrier / explicit s_waitcnt: the paired tier kernel (one and two
    column tiles; its gate inputs arrive through loads the compiler's wait insertion does not see) and the one-gate-per-wave kernel of
    the naive sets — twenty launches, every one bit for bit the first."""
    torch.manual_seed(4)
    m = build_module(dict(kind=kind, input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=r, is_naive=naive), dev())
    x = torch.rand(B, T, inp, device=dev())
    with torch.no_grad():
        ref = m(x)
        ref_out, ref_h = ref[0].clone(), (ref[1][0] if kind == "ttlstm" else ref[1]).clone()
        for rep in range(20):
            got = m(x)
            assert torch.equal(got[0], ref_out), rep
            assert torch.equal(got[1][0] if kind == "ttlstm" else got[1], ref_h), rep


@pytest.mark.parametrize("case,route", [("small", "default"), ("small", "nogemm"), ("mid", "nogemm"), ("mid", "default"),
                                        ("cfg4", "default"), ("cfg2", "default"), ("cfg3", "default")])
def test_forward_200_launches_bitwise_per_kernel(case, route):
    """200 launches of the r = 16 two-layer model on the route that runs k_ttlinear_fwd_f10 +
    k_lstm_fwd_f10<KS=2> (B*T < 2*in, or any size with the dense-GEMM switch off), of the full-size cfg4 (two samples per
    workgroup) and of the cfg2 / cfg3 kernels, layer by layer through the C ABI (tools/stress_determinism.py): the hoisted
    input projection and the outputs of every layer must reproduce the first launch bit for bit; a difference is
    reported with the kernel (K-in: the workspace differs; K-rec: only `out` does) and the first (b, t, unit)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "stress_determinism", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                           "stress_determinism.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    recs = tool.run([case], [route], 200)
    assert recs[0]["bad_launches"] == 0, recs[0]


@pytest.mark.parametrize("kind,inp,H,L,d,r,B,T,dtype,route", [
    ("ttlstm", 1, 256, 1, 3, 8, 9, 70, torch.float32, {}),                       # cfg2 kernels, in=1 path
    ("ttgru", 1, 256, 1, 3, 8, 7, 33, torch.bfloat16, {}),                       # cfg3 kernels
    ("ttgru", 1, 256, 1, 3, 8, 7, 33, torch.float32, {}),
    ("ttlstm", 40, 256, 2, 3, 16, 80, 40, torch.float32, {}),                    # dense-GEMM K-in, KS=2 K-rec
    ("ttlstm", 40, 256, 2, 3, 16, 80, 40, torch.float32, {"TTRNN_NO_GEMM": "1"}),   # fused-core K-in (round-1 suspect route)
    ("ttlstm", 40, 256, 2, 3, 16, 5, 6, torch.float32, {}),                      # B*T < 2*in
    ("ttlstm", 40, 256, 3, 3, 16, 300, 12, torch.float32, {}),                   # two samples per workgroup (B > #CUs)
    ("ttlstm", 1, 128, 1, 2, 4, 6, 50, torch.float32, {}),                       # cfg1 kernels
    ("ttlstm", 1024, 1024, 1, 4, 32, 3, 5, torch.float32, {}),                   # cfg5 kernels (pair)
    ("ttlstm", 28, 96, 2, 2, 3, 5, 9, torch.float32, {}),                        # shapes without a specialised kernel:
    ("ttgru", 28, 96, 2, 3, 5, 5, 9, torch.float32, {}),                         # runtime-shape MFMA kernels (ttrnn_g2.hip)
    ("ttlstm", 40, 512, 2, 3, 4, 32, 70, torch.float32, {}),                     # ... with the dense-gradient backward
    ("ttgru", 1, 384, 1, 3, 5, 40, 40, torch.float32, {}),
    ("ttlstm", 28, 96, 2, 2, 3, 5, 9, torch.float32, {"TTRNN_NO_G2": "1"}),      # any-shape VALU kernels
])
def test_poisoned_allocations_do_not_change_results(kind, inp, H, L, d, r, B, T, dtype, route):
    """Every buffer the host side allocates without initialising (outputs, workspaces, packed cores, reserves, gradient
    buffers) is filled with random bytes — NaN / Inf patterns included — before each launch
    (ttrnn_hip.functional.POISON_ALLOCATIONS).  A kernel that reads memory nobody wrote, or leaves part of an output
    unwritten, shows up as a changed or non-finite result here on EVERY box, instead of only on boxes whose fresh
    allocations are not zero.  Forward: bitwise equal to the clean launch (no atomics); gradients: equal to rounding."""
    from ttrnn_hip import functional as F
    torch.manual_seed(17)
    m = build_module(dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=d, tt_rank=r), dev()).to(dtype)
    x = torch.rand(B, T, inp, device=dev()).to(dtype)
    w = torch.randn(B, T, H, device=dev())

    def run():
        m.zero_grad()
        xg = x.clone().requires_grad_(True)
        res = m(xg)
        out = res[0]
        hT = res[1][0] if kind == "ttlstm" else res[1]
        ((out.float() * w).sum() + hT.float().sum()).backward()
        with torch.no_grad():
            inf = m(x)[0]
        return out.detach().clone(), inf.clone(), xg.grad.float().clone(), [p.grad.float().clone() for p in m.parameters()]

    try:
        OPT.update(route)
        clean = run()
        F.POISON_ALLOCATIONS = True
        for _ in range(3):
            got = run()
            assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1]), "forward changed under poisoned buffers"
            assert torch.isfinite(got[2]).all()
            assert _maxabs(got[2], clean[2]) <= 1e-4 * max(float(clean[2].abs().max()), 1e-6)
            for (name, _), a, b in zip(m.named_parameters(), got[3], clean[3]):
                assert torch.isfinite(a).all(), name
                # atomic flush order differs from launch to launch; bf16 gradients round to 2^-8 relative on top
                gtol = 2e-3 if dtype == torch.float32 else 1.2e-2
                assert _maxabs(a, b) <= gtol * max(float(b.abs().max()), 1e-6), name
    finally:
        F.POISON_ALLOCATIONS = False
        for k in route:
            OPT.pop(k)


# ---- (3b) runtime-shape two-stage MFMA kernels (csrc/ttrnn_g2.hip) ------------------------------------------------------------
G2_GRID = [
    # kind, in, H, L, d, r, B, T, new_core — the (hidden_size, ncores, ttrank, extra core) combinations the reference's
    # experiment flags produce (pmnist_test.py:47-56, params_model.py), none of which has a shape-specialised kernel ...
    ("ttlstm", 28, 128, 1, 2, 3, 4, 11, None),
    ("ttgru", 28, 64, 2, 2, 3, 9, 11, None),
    ("ttlstm", 40, 512, 1, 3, 4, 3, 8, None),
    ("ttlstm", 40, 768, 1, 4, 6, 3, 6, None),
    ("ttgru", 40, 768, 1, 3, 2, 3, 6, None),
    ("ttlstm", 1, 1024, 1, 3, 8, 3, 5, None),
    ("ttlstm", 1, 256, 1, 2, 8, 4, 12, None),
    ("ttlstm", 28, 64, 1, 2, 3, 5, 7, "first"),
    ("ttgru", 28, 64, 1, 2, 3, 5, 7, "last"),
    ("ttlstm", 40, 256, 1, 4, 5, 5, 7, None),
    ("ttlstm", 1, 256, 1, 4, 2, 70, 33, None),
    # ... with enough rows for the dense-gradient backward of every matrix (B*T >= 4*in)
    ("ttlstm", 28, 128, 1, 2, 3, 32, 20, None),
    ("ttgru", 28, 128, 2, 2, 3, 32, 20, None),
    ("ttlstm", 40, 512, 2, 3, 4, 32, 70, None),
    ("ttlstm", 1, 512, 1, 3, 8, 40, 60, None),
    ("ttgru", 1, 384, 1, 3, 5, 40, 40, None),
    ("ttlstm", 10, 96, 1, 2, 5, 30, 20, None),
    # ... and the benchmark shapes with the specialised kernels switched off (force_g2)
    ("ttlstm", 1, 256, 1, 3, 8, 5, 20, None),
    ("ttgru", 1, 256, 1, 3, 8, 5, 20, None),
    ("ttlstm", 40, 256, 2, 3, 16, 6, 9, None),
    ("ttlstm", 1, 128, 1, 2, 4, 7, 30, None),
    ("ttlstm", 40, 256, 3, 3, 16, 300, 8, None),        # B > #CUs: four waves per workgroup, several samples per CU
    # ... shapes whose forward fits the tier's LDS budget and whose reverse-time kernel does not: forward here, BPTT on the
    # any-shape kernels, both reading / writing the same reserve
    ("ttlstm", 12, 768, 1, 2, 16, 3, 5, None),
    ("ttgru", 12, 1024, 1, 2, 16, 2, 4, None),
    # ... extra-core shapes of the pMNIST flag space (pmnist_test.py --extra_core last): the first one's reverse-time kernel fits
    # LDS with NEITHER split point (dC1 image 131 / 139 KB) — forward on the tier, BPTT on the any-shape kernels
    ("ttlstm", 1, 512, 1, 2, 16, 3, 9, "last"),
    ("ttgru", 1, 512, 1, 2, 16, 3, 9, "last"),
    ("ttlstm", 1, 512, 1, 3, 16, 3, 7, "last"),
]


@pytest.mark.parametrize("kind,inp,H,L,d,r,B,T,new_core", G2_GRID)
def test_runtime_shape_kernels_vs_oracle(kind, inp, H, L, d, r, B, T, new_core):
    """Forward and every gradient of the runtime-shape MFMA route against the oracle (1e-5 abs / 1e-4 of the tensor max),
    and the route check itself: with `no_g2` the same module takes the any-shape VALU kernels and must agree."""
    import ttrnn_hip
    torch.manual_seed(7)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=d, tt_rank=r, new_core=new_core)
    m = build_module(meta, dev())
    lstm = kind == "ttlstm"
    x = torch.randn(B, T, inp)
    w = torch.randn(B, T, H)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, L, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    if lstm:
        ro, (rh, rc) = O.lstm_forward(layers, xr)
        ((ro * w).sum() + rc.sum() + rh.sum()).backward()
    else:
        ro, rh = O.gru_forward(layers, xr)
        ((ro * w).sum() + rh.sum()).backward()
    with ttrnn_hip.option("force_g2", 1):
        xg = x.to(dev()).requires_grad_(True)
        res = m(xg)
        out = res[0]
        if lstm:
            ((out * w.to(dev())).sum() + res[1][1].sum() + res[1][0].sum()).backward()
        else:
            ((out * w.to(dev())).sum() + res[1].sum()).backward()
    assert _maxabs(out.detach(), ro.detach()) <= 1e-5
    assert _maxabs(res[1][0] if lstm else res[1], rh.detach()) <= 1e-5
    assert _maxabs(xg.grad, xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-6)
    for name, p in m.named_parameters():
        ref = leaves[name].grad
        assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
    with ttrnn_hip.option("no_g2", 1), ttrnn_hip.option("force_generic", 1), torch.no_grad():
        other = m(x.to(dev()))[0]
    assert _maxabs(other, out.detach()) <= 5e-6
    assert not torch.equal(other, out.detach()) or B * T * H < 64      # two different routes really ran


@pytest.mark.parametrize("kind,inp,H,L,d,r,B,T", [("ttlstm", 40, 256, 2, 3, 4, 6, 9), ("ttgru", 28, 128, 1, 2, 5, 7, 11),
                                                   ("ttlstm", 1, 256, 1, 3, 8, 5, 12), ("ttgru", 1, 256, 1, 3, 8, 4, 10),
                                                   ("ttlstm", 40, 512, 1, 3, 4, 3, 7),
                                                   # joint rank 64: the reverse-time kernel fits LDS with four waves only
                                                   ("ttlstm", 1, 512, 1, 2, 16, 3, 6), ("ttlstm", 1, 512, 1, 4, 16, 2, 5),
                                                   # ... and d = 3: the forward's operand image fits with its I_t = 8 real rows only
                                                   ("ttlstm", 1, 512, 1, 3, 16, 2, 5), ("ttgru", 1, 512, 1, 3, 16, 3, 4)])
def test_naive_per_gate_sets_run_on_the_fused_path(kind, inp, H, L, d, r, B, T):
    """is_naive=True (TTLinearSet, tt_linearset.py:5-38; LSTM without any bias, GRU with biases: tt_lstm.py:17-21,
    gru.py:150-153) is presented to the library as ONE TT-matrix with a gate-selector core: no per-step Python loop, the
    persistent MFMA kernels run, outputs and every per-gate gradient match the oracle's per-gate evaluation."""
    from ttrnn_hip import functional as F
    torch.manual_seed(21)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=d, tt_rank=r, is_naive=True)
    m = build_module(meta, dev())
    assert not m._needs_stepping()
    lstm = kind == "ttlstm"
    # (round 5: the naive sets of H = 256, r = 8 have a fused-core forward kernel of their own, one gate per wave: ttrnn_fast_f10n.hip)
    assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == ("fused_core" if (H == 256 and d == 3 and r == 8) else "runtime_mfma")
    # (round 6: ... and a reverse-time kernel on the per-gate fused cores, k_rnn_bwd_f10n; option naive_bwd_on_tier = the tier's kernel)
    first_tier = H == 256 and d == 3 and r == 8
    assert F.rnn_backward_route(m._all_layers[0]._layer_spec(), B, T) == ("fused_core" if first_tier else "runtime_mfma")
    import ttrnn_hip
    with ttrnn_hip.option("naive_bwd_on_tier", 1):
        assert F.rnn_backward_route(m._all_layers[0]._layer_spec(), B, T) == "runtime_mfma"
    x = torch.randn(B, T, inp)
    w = torch.randn(B, T, H)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, L, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    ro = (O.lstm_forward(layers, xr) if lstm else O.gru_forward(layers, xr))[0]
    (ro * w).sum().backward()
    xg = x.to(dev()).requires_grad_(True)
    out = m(xg)[0]
    (out * w.to(dev())).sum().backward()
    assert _maxabs(out.detach(), ro.detach()) <= 1e-5
    assert _maxabs(xg.grad, xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-6)
    seen = 0
    for name, p in m.named_parameters():
        key = name.replace(".gate", ".gates.")        # gate{i} (attribute) and gates.{i} (ModuleList) are the same Parameters
        if key not in leaves:
            continue
        seen += 1
        ref = leaves[key].grad
        assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
    assert seen >= 2 * L * d * (4 if lstm else 3)
    # the block-diagonal promise (ttrnn_rnn_desc::hid_blocks) only skips exact zeros: same outputs as the dense evaluation
    spec = m._all_layers[0]._layer_spec()
    assert spec.hid_blocks == (4 if lstm else 3)
    for c in m._all_layers:
        c._layer_spec().hid_blocks = 1          # the cached spec object: the next launches describe a dense joint matrix
    with torch.no_grad():
        dense = m(x.to(dev()))[0]
    assert _maxabs(dense, out.detach()) <= 2e-6
    # ... and the promise is checked on the device: a non-zero entry outside a gate's rank block is counted
    import ttrnn_hip
    cell = m._all_layers[0]
    spec.hid_blocks = 4 if lstm else 3
    cin, bin_, chid, bhid = cell._operands()
    ttrnn_hip.device_status(reset=True)
    with torch.no_grad():
        F.tt_rnn_layer(spec, x.to(dev()), None, None, cin, bin_, chid, bhid)
    assert ttrnn_hip.device_status(reset=True)["block_violations"] == 0
    bad = [c.detach().clone() for c in chid]
    zeros = (bad[1] == 0).nonzero()
    assert len(zeros) > 0                      # the block-diagonal core does have structural zeros
    bad[1][tuple(zeros[0])] = 0.25
    with torch.no_grad():
        promised = F.tt_rnn_layer(spec, x.to(dev()), None, None, cin, bin_, bad, bhid)[0]
    violations = ttrnn_hip.device_status(reset=True)["block_violations"]
    spec.hid_blocks = 1
    with torch.no_grad():
        as_dense = F.tt_rnn_layer(spec, x.to(dev()), None, None, cin, bin_, bad, bhid)[0]
    spec.hid_blocks = 4 if lstm else 3
    # either the shape did not let the kernels use the promise (block boundaries off the tile grid: evaluated as a dense
    # matrix, nothing ignored) or the false promise was noticed
    assert violations >= 1 or _maxabs(promised, as_dense) <= 2e-6, (violations, _maxabs(promised, as_dense))
    print(kind, H, d, r, "false block promise: violations counted", violations, "| promised - dense|", _maxabs(promised, as_dense))


@pytest.mark.parametrize("kind,inp,H,d,r,naive,B,T", [("ttlstm", 40, 128, 4, 4, False, 40, 16), ("ttgru", 16, 64, 3, 3, True, 32, 10),
                                                       ("ttlstm", 12, 128, 3, 4, True, 40, 16), ("ttgru", 40, 256, 4, 8, False, 64, 20)])
def test_dense_gradient_pull_back_of_four_core_matrices(kind, inp, H, d, r, naive, B, T):
    """ttrnn_fast_proj.hip, d = 4 (round 5): the dense weight gradient dW = x^T dy of a four-core TT-matrix — a d = 4 layer, or the joint
    matrix of a naive per-gate set of three-core TTLinears (tt_linearset.py:5-38) — is pulled back onto the cores as (G0, G1, G2 G3)
    through the three-core launches + one more, instead of the any-shape chain kernel on the identity rows (option no_proj4: as before).
    Every gradient against the oracle, the two routes against each other, and bitwise repeatable."""
    import ttrnn_hip
    torch.manual_seed(17)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=1, n_cores=d, tt_rank=r, is_naive=naive)
    m = build_module(meta, dev())
    lstm = kind == "ttlstm"
    x = torch.randn(B, T, inp)
    w = torch.randn(B, T, H)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True)
    ro = (O.lstm_forward(layers, x) if lstm else O.gru_forward(layers, x))[0]
    (ro * w).sum().backward()

    def grads():
        m.zero_grad()
        out = m(x.to(dev()))[0]
        (out * w.to(dev())).sum().backward()
        return {n: p.grad.clone() for n, p in m.named_parameters()}

    new = grads()
    again = grads()
    with ttrnn_hip.option("no_proj4", 1):
        old = grads()
    seen = 0
    for name, g in new.items():
        assert torch.equal(g, again[name]), name
        key = name.replace(".gate", ".gates.")
        if key in leaves:
            seen += 1
            ref = leaves[key].grad
            assert _maxabs(g, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
        assert _maxabs(g, old[name]) <= 2e-5 * max(float(old[name].abs().max()), 1e-6), name
    assert seen >= 2 * d
    assert any(not torch.equal(new[n], old[n]) for n in new)      # two different routes really ran


@pytest.mark.parametrize("kind,r,naive", [("ttlstm", 8, True), ("ttgru", 8, True), ("ttlstm", 16, False), ("ttgru", 16, False)])
def test_paired_kernel_at_benchmark_size_is_bit_identical_to_single(kind, r, naive):
    """benchmarking.py's defaults with --naive_tt / --ttrank 16 (in = 256, H = 512, 160 steps) at a batch of 513 — more samples than
    CUs, odd: the DEFAULT route pairs them (the last workgroup holds one sample) — against the one-sample-per-workgroup kernel
    (option g2_pair_never): outputs, final states and the training reserve (compared through the gradients of a masked loss) bit for bit."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    torch.manual_seed(3)
    meta = dict(kind=kind, input_size=256, hidden_size=512, num_layers=1, n_cores=3, tt_rank=r, is_naive=naive)
    m = build_module(meta, dev())
    B, T = 513, 160
    lstm = kind == "ttlstm"
    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_samples_per_workgroup(spec, B, T) == 2
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, T, 256, generator=g).to(dev())
    w = torch.zeros(B, T, 512)
    w[::37, ::13] = torch.randn(B, T, 512, generator=g)[::37, ::13]
    w[B - 1, T - 1] = 1.0
    w = w.to(dev())

    def run():
        m.zero_grad()
        res = m(x)
        (res[0] * w).sum().backward()
        return res[0].detach(), (res[1][0] if lstm else res[1]).detach(), {n: p.grad.clone() for n, p in m.named_parameters()}

    out2, h2, g2 = run()
    with ttrnn_hip.option("g2_pair_never", 1):
        assert F.rnn_samples_per_workgroup(spec, B, T) == 1
        out1, h1, g1 = run()
    assert torch.isfinite(out2).all()
    assert torch.equal(out1, out2) and torch.equal(h1, h2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.parametrize("kind,inp,H,d,r,naive", [("ttlstm", 40, 512, 3, 4, False), ("ttgru", 28, 128, 2, 5, False),
                                                   ("ttlstm", 40, 256, 3, 4, True), ("ttgru", 12, 768, 4, 6, False)])
def test_tier_input_matrix_from_merged_cores(kind, inp, H, d, r, naive):
    """K-in of the runtime tier (input_size != 1) is a dense GEMM whose matrix is built from the TT cores at every launch, by the any-shape
    chain kernel on the identity rows; option g2_dense_from_merged builds it from the MERGED cores instead (k_g2_merge + k_g2_dense: an A/B kept
    in the library, no measurable difference in the harness).  Same matrix up to the order of the sums: outputs within 2e-6 of each
    other, both within 1e-5 of the oracle."""
    import ttrnn_hip
    torch.manual_seed(9)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=1, n_cores=d, tt_rank=r, is_naive=naive)
    m = build_module(meta, dev())
    B, T = 5, 7
    x = torch.randn(B, T, inp)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, _ = O.layers_from_state_dict(sd, 1, requires_grad=False)
    with torch.no_grad():
        ro = (O.lstm_forward(layers, x) if kind == "ttlstm" else O.gru_forward(layers, x))[0]
        with ttrnn_hip.option("force_g2", 1):
            new = m(x.to(dev()))[0]
            with ttrnn_hip.option("g2_dense_from_merged", 1):
                old = m(x.to(dev()))[0]
    assert _maxabs(new, ro) <= 1e-5 and _maxabs(old, ro) <= 1e-5
    assert _maxabs(new, old) <= 2e-6
    assert not torch.equal(new, old)


@pytest.mark.parametrize("inp,B,T,state,need_out", [(1, 5, 40, "none", True), (1, 3, 784, "big", True), (40, 6, 9, "small", True),
                                                     (28, 4, 12, "big", False), (1, 70, 33, "small", True)])
def test_naive_lstm_fused_core_kernel(inp, B, T, state, need_out):
    """k_rnn_fwd_f10n (ttrnn_fast_f10n.hip): the naive per-gate TT-LSTM (tt_linearset.py:5-38, tt_lstm.py:17-21; pmnist_test.py
    --naive_tt) of H = 256, d = 3, r = 8 on a fused-core kernel with ONE GATE PER WAVE, behind the runtime tier's K-in, instead of the
    tier's own recurrent kernel (option naive_fwd_on_tier).  Outputs, final states and every per-gate gradient (the tier's reverse kernel reads the
    reserve this kernel writes) against the oracle; the two forward kernels against each other; a false block promise is counted."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    torch.manual_seed(23)
    meta = dict(kind="ttlstm", input_size=inp, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8, is_naive=True)
    m = build_module(meta, dev())
    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_route(spec, B, T) == "fused_core"
    with ttrnn_hip.option("naive_fwd_on_tier", 1):
        assert F.rnn_route(spec, B, T) == "runtime_mfma"
    x = torch.randn(B, T, inp)
    w = torch.randn(B, T, 256)
    h0 = c0 = None
    if state != "none":
        h0 = torch.randn(B, 256) * (7.0 if state == "big" else 0.3)
        c0 = torch.randn(B, 256)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    ro, (rh, rc) = O.lstm_forward(layers, xr, None if h0 is None else (h0, c0))
    ((ro * w).sum() + rc.sum() + rh.sum()).backward()
    init = None if h0 is None else (h0.to(dev()), c0.to(dev()))
    xg = x.to(dev()).requires_grad_(True)
    out, (hT, cT) = m(xg, init)
    ((out * w.to(dev())).sum() + cT.sum() + hT.sum()).backward()
    tol = 1e-5 * max(1.0, float(ro.detach().abs().max()))
    assert _maxabs(out.detach(), ro.detach()) <= tol
    assert _maxabs(hT.detach(), rh.detach()) <= tol and _maxabs(cT.detach(), rc.detach()) <= 1e-5 * max(1.0, float(rc.detach().abs().max()))
    assert _maxabs(xg.grad, xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-6)
    seen = 0
    for name, p in m.named_parameters():
        key = name.replace(".gate", ".gates.")
        if key in leaves:
            seen += 1
            ref = leaves[key].grad
            assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
    assert seen >= 24
    with torch.no_grad():
        fused = m(x.to(dev()), init, need_outputs=need_out) if not need_out else m(x.to(dev()), init)
        with ttrnn_hip.option("naive_fwd_on_tier", 1):
            tier = m(x.to(dev()), init, need_outputs=need_out) if not need_out else m(x.to(dev()), init)
    if need_out:
        assert torch.equal(fused[0], out.detach())                      # eval and training forwards: the same kernel, the same bits
        assert _maxabs(fused[0], tier[0]) <= 2e-6 * max(1.0, float(ro.detach().abs().max()))
        assert not torch.equal(fused[0], tier[0])
    assert _maxabs(fused[1][0], tier[1][0]) <= 2e-6 * max(1.0, float(rh.detach().abs().max()))
    assert _maxabs(fused[1][1], tier[1][1]) <= 2e-6 * max(1.0, float(rc.detach().abs().max()))
    # a false block promise (a non-zero entry outside a gate's rank block) is counted by this route too
    cell = m._all_layers[0]
    cin, bin_, chid, bhid = cell._operands()
    bad = [cc.detach().clone() for cc in chid]
    zeros = (bad[2] == 0).nonzero()
    bad[2][tuple(zeros[0])] = 0.25
    ttrnn_hip.device_status(reset=True)
    with torch.no_grad():
        F.tt_rnn_layer(spec, x.to(dev()), None, None, cin, bin_, chid, bhid)
    assert ttrnn_hip.device_status(reset=True)["block_violations"] == 0
    with torch.no_grad():
        F.tt_rnn_layer(spec, x.to(dev()), None, None, cin, bin_, bad, bhid)
    assert ttrnn_hip.device_status(reset=True)["block_violations"] >= 1


@pytest.mark.parametrize("inp,B,T,state", [(1, 5, 40, "none"), (1, 3, 300, "big"), (40, 6, 9, "small"), (28, 70, 12, "big")])
def test_naive_gru_fused_core_kernel(inp, B, T, state):
    """The same kernel for the naive per-gate TT-GRU (three gate waves; gru.py:33-44,150-153: per-gate biases, the n gate's hidden bias
    inside r * (...)), H = 256, d = 3, r = 8: outputs, final state, every per-gate gradient against the oracle; against the tier's
    kernel (option naive_fwd_on_tier); a decaying huge h_0 (the state's exponent is re-derived every step while it is positive)."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    torch.manual_seed(29)
    meta = dict(kind="ttgru", input_size=inp, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8, is_naive=True)
    m = build_module(meta, dev())
    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_route(spec, B, T) == "fused_core"
    with ttrnn_hip.option("naive_fwd_on_tier", 1):
        assert F.rnn_route(spec, B, T) == "runtime_mfma"
    x = torch.randn(B, T, inp)
    w = torch.randn(B, T, 256)
    h0 = None if state == "none" else torch.randn(B, 256) * (9.0 if state == "big" else 0.3)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    ro, rh = O.gru_forward(layers, xr, h0)
    ((ro * w).sum() + rh.sum()).backward()
    init = None if h0 is None else h0.to(dev())
    xg = x.to(dev()).requires_grad_(True)
    out, hT = m(xg, init)
    ((out * w.to(dev())).sum() + hT.sum()).backward()
    tol = 1e-5 * max(1.0, float(ro.detach().abs().max()))
    assert _maxabs(out.detach(), ro.detach()) <= tol and _maxabs(hT.detach(), rh.detach()) <= tol
    assert _maxabs(xg.grad, xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-6)
    seen = 0
    for name, p in m.named_parameters():
        key = name.replace(".gate", ".gates.")
        if key in leaves:
            seen += 1
            ref = leaves[key].grad
            assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
    assert seen >= 18
    with torch.no_grad():
        fused = m(x.to(dev()), init)
        with ttrnn_hip.option("naive_fwd_on_tier", 1):
            tier = m(x.to(dev()), init)
    assert torch.equal(fused[0], out.detach())
    assert _maxabs(fused[0], tier[0]) <= 2e-6 * max(1.0, float(ro.detach().abs().max()))
    assert not torch.equal(fused[0], tier[0])


@pytest.mark.parametrize("kind,inp,H,d,r,B,T", [("ttlstm", 40, 768, 2, 2, 5, 9), ("ttgru", 1, 512, 2, 8, 4, 12), ("ttlstm", 40, 768, 4, 8, 300, 6),
                                                 ("ttgru", 28, 1024, 2, 4, 3, 5), ("ttlstm", 1, 384, 4, 4, 70, 8)])
def test_tier_column_tiles_inside_a_unit(kind, inp, H, d, r, B, T):
    """G2Mat::cin (round 5): with more than one column tile in stage 2 (I_t > 16: every d = 2 / d = 4 shape from H = 384 up, the speaker
    encoder's own H = 768, d = 2, r = 2) a forward unit is a ROW tile with its column tiles inside — one fragment, N2T accumulator pairs —
    where that makes a streamed head resident; option g2_no_cin = a unit per (row tile, column tile), as before.  The same products (the partial sums of a
    unit's k range may be split over the waves differently): against each other and against the oracle."""
    import ttrnn_hip
    torch.manual_seed(37)
    m = build_module(dict(kind=kind, input_size=inp, hidden_size=H, num_layers=1, n_cores=d, tt_rank=r), dev())
    lstm = kind == "ttlstm"
    x = torch.randn(B, T, inp)
    h0 = torch.randn(B, H) * 0.4
    c0 = torch.randn(B, H)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, _ = O.layers_from_state_dict(sd, 1, requires_grad=False)
    with torch.no_grad():
        ro = (O.lstm_forward(layers, x, (h0, c0)) if lstm else O.gru_forward(layers, x, h0))
        init = (h0.to(dev()), c0.to(dev())) if lstm else h0.to(dev())
        new = m(x.to(dev()), init)
        with ttrnn_hip.option("g2_no_cin", 1):
            old = m(x.to(dev()), init)
    if (kind, inp, H, d, r) == ("ttlstm", 40, 768, 2, 2):
        # the speaker encoder's own shape left the tier in round 6 (k_lstm_fwd_w2, ttrnn_fast_w2.hip): the first-tier route is what
        # runs by default — checked against the oracle here — and option enc_fwd_on_tier brings the tier back for the comparison below
        from ttrnn_hip import functional as F
        assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == "fused_core"
        assert _maxabs(new[0], ro[0]) <= 1e-5
        with torch.no_grad(), ttrnn_hip.option("enc_fwd_on_tier", 1):
            assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == "runtime_mfma"
            new = m(x.to(dev()), init)
            with ttrnn_hip.option("g2_no_cin", 1):
                old = m(x.to(dev()), init)
    assert _maxabs(new[0], ro[0]) <= 1e-5 and _maxabs(old[0], ro[0]) <= 1e-5
    # (the two plans may split a unit's k range over the waves differently: same products, another order of the partial sums)
    assert _maxabs(new[0], old[0]) <= 2e-6
    assert _maxabs(new[1][0] if lstm else new[1], old[1][0] if lstm else old[1]) <= 2e-6


PAIR_CASES = [
    # kind, in, H, d, r, naive, B, T, big_h0 — heads the tier streams from L2 every step (no plan keeps them in registers)
    ("ttlstm", 40, 512, 3, 8, True, 5, 6, False),       # benchmarking.py --naive_tt; odd batch: the last workgroup holds one sample
    ("ttlstm", 1, 512, 3, 8, True, 4, 9, True),
    ("ttgru", 28, 512, 3, 8, True, 6, 5, True),
    ("ttgru", 40, 384, 3, 16, True, 4, 6, False),       # joint rank 48
    ("ttlstm", 1, 384, 3, 4, True, 3, 7, False),
    # I_t = 16: the pair fills TWO column tiles of stage 2 (benchmarking.py --ttrank 16)
    ("ttlstm", 40, 512, 3, 16, False, 5, 6, True),
    ("ttgru", 1, 512, 3, 16, False, 4, 8, False),
    ("ttgru", 40, 384, 3, 32, False, 3, 5, False),
]


@pytest.mark.parametrize("kind,inp,H,d,r,naive,B,T,big_h0", PAIR_CASES)
def test_runtime_tier_two_samples_per_workgroup(kind, inp, H, d, r, naive, B, T, big_h0):
    """k_g2_fwd_p: where the runtime tier streams the merged head from L2 every step and the batch exceeds the CU count, two samples
    share a workgroup — and every streamed block (`--naive_tt` at H = 512: 512 KB per step).  option g2_pair_always takes small batches there:
    outputs, final states and the training reserve (through the gradients the reverse kernel derives from it) against the oracle,
    and BIT-identical to the one-sample-per-workgroup kernel (same products, same order, per sample)."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    torch.manual_seed(31)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=1, n_cores=d, tt_rank=r, is_naive=naive)
    m = build_module(meta, dev())
    lstm = kind == "ttlstm"
    spec = m._all_layers[0]._layer_spec()
    x = torch.randn(B, T, inp)
    w = torch.randn(B, T, H)
    h0 = torch.randn(B, H) * (5.0 if big_h0 else 0.3)
    c0 = torch.randn(B, H)
    from oracle import ttrnn_oracle as O
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    if lstm:
        ro, (rh, rc) = O.lstm_forward(layers, xr, (h0, c0))
        ((ro * w).sum() + rc.sum() + rh.sum()).backward()
    else:
        ro, rh = O.gru_forward(layers, xr, h0)
        ((ro * w).sum() + rh.sum()).backward()
    init = (h0.to(dev()), c0.to(dev())) if lstm else h0.to(dev())

    def run(train):
        xg = x.to(dev()).requires_grad_(train)
        with torch.set_grad_enabled(train):
            res = m(xg, init)
            if train:
                m.zero_grad()
                ((res[0] * w.to(dev())).sum() + (res[1][1].sum() + res[1][0].sum() if lstm else res[1].sum())).backward()
        return res, xg

    assert F.rnn_route(spec, B, T) == "runtime_mfma"
    assert F.rnn_samples_per_workgroup(spec, B, T) == 1
    with ttrnn_hip.option("g2_pair_always", 1):
        assert F.rnn_samples_per_workgroup(spec, B, T) == 2
        assert F.rnn_samples_per_workgroup(spec, 1, T) == 1
        res, xg = run(True)
        grads = {n: p.grad.clone() for n, p in m.named_parameters()}
        with ttrnn_hip.option("g2_pair_never", 1):
            assert F.rnn_samples_per_workgroup(spec, B, T) == 1
    out = res[0].detach()
    assert _maxabs(out, ro.detach()) <= 1e-5 * max(1.0, float(ro.detach().abs().max()))
    assert _maxabs((res[1][0] if lstm else res[1]).detach(), rh.detach()) <= 1e-5 * max(1.0, float(rh.detach().abs().max()))
    if lstm:
        assert _maxabs(res[1][1].detach(), rc.detach()) <= 1e-5 * max(1.0, float(rc.detach().abs().max()))
    assert _maxabs(xg.grad, xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-6)
    for name, g in grads.items():
        key = name.replace(".gate", ".gates.")
        if key in leaves:
            ref = leaves[key].grad
            assert _maxabs(g, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
    single, _ = run(False)
    assert torch.equal(single[0], out)
    assert torch.equal(single[1][0] if lstm else single[1], (res[1][0] if lstm else res[1]).detach())
    # more samples than CUs: the default route pairs them
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert F.rnn_samples_per_workgroup(spec, cus + 1, T) == 2
    assert F.rnn_samples_per_workgroup(spec, cus, T) == 1


def test_runtime_shape_kernels_bf16_storage_and_states():
    """bf16 storage (fp32 state / accumulation) and non-zero initial states through the runtime-shape route."""
    import ttrnn_hip
    torch.manual_seed(12)
    meta = dict(kind="ttlstm", input_size=40, hidden_size=512, num_layers=2, n_cores=3, tt_rank=4)
    m = build_module(meta, dev())
    x = torch.randn(6, 14, 40)
    h0, c0 = torch.randn(6, 512) * 0.5, torch.randn(6, 512) * 0.5
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ro, rh, rc = _oracle_forward("ttlstm", sd, 2, x, (h0, c0))
    with torch.no_grad():
        out, (hT, cT) = m(x.to(dev()), (h0.to(dev()), c0.to(dev())))
    assert _maxabs(out, ro) <= 1e-5 and _maxabs(cT, rc) <= 1e-5 and _maxabs(hT, rh) <= 1e-5
    mb = build_module(dict(meta, kind="ttgru", num_layers=1), dev()).to(torch.bfloat16)
    sdb = {k: v.detach().cpu().float() for k, v in mb.state_dict().items()}
    xb = torch.rand(5, 30, 40).to(torch.bfloat16)
    rob, rhb, _ = _oracle_forward("ttgru", sdb, 1, xb.float())
    with torch.no_grad():
        ob, hb = mb(xb.to(dev()))
    assert ob.dtype == torch.bfloat16
    assert _maxabs(ob.float(), rob) <= 2e-2 and _maxabs(hb.float(), rhb) <= 2e-2


def test_dtype_and_device_mismatches_are_refused():
    """a bf16 input into an fp32 module used to reinterpret the fp32 bias as bf16; now it raises."""
    import ttrnn_hip
    m = build_module(dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), dev())
    with pytest.raises(ttrnn_hip.TtrnnError):
        m(torch.rand(2, 3, 1, device=dev()).to(torch.bfloat16))
    with pytest.raises(ttrnn_hip.TtrnnError):
        m(torch.rand(2, 3, 1))                                    # CPU tensor: no CPU path
    from t3nsor.layers import TTLinear
    with contextlib.redirect_stdout(io.StringIO()):
        lin = TTLinear(in_features=256, out_features=10, d=3, tt_rank=8).to(dev())
    with pytest.raises(ttrnn_hip.TtrnnError):
        lin(torch.rand(4, 256, device=dev()).to(torch.bfloat16))


def test_gru_four_wave_kernel_matches_eight_wave_kernel_and_oracle():
    """The bf16 TT-GRU shape (cfg3) on the four-wave kernel whose lanes hold r, z, n of their own units (three rotated
    MFMA tiles per pair of unit rows, ttrnn_fast_f10gq.hip; an A/B variant behind option f10gq_bf16 — it measured slower than
    the default) against the eight-wave kernel with its LDS gate vector and the fp32 oracle: forward with an initial state, input_size 1 and 40 (the scalar shortcut and the hoisted
    projection), and the gradients the forward's reserve feeds."""
    import ttrnn_hip
    torch.manual_seed(77)
    for inp, B, T in ((1, 9, 37), (40, 70, 11)):
        meta = dict(kind="ttgru", input_size=inp, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8)
        m = build_module(meta, dev()).to(torch.bfloat16)
        x = torch.randn(B, T, inp).to(torch.bfloat16)
        h0 = (torch.randn(B, 256) * 0.5).to(torch.bfloat16)
        w = torch.randn(B, T, 256, device=dev())
        res = {}
        for name, f10gq in (("four", 1), ("eight", 0)):
            m.zero_grad()
            with ttrnn_hip.option("f10gq_bf16", f10gq):
                xg = x.to(dev()).requires_grad_(True)
                out, hT = m(xg, h0.to(dev()))
                (out.float() * w).sum().backward()
            res[name] = (out.detach().float().cpu(), hT.detach().float().cpu(), xg.grad.float().cpu(),
                         {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters()})
        sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
        ref = _oracle_forward("ttgru", sd, 1, x.float(), h0.float())[0]
        assert _maxabs(res["four"][0], ref) <= 2e-2 and _maxabs(res["four"][0], res["eight"][0]) <= 1.6e-2   # one bf16 ulp of |h| <= 2
        assert _maxabs(res["four"][1], res["eight"][1]) <= 1.6e-2
        for n in res["four"][3]:
            a, bq = res["four"][3][n], res["eight"][3][n]
            assert torch.isfinite(a).all() and _maxabs(a, bq) <= 3e-2 * max(float(bq.abs().max()), 1e-6), n


_SKIP_OUT_CASES = {
    "fused_core_r16_b300": (dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=3, n_cores=3, tt_rank=16), 300, 7, "f32"),
    "fused_core_r16_b6_eight_waves": (dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=1, n_cores=3, tt_rank=16), 6, 9, "f32"),
    "fused_core_r8_in1": (dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), 6, 30, "f32"),
    "fused_core_gru_bf16": (dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), 5, 40, "bf16"),
    "fused_core_gru_fp32": (dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), 5, 40, "f32"),
    "fused_core_gru_fp32_in40": (dict(kind="ttgru", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=8), 70, 11, "f32"),
    "stagewise_h128_r4": (dict(kind="ttlstm", input_size=1, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4), 5, 20, "f32"),
    "runtime_mfma_lstm": (dict(kind="ttlstm", input_size=28, hidden_size=192, num_layers=1, n_cores=2, tt_rank=6), 4, 7, "f32"),
    "runtime_mfma_gru_2layers": (dict(kind="ttgru", input_size=28, hidden_size=128, num_layers=2, n_cores=3, tt_rank=4), 4, 7, "f32"),
    "merged_big_pair": (dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32), 3, 5, "f32"),
    "merged_big_pair_bf16": (dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32), 3, 5, "bf16"),
    "merged_big_single_b130": (dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32), 130, 2, "f32"),
}


@pytest.mark.parametrize("case", sorted(_SKIP_OUT_CASES))
def test_last_layer_outputs_can_be_skipped_in_inference(case):
    """need_outputs=False (speaker_encoder.py:80-86 consumes only the last hidden state, mnist_classifier.py:52-55 only the
    last step): under no_grad the last layer does not write `out` (ttrnn_rnn_out_optional: every route guards the store since
    round 3 — fused-core four- and eight-wave kernels, the bf16 GRU kernel, stage-wise, runtime-shape, merged-big pair and
    single-workgroup kernels, any-shape VALU kernels and both math modes); the final states must be bit-identical to the
    ordinary call, with and without prepared weights; autograd runs ignore the flag (the backward pass reads `out`)."""
    import ctypes
    import ttrnn_hip
    from ttrnn_hip import _lib
    torch.manual_seed(8)
    meta, B, T, storage = _SKIP_OUT_CASES[case]
    lstm = meta["kind"] == "ttlstm"
    m = build_module(meta, dev()).eval()
    x = torch.randn(B, T, meta["input_size"], device=dev())
    if storage == "bf16":
        m = m.to(torch.bfloat16)
        x = x.to(torch.bfloat16)
    desc = m._all_layers[-1]._layer_spec().desc(B, T, 0 if storage == "f32" else 1)
    assert _lib.load().ttrnn_rnn_out_optional(ctypes.byref(desc)) == 1
    states = (lambda r: r[1]) if lstm else (lambda r: (r[1],))
    settings = [dict()] + ([dict(fp32_math="exact")] if storage == "f32" else []) + [dict(force_generic=1)]
    for setting in settings:
        ctx = ttrnn_hip.fp32_math(setting["fp32_math"]) if "fp32_math" in setting else \
            (ttrnn_hip.option("force_generic", 1) if "force_generic" in setting else contextlib.nullcontext())
        with ctx, torch.no_grad():
            ref = m(x)
            res = m(x, need_outputs=False)
            assert res[0] is None and ref[0] is not None, setting
            for a, b_ in zip(states(res), states(ref)):
                assert torch.equal(a, b_), setting
            m.prepare_for_inference()
            res2 = m(x, need_outputs=False)
            assert res2[0] is None
            for a, b_ in zip(states(res2), states(ref)):
                assert torch.equal(a, b_), setting
            m.release_prepared()
    with torch.no_grad():
        ref = m(x)
    out3 = m(x, need_outputs=False)[0]               # recording: the backward pass needs the outputs
    assert out3 is not None and torch.equal(out3, ref[0])


def test_prepared_weights_inference_matches_and_tracks_updates():
    """prepare_for_inference(): repeated no-grad forwards reuse the packed cores and the weight-only part of the call
    (ttrnn_rnn_forward_phase: PREPARE once per input shape, RUN per call).  Results must be bit-identical to the ordinary
    call — on the headline shape, whose route separates the phases (one launch per forward), and on routes that do not —
    and an in-place parameter update must be noticed (version counters) instead of answering from stale fragments."""
    import ctypes
    import ttrnn_hip
    from ttrnn_hip import _lib
    torch.manual_seed(7)
    for meta, B, T, split in ((dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), 5, 40, 1),
                              # (fp32 GRU: fused-core route since round 5 — its scale header and fragments are weight-only work)
                              (dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), 5, 40, 1),
                              (dict(kind="ttgru", input_size=28, hidden_size=128, num_layers=1, n_cores=3, tt_rank=4), 5, 40, 0),
                              # (round 6: the reference's encoder layer — TT-LSTM with two and four cores, TT-GRU — header + fragments are weight-only work)
                              (dict(kind="ttlstm", input_size=40, hidden_size=768, num_layers=1, n_cores=2, tt_rank=2), 5, 12, 1),
                              (dict(kind="ttlstm", input_size=40, hidden_size=768, num_layers=1, n_cores=4, tt_rank=4), 4, 9, 1),
                              (dict(kind="ttgru", input_size=40, hidden_size=768, num_layers=1, n_cores=2, tt_rank=2), 5, 12, 1),
                              (dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=16), 6, 9, 0),
                              (dict(kind="ttlstm", input_size=28, hidden_size=192, num_layers=1, n_cores=2, tt_rank=6), 4, 7, 0),
                              # naive per-gate sets: the operands are torch.cat COPIES of the parameters — the
                              # freshness stamp must watch the gates' own parameters
                              (dict(kind="ttlstm", input_size=28, hidden_size=64, num_layers=2, n_cores=2, tt_rank=3, is_naive=True), 4, 7, 0),
                              (dict(kind="ttgru", input_size=1, hidden_size=128, num_layers=1, n_cores=3, tt_rank=4, is_naive=True), 4, 9, 0)):
        m = build_module(meta, dev()).eval()
        x = torch.randn(B, T, meta["input_size"], device=dev())
        desc = m._all_layers[0]._layer_spec().desc(B, T, 0)
        assert _lib.load().ttrnn_rnn_prepare_supported(ctypes.byref(desc)) == split
        with torch.no_grad():
            ref = m(x)[0]
            m.prepare_for_inference()
            a = m(x)[0]
            b = m(x)[0]                                   # second call: the cached workspace
            assert torch.equal(a, ref) and torch.equal(b, ref)
            # a workspace is kept only where it holds weight-only results (a route that splits the phases); elsewhere it is
            # per-call scratch (hundreds of MB for a stacked layer) and must not be pinned per shape
            prep0 = m._all_layers[0]._prepared
            assert len(prep0.workspaces) == split
            for k in range(1, prep0.MAX_WORKSPACES + 3):      # variable-length inference: the per-shape cache is bounded
                m(torch.randn(B, T + k, meta["input_size"], device=dev()))
            assert len(prep0.workspaces) == (prep0.MAX_WORKSPACES if split else 0)
            import copy
            assert all(getattr(c, "_prepared", None) is None for c in copy.deepcopy(m)._all_layers)
            x2 = torch.randn(B + 1, T + 3, meta["input_size"], device=dev())
            assert torch.equal(m(x2)[0], m.release_prepared()(x2)[0])
            m.prepare_for_inference()
            m(x)
            for p in m.parameters():                       # an optimizer-style in-place update
                p.mul_(1.25)
            upd = m(x)[0]                                  # must be prepared again by itself
            m.release_prepared()
            assert torch.equal(upd, m(x)[0]) and not torch.equal(upd, ref)
            m.prepare_for_inference()
            with ttrnn_hip.fp32_math("exact"):             # an option change invalidates prepared workspaces
                e1 = m(x)[0]
                m.release_prepared()
                assert torch.equal(e1, m(x)[0])
        # autograd runs never use the prepared state
        m.prepare_for_inference()
        m.train()
        assert m._all_layers[0]._prepared is None


# ---- (4) fp32 math modes: three-way bf16 split (default) vs fp32 MFMA ("exact") -------------------------
# Every test above runs in the library's default mode (split where a split kernel exists: the cfg2 hidden shape);
# the ones below pin BOTH modes explicitly on that shape.
@pytest.fixture(params=["split", "exact"])
def math_mode(request):
    import ttrnn_hip
    with ttrnn_hip.fp32_math(request.param):
        yield request.param


def test_default_math_mode_is_split():
    import os
    import ttrnn_hip
    if "TTRNN_FP32_MATH" not in os.environ:
        assert ttrnn_hip.get_fp32_math() == "split"


@pytest.mark.parametrize("name", ["g5_seq_cfg2", "g5_seq_cfg2_scaled"])
def test_math_modes_forward_golden(math_mode, name):
    """The reference's own outputs, one tolerance for both modes (1e-5 abs)."""
    case = Case(name)
    m = _loaded_module(case)
    with torch.no_grad():
        res = _run(case, m)
    _check_forward(case, res, 1e-5)      # <= 1e-5 abs, the 784-step sequences included


def test_math_modes_cell_step_golden(math_mode):
    test_cell_step_golden("g4_cell_cfg2")


def test_math_modes_training_forward_feeds_backward(math_mode):
    """Training mode (reserve written by the forward kernel of either mode, consumed by the reverse-time kernel):
    forward and gradients against the reference's."""
    _check_gradients_golden("g6_bwd_cfg2")


def test_split_math_error_vs_fp64_is_fp32_class():
    """cfg2 shapes over the full 784 steps against the oracle evaluated in float64: the split mode must be as
    close to the exact result as ordinary fp32 arithmetic is (the fp32-MFMA mode and the torch-CPU fp32 oracle)."""
    import ttrnn_hip
    m = _cfg2_module()
    torch.manual_seed(99)
    x = torch.rand(4, 784, 1)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, _, c64 = _oracle_forward("ttlstm", sd, 1, x.double())
    r32, _, c32 = _oracle_forward("ttlstm", sd, 1, x)
    errs = {"cpu_fp32": max(_maxabs(r32, r64), _maxabs(c32, c64))}
    for mode in ("exact", "split"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            out, (hT, cT) = m(x.to(dev()))
        errs[mode] = max(_maxabs(out, r64), _maxabs(cT, c64))
    print("max abs error vs float64 oracle:", errs)
    assert errs["split"] <= 2e-6 and errs["exact"] <= 2e-6
    assert errs["split"] <= 2.0 * max(errs["exact"], errs["cpu_fp32"]) + 1e-7


@pytest.mark.parametrize("wscale,xscale,T,tol", [(1.5, 2.0, 96, 5e-6), (2.5, 3.0, 6, 2e-5)])
def test_split_math_large_magnitude_inputs_and_states(wscale, xscale, T, tol):
    """Splitting must hold up away from the tiny activations of a fresh init: every parameter scaled (the TT-matrix
    grows with the cube), N(0,1) inputs scaled, non-zero initial state — both modes against the float64 oracle.
    (The recurrence turns chaotic once the gates saturate — at 2x parameters the reference's own fp32 run is 5e-2
    off its fp64 run after 96 steps — so the long case stays at 1.5x and the strongly saturated case is short; there the
    gate pre-activations reach |50|, where one fp32 ulp is 4e-6 and the order of a 256-term sum shows: every GPU path
    (split, fused fp32 MFMA, stage-wise fp32 MFMA) lands between 3e-5 and 5e-5 absolute on |c| up to 4.3.)"""
    import ttrnn_hip
    m = _cfg2_module()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(wscale)
    torch.manual_seed(3)
    x = xscale * torch.randn(3, T, 1)
    h0, c0 = torch.randn(3, 256) * 0.5, torch.randn(3, 256)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, _, c64 = _oracle_forward("ttlstm", sd, 1, x.double(), (h0.double(), c0.double()))
    for mode in ("exact", "split"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            out, (hT, cT) = m(x.to(dev()), (h0.to(dev()), c0.to(dev())))
        err = max(_maxabs(out, r64), _maxabs(cT, c64))
        print(mode, "max abs error vs float64 oracle (|c| up to %.2f):" % float(c64.abs().max()), err)
        assert err <= tol * max(1.0, float(c64.abs().max()))      # relative to the state's scale


@pytest.mark.parametrize("route", ["fused_core", "runtime_mfma"])
@pytest.mark.parametrize("case", ["tiny_weights", "huge_weights", "huge_h0", "zero_core", "mixed_magnitudes"])
def test_split_math_operand_ranges(case, route):
    """The split mode of the fused-core LSTM kernels multiplies two-piece fp16 operands under power-of-two scales chosen
    per launch from the cores' and h_0's maxima (ttrnn_f10_dev.h): nothing may overflow fp16's range or lose the small
    entries, whatever the magnitudes.  Both modes against the float64 oracle, error relative to the largest state."""
    import ttrnn_hip
    m = _cfg2_module()
    torch.manual_seed(17)
    T = 5
    h0, c0 = torch.randn(3, 256) * 0.3, torch.randn(3, 256) * 0.3
    x = torch.randn(3, T, 1)
    with torch.no_grad():
        cores = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n]
        assert len(cores) == 3
        if case == "tiny_weights":
            for p in cores:
                p.mul_(1e-4)                                  # TT-matrix entries ~1e-13
        elif case == "huge_weights":
            for p in cores:
                p.mul_(40.0)                                  # TT-matrix x 64 000: pre-activations in the thousands
        elif case == "huge_h0":
            h0 = torch.randn(3, 256) * 300.0                  # far outside (-1, 1): only a caller's h_0 can be
        elif case == "zero_core":
            cores[1].zero_()
        elif case == "mixed_magnitudes":
            # rows of very different size inside one core: entries down to 1e-9 of the maximum
            for k, step, f in ((2, 3, 1e-6), (0, 2, 1e-5)):
                w = cores[k].detach().clone().reshape(-1)
                w[::step] *= f
                cores[k].copy_(w.reshape(cores[k].shape))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, _, c64 = _oracle_forward("ttlstm", sd, 1, x.double(), (h0.double(), c0.double()))
    scale = max(1e-30, float(c64.abs().max()), float(r64.abs().max()))
    errs = {}
    for mode in ("exact", "split"):
        # the runtime-shape tier (ttrnn_g2.hip) uses the same two-piece fp16 operands in its stage 2, with its own scales
        with ttrnn_hip.fp32_math(mode), ttrnn_hip.option("force_g2", 1 if (route == "runtime_mfma" and mode == "split") else 0), \
                torch.no_grad():
            if mode == "split":
                from ttrnn_hip import functional as F
                assert F.rnn_route(m._all_layers[0]._layer_spec(), 3, T) == route
            out, (hT, cT) = m(x.to(dev()), (h0.to(dev()), c0.to(dev())))
        assert torch.isfinite(out).all() and torch.isfinite(cT).all(), (case, mode)
        errs[mode] = max(_maxabs(out, r64), _maxabs(cT, c64))
    print(case, "max abs error vs float64 (state scale %.3g):" % scale, errs)
    # saturated gates amplify one fp32 ulp of a pre-activation in the thousands (2e-4) into the state: both modes alike
    tol = 2e-3 if case in ("huge_weights", "huge_h0") else 2e-6
    assert errs["split"] <= tol * max(1.0, scale)
    assert errs["split"] <= 3.0 * errs["exact"] + 2e-7 * max(1.0, scale)


@pytest.mark.parametrize("case", ["fresh", "tiny_weights", "huge_weights", "huge_h0", "zero_core", "mixed_magnitudes"])
def test_two_core_kernel_operand_ranges(case):
    """ttrnn_fast_f2.hip (d = 2: H = 128, ranks 4 — BASELINE configs[0], pMNIST's default --ncores 2): both chain stages on
    two-piece fp16 operands under diagonal power-of-two scales (per i1 / rank index of core 1, per row of core 0, per sample for a
    caller's h_0).  784 steps for the fresh model, short runs for the operand-range cases, both math modes (exact = the
    fp32-MFMA stage-wise kernel) against the float64 oracle; batch split and repeat launches bit for bit."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    torch.manual_seed(29)
    m = build_module(dict(kind="ttlstm", input_size=1, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4), dev())
    T = 784 if case == "fresh" else 6
    B = 5
    g = torch.Generator().manual_seed(31)
    x = torch.rand(B, T, 1, generator=g) if case == "fresh" else torch.randn(B, T, 1, generator=g)
    h0, c0 = torch.randn(B, 128, generator=g) * 0.3, torch.randn(B, 128, generator=g) * 0.3
    with torch.no_grad():
        cores = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n]
        assert len(cores) == 2
        if case == "tiny_weights":
            for p in cores:
                p.mul_(1e-5)
        elif case == "huge_weights":
            for p in cores:
                p.mul_(200.0)
        elif case == "huge_h0":
            h0 = torch.randn(B, 128, generator=g) * torch.tensor([0.1, 3.0, 40.0, 500.0, 6000.0]).view(B, 1)
        elif case == "zero_core":
            cores[0].zero_()
        elif case == "mixed_magnitudes":
            for k, step, f in ((1, 3, 1e-6), (0, 2, 1e-5)):
                w = cores[k].detach().clone().reshape(-1)
                w[::step] *= f
                cores[k].copy_(w.reshape(cores[k].shape))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, _, c64 = _oracle_forward("ttlstm", sd, 1, x.double(), (h0.double(), c0.double()))
    scale = max(1e-30, float(c64.abs().max()), float(r64.abs().max()))
    errs = {}
    xd, hd, cd = x.to(dev()), h0.to(dev()), c0.to(dev())
    for mode in ("exact", "split"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == ("fused_core" if mode == "split" else "stagewise_mfma")
            out, (hT, cT) = m(xd, (hd, cd))
            if mode == "split":
                again, _ = m(xd, (hd, cd))
                assert torch.equal(out, again)                               # repeat launch
                part, _ = m(xd[1:3], (hd[1:3], cd[1:3]))
                assert torch.equal(out[1:3], part)                           # samples never interact
                assert torch.equal(out[:, -1], hT)
                if case != "huge_weights":      # (TT-matrix x 40 000: the recurrence amplifies one ulp by 4e4 per step — sign flips of
                    nost = m(xd)[0]             # saturated units after six steps in ANY arithmetic; the run above stays comparable)
                    r0, _, _ = _oracle_forward("ttlstm", sd, 1, x.double())      # zero initial state: the H0 = false instantiation
                    assert _maxabs(nost, r0) <= 2e-6 * max(1.0, float(r0.abs().max()))
        assert torch.isfinite(out).all() and torch.isfinite(cT).all(), (case, mode)
        errs[mode] = max(_maxabs(out, r64), _maxabs(cT, c64))
    print(case, "two-core kernel: max abs error vs float64 (state scale %.3g):" % scale, errs)
    tol = 2e-3 if case in ("huge_weights", "huge_h0") else 2e-6
    assert errs["split"] <= tol * max(1.0, scale)
    assert errs["split"] <= 3.0 * errs["exact"] + 2e-7 * max(1.0, scale)


def test_two_core_kernel_guard_falls_back_on_outlier_rows():
    """k_f2_prep's guard: the scales of the two-core kernel are u[i1] + v[a] (the most general form both stages can share), so one
    core-1 entry x 1e5 drags the other rank rows of its i1 slice 17 binades down — second fp16 pieces subnormal, 12 of 22 bits
    left.  Such weights leave for the fp32-MFMA stage-wise kernel queued behind the launch: the result then equals the exact
    mode's bit for bit, the trip is counted (ttrnn_device_status), and a fresh model does not trip."""
    import ttrnn_hip
    torch.manual_seed(37)
    m = build_module(dict(kind="ttlstm", input_size=1, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4), dev())
    x = torch.rand(4, 9, 1, device=dev())
    ttrnn_hip.device_status(reset=True)
    with torch.no_grad():
        fresh = m(x)[0]
        assert ttrnn_hip.device_status()["guard_trips"] == 0
        with ttrnn_hip.fp32_math("exact"):
            fresh_exact = m(x)[0]
        assert not torch.equal(fresh, fresh_exact) and _maxabs(fresh, fresh_exact) <= 1e-6       # two different kernels ran
        core1 = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n][1]
        flat = core1.detach().clone().contiguous().view(-1)
        flat[(5 * flat.numel()) // 11] *= 1e5
        core1.copy_(flat.view(core1.shape))
        tripped = m(x)[0]
        st = ttrnn_hip.device_status(reset=True)
        assert st["guard_trips"] == 1, st
        with ttrnn_hip.fp32_math("exact"):
            exact = m(x)[0]
        assert torch.equal(tripped, exact)
        m.prepare_for_inference()                         # the guard word lives in the prepared workspace too
        assert torch.equal(m(x)[0], exact) and torch.equal(m(x)[0], exact)
        assert ttrnn_hip.device_status(reset=True)["guard_trips"] == 2


OUTLIER_SHAPES = {
    # name: (module meta, B, T, route the forward must take in split mode, options for the split run)
    "fused_core_r8": (dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), 3, 5, "fused_core", {}),
    "fused_core_r16": (dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=1, n_cores=3, tt_rank=16), 90, 4, "fused_core",
                       {"gemm_pieces": 2}),
    "runtime_mfma": (dict(kind="ttlstm", input_size=28, hidden_size=192, num_layers=1, n_cores=2, tt_rank=6), 5, 5, "runtime_mfma", {}),
    "runtime_mfma_d3": (dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), 3, 5, "runtime_mfma",
                        {"force_g2": 1}),
    "runtime_mfma_gru": (dict(kind="ttgru", input_size=40, hidden_size=128, num_layers=1, n_cores=3, tt_rank=4), 20, 5, "runtime_mfma", {}),
    "merged_big": (dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32), 2, 3, "merged_big", {}),
    # round 4: the two-core kernel (ttrnn_fast_f2.hip: cfg1 / pMNIST --ncores 2), in = 1 (unit rows) and in = H (a stacked layer's gin)
    "two_core_f2": (dict(kind="ttlstm", input_size=1, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4), 3, 6, "fused_core", {}),
    "two_core_f2_stack": (dict(kind="ttlstm", input_size=128, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4), 5, 4, "fused_core", {}),
}


@pytest.mark.parametrize("case", ["hid_core0_1e3", "hid_core1_1e5", "hid_corelast_1e7", "hid_corelast_1e5", "h0_unit_1e4",
                                  "in_core_1e6", "x_elem_1e6"])
@pytest.mark.parametrize("shape", sorted(OUTLIER_SHAPES))
def test_split_math_outlier_up(shape, case):
    """ONE large value inside an otherwise ordinary operand: a single core entry x 1e3 / 1e5 / 1e7, one unit of
    h_0 x 1e4 inside an N(0, 0.1) state, one entry of an input-matrix core x 1e6 (a column band of the dense W_in), one element
    of x x 1e6.  Power-of-two scales taken from an operand's MAXIMUM would push every other entry 10-23 binades down and
    cost the two-piece fp16 operands 5-12 of their 22 bits — silently, on the bulk of the operand.  The scales are diagonal
    (per row / column / rank slice of the cores, per row of x: ttrnn_f10_dev.h, ttrnn_g2.hip, ttrnn_fast_bigh.hip,
    ttrnn_fast_gemm.hip), so the split mode must stay where the fp32-MFMA / fp32-FMA mode is against float64."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    meta, B, T, route, opts = OUTLIER_SHAPES[shape]
    torch.manual_seed(41)
    m = build_module(meta, dev())
    H, inp = meta["hidden_size"], meta["input_size"]
    lstm = meta["kind"] == "ttlstm"
    g = torch.Generator().manual_seed(43)
    x = torch.randn(B, T, inp, generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.1
    c0 = torch.randn(B, H, generator=g) * 0.3
    hid = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n]
    inw = [p for n, p in m.named_parameters() if "input_weights.parameters" in n]

    def bump(core, factor, pos=(7, 13)):
        with torch.no_grad():
            flat = core.detach().clone().contiguous().view(-1)
            flat[(pos[0] * flat.numel()) // pos[1]] *= factor
            core.copy_(flat.view(core.shape))

    if case == "hid_core0_1e3":
        bump(hid[0], 1e3)
    elif case == "hid_core1_1e5":
        bump(hid[min(1, len(hid) - 1)], 1e5)
    elif case == "hid_corelast_1e7":
        bump(hid[-1], 1e7)
    elif case == "hid_corelast_1e5":
        bump(hid[-1], 1e5, (5, 11))
    elif case == "h0_unit_1e4":
        h0[:, 77 % H] *= 1e4
    elif case == "in_core_1e6":
        bump(inw[-1], 1e6)
    elif case == "x_elem_1e6":
        x[1, 2, 3 % inp] *= 1e6
        x[B - 1, 0, inp - 1] *= 1e6
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    init = (h0.double(), c0.double()) if lstm else h0.double()
    ref = _oracle_forward(meta["kind"], sd, 1, x.double(), init)
    r64 = ref[0]
    scale = max(1.0, float(r64.abs().max()), float(ref[2].abs().max()) if lstm else 0.0)
    errs = {}
    for mode in ("exact", "split"):
        with contextlib.ExitStack() as stack:
            stack.enter_context(ttrnn_hip.fp32_math(mode))
            if mode == "split":
                for k, v in opts.items():
                    stack.enter_context(ttrnn_hip.option(k, v))
                assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == route
            with torch.no_grad():
                res = m(x.to(dev()), (h0.to(dev()), c0.to(dev())) if lstm else h0.to(dev()))
        out = res[0]
        assert torch.isfinite(out).all(), (shape, case, mode)
        errs[mode] = _maxabs(out, r64)
        if lstm:
            errs[mode] = max(errs[mode], _maxabs(res[1][1], ref[2]))
    print(shape, case, "max abs error vs float64 (state scale %.3g):" % scale, errs)
    # the yardstick is the library's own fp32 arithmetic on the same input (saturated gates and pre-activations in the
    # millions amplify one fp32 ulp whatever the mode); the floor is a few ulps of the state's scale.
    # Factor 3 wherever the large value sits in a WEIGHT or in x.  Two cases show the format itself instead — two fp16 pieces
    # carry 22 significand bits against fp32's 24, i.e. up to 8x the relative error of ONE product: (a) a GRU computes
    # n = tanh(in_n + r * hid_n) (gru.py:42-43) — with |hid_n| ~ 1e4 behind a large core entry the product r * hid_n feeds a
    # non-saturated tanh, so the relative precision of that single sum is what the state sees (an LSTM's gates just
    # saturate); (b) one unit of h_0 x 1e4: the scale of h_0 is per SAMPLE (it is the dynamic operand), so for one step the
    # other units of that sample keep 17-19 bits; both modes then sit at 1e-6 ... 1e-5 of a pre-activation in the hundreds.
    factor = 8.0 if (meta["kind"] == "ttgru" or case == "h0_unit_1e4") else 3.0
    assert errs["split"] <= factor * errs["exact"] + 4e-7 * scale


@pytest.mark.parametrize("kind", ["ttgru", "ttlstm"])
def test_runtime_tier_initial_state_far_outside_unit_range(kind):
    """The runtime-shape tier's fp16 stage-2 operands assume |h| <= 1; a caller's h_0 is carried with a per-sample power of
    two — for a GRU at every step, because h_t = (1 - z) n + z h_{t-1} can stay as large as h_0 for many steps."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    torch.manual_seed(23)
    m = build_module(dict(kind=kind, input_size=28, hidden_size=192, num_layers=1, n_cores=2, tt_rank=6), dev())
    B, T = 5, 12
    x = torch.randn(B, T, 28)
    h0 = torch.randn(B, 192) * torch.tensor([0.1, 3.0, 40.0, 500.0, 6000.0]).view(B, 1)
    c0 = torch.randn(B, 192)
    assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == "runtime_mfma"
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    init = (h0.double(), c0.double()) if kind == "ttlstm" else h0.double()
    ref = _oracle_forward(kind, sd, 1, x.double(), init)[0]
    with torch.no_grad():
        res = m(x.to(dev()), (h0.to(dev()), c0.to(dev())) if kind == "ttlstm" else h0.to(dev()))
    out = res[0].float().cpu()
    assert torch.isfinite(out).all()
    # the reference's own fp32 arithmetic on the same inputs: a state of 10^4 puts pre-activations at 10^4..10^5, where one
    # fp32 ulp (4e-3) moves a gate by 1e-3 and the GRU's z * h term by 10 — the yardstick for the largest samples
    sd32 = {k: v.float() for k, v in sd.items()}
    init32 = (h0, c0) if kind == "ttlstm" else h0
    ref32 = _oracle_forward(kind, sd32, 1, x, init32)[0]
    for b in range(B):       # error relative to each sample's own scale (the GRU keeps |h| near |h_0| for a while)
        scale = max(1.0, float(ref[b].abs().max()))
        err, err32 = _maxabs(out[b], ref[b]), _maxabs(ref32[b], ref[b])
        assert err <= max(2e-5 * scale, 8.0 * err32), (b, err, err32, scale)


@pytest.mark.parametrize("seed", list(range(12)))
def test_runtime_tier_random_shapes_and_magnitudes(seed):
    """Random (cell, H, ncores, rank, input size), every core multiplied by its own random power of ten, random initial state
    magnitude: the runtime-shape forward (fp16 stage-2 operands, scales from the merged cores' maxima) against float64."""
    import random
    from ttrnn_hip import functional as F
    rnd = random.Random(1000 + seed)
    kind = rnd.choice(["ttlstm", "ttgru"])
    H = rnd.choice([64, 96, 128, 192, 320, 512])
    d = rnd.choice([2, 3, 4]) if H != 96 else rnd.choice([2, 3])
    r = rnd.choice([2, 3, 4, 6, 8])
    inp = rnd.choice([1, 12, 28, 40])
    torch.manual_seed(seed)
    m = build_module(dict(kind=kind, input_size=inp, hidden_size=H, num_layers=1, n_cores=d, tt_rank=r), dev())
    B, T = 4, 6
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "parameters" in n:
                p.mul_(10.0 ** rnd.uniform(-2.0, 0.7))
    if F.rnn_route(m._all_layers[0]._layer_spec(), B, T) != "runtime_mfma":
        pytest.skip("shape has a specialised kernel")
    x = torch.randn(B, T, inp) * 10.0 ** rnd.uniform(-2, 1)
    h0 = torch.randn(B, H) * 10.0 ** rnd.uniform(-3, 2)
    c0 = torch.randn(B, H)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    init = (h0.double(), c0.double()) if kind == "ttlstm" else h0.double()
    ref = _oracle_forward(kind, sd, 1, x.double(), init)[0]
    with torch.no_grad():
        out = m(x.to(dev()), (h0.to(dev()), c0.to(dev())) if kind == "ttlstm" else h0.to(dev()))[0].float().cpu()
    assert torch.isfinite(out).all()
    scale = max(1.0, float(ref.abs().max()))
    err = _maxabs(out, ref)
    print(kind, "H", H, "d", d, "r", r, "in", inp, "max|ref| %.3g err %.3g" % (float(ref.abs().max()), err))
    assert err <= 5e-5 * scale


@pytest.mark.parametrize("seed", list(range(8)))
def test_fused_core_stack_random_magnitudes(seed):
    """Two stacked H = 256 TT-LSTM layers (ranks 8 / 16: one-wave and k-split fused-core kernels, the input projections as the
    two-piece fp16 GEMM) with every core scaled by its own random power of ten, random input and state magnitudes, against
    the float64 oracle; the outputs must also be identical bit for bit when the batch is cut in two."""
    import random
    import ttrnn_hip
    from ttrnn_hip import functional as F
    rnd = random.Random(77 + seed)
    r = rnd.choice([8, 16])
    torch.manual_seed(seed)
    m = build_module(dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=r), dev())
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "parameters" in n:
                p.mul_(10.0 ** rnd.uniform(-1.5, 0.5))
    B, T = rnd.choice([20, 33]), rnd.choice([5, 9])
    assert F.rnn_route(m._all_layers[1]._layer_spec(), B, T) == "fused_core"
    x = torch.randn(B, T, 40) * 10.0 ** rnd.uniform(-2, 1.5)
    h0 = torch.randn(B, 256) * 10.0 ** rnd.uniform(-2, 2)
    c0 = torch.randn(B, 256) * 10.0 ** rnd.uniform(-1, 1)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    ref = _oracle_forward("ttlstm", sd, 2, x.double(), (h0.double(), c0.double()))[0]
    xd, hd, cd = x.to(dev()), h0.to(dev()), c0.to(dev())
    with ttrnn_hip.option("gemm_pieces", 2), torch.no_grad():
        out = m(xd, (hd, cd))[0]
        cut = B - 3                      # still >= 2 * in rows: the same K-in route as the whole batch
        oa = m(xd[:cut], (hd[:cut], cd[:cut]))[0]
    assert torch.isfinite(out).all()
    err = _maxabs(out, ref)
    scale = max(1.0, float(ref.abs().max()))
    print("r", r, "B", B, "T", T, "max|ref| %.3g err %.3g" % (float(ref.abs().max()), err))
    assert err <= 5e-5 * scale
    # the scale of a caller's h_0 is taken per sample (f10h_h0_expo): a sample's result does not depend on its batch mates
    assert torch.equal(out[:cut], oa)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_half_piece_gemm_input_ranges(storage):
    """The batched input projection runs as a GEMM on two-piece fp16 operands with one power-of-two scale per row of x and
    one for the matrix (ttrnn_fast_gemm.hip): rows of wildly different magnitude, zero rows and outliers inside a row
    must come out as they do with three bf16 pieces (option gemm_pieces = 3; by default the library picks by problem size)
    and as the float64 oracle says."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    torch.manual_seed(5)
    kind = "ttlstm" if storage == "f32" else "ttgru"
    meta = dict(kind=kind, input_size=40, hidden_size=256 if storage == "f32" else 512, num_layers=1, n_cores=3, tt_rank=16 if storage == "f32" else 4)
    m = build_module(meta, dev())
    B, T = 64, 16
    x = torch.randn(B, T, 40) * (10.0 ** (torch.rand(B, T, 1) * 9 - 6))      # row scales 1e-6 .. 1e3
    x[3, 2] = 0.0
    x[7, 3] = 1e-30 * torch.randn(40)                                          # a row far below every other (scale clamp)
    x[5, 1, 7] = 2.0e4                                                         # outlier inside a small row
    x[:, 0] *= 1e-3
    if storage == "bf16":
        m = m.to(torch.bfloat16)
        x = x.to(torch.bfloat16)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    ref = _oracle_forward(kind, sd, 1, x.double())[0]
    outs = {}
    for name, val in (("half", 2), ("bf16x3", 3)):
        with ttrnn_hip.option("gemm_pieces", val), torch.no_grad():
            outs[name] = m(x.to(dev()))[0].float()
    assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) in ("fused_core", "runtime_mfma")
    # rows scaled by 1e3 put pre-activations in the thousands, where one fp32 ulp is 1e-4: both variants sit at 2e-5
    tol = 1e-4 if storage == "f32" else 2e-2
    errs = {k: _maxabs(v, ref) for k, v in outs.items()}
    print(storage, "max abs error vs float64:", errs, "between the two:", _maxabs(outs["half"], outs["bf16x3"]))
    assert torch.isfinite(outs["half"]).all()
    assert errs["half"] <= tol and errs["half"] <= 2.0 * errs["bf16x3"] + (2e-7 if storage == "f32" else 4e-3)


@pytest.mark.parametrize("shape", ["fused_core_rank16", "merged_big", "merged_big_bf16"])
def test_half_piece_dense_weight_gradient_column_ranges(shape):
    """The dense weight gradient dW = x^T dy on two-piece fp16 operands (ttrnn_fast_gemm.hip, HALF): the contraction runs
    over the rows, so the power-of-two scales are per COLUMN of x and of dy, taken from column maxima measured per launch.
    Columns of wildly different magnitude, a zero column and an outlier row must give the gradients the three-bf16-piece
    variant (option gemm_pieces = 3) and the float64 oracle give.  (By default the library picks the variant by size.)"""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(77)
    bf16 = shape.endswith("_bf16")
    if shape.startswith("merged_big"):
        meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
        B, T, n_in = 4, 40, 1024
    else:
        meta = dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=1, n_cores=3, tt_rank=16)
        B, T, n_in = 48, 30, 40
    m = build_module(meta, dev())
    x = torch.randn(B, T, n_in) * (10.0 ** (torch.rand(1, 1, n_in) * 8 - 5))     # column scales 1e-5 .. 1e3
    x[:, :, 3] = 0.0
    x[1, 2] *= 50.0                                                              # an outlier row
    w = torch.randn(B, T, meta["hidden_size"])
    if bf16:                              # bf16 storage: parameters, x and out in bf16 (the oracle sees the rounded values)
        m = m.to(torch.bfloat16)
        x = x.to(torch.bfloat16)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    ro, _ = O.lstm_forward(layers, x.double(), None)
    (ro * w.double()).sum().backward()
    grads = {}
    for name, val in (("half", 2), ("bf16x3", 3)):
        m.zero_grad()
        with ttrnn_hip.option("gemm_pieces", val):
            out, _ = m(x.to(dev()))
            (out.float() * w.to(dev())).sum().backward()
        grads[name] = {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}
    worst = {"half": 0.0, "bf16x3": 0.0}
    differ = False
    for n, _ in m.named_parameters():
        ref = leaves[n].grad
        sc = max(float(ref.abs().max()), 1e-30)
        for k in worst:
            assert torch.isfinite(grads[k][n]).all(), (k, n)
            worst[k] = max(worst[k], _maxabs(grads[k][n].double(), ref) / sc)
        differ = differ or not torch.equal(grads["half"][n], grads["bf16x3"][n])
    print(shape, "max gradient error relative to each tensor's maximum:", worst)
    assert differ                                                 # the two variants did run
    # (the input columns span eight decades: on the big shape the whole backward — reverse-time kernel, projections — sits at
    # 8e-4 of the largest gradient entry with three bf16 pieces; the yardstick is that variant, not an absolute figure)
    # bf16 storage: out, h and the returned gradients are rounded to bf16 (2^-9 relative each)
    assert worst["half"] <= (5e-2 if bf16 else 2e-3) and worst["half"] <= 3.0 * worst["bf16x3"] + 1e-6


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_wide_tile_gemm_matches_three_piece_variant(storage):
    """From 1024 workgroup tiles on, the two-piece input-projection GEMM takes 256-feature tiles (k_gemm_split<., HALF, 2>):
    16 384 rows into the cfg5-class matrix (1024 -> 4096), both storage types, against the three-bf16-piece GEMM with its
    128-feature tiles on the same module and inputs (the recurrent kernel is the same in both runs)."""
    import ttrnn_hip
    torch.manual_seed(101)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    B, T = 1024, 16                       # 16 384 rows, few steps (the recurrence amplifies a GEMM difference step by step)
    x = torch.randn(B, T, 1024, device=dev()) * (10.0 ** (torch.rand(B, T, 1, device=dev()) * 3 - 3))     # rows 1e-3 .. 1
    if storage == "bf16":
        m = m.to(torch.bfloat16)
        x = x.to(torch.bfloat16)
    outs = {}
    for name, val in (("half_wide", 2), ("bf16x3", 3)):
        with ttrnn_hip.option("gemm_pieces", val), torch.no_grad():
            out, (hT, cT) = m(x)
        outs[name] = (out.float(), cT.float())
    assert torch.isfinite(outs["half_wide"][0]).all()
    d_out = _maxabs(outs["half_wide"][0], outs["bf16x3"][0])
    d_c = _maxabs(outs["half_wide"][1], outs["bf16x3"][1])
    print(storage, "wide two-piece vs three-piece GEMM: max |d out|", d_out, "max |d c_T|", d_c)
    assert not torch.equal(outs["half_wide"][0], outs["bf16x3"][0]) or storage == "bf16"
    # fp32: both are fp32-class; bf16: one output ulp.  (With rows up to 1e2 the pre-activations reach the hundreds, where two
    # fp32-class GEMMs differ by a few ulps = 1e-4, and so do the outputs: 9e-5 measured.)
    assert d_out <= (5e-6 if storage == "f32" else 8e-3) and d_c <= (2e-5 if storage == "f32" else 3e-2)


@pytest.mark.parametrize("variant", ["on_the_fly", "pre_split_planes"])
def test_half_piece_gemm_rows_near_fp32_limits(variant):
    """the scale exponent of a row / column used to be clamped to +-40, so a finite row with max |x| >= 2^42 left the
    fp16 range after scaling (inf, then NaN from the residual).  The exponent now follows the row up to the fp32 maximum and
    the two inverse scales are applied one after the other (smaller first, never as a product): rows at 1e15, 1e30 and 3e38 next to ordinary ones stay finite and agree with the three-bf16-piece GEMM (which has fp32's exponent range and no
    scales) and with the float64 oracle; so does a row whose large entries meet a tiny column of W."""
    import ttrnn_hip
    torch.manual_seed(2026)
    if variant == "pre_split_planes":       # k_gemm3h: taken from 1024 workgroup tiles (256 x 256) on
        meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
        B, T = 1024, 16
    else:                                   # k_gemm_split<., HALF>
        meta = dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=1, n_cores=3, tt_rank=16)
        B, T = 64, 16
    n_in = meta["input_size"]
    m = build_module(meta, dev())
    x = torch.randn(B, T, n_in)
    x[2, 1] *= 1e15
    x[4, 0] *= 1e30
    x[6, 3, :4] = torch.tensor([3.0e38, -3.0e38, 3.0e38, 3.0e38])      # the row maximum at the top of the fp32 range
    x[8, 2] *= 1e-35
    x[9, 5, 3] = 2.5e38                      # one huge entry in an ordinary row
    xd = x.to(dev())
    outs = {}
    for name, val in (("half", 2), ("bf16x3", 3)):
        with ttrnn_hip.option("gemm_pieces", val), torch.no_grad():
            out, (hT, cT) = m(xd)
        outs[name] = (out.float().cpu(), cT.float().cpu())
    assert torch.isfinite(outs["half"][0]).all() and torch.isfinite(outs["half"][1]).all()
    # the samples with huge rows: gates saturate, the result is decided by signs — identical up to the cancellation cases
    # of a 1e38-sized sum, which no fp32 evaluation order resolves (the float64 oracle is the referee for the others)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    ordinary = [b for b in range(min(B, 32)) if b not in (2, 4, 6, 9)]
    ref = _oracle_forward("ttlstm", sd, 1, x[ordinary].double())[0]
    err_half = _maxabs(outs["half"][0][ordinary], ref)
    err_3 = _maxabs(outs["bf16x3"][0][ordinary], ref)
    d_big = _maxabs(outs["half"][0][[2, 4, 6, 9]], outs["bf16x3"][0][[2, 4, 6, 9]])
    print(variant, "ordinary samples vs float64: half %.3g bf16x3 %.3g; huge-row samples half vs bf16x3: %.3g" % (err_half, err_3, d_big))
    assert err_half <= 2e-6 and err_half <= 2.0 * err_3 + 2e-7
    frac_close = float(((outs["half"][0][[2, 4, 6, 9]] - outs["bf16x3"][0][[2, 4, 6, 9]]).abs() <= 1e-4).float().mean())
    assert frac_close >= 0.999, frac_close


def test_math_modes_full_size_properties(math_mode):
    """cfg2 at full size: batch independence, causality, bitwise repeatability — in either mode."""
    m = _cfg2_module()
    torch.manual_seed(1111)
    x = torch.rand(64, 784, 1, device=dev())
    with torch.no_grad():
        out, (hT, cT) = m(x)
        out2, _ = m(x)
        out_a, _ = m(x[:17])
        out_p, _ = m(x[:, :100].contiguous())
    assert torch.equal(out, out2)
    assert torch.equal(out[:17], out_a)
    assert torch.equal(out[:, :100], out_p)
    assert torch.equal(out[:, -1], hT)
    assert torch.isfinite(out).all() and torch.isfinite(cT).all()


# ---- (5) fused-core kernels: persistent row loops, stacked layers, switches ---------------------------------------
@pytest.mark.parametrize("rank,B,T,x_grad", [(8, 41, 23, True), (16, 37, 19, True), (16, 37, 19, False),
                                             (16, 48, 27, True), (8, 53, 25, False)])
def test_stacked_layers_many_rows_vs_generic(rank, B, T, x_grad):
    """Two stacked TT-LSTM layers (input projections and weight-gradient passes run on the fused-core kernels, whose
    workgroups WALK over B*T > 256 rows) against the any-shape kernels on the same module: forward, input gradient
    and every parameter gradient.  Without an input gradient the first layer's in=40 matrix takes the fused-core
    weight-gradient kernel too (it produces dx only for hidden-shaped inputs).  From B*T >= 512 rows on the input
    projections run as dense split-bf16 GEMMs, from B*T >= 1024 the weight gradients go through the dense gradient
    x^T dy and dx through a second GEMM (ttrnn_fast_gemm.hip): the last two cases."""
    import os
    torch.manual_seed(77 + rank)
    meta = dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=rank)
    m = build_module(meta, dev())
    x = torch.rand(B, T, 40, device=dev())
    w = torch.randn(B, T, 256, device=dev())
    outs = []
    for force in ("0", "1"):
        OPT["TTRNN_FORCE_GENERIC"] = force
        try:
            m.zero_grad()
            xg = x.clone().requires_grad_(x_grad)
            out, (h, c) = m(xg)
            ((out * w).sum() + c.sum() + h.sum()).backward()
            outs.append((out.detach().clone(), xg.grad.clone() if x_grad else torch.zeros(1),
                         [p.grad.clone() for p in m.parameters()]))
        finally:
            OPT["TTRNN_FORCE_GENERIC"] = "0"
    assert _maxabs(outs[0][0], outs[1][0]) <= 5e-6
    assert _maxabs(outs[0][1], outs[1][1]) <= 1e-4 * max(1e-3, float(outs[1][1].abs().max()))
    for (name, _), a, b in zip(m.named_parameters(), outs[0][2], outs[1][2]):
        assert _maxabs(a, b) <= 1e-4 * max(float(b.abs().max()), 1e-6), name


def test_fused_core_switch_off_matches():
    """TTRNN_NO_F10=1 (stage-wise kernels instead of the fused-core ones) gives the same results within fp32 tolerance."""
    import os
    m = _cfg2_module()
    torch.manual_seed(8)
    x = torch.rand(6, 50, 1, device=dev())
    res = []
    for flag in ("0", "1"):
        OPT["TTRNN_NO_F10"] = flag
        try:
            m.zero_grad()
            out, (h, c) = m(x)
            (out.square().sum() + c.sum()).backward()
            res.append((out.detach().clone(), [p.grad.clone() for p in m.parameters()]))
        finally:
            OPT["TTRNN_NO_F10"] = "0"
    assert _maxabs(res[0][0], res[1][0]) <= 2e-6
    for a, b in zip(res[0][1], res[1][1]):
        assert _maxabs(a, b) <= 1e-4 * max(float(b.abs().max()), 1e-6)


@pytest.mark.parametrize("rank", [8, 16])
def test_fused_core_edge_cases_vs_oracle(rank):
    """Fused-core kernels at the corners: no biases, B = 1, T = 1 and T = 2, explicit and absent initial state."""
    torch.manual_seed(300 + rank)
    with contextlib.redirect_stdout(io.StringIO()):
        from tensorized_rnn.tt_lstm import TTLSTM
        m = TTLSTM(1, 256, 1, dev(), n_cores=3, tt_rank=rank, bias=False)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert not any(k.endswith("bias") for k in sd)
    for B, T, with_init in [(1, 1, False), (1, 2, True), (3, 1, True), (2, 5, False)]:
        x = torch.randn(B, T, 1)
        init = (torch.randn(B, 256) * 0.3, torch.randn(B, 256) * 0.3) if with_init else None
        ro, rh, rc = _oracle_forward("ttlstm", sd, 1, x, init)
        with torch.no_grad():
            out, (hT, cT) = m(x.to(dev()), None if init is None else (init[0].to(dev()), init[1].to(dev())))
        assert _maxabs(out, ro) <= 1e-5 and _maxabs(hT, rh) <= 1e-5 and _maxabs(cT, rc) <= 1e-5, (B, T, with_init)


def test_big_shape_merge_levels_and_bf16_storage():
    """cfg5-class matrix (H = in = 1024, d = 4, r = 32): the three contraction groupings (TTRNN_BIG_MERGE = 2, 1, 0) agree
    with the oracle, and bf16 storage runs through the same kernels (2e-2 vs the fp32 oracle on bf16-rounded weights)."""
    import os
    torch.manual_seed(55)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    x = torch.randn(3, 4, 1024)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ro, rh, rc = _oracle_forward("ttlstm", sd, 1, x)
    try:
        for level in ("2", "1", "0"):
            OPT["TTRNN_BIG_MERGE"] = level
            with torch.no_grad():
                out, (hT, cT) = m(x.to(dev()))
            assert _maxabs(out, ro) <= 1e-5 and _maxabs(cT, rc) <= 1e-5, level
    finally:
        OPT.pop("TTRNN_BIG_MERGE", None)
    mb = build_module(meta, dev()).to(torch.bfloat16)
    sdb = {k: v.detach().cpu().float() for k, v in mb.state_dict().items()}
    xb = x.to(torch.bfloat16)
    rob, _, rcb = _oracle_forward("ttlstm", sdb, 1, xb.float())
    with torch.no_grad():
        outb, (hb, cb) = mb(xb.to(dev()))
    assert outb.dtype == torch.bfloat16
    assert _maxabs(outb.float(), rob) <= 2e-2 and _maxabs(cb.float(), rcb) <= 2e-2


def test_big_shape_two_workgroups_per_sample_matches_one():
    """cfg5-class K-rec with two cooperating workgroups per sample (halves of h swapped through global memory once per
    step) against the one-workgroup kernel: many steps, many samples, bitwise-equal arithmetic order per hidden unit."""
    import os
    torch.manual_seed(56)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    x = torch.randn(24, 96, 1024, device=dev())
    h0, c0 = torch.randn(24, 1024, device=dev()) * 0.3, torch.randn(24, 1024, device=dev()) * 0.3
    res = []
    try:
        for flag in ("0", "1"):
            OPT["TTRNN_BIG_NO_PAIR"] = flag
            with torch.no_grad():
                out, (hT, cT) = m(x, (h0, c0))
            res.append((out.clone(), cT.clone()))
    finally:
        OPT.pop("TTRNN_BIG_NO_PAIR", None)
    assert torch.isfinite(res[0][0]).all()
    assert _maxabs(res[0][0], res[1][0]) <= 2e-6 and _maxabs(res[0][1], res[1][1]) <= 2e-6


@pytest.mark.parametrize("case", ["fresh_init", "tiny_weights", "large_weights", "huge_weights_one_step", "huge_h0",
                                  "mixed_magnitudes"])
def test_big_shape_half_piece_operand_ranges(case):
    """cfg5-class K-rec in split mode (ttrnn_fast_bigh.hip): both chain stages on two-piece fp16 operands under
    power-of-two scales taken from the merged cores' maxima, the stage-1 sums rescaled before they are split, a caller's
    h_0 scaled per sample.  Against the float64 oracle, next to the fp32-MFMA pair kernel (TTRNN_FP32_MATH=exact) on the
    same inputs: finite whatever the magnitudes, and the same error class.  (With every hidden core x 3 and beyond — the
    TT-matrix x 81 — this recurrence is chaotic: the fp32-MFMA kernel is 1.5e-2 off float64 after six steps at x 3 and 2
    at x 5, the split kernel alike; so the long case stays at x 2 and the x 8 case — TT-matrix x 4096, pre-activations in
    the hundreds, there for the range of the scales — runs one step.)"""
    import ttrnn_hip
    torch.manual_seed(91)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    B, T = 3, (1 if case == "huge_weights_one_step" else 6)
    x = torch.randn(B, T, 1024)
    h0, c0 = torch.randn(B, 1024) * 0.3, torch.randn(B, 1024) * 0.3
    with torch.no_grad():
        cores = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n]
        assert len(cores) == 4
        if case == "tiny_weights":
            for p in cores:
                p.mul_(1e-3)                                  # TT-matrix entries x 1e-12
        elif case == "large_weights":
            for p in cores:
                p.mul_(2.0)                                   # TT-matrix x 16
        elif case == "huge_weights_one_step":
            for p in cores:
                p.mul_(8.0)                                   # TT-matrix x 4096: pre-activations in the hundreds
        elif case == "huge_h0":
            h0 = torch.randn(B, 1024) * torch.tensor([2.0, 300.0, 20000.0]).view(B, 1)
        elif case == "mixed_magnitudes":
            for k, step, f in ((3, 3, 1e-6), (0, 2, 1e-5), (1, 5, 1e-4)):
                w = cores[k].detach().clone().reshape(-1)
                w[::step] *= f
                cores[k].copy_(w.reshape(cores[k].shape))
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    r64, _, c64 = _oracle_forward("ttlstm", sd, 1, x.double(), (h0.double(), c0.double()))
    scale = max(1.0, float(c64.abs().max()), float(r64.abs().max()))
    errs = {}
    for mode in ("exact", "split"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            out, (hT, cT) = m(x.to(dev()), (h0.to(dev()), c0.to(dev())))
        assert torch.isfinite(out).all() and torch.isfinite(cT).all(), (case, mode)
        errs[mode] = max(_maxabs(out.double(), r64), _maxabs(cT.double(), c64))
    print(case, "max abs error vs float64 (state scale %.3g):" % scale, errs)
    tol = 2e-4 if case in ("large_weights", "huge_weights_one_step", "huge_h0") else 2e-6
    assert errs["split"] <= tol * scale
    assert errs["split"] <= 3.0 * errs["exact"] + 2e-7 * scale


def test_big_shape_half_piece_kernel_batch_independent_and_repeatable():
    """The same sample gives the same bits whatever else is in the batch and on every launch (the scales come from the
    weights and from the sample's own h_0 only); the fp32-MFMA pair kernel stays selectable (big_fp32_mfma) and agrees."""
    import ttrnn_hip
    torch.manual_seed(92)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    x = torch.randn(7, 40, 1024, device=dev())
    h0 = torch.randn(7, 1024, device=dev()) * torch.tensor([0.2, 0.5, 1.0, 3.0, 0.1, 50.0, 0.3], device=dev()).view(7, 1)
    c0 = torch.randn(7, 1024, device=dev()) * 0.3
    with torch.no_grad():
        out, (hT, cT) = m(x, (h0, c0))
        out2, (_, cT2) = m(x, (h0, c0))
        sub = [5, 1, 6]
        outs, (_, cTs) = m(x[sub].contiguous(), (h0[sub].contiguous(), c0[sub].contiguous()))
        with ttrnn_hip.option("big_fp32_mfma", 1):
            outf, (_, cTf) = m(x, (h0, c0))
    assert torch.isfinite(out).all()
    assert torch.equal(out, out2) and torch.equal(cT, cT2)
    assert torch.equal(out[sub], outs) and torch.equal(cT[sub], cTs)
    assert not torch.equal(out, outf)                         # a different kernel did run
    assert _maxabs(out, outf) <= 2e-5 and _maxabs(cT, cTf) <= 2e-4      # sample 5 starts from |h_0| ~ 150


def test_big_shape_gradients_vs_oracle():
    """cfg5-class BPTT through the merged two-core matrix (reverse-time kernel with two workgroups per sample, weight
    gradients accumulated in MFMA registers, product rule back to the four cores) against the oracle's autograd: every
    core and bias gradient, the input gradient (batched transposed chain) and the initial-state gradients."""
    from oracle import ttrnn_oracle as O
    torch.manual_seed(57)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    B, T = 3, 5
    x = torch.randn(B, T, 1024)
    h0, c0 = torch.randn(B, 1024) * 0.3, torch.randn(B, 1024) * 0.3
    w = torch.randn(B, T, 1024)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True)
    xr, h0r, c0r = x.clone().requires_grad_(True), h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r))
    ((ro * w).sum() + rc.sum() + 0.5 * rh.sum()).backward()
    xg, h0g, c0g = (t.to(dev()).requires_grad_(True) for t in (x, h0, c0))
    out, (hT, cT) = m(xg, (h0g, c0g))
    ((out * w.to(dev())).sum() + cT.sum() + 0.5 * hT.sum()).backward()
    assert _maxabs(out.detach(), ro.detach()) <= 1e-5
    for name, p in m.named_parameters():
        ref = leaves[name].grad
        assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6), name
    for got, ref in ((xg.grad, xr.grad), (h0g.grad, h0r.grad), (c0g.grad, c0r.grad)):
        assert _maxabs(got, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-6)


def test_big_shape_reverse_kernel_guard_falls_back_on_outlier_weights():
    """The cfg5-class reverse-time kernel carries each transposed merged core under ONE power-of-two scale.  One core entry
    x 1e6 would push the rest of the matrix into fp16's subnormal range; the prep kernel measures the pieces' representation
    error per row, the fp16 kernel steps aside (device counter guard_trips) and the fp32-MFMA pair kernel queued behind it
    runs instead: gradients must be as good as with the fp32-MFMA kernel selected by hand, and an ordinary model must NOT
    trip the guard."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(95)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    B, T = 3, 4
    x = torch.randn(B, T, 1024)
    h0, c0 = torch.randn(B, 1024) * 0.3, torch.randn(B, 1024) * 0.3
    w = torch.randn(B, T, 1024)

    def grads(opts):
        m.zero_grad()
        with contextlib.ExitStack() as stack:
            for k, v in opts.items():
                stack.enter_context(ttrnn_hip.option(k, v))
            xg = x.to(dev()).requires_grad_(True)
            out, (hT, cT) = m(xg, (h0.to(dev()), c0.to(dev())))
            ((out * w.to(dev())).sum() + cT.sum()).backward()
        return {n: p.grad.detach().double().cpu().clone() for n, p in m.named_parameters()}, xg.grad.double().cpu()

    ttrnn_hip.device_status(reset=True)
    grads({})
    assert ttrnn_hip.device_status()["guard_trips"] == 0            # fresh init: the fp16 kernel runs
    with torch.no_grad():
        core = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n][1]
        flat = core.detach().clone().contiguous().view(-1)
        flat[(5 * flat.numel()) // 11] *= 1e6
        core.copy_(flat.view(core.shape))
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr = x.double().clone().requires_grad_(True)
    ro, (rh, rc) = O.lstm_forward(layers, xr, (h0.double(), c0.double()))
    ((ro * w.double()).sum() + rc.sum()).backward()
    got, gx = grads({})
    assert ttrnn_hip.device_status()["guard_trips"] >= 1            # ... and stepped aside here
    ref32, gx32 = grads({"big_fp32_mfma": 1})
    worst = {"guarded": 0.0, "fp32_mfma": 0.0}
    for n, _ in m.named_parameters():
        ref = leaves[n].grad
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        worst["guarded"] = max(worst["guarded"], _maxabs(got[n], ref) / sc)
        worst["fp32_mfma"] = max(worst["fp32_mfma"], _maxabs(ref32[n], ref) / sc)
    sx = max(float(xr.grad.abs().max()), 1e-30)
    worst["guarded"] = max(worst["guarded"], _maxabs(gx, xr.grad) / sx)
    worst["fp32_mfma"] = max(worst["fp32_mfma"], _maxabs(gx32, xr.grad) / sx)
    print("max gradient error relative to each tensor's maximum:", worst)
    assert worst["guarded"] <= 3.0 * worst["fp32_mfma"] + 1e-6


def test_pair_kernel_timeout_poisons_and_is_counted():
    """The two-workgroups-per-sample kernels wait for their partner with a bounded spin.  Option pair_fault launches the
    forward pair kernel one workgroup short (the last sample's partner never runs): that sample must come out as NaN —
    never as a plausible result — the other samples must be untouched, and the event must be visible through
    ttrnn_device_status (counter pair_timeouts), in both math modes (fp16-piece and fp32-MFMA pair kernels)."""
    import ttrnn_hip
    torch.manual_seed(96)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    B, T = 3, 3
    x = torch.randn(B, T, 1024, device=dev())
    for mode in ("split", "exact"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            good, (gh, gc) = m(x)
            ttrnn_hip.device_status(reset=True)
            with ttrnn_hip.option("pair_fault", 1):
                out, (hT, cT) = m(x)
            torch.cuda.synchronize()
        st = ttrnn_hip.device_status(reset=True)
        assert st["pair_timeouts"] > 0, (mode, st)
        assert torch.isnan(hT[B - 1]).any() and torch.isnan(cT[B - 1]).any(), mode
        assert torch.equal(out[:B - 1], good[:B - 1]) and torch.equal(hT[:B - 1], gh[:B - 1]), mode
    with torch.no_grad():
        again, _ = m(x)                                   # the next ordinary launch is unaffected
    assert torch.isfinite(again).all() and ttrnn_hip.device_status()["pair_timeouts"] == 0


@pytest.mark.parametrize("case", ["plain", "decades", "sparse_steps"])
def test_big_shape_half_piece_reverse_kernel_ranges(case):
    """cfg5-class reverse-time kernel in split mode (ttrnn_fast_bigbh.hip): gate gradients have no bound known before the
    launch, so every step the workgroup scales them by a power of two taken from their own maximum before they are split
    into fp16 pieces.  Output gradients spanning ten decades across steps and samples, steps with no gradient at all, and
    plain ones: every parameter / input / initial-state gradient against the float64 oracle's autograd, next to the fp32-MFMA
    pair kernel (option big_fp32_mfma) on the same inputs; bitwise repeatable and independent of the rest of the batch."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(93)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    B, T = 4, 7
    x = torch.randn(B, T, 1024)
    h0, c0 = torch.randn(B, 1024) * 0.3, torch.randn(B, 1024) * 0.3
    w = torch.randn(B, T, 1024)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))          # 1e-6 .. 1e4 per (sample, step)
    elif case == "sparse_steps":
        w[:, 1:5] = 0.0                                           # no output gradient on steps 1..4
        w[2] = 0.0                                                # nor anywhere on sample 2
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r, c0r = (t.double().clone().requires_grad_(True) for t in (x, h0, c0))
    ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r))
    wsum = 0.0 if case == "sparse_steps" else 1.0                 # sparse: sample 2 gets no gradient from the states either
    ((ro * w.double()).sum() + wsum * (rc.sum() + 0.5 * rh.sum())).backward()

    def run(sel=None):
        m.zero_grad()
        xs, hs, cs, ws = (t if sel is None else t[sel] for t in (x, h0, c0, w))
        xg, h0g, c0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (xs, hs, cs))
        out, (hT, cT) = m(xg, (h0g, c0g))
        ((out * ws.to(dev())).sum() + wsum * (cT.sum() + 0.5 * hT.sum())).backward()
        return {"x": xg.grad.clone(), "h0": h0g.grad.clone(), "c0": c0g.grad.clone(),
                **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}

    got = run()
    again = run()
    with ttrnn_hip.option("big_fp32_mfma", 1):
        fp32 = run()
    sub = run([2, 0])
    refs = {"x": xr.grad, "h0": h0r.grad, "c0": c0r.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    worst = {"split": 0.0, "fp32_mfma": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        worst["split"] = max(worst["split"], _maxabs(got[n].double(), ref) / sc)
        worst["fp32_mfma"] = max(worst["fp32_mfma"], _maxabs(fp32[n].double(), ref) / sc)
    for n in ("x", "h0", "c0"):        # the reverse-time kernel's own results: repeatable, independent of the rest of the batch
        assert torch.equal(got[n], again[n]), n                   # (bias / core gradients are flushed with atomics)
        assert torch.equal(got[n][[2, 0]], sub[n]), n
    if case == "sparse_steps":
        assert float(got["x"][2].abs().max()) == 0.0 and float(got["h0"][2].abs().max()) == 0.0
    print(case, "max gradient error relative to each tensor's maximum:", worst)
    assert not torch.equal(got["h0"], fp32["h0"])                 # a different kernel did run
    assert worst["split"] <= 2e-5 and worst["split"] <= 3.0 * worst["fp32_mfma"] + 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_big_shape_backward_kernels_agree(dtype):
    """The cfg5-class backward paths on the same module and inputs: pair reverse-time kernel + weight gradients through the
    dense-gradient GEMM and its projections (default); one workgroup per sample + the per-row merged-chain weight-gradient
    kernel (TTRNN_BIG_NO_PAIR=1, TTRNN_BIGW_SLICES=1; B*T = 260 > 64 row chunks); any-shape kernels (TTRNN_NO_BIGB=1).
    No input gradient, zero initial state."""
    import os
    torch.manual_seed(58)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev()).to(dtype)
    B, T = 20, 13
    x = torch.randn(B, T, 1024, device=dev()).to(dtype)
    w = torch.randn(B, T, 1024, device=dev())
    res = []
    try:
        for env in ({}, {"TTRNN_BIG_NO_PAIR": "1", "TTRNN_BIGW_SLICES": "1"}, {"TTRNN_NO_BIGB": "1"}):
            OPT.update(env)
            m.zero_grad()
            out, (hT, cT) = m(x)
            ((out.float() * w).sum() + cT.float().sum()).backward()
            res.append([p.grad.float().clone() for p in m.parameters()])
            for k in env:
                OPT.pop(k)
    finally:
        for k in ("TTRNN_BIG_NO_PAIR", "TTRNN_BIGW_SLICES", "TTRNN_NO_BIGB"):
            OPT.pop(k, None)
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    for (name, _), a, b, c in zip(m.named_parameters(), *res):
        scale = max(float(c.abs().max()), 1e-6)
        assert _maxabs(a, c) <= tol * scale, ("pair", name)
        assert _maxabs(b, c) <= tol * scale, ("single", name)


def test_big_shape_ttlinear_backward_vs_oracle():
    """Standalone TTLinear of the cfg5 matrix (1024 -> 4096, d = 4, r = 32): dx, core and bias gradients of the merged-core
    kernels against the oracle's autograd over 70 rows, then dx alone with frozen weights."""
    from oracle import ttrnn_oracle as O
    from t3nsor.layers import TTLinear
    torch.manual_seed(59)
    lin = TTLinear(out_features=4096, shape=[[4, 4, 8, 8], [8, 8, 8, 8]], bias=True, auto_shapes=False, d=4,
                   tt_rank=32).to(dev())
    x = torch.randn(70, 1024)
    w = torch.randn(70, 4096)
    cores = [c.detach().cpu().clone().requires_grad_(True) for c in lin.weight_t.tt_cores]
    bias = lin.bias.detach().cpu().clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    (O.ttlinear(cores, bias, xr) * w).sum().backward()
    xg = x.to(dev()).requires_grad_(True)
    y = lin(xg)
    (y * w.to(dev())).sum().backward()
    assert _maxabs(xg.grad, xr.grad) <= 1e-4 * float(xr.grad.abs().max())
    for k in range(4):
        assert _maxabs(lin.weight_t.tt_cores[k].grad, cores[k].grad) <= 1e-4 * float(cores[k].grad.abs().max()), k
    assert _maxabs(lin.bias.grad, bias.grad) <= 1e-4 * float(bias.grad.abs().max())
    for p in lin.parameters():
        p.requires_grad_(False)
    xg2 = x.to(dev()).requires_grad_(True)
    (lin(xg2) * w.to(dev())).sum().backward()
    assert _maxabs(xg2.grad, xr.grad) <= 1e-4 * float(xr.grad.abs().max())


def test_dense_gemm_paths_switch_off_matches():
    """TTRNN_NO_GEMM=1 (input projections, weight gradients and dx row by row through the TT chain kernels) against the
    dense-GEMM paths on the same 3-layer cfg4-shaped module over 1 300 rows: forward, dx and every parameter gradient."""
    import os
    torch.manual_seed(91)
    meta = dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=3, n_cores=3, tt_rank=16)
    m = build_module(meta, dev())
    x = torch.rand(50, 26, 40, device=dev())
    w = torch.randn(50, 26, 256, device=dev())
    res = []
    for flag in ("0", "1"):
        OPT["TTRNN_NO_GEMM"] = flag
        try:
            m.zero_grad()
            xg = x.clone().requires_grad_(True)
            out, (h, c) = m(xg)
            ((out * w).sum() + c.sum()).backward()
            res.append((out.detach().clone(), xg.grad.clone(), [p.grad.clone() for p in m.parameters()]))
        finally:
            OPT.pop("TTRNN_NO_GEMM", None)
    assert _maxabs(res[0][0], res[1][0]) <= 5e-6
    assert _maxabs(res[0][1], res[1][1]) <= 1e-4 * max(1e-3, float(res[1][1].abs().max()))
    for (name, _), a, b in zip(m.named_parameters(), res[0][2], res[1][2]):
        assert _maxabs(a, b) <= 1e-4 * max(float(b.abs().max()), 1e-6), name


def test_dense_gradient_path_bf16_gru_vs_chain():
    """bf16-storage TT-GRU (cfg3 shape) over 1 280 rows: weight gradients through the dense gradient (bf16 x rows, fp32
    gate gradients) against the row-by-row fused-core kernel."""
    import os
    torch.manual_seed(92)
    meta = dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8)
    m = build_module(meta, dev()).to(torch.bfloat16)
    x = torch.rand(40, 32, 1, device=dev()).to(torch.bfloat16)
    res = []
    for flag in ("0", "1"):
        OPT["TTRNN_NO_GEMM"] = flag
        try:
            m.zero_grad()
            out, h = m(x)
            out.float().square().sum().backward()
            res.append([p.grad.float().clone() for p in m.parameters()])
        finally:
            OPT.pop("TTRNN_NO_GEMM", None)
    for (name, _), a, b in zip(m.named_parameters(), *res):
        assert _maxabs(a, b) <= 2e-2 * max(float(b.abs().max()), 1e-6), name


@pytest.mark.parametrize("rank,inp", [(16, 40), (8, 1)])
def test_two_samples_per_workgroup_matches_one(rank, inp):
    """More samples than CUs: the fused-core forward kernel carries two samples per workgroup (B = 301: the last workgroup
    has a single live sample).  Against one sample per workgroup (TTRNN_F10_NB1=1) on the same module: outputs and final
    states bit for bit (same arithmetic per sample), and the gradients computed from the reserve it wrote."""
    import os
    torch.manual_seed(93)
    meta = dict(kind="ttlstm", input_size=inp, hidden_size=256, num_layers=2, n_cores=3, tt_rank=rank)
    m = build_module(meta, dev())
    B, T = 301, 9
    x = torch.rand(B, T, inp, device=dev())
    h0, c0 = torch.randn(B, 256, device=dev()) * 0.3, torch.randn(B, 256, device=dev()) * 0.3
    w = torch.randn(B, T, 256, device=dev())
    res = []
    for flag in ("0", "1"):
        OPT["TTRNN_F10_NB1"] = flag
        try:
            m.zero_grad()
            out, (h, c) = m(x, (h0, c0))
            ((out * w).sum() + c.sum()).backward()
            res.append((out.detach().clone(), h.detach().clone(), c.detach().clone(), [p.grad.clone() for p in m.parameters()]))
        finally:
            OPT.pop("TTRNN_F10_NB1", None)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    for a, b in zip(res[0][3], res[1][3]):
        assert _maxabs(a, b) <= 1e-4 * max(float(b.abs().max()), 1e-6)


def test_dense_gemm_paths_gru_two_layers():
    """Two stacked fp32 TT-GRU layers over 1 150 rows: the second layer's hidden-shaped input matrix takes the dense-gradient
    GEMM (out = 768: three 256-column tiles) and the dx GEMM with K = 768, M = 256 (two feature tiles: the plain, not the
    XCD-blocked, tile order) — against the row-by-row chain kernels (TTRNN_NO_GEMM=1)."""
    import os
    torch.manual_seed(94)
    meta = dict(kind="ttgru", input_size=40, hidden_size=256, num_layers=2, n_cores=3, tt_rank=8)
    m = build_module(meta, dev())
    x = torch.rand(46, 25, 40, device=dev())
    w = torch.randn(46, 25, 256, device=dev())
    res = []
    for flag in ("0", "1"):
        OPT["TTRNN_NO_GEMM"] = flag
        try:
            m.zero_grad()
            xg = x.clone().requires_grad_(True)
            out, h = m(xg)
            ((out * w).sum() + h.sum()).backward()
            res.append((out.detach().clone(), xg.grad.clone(), [p.grad.clone() for p in m.parameters()]))
        finally:
            OPT.pop("TTRNN_NO_GEMM", None)
    assert _maxabs(res[0][0], res[1][0]) <= 5e-6
    assert _maxabs(res[0][1], res[1][1]) <= 1e-4 * max(1e-3, float(res[1][1].abs().max()))
    for (name, _), a, b in zip(m.named_parameters(), res[0][2], res[1][2]):
        assert _maxabs(a, b) <= 1e-4 * max(float(b.abs().max()), 1e-6), name


def test_dense_gemm_error_vs_fp64_is_fp32_class():
    """3-layer cfg4-shaped model over 2 560 rows (input projections as dense split-bf16 GEMMs, one accumulator per tile)
    against the oracle evaluated in float64: as close as the fp32-MFMA chain kernels and the torch-CPU fp32 oracle."""
    import ttrnn_hip
    torch.manual_seed(95)
    meta = dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=3, n_cores=3, tt_rank=16)
    m = build_module(meta, dev())
    x = torch.rand(64, 40, 40)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, _, c64 = _oracle_forward("ttlstm", sd, 3, x.double())
    r32, _, c32 = _oracle_forward("ttlstm", sd, 3, x)
    errs = {"cpu_fp32": max(_maxabs(r32, r64), _maxabs(c32, c64))}
    for mode in ("exact", "split"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            out, (hT, cT) = m(x.to(dev()))
        errs[mode] = max(_maxabs(out, r64), _maxabs(cT, c64))
    print("max abs error vs float64 oracle:", errs)
    assert errs["split"] <= 2e-6 and errs["exact"] <= 2e-6
    assert errs["split"] <= 2.0 * max(errs["exact"], errs["cpu_fp32"]) + 1e-7


# ---- (12) by-products of the reverse-time kernels feeding the weight-gradient step --------------------------------------------
@pytest.mark.parametrize("kind,inp,H,d,L,r,B,T,dtype,with_h0", [
    ("ttlstm", 1, 256, 3, 1, 8, 9, 33, "f32", False),          # cfg2 class: in1 sums + column maxima
    ("ttlstm", 1, 256, 3, 1, 8, 70, 20, "f32", True),          # dense hidden gradient (B*T >= 4*H)
    ("ttgru", 1, 256, 3, 1, 8, 9, 33, "f32", False),
    ("ttgru", 1, 256, 3, 1, 8, 70, 20, "bf16", False),         # cfg3 class
    ("ttgru", 1, 256, 3, 1, 8, 70, 20, "f32", True),           # h0 given, entries up to ~60: the state bound is max(1, |h0|)
    ("ttlstm", 40, 256, 3, 2, 16, 48, 27, "f32", False),       # cfg4 class: maxima only, stacked layer's input bounded by 1
    ("ttlstm", 40, 512, 3, 1, 8, 32, 40, "f32", False),         # runtime-shape tier (the reference's default size): maxima kept in LDS
    ("ttgru", 28, 128, 3, 2, 4, 40, 30, "f32", True),          # runtime-shape tier, GRU (rows 0 and 1 differ in the n gate), two layers
    ("ttlstm", 1024, 1024, 4, 1, 32, 4, 24, "f32", False),     # cfg5 class: merged-big reverse kernels (pair, fp16 pieces)
    ("ttlstm", 1024, 1024, 4, 1, 32, 3, 10, "bf16", False),
])
def test_reverse_kernel_by_products_feed_the_weight_gradients(kind, inp, H, d, L, r, B, T, dtype, with_h0):
    """ttrnn_rnn_backward_ex (include/ttrnn.h): the fused-core reverse-time kernels return the column maxima of the gate
    gradients and, for input_size == 1, sum_n x[n] dg[n] and sum_n dg[n].  (a) The rows are what torch computes from the
    returned gate gradients — the maxima bit for bit; (b) every parameter gradient with the by-products in use
    (ttrnn_ttlinear_backward_hinted: no in1 reduction pass, two-piece fp16 dense gradient under the producer's column
    bounds) is as close to the float64 oracle as without them; (c) the two paths did differ (the switch works)."""
    import ttrnn_hip.functional as F
    from oracle import ttrnn_oracle as O
    torch.manual_seed(5 + B + T)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=d, tt_rank=r)
    m = build_module(meta, dev())
    x = torch.randn(B, T, inp) * 0.7
    w = torch.randn(B, T, H)
    h0 = torch.randn(B, H) * 0.5 if with_h0 else None
    if with_h0:
        h0[:, ::37] *= 40.0                # far outside (-1, 1): rows 0 of the hidden matrix's operand (a bound of 1 would overflow)
    if dtype == "bf16":
        m = m.to(torch.bfloat16)
        x = x.to(torch.bfloat16)
        h0 = h0.to(torch.bfloat16) if h0 is not None else None
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, L, requires_grad=True, dtype=torch.float64)
    if kind == "ttlstm":
        init = (h0.double(), torch.zeros(B, H, dtype=torch.float64)) if with_h0 else None
        ro, _ = O.lstm_forward(layers, x.double(), init)
    else:
        ro, _ = O.gru_forward(layers, x.double(), h0.double() if with_h0 else None)
    (ro * w.double()).sum().backward()
    grads = {}
    captured = []
    for use in (True, False):
        F.USE_BWD_STATS = use
        F.DEBUG_BWD_STATS = captured if use else None
        try:
            m.zero_grad()
            if kind == "ttlstm":
                init = (h0.to(dev()), torch.zeros(B, H, device=dev(), dtype=x.dtype)) if with_h0 else None
                out = m(x.to(dev()), init)[0]
            else:
                out = m(x.to(dev()), h0.to(dev()) if with_h0 else None)[0]
            (out.float() * w.to(dev())).sum().backward()
            torch.cuda.synchronize()
        finally:
            F.USE_BWD_STATS = True
            F.DEBUG_BWD_STATS = None
        grads[use] = {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}
    # (a) the rows against torch reductions of the returned gate gradients (layers run last to first)
    assert len(captured) == L
    for li, (mask, stats, dg_in, dg_hid, rowmax) in zip(reversed(range(L)), captured):
        assert mask & 1, "the fused-core reverse kernel should deliver the column maxima for this shape"
        GH = dg_in.shape[-1]
        assert torch.equal(stats[0], dg_in.reshape(-1, GH).abs().amax(0))
        assert torch.equal(stats[1], dg_hid.reshape(-1, GH).abs().amax(0))
        # TTRNN_BWD_STATS_ROWMAX (two-piece TT-LSTM kernel): every row's maximum, bit for bit — the dx GEMM's row scales
        assert (rowmax is not None) == bool(mask & 4)
        assert rowmax is not None or not (kind == "ttlstm" and H == 256 and dtype == "f32")
        if rowmax is not None:
            assert torch.equal(rowmax, dg_in.reshape(-1, GH).abs().amax(1))
        if inp == 1 and li == 0:
            assert mask & 2
            xs = x.to(dev()).double().reshape(-1, 1)
            ref2 = (xs * dg_in.reshape(-1, GH).double()).sum(0)
            ref3 = dg_in.reshape(-1, GH).double().sum(0)
            mag = float((xs.abs() * dg_in.reshape(-1, GH).double().abs()).sum(0).max())
            assert _maxabs(stats[2].double(), ref2) <= 2e-6 * mag
            assert _maxabs(stats[3].double(), ref3) <= 2e-6 * float(dg_in.reshape(-1, GH).double().abs().sum(0).max())
    # (b), (c)
    worst = {True: 0.0, False: 0.0}
    differ = False
    for n, _ in m.named_parameters():
        ref = leaves[n].grad
        sc = max(float(ref.abs().max()), 1e-30)
        for k in worst:
            assert torch.isfinite(grads[k][n]).all(), (k, n)
            worst[k] = max(worst[k], _maxabs(grads[k][n].double(), ref) / sc)
        differ = differ or not torch.equal(grads[True][n], grads[False][n])
    print(kind, inp, dtype, "max gradient error relative to each tensor's maximum: with by-products %.3g, without %.3g"
          % (worst[True], worst[False]))
    # (the big shape's dense gradients take the two-piece variant from 2^36 multiply-adds on by themselves; at this test's
    # size the by-products switch them from three bf16 pieces to two fp16 pieces, as for the small shapes)
    # (rounding the gradients to bf16 can hide the difference; and where G*H is no multiple of the split dense gradient's 256-column
    # tile — the GRU of H = 128: 384 — the gradient runs on the fp32 MFMA with or without bounds: since round 4, when the bias
    # sums stopped going through atomics, the two runs are then equal bit for bit)
    n_gate_cols = (4 if kind == "ttlstm" else 3) * H
    assert differ or dtype == "bf16" or n_gate_cols % 256 != 0
    assert worst[True] <= (5e-2 if dtype == "bf16" else 2e-4) and worst[True] <= 3.0 * worst[False] + 1e-6


@pytest.mark.parametrize("kind,inp,H,d,L,r,B,T,dtype,with_h0,expect_shift", [
    ("ttlstm", 1, 256, 3, 1, 8, 40, 35, "f32", False, True),
    ("ttlstm", 1, 256, 3, 1, 8, 40, 35, "f32", True, True),
    ("ttgru", 1, 256, 3, 1, 8, 37, 40, "f32", True, True),        # h0 rows enter the column-maximum pass
    ("ttgru", 1, 256, 3, 1, 8, 37, 40, "bf16", True, True),
    ("ttlstm", 40, 256, 3, 2, 16, 30, 43, "f32", False, True),
    ("ttlstm", 1024, 1024, 4, 1, 32, 3, 33, "f32", True, False),  # merged-big route: honoured, not advertised (slower)
    ("ttlstm", 16, 64, 2, 1, 4, 30, 41, "f32", True, True),       # runtime-shape tier: any-shape dense gradient
    ("ttlstm", 1, 256, 3, 1, 8, 70, 20, "f32", True, False),      # sequences shorter than a 32-row chunk: rows materialised
    ("ttlstm", 1, 256, 3, 1, 8, 5, 37, "f32", True, False),       # few rows: the per-row kernels, rows materialised
])
def test_hidden_weight_gradient_reads_previous_states_in_place(kind, inp, H, d, L, r, B, T, dtype, with_h0, expect_shift):
    """hints x_period / x_first (include/ttrnn.h: ttrnn_lin_hints): the dense-gradient routes read the h_{t-1} rows of the
    hidden matrix's weight gradient from the layer's outputs (row n - 1; h_0 or zeros at the sequence starts) instead of a
    materialised [h_0, out[:, :-1]].  Same kernels on the same values: every gradient agrees with the one the materialised
    rows give to the run-to-run noise of the float atomics downstream; ttrnn_ttlinear_backward_shift_ok says which calls
    take such a route."""
    import ctypes
    import ttrnn_hip.functional as F
    from ttrnn_hip import _lib
    torch.manual_seed(3 + B + T)
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=L, n_cores=d, tt_rank=r)
    m = build_module(meta, dev())
    x = torch.randn(B, T, inp) * 0.7
    w = torch.randn(B, T, H)
    h0 = torch.randn(B, H) * 1.5 if with_h0 else None
    if dtype == "bf16":
        m = m.to(torch.bfloat16)
        x = x.to(torch.bfloat16)
        h0 = h0.to(torch.bfloat16) if h0 is not None else None
    cell = m._all_layers[-1]
    ok = _lib.load().ttrnn_ttlinear_backward_shift_ok(ctypes.byref(cell._layer_spec().hid_spec.desc),
                                                      _lib.TTRNN_BF16 if dtype == "bf16" else _lib.TTRNN_F32, _lib.TTRNN_F32,
                                                      B * T, T, 0)
    assert bool(ok) == expect_shift
    grads = {}
    for use in (True, False):
        F.USE_ROW_SHIFT = use
        try:
            m.zero_grad()
            if kind == "ttlstm":
                init = (h0.to(dev()), torch.zeros(B, H, device=dev(), dtype=x.dtype)) if with_h0 else None
                out = m(x.to(dev()), init)[0]
            else:
                out = m(x.to(dev()), h0.to(dev()) if with_h0 else None)[0]
            (out.float() * w.to(dev())).sum().backward()
            torch.cuda.synchronize()
        finally:
            F.USE_ROW_SHIFT = True
        grads[use] = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    for n in grads[True]:
        assert torch.isfinite(grads[True][n].float()).all(), n
        # (not bitwise: bias column sums and core-gradient partial sums leave their workgroups through float atomics, whose
        # order varies from launch to launch; a wrong row anywhere would show at the 1e-2 level)
        sc = max(float(grads[False][n].float().abs().max()), 1e-30)
        assert _maxabs(grads[True][n].float(), grads[False][n].float()) <= (1e-2 if dtype == "bf16" else 1e-5) * sc, n


@pytest.mark.parametrize("with_h0", [False, True])
def test_big_shape_dense_gradient_honours_row_shift_when_asked(with_h0):
    """The merged-big TTLinear backward reads shifted rows when the hints ask for it (ttrnn_ttlinear_backward_shift_ok does
    not advertise it there: measured slower than the materialised copy on cfg5) — same gradients as the materialised rows."""
    import ttrnn_hip.functional as F
    torch.manual_seed(9)
    meta = dict(kind="ttlstm", input_size=1024, hidden_size=1024, num_layers=1, n_cores=4, tt_rank=32)
    m = build_module(meta, dev())
    cell = m._all_layers[0]
    spec = cell._layer_spec().hid_spec
    cin, bin_, chid, bhid = cell._operands()
    B, T, H = 3, 40, 1024
    out = torch.tanh(torch.randn(B, T, H, device=dev()))
    h0 = torch.randn(B, H, device=dev()) if with_h0 else None
    dy = torch.randn(B * T, 4 * H, device=dev()) * 0.1
    packed = spec.pack(list(chid))
    first = h0 if with_h0 else torch.zeros(B, H, device=dev())
    hprev = torch.cat([first.unsqueeze(1), out[:, :-1]], dim=1).reshape(B * T, H).contiguous()
    _, ref, _ = F._ttlinear_backward(spec, packed, hprev, dy, False, True, False)
    _, got, _ = F._ttlinear_backward(spec, packed, out.reshape(B * T, H), dy, False, True, False,
                                     hints={"x_period": T, "x_first": h0})
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert _maxabs(got, ref) <= 1e-5 * float(ref.abs().max())


# ---- (13) fused-core reverse-time kernel on two fp16 pieces (ttrnn_fast_f10bh.hip) ------------------------------------------------
@pytest.mark.parametrize("rank,inp", [(8, 1), (16, 40)])
@pytest.mark.parametrize("case", ["plain", "decades", "sparse_steps", "last_step_only"])
def test_fused_core_half_piece_reverse_kernel_ranges(case, rank, inp):
    """cfg2 / cfg4-class reverse-time kernel in split mode: the weights' rows carry their own power-of-two scales, every
    step's gate gradients are scaled from their exact maximum and T01's results from a bound (no overflow possible).
    Output gradients spanning ten decades across steps and samples, steps with no gradient at all, a loss on the last step
    only (the gradient decays over 60 steps) and plain ones: every parameter / input / initial-state gradient against the
    float64 oracle's autograd, next to the three-bf16-piece kernel (option gemm_pieces = 3) on the same inputs; the kernel's
    own results bitwise repeatable and independent of the rest of the batch."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(193 + rank)
    H = 256
    meta = dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=rank)
    m = build_module(meta, dev())
    B, T = 5, (60 if case == "last_step_only" else 9)
    x = torch.randn(B, T, inp)
    h0, c0 = torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))          # 1e-6 .. 1e4 per (sample, step)
    elif case == "sparse_steps":
        w[:, 1:5] = 0.0
        w[2] = 0.0
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r, c0r = (t.double().clone().requires_grad_(True) for t in (x, h0, c0))
    ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r))
    wsum = 0.0 if case in ("sparse_steps", "last_step_only") else 1.0
    ((ro * w.double()).sum() + wsum * (rc.sum() + 0.5 * rh.sum())).backward()

    def run(sel=None):
        m.zero_grad()
        xs, hs, cs, ws = (t if sel is None else t[sel] for t in (x, h0, c0, w))
        xg, h0g, c0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (xs, hs, cs))
        out, (hT, cT) = m(xg, (h0g, c0g))
        ((out * ws.to(dev())).sum() + wsum * (cT.sum() + 0.5 * hT.sum())).backward()
        return {"x": xg.grad.clone(), "h0": h0g.grad.clone(), "c0": c0g.grad.clone(),
                **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}

    got = run()
    again = run()
    with ttrnn_hip.option("gemm_pieces", 3):
        three = run()
    sub = run([2, 0])
    refs = {"x": xr.grad, "h0": h0r.grad, "c0": c0r.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    worst = {"two_fp16": 0.0, "three_bf16": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        worst["two_fp16"] = max(worst["two_fp16"], _maxabs(got[n].double(), ref) / sc)
        worst["three_bf16"] = max(worst["three_bf16"], _maxabs(three[n].double(), ref) / sc)
    for n in ("h0", "c0") + (("x",) if inp != 1 else ()):          # the reverse-time kernel's own results
        assert torch.equal(got[n], again[n]), n
        assert torch.equal(got[n][[2, 0]], sub[n]), n
    if case == "sparse_steps":
        assert float(got["h0"][2].abs().max()) == 0.0
    if case == "last_step_only":       # sixty steps back the gradient is many decades down, and still what float64 gives
        rel = _maxabs(got["h0"].double(), h0r.grad) / max(float(h0r.grad.abs().max()), 1e-300)
        print("d_h0 after 60 steps: max |ref| %.3g, relative error %.3g" % (float(h0r.grad.abs().max()), rel))
        assert rel <= 1e-4
    print(case, rank, "max gradient error relative to each tensor's maximum:", worst)
    assert not torch.equal(got["h0"], three["h0"])                 # a different kernel did run
    assert worst["two_fp16"] <= 2e-5 and worst["two_fp16"] <= 3.0 * worst["three_bf16"] + 1e-6


@pytest.mark.parametrize("rank", [8, 16])
@pytest.mark.parametrize("which,factor", [(2, 1e7), (1, 1e5), (0, 1e6)])
def test_fused_core_half_piece_reverse_kernel_outlier_weights(rank, which, factor):
    """The two-piece kernel scales every ROW of W10 and of G2 by its own power of two: one huge core entry costs only the rows it
    touches, and inside such a row the small entries keep an absolute error of 2^-25 of the row's maximum — the error bound of an
    fp32 dot product with that row, so no guard is needed (ttrnn_fast_f10bh.hip).  One entry of each hidden core in turn x 1e5
    ... 1e7: every gradient as close to the float64 oracle as the three-bf16-piece kernel's."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(195)
    H = 256
    meta = dict(kind="ttlstm", input_size=1, hidden_size=H, num_layers=1, n_cores=3, tt_rank=rank)
    m = build_module(meta, dev())
    B, T = 3, 6
    x = torch.randn(B, T, 1)
    w = torch.randn(B, T, H)

    def grads(opts):
        m.zero_grad()
        with contextlib.ExitStack() as stack:
            for k, v in opts.items():
                stack.enter_context(ttrnn_hip.option(k, v))
            out, (hT, cT) = m(x.to(dev()))
            ((out * w.to(dev())).sum() + cT.sum()).backward()
        return {n: p.grad.detach().double().cpu().clone() for n, p in m.named_parameters()}

    with torch.no_grad():
        core = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n][which]
        flat = core.detach().clone().contiguous().view(-1)
        flat[(5 * flat.numel()) // 11] *= factor
        core.copy_(flat.view(core.shape))
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    ro, (rh, rc) = O.lstm_forward(layers, x.double(), None)
    ((ro * w.double()).sum() + rc.sum()).backward()
    got = grads({})
    three = grads({"gemm_pieces": 3})
    worst = {"two_fp16": 0.0, "three_bf16": 0.0}
    for n, _ in m.named_parameters():
        ref = leaves[n].grad
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        worst["two_fp16"] = max(worst["two_fp16"], _maxabs(got[n], ref) / sc)
        worst["three_bf16"] = max(worst["three_bf16"], _maxabs(three[n], ref) / sc)
    print("core", which, "x", factor, "rank", rank, "max gradient error relative to each tensor's maximum:", worst)
    assert worst["two_fp16"] <= 3.0 * worst["three_bf16"] + 1e-6


@pytest.mark.parametrize("inp", [1, 24])
@pytest.mark.parametrize("case", ["plain", "decades", "last_step_only"])
def test_fused_core_gru_reverse_kernel_rank_16(case, inp):
    """round 6: `benchmarking.py --hidden_size 256 --gru --ttrank 16` — the TT-GRU of rank 16 on the two-piece
    fused-core reverse-time kernel (k_gru_bwd_f10h<ShpH256R16G>: twelve T2 pairs, two per wave on waves 0-3) instead of the stage-wise
    kernel; against the float64 oracle and against the route it replaces (option gru_r16_bwd_on_tier) reading the same forward records."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    from oracle import ttrnn_oracle as O
    torch.manual_seed(311)
    H = 256
    meta = dict(kind="ttgru", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=16)
    m = build_module(meta, dev())
    B, T = 5, (50 if case == "last_step_only" else 9)
    x = torch.randn(B, T, inp)
    h0 = torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_backward_route(spec, B, T) == "fused_core"
    with ttrnn_hip.option("gru_r16_bwd_on_tier", 1):
        assert F.rnn_backward_route(spec, B, T) != "fused_core"
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r = (t.double().clone().requires_grad_(True) for t in (x, h0))
    ro, rh = O.gru_forward(layers, xr, h0r)
    wsum = 0.0 if case == "last_step_only" else 1.0
    ((ro * w.double()).sum() + wsum * 0.5 * rh.sum()).backward()

    def run():
        m.zero_grad()
        xg, h0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (x, h0))
        out, hT = m(xg, h0g)
        ((out * w.to(dev())).sum() + wsum * 0.5 * hT.sum()).backward()
        return {"h0": h0g.grad.clone(), "x": xg.grad.clone(), **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}

    got = run()
    again = run()
    with ttrnn_hip.option("gru_r16_bwd_on_tier", 1):
        old = run()
    refs = {"h0": h0r.grad, "x": xr.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    worst = {"fused": 0.0, "replaced": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        worst["fused"] = max(worst["fused"], _maxabs(got[n].double(), ref) / sc)
        worst["replaced"] = max(worst["replaced"], _maxabs(old[n].double(), ref) / sc)
    assert torch.equal(got["h0"], again["h0"])
    print(case, inp, "max gradient error relative to each tensor's maximum:", worst)
    assert worst["fused"] <= 2e-5 and worst["fused"] <= 3.0 * worst["replaced"] + 1e-6


@pytest.mark.parametrize("kind", ["ttlstm", "ttgru"])
@pytest.mark.parametrize("case", ["plain", "decades", "sparse_steps", "last_step_only", "no_state", "outlier", "bench_size"])
def test_naive_sets_reverse_kernel(kind, case):
    """round 6: the naive per-gate sets of H = 256, d = 3, r = 8 (tt_linearset.py:5-38; pMNIST --naive_tt [--gru])
    on a reverse-time kernel of their own — k_rnn_bwd_f10n: T01 per gate on the gate's fused core, T2 over all gates' k-blocks — instead
    of the tier's kernel on the joint matrix.  Every gradient against the float64 oracle (per-gate evaluation) and against the route
    it replaces (option naive_bwd_on_tier) reading the same forward records; output gradients over ten decades, steps and samples without
    gradient, a loss on the last step only, no initial state, one core entry x 1e3, and the benchmark's size (B = 64, T = 784:
    against the tier, and twice for the bits)."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    from oracle import ttrnn_oracle as O
    torch.manual_seed(331)
    H, inp = 256, (1 if case == "bench_size" else 24)
    lstm = kind == "ttlstm"
    meta = dict(kind=kind, input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=8, is_naive=True)
    m = build_module(meta, dev())
    if case == "outlier":
        cores = [p for n, p in m.named_parameters() if "hidden_weights" in n and p.dim() > 1]
        with torch.no_grad():
            flat = cores[-1].detach().clone().contiguous().view(-1)
            flat[(5 * flat.numel()) // 11] *= 1e3
            cores[-1].copy_(flat.view(cores[-1].shape))
    B, T = (64, 784) if case == "bench_size" else (5, 40 if case == "last_step_only" else 9)
    x = torch.randn(B, T, inp)
    state = case != "no_state"
    h0 = torch.randn(B, H) * 0.3 if state else None
    c0 = torch.randn(B, H) * 0.3 if (state and lstm) else None
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))
    elif case == "sparse_steps":
        w[:, 1:5] = 0.0
        w[2] = 0.0
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    wsum = 0.0 if case in ("sparse_steps", "last_step_only") else 1.0
    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_backward_route(spec, B, T) == "fused_core"

    def run():
        m.zero_grad()
        xg = x.to(dev()).contiguous().requires_grad_(True)
        h0g = None if h0 is None else h0.to(dev()).contiguous().requires_grad_(True)
        c0g = None if c0 is None else c0.to(dev()).contiguous().requires_grad_(True)
        if lstm:
            out, (hT, cT) = m(xg, None if h0g is None else (h0g, c0g))
            loss = (out * w.to(dev())).sum() + wsum * (cT.sum() + 0.5 * hT.sum())
        else:
            out, hT = m(xg, h0g)
            loss = (out * w.to(dev())).sum() + wsum * 0.5 * hT.sum()
        loss.backward()
        g = {"x": xg.grad.clone(), **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}
        if h0g is not None:
            g["h0"] = h0g.grad.clone()
        if c0g is not None:
            g["c0"] = c0g.grad.clone()
        return g

    got, again = run(), run()
    with ttrnn_hip.option("naive_bwd_on_tier", 1):
        assert F.rnn_backward_route(spec, B, T) == "runtime_mfma"
        old = run()
    for n in got:
        assert torch.isfinite(got[n]).all(), n
        assert torch.equal(got[n], again[n]) or n not in ("x", "h0", "c0"), n      # the reverse kernel's own results: bit for bit
    if case == "sparse_steps" and state:
        assert float(got["h0"][2].abs().max()) == 0.0
    if case == "bench_size":
        for n in got:
            sc = max(float(old[n].abs().max()), 1e-30)
            assert _maxabs(got[n], old[n]) <= 2e-4 * sc, (n, _maxabs(got[n], old[n]) / sc)
        return
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr = x.double().clone().requires_grad_(True)
    h0r = None if h0 is None else h0.double().clone().requires_grad_(True)
    c0r = None if c0 is None else c0.double().clone().requires_grad_(True)
    if lstm:
        ro, (rh, rc) = O.lstm_forward(layers, xr, None if h0r is None else (h0r, c0r))
        ((ro * w.double()).sum() + wsum * (rc.sum() + 0.5 * rh.sum())).backward()
    else:
        ro, rh = O.gru_forward(layers, xr, h0r)
        ((ro * w.double()).sum() + wsum * 0.5 * rh.sum()).backward()
    refs = {"x": xr.grad}
    for n, _ in m.named_parameters():
        key = n.replace(".gate", ".gates.")        # gate{i} (attribute) and gates.{i} (ModuleList) are the same Parameters
        if key in leaves and leaves[key].grad is not None:
            refs[n] = leaves[key].grad
    assert len(refs) >= 1 + 2 * 3 * (4 if lstm else 3)
    if h0r is not None:
        refs["h0"] = h0r.grad
    if c0r is not None:
        refs["c0"] = c0r.grad
    worst = {"fused": 0.0, "replaced": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        worst["fused"] = max(worst["fused"], _maxabs(got[n].double(), ref) / sc)
        worst["replaced"] = max(worst["replaced"], _maxabs(old[n].double(), ref) / sc)
    print(kind, case, "max gradient error relative to each tensor's maximum:", worst)
    tol = 5e-3 if case == "outlier" else 2e-5
    assert worst["fused"] <= tol and worst["fused"] <= 3.0 * worst["replaced"] + 1e-6


@pytest.mark.parametrize("case", ["plain", "decades", "last_step_only", "no_h0"])
def test_fused_core_gru_reverse_kernel_h512(case):
    """round 6: the reference's benchmark defaults with --gru (TT-GRU in = 256, H = 512, d = 3, r = 8) — the
    reverse-time recurrence on k_gru_bwd_f10h<ShpH512R8G> (eight gate waves, K1 = 96, sixteen T2 pairs) instead of the tier's kernel;
    against the float64 oracle and against the route it replaces (option gru_h512_bwd_on_tier) reading the same forward records."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    from oracle import ttrnn_oracle as O
    torch.manual_seed(317)
    H, inp = 512, 256
    meta = dict(kind="ttgru", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=8)
    m = build_module(meta, dev())
    B, T = 4, (40 if case == "last_step_only" else 7)
    x = torch.randn(B, T, inp)
    h0 = None if case == "no_h0" else torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_backward_route(spec, B, T) == "fused_core"
    with ttrnn_hip.option("gru_h512_bwd_on_tier", 1):
        assert F.rnn_backward_route(spec, B, T) == "runtime_mfma"
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr = x.double().clone().requires_grad_(True)
    h0r = None if h0 is None else h0.double().clone().requires_grad_(True)
    ro, rh = O.gru_forward(layers, xr, h0r)
    wsum = 0.0 if case == "last_step_only" else 1.0
    ((ro * w.double()).sum() + wsum * 0.5 * rh.sum()).backward()

    def run():
        m.zero_grad()
        xg = x.to(dev()).contiguous().requires_grad_(True)
        h0g = None if h0 is None else h0.to(dev()).contiguous().requires_grad_(True)
        out, hT = m(xg, h0g)
        ((out * w.to(dev())).sum() + wsum * 0.5 * hT.sum()).backward()
        g = {"x": xg.grad.clone(), **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}
        if h0g is not None:
            g["h0"] = h0g.grad.clone()
        return g

    got = run()
    again = run()
    with ttrnn_hip.option("gru_h512_bwd_on_tier", 1):
        old = run()
    refs = {"x": xr.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    if h0r is not None:
        refs["h0"] = h0r.grad
    worst = {"fused": 0.0, "replaced": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        worst["fused"] = max(worst["fused"], _maxabs(got[n].double(), ref) / sc)
        worst["replaced"] = max(worst["replaced"], _maxabs(old[n].double(), ref) / sc)
    assert torch.equal(got["x"], again["x"])
    print(case, "max gradient error relative to each tensor's maximum:", worst)
    assert worst["fused"] <= 2e-5 and worst["fused"] <= 3.0 * worst["replaced"] + 1e-6


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["plain", "decades", "sparse_steps", "last_step_only"])
def test_fused_core_half_piece_gru_reverse_kernel_ranges(case, dtype):
    """cfg3-class reverse-time kernel (TT-GRU, fp32 and bf16 storage) on two fp16 pieces (k_gru_bwd_f10h): same scheme and the
    same cases as the LSTM kernel's test above, next to the three-bf16-piece kernel (option gemm_pieces = 3); h_0 given, so the
    direct path dh_{t-1} += dh_t z and d_h0 are exercised."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(293)
    H = 256
    meta = dict(kind="ttgru", input_size=1, hidden_size=H, num_layers=1, n_cores=3, tt_rank=8)
    m = build_module(meta, dev())
    B, T = 5, (60 if case == "last_step_only" else 9)
    x = torch.randn(B, T, 1)
    h0 = torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))
    elif case == "sparse_steps":
        w[:, 1:5] = 0.0
        w[2] = 0.0
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    if dtype == "bf16":
        m = m.to(torch.bfloat16)
        x, h0 = x.to(torch.bfloat16), h0.to(torch.bfloat16)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r = (t.double().clone().requires_grad_(True) for t in (x, h0))
    ro, rh = O.gru_forward(layers, xr, h0r)
    wsum = 0.0 if case in ("sparse_steps", "last_step_only") else 1.0
    ((ro * w.double()).sum() + wsum * 0.5 * rh.sum()).backward()

    def run(sel=None):
        m.zero_grad()
        xs, hs, ws = (t if sel is None else t[sel] for t in (x, h0, w))
        xg, h0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (xs, hs))
        out, hT = m(xg, h0g)
        ((out.float() * ws.to(dev())).sum() + wsum * 0.5 * hT.float().sum()).backward()
        return {"h0": h0g.grad.clone(), **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}

    got = run()
    again = run()
    with ttrnn_hip.option("gemm_pieces", 3):
        three = run()
    sub = run([2, 0])
    refs = {"h0": h0r.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    worst = {"two_fp16": 0.0, "three_bf16": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n].float()).all(), n
        worst["two_fp16"] = max(worst["two_fp16"], _maxabs(got[n].double(), ref) / sc)
        worst["three_bf16"] = max(worst["three_bf16"], _maxabs(three[n].double(), ref) / sc)
    assert torch.equal(got["h0"], again["h0"])                    # the reverse-time kernel's own result: repeatable,
    assert torch.equal(got["h0"][[2, 0]], sub["h0"])              # independent of the rest of the batch
    if case == "sparse_steps":
        assert float(got["h0"][2].float().abs().max()) == 0.0
    print(case, dtype, "max gradient error relative to each tensor's maximum:", worst)
    tol = 5e-2 if dtype == "bf16" else 2e-5
    assert worst["two_fp16"] <= tol and worst["two_fp16"] <= 3.0 * worst["three_bf16"] + 1e-6


def test_gru_forward_kernel_with_in_wave_s2_matches_eight_wave_kernel_and_oracle():
    """cfg3's default forward kernel (k_gru_fwd_f10v: four waves, the S2 operand gathered inside the gate waves with one DPP shift
    and one ds_bpermute per lane) against the eight-wave kernel it replaced (option gru_eight_wave) and the fp32 oracle: the two
    kernels multiply the same bf16 operands and differ by at most one bf16 ulp of an intermediate; gin-fed layers (stacked,
    input_size 40), h_0 given, training forward (reserve) included."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(31)
    for inp, L, B, T, with_h0 in ((1, 1, 9, 50, False), (1, 1, 70, 33, True), (40, 2, 6, 21, True)):
        meta = dict(kind="ttgru", input_size=inp, hidden_size=256, num_layers=L, n_cores=3, tt_rank=8)
        m = build_module(meta, dev()).to(torch.bfloat16)
        x = torch.rand(B, T, inp).to(torch.bfloat16)
        h0 = (torch.randn(B, 256) * 0.5).to(torch.bfloat16) if with_h0 else None
        sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items()}
        layers, _ = O.layers_from_state_dict(sd, L)
        ro, rh = O.gru_forward(layers, x.float(), h0.float() if with_h0 else None)
        outs = {}
        for name, on in (("in_wave", 0), ("eight_wave", 1)):
            with ttrnn_hip.option("gru_eight_wave", on), torch.no_grad():
                outs[name] = m(x.to(dev()), h0.to(dev()) if with_h0 else None)
        a, b = outs["in_wave"][0].float(), outs["eight_wave"][0].float()
        assert torch.isfinite(a).all()
        assert _maxabs(a, b) <= 2.0 ** -7                      # a bf16 ulp of values below 1 (mostly identical)
        assert _maxabs(a, ro) <= 2e-2 and _maxabs(b, ro) <= 2e-2
        assert _maxabs(outs["in_wave"][1].float(), rh) <= 2e-2
        # training forward writes the reserve: the backward must see the same state
        xg = x.to(dev())
        o1 = m(xg, h0.to(dev()) if with_h0 else None)[0]
        assert torch.equal(o1.detach(), outs["in_wave"][0])


@pytest.mark.parametrize("H,inp,B,T,with_state", [(256, 1, 9, 60, False), (256, 1, 70, 33, True), (256, 40, 300, 12, True)])
def test_single_barrier_forward_kernel_matches_two_barrier_kernel_and_oracle(H, inp, B, T, with_state):
    """k_lstm_fwd_f10s (ttrnn_fast_f10s.hip, round 5: S2 of the new state inside the gate waves, ONE barrier per step; measured
    3.5 % slower than the two-barrier kernel on cfg2 and kept behind option f10s as the A/B record of DESIGN.md lesson 56)
    against the default kernel and the float64 oracle: same scales, same S10; S2 sums its four terms in two chained MFMAs instead
    of one, so the two kernels agree to an ulp of an accumulator, and neither is further from float64 than the other.  Training
    forward (reserve) + backward included; batch rows independent, repeatable."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    from oracle import ttrnn_oracle as O
    torch.manual_seed(H + inp + B)
    m = build_module(dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=8), dev())
    x = torch.rand(B, T, inp)
    init = (torch.randn(B, H) * 0.5, torch.randn(B, H)) if with_state else None
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr = x.double().clone().requires_grad_(True)
    ro, (rh, rc) = O.lstm_forward(layers, xr, None if init is None else tuple(t.double() for t in init))
    assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == "fused_core"
    di = None if init is None else tuple(t.to(dev()) for t in init)
    outs = {}
    for name, on in (("one_barrier", 1), ("two_barriers", 0)):
        with ttrnn_hip.option("f10s", on), torch.no_grad():
            outs[name] = m(x.to(dev()), di)
    a, b_ = outs["one_barrier"], outs["two_barriers"]
    ea, eb = _maxabs(a[0], ro), _maxabs(b_[0], ro)
    print("H=%d in=%d B=%d: |one - two| %.3g, vs float64: one %.3g two %.3g" % (H, inp, B, _maxabs(a[0], b_[0]), ea, eb))
    assert _maxabs(a[0], b_[0]) <= 5e-7 and _maxabs(a[1][1], b_[1][1]) <= 1e-6
    assert ea <= 2e-6 and ea <= 2.0 * eb + 1e-7
    assert _maxabs(a[1][0], rh) <= 2e-6 and _maxabs(a[1][1], rc) <= 4e-6
    w = torch.randn(B, T, H)
    ((ro * w.double()).sum() + 0.5 * rh.sum() + 0.25 * rc.sum()).backward()
    with ttrnn_hip.option("f10s", 1):
        with torch.no_grad():
            again = m(x.to(dev()), di)
            sub = m(x[[2, 0]].to(dev()), None if di is None else (di[0][[2, 0]], di[1][[2, 0]]))
        assert torch.equal(again[0], a[0]) and torch.equal(sub[0], a[0][[2, 0]])
        # training forward + backward through the reverse-time kernel
        m.zero_grad()
        xg = x.to(dev()).requires_grad_(True)
        out, (hT, cT) = m(xg, di)
        assert torch.equal(out.detach(), a[0])
        ((out * w.to(dev())).sum() + 0.5 * hT.sum() + 0.25 * cT.sum()).backward()
    worst = 0.0
    for n, p in m.named_parameters():
        ref = leaves[n].grad
        worst = max(worst, _maxabs(p.grad, ref) / max(float(ref.abs().max()), 1e-30))
    worst = max(worst, _maxabs(xg.grad, xr.grad) / max(float(xr.grad.abs().max()), 1e-30))
    assert worst <= 1e-4


@pytest.mark.parametrize("kind", ["ttlstm", "ttgru"])
def test_fused_setup_launch_is_bit_identical(kind):
    """ABI 6: ttrnn_rnn_forward_cores on the input_size == 1 fused-core shapes (cfg2's TT-LSTM, the fp32 TT-GRU) does packing, the
    unit-row input projection, the scale header and the MFMA fragments in ONE set-up launch (ttrnn_fast_setup.hip) instead of four.
    Same expressions as the kernels it replaces: outputs, final states, the packed cores and EVERY gradient must be bit-identical
    to the separate launches (option no_fused_setup switches the fused launch off) — strided Parameters (the reference's layout),
    non-contiguous after an in-place update, with and without biases and initial states."""
    import ctypes
    import ttrnn_hip
    from ttrnn_hip import _lib
    torch.manual_seed(77)
    # (B T >= 4 in rows: fewer rows take the per-row weight-gradient kernels, whose atomics are not repeatable — DESIGN 9)
    for bias, with_state, B, T in ((True, False, 32, 40), (False, True, 70, 17), (True, True, 130, 9)):
        meta = dict(kind=kind, input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8, bias=bias)
        m = build_module(meta, dev())
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(1.0 + 0.1 * torch.rand_like(p))
        x = torch.randn(B, T, 1, device=dev())
        h0 = torch.randn(B, 256, device=dev()) * 0.5 if with_state else None
        init = None if h0 is None else ((h0, torch.randn(B, 256, device=dev())) if kind == "ttlstm" else h0)
        desc = m._all_layers[0]._layer_spec().desc(B, T, 0)
        res = {}
        for name, on in (("fused", 0), ("separate", 1)):
            with ttrnn_hip.option("no_fused_setup", on):
                assert _lib.load().ttrnn_rnn_forward_cores_fused(ctypes.byref(desc)) == (1 if not on else 0)
                with torch.no_grad():
                    r = m(x, init)
                m.zero_grad()
                o = m(x, init)            # (x not differentiated: a differentiated first-layer input takes the per-row
                hT = o[1][0] if kind == "ttlstm" else o[1]      # weight-gradient kernels, whose atomics are not repeatable — DESIGN 9)
                ((o[0] * torch.linspace(-1, 1, 256, device=dev())).sum() + hT.sum()).backward()
                res[name] = (r, o, None, {n: p.grad.clone() for n, p in m.named_parameters()})
        fa, se = res["fused"], res["separate"]
        assert torch.equal(fa[0][0], se[0][0]) and torch.equal(fa[1][0], se[1][0])
        sa = fa[0][1] if kind == "ttlstm" else (fa[0][1],)
        sb = se[0][1] if kind == "ttlstm" else (se[0][1],)
        for a, b_ in zip(sa, sb):
            assert torch.equal(a, b_)
        for n in fa[3]:
            assert torch.equal(fa[3][n], se[3][n]), n
    with ttrnn_hip.fp32_math("exact"):      # other math mode: no fused launch, the call is pack + forward
        assert _lib.load().ttrnn_rnn_forward_cores_fused(ctypes.byref(desc)) == 0


@pytest.mark.parametrize("rank,inp,with_state", [(8, 1, False), (8, 40, True), (16, 40, True)])
def test_reverse_kernel_with_precomputed_gate_factors(rank, inp, with_state):
    """k_lstm_bwd_f10p (round 5 A/B kernel, option f10p: waves 4-7 turn the forward record into the gate-gradient factors
    one step ahead, waves 0-3 run seven multiply-adds per unit; measured 3 % slower than k_lstm_bwd_f10h and not the default —
    DESIGN.md lesson 57) against the default reverse kernel and the float64 oracle: every gradient incl. d_h0 / d_c0 and the
    by-products' consumers (bias gradients, input_size == 1 sums), repeatable, masked samples exactly zero."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    torch.manual_seed(rank + inp)
    H, B, T = 256, 70, 23
    m = build_module(dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=rank), dev())
    x = torch.randn(B, T, inp)
    w = torch.randn(B, T, H)
    w[[2, 40]] = 0.0
    init = (torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3) if with_state else None
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    ir = None if init is None else tuple(t.double().clone().requires_grad_(True) for t in init)
    ro, (rh, rc) = O.lstm_forward(layers, x.double(), ir)
    wfin = torch.ones(B, 1, dtype=torch.float64)
    wfin[[2, 40]] = 0.0
    ((ro * w.double()).sum() + 0.5 * (rh * wfin).sum() + 0.25 * (rc * wfin).sum()).backward()

    def run(f10p):
        with ttrnn_hip.option("f10p", f10p):
            m.zero_grad()
            di = None if init is None else tuple(t.to(dev()).requires_grad_(True) for t in init)
            out, (hT, cT) = m(x.to(dev()), di)
            wf = wfin.float().to(dev())
            ((out * w.to(dev())).sum() + 0.5 * (hT * wf).sum() + 0.25 * (cT * wf).sum()).backward()
            g = {n: p.grad.clone() for n, p in m.named_parameters()}
            if di is not None:
                g["h0"], g["c0"] = di[0].grad.clone(), di[1].grad.clone()
            return g

    got, again, other = run(1), run(1), run(0)
    refs = {n: leaves[n].grad for n, _ in m.named_parameters()}
    if ir is not None:
        refs["h0"], refs["c0"] = ir[0].grad, ir[1].grad
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        assert _maxabs(got[n].double(), ref) <= 2e-5 * sc, n
        assert _maxabs(got[n], other[n]) <= 4e-6 * sc, n
        assert torch.equal(got[n], again[n]), n
    if init is not None:
        assert float(got["h0"][[2, 40]].abs().max()) == 0.0 and float(got["c0"][[2, 40]].abs().max()) == 0.0


def _cfg3_fp32_module(inp=1, L=1, rank=8):
    torch.manual_seed(1111)
    return build_module(dict(kind="ttgru", input_size=inp, hidden_size=256, num_layers=L, n_cores=3, tt_rank=rank), dev())


def test_gru_fp32_fused_core_error_vs_fp64_is_fp32_class():
    """The reference's GRU is fp32 only (tensorized_rnn/gru.py:25-50).  Its cfg3 shape on the two-piece fused-core kernel
    (k_gru_fwd_f10vh, ttrnn_fast_f10gh.hip: the default of the split mode since round 5) over the full 784 steps against the
    oracle evaluated in float64: as close to the exact result as ordinary fp32 arithmetic (the fp32-MFMA mode and the torch-CPU
    fp32 oracle); the runtime-shape tier's kernel (option gru_fwd_on_tier: the route fp32 GRUs took until round 4) beside it."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    m = _cfg3_fp32_module()
    torch.manual_seed(99)
    x = torch.rand(4, 784, 1)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, h64, _ = _oracle_forward("ttgru", sd, 1, x.double())
    r32, h32, _ = _oracle_forward("ttgru", sd, 1, x)
    errs = {"cpu_fp32": _maxabs(r32, r64)}
    for mode, on in (("exact", 0), ("split", 0), ("tier", 1)):
        with ttrnn_hip.fp32_math("exact" if mode == "exact" else "split"), ttrnn_hip.option("gru_fwd_on_tier", on), torch.no_grad():
            route = F.rnn_route(m._all_layers[0]._layer_spec(), 4, 784)
            assert route == {"exact": "stagewise_mfma", "split": "fused_core", "tier": "runtime_mfma"}[mode], (mode, route)
            out, hT = m(x.to(dev()))
        assert torch.equal(out[:, -1], hT)
        errs[mode] = _maxabs(out, r64)
    print("TT-GRU fp32, max abs error vs float64 oracle:", errs)
    assert errs["split"] <= 2e-6 and errs["exact"] <= 2e-6
    assert errs["split"] <= 2.0 * max(errs["exact"], errs["cpu_fp32"]) + 1e-7


@pytest.mark.parametrize("case", ["fresh", "tiny_weights", "huge_weights", "huge_h0", "decaying_h0", "zero_core", "mixed_magnitudes",
                                  "outlier_entry"])
def test_gru_fp32_fused_core_operand_ranges(case):
    """k_gru_fwd_f10vh multiplies two-piece fp16 operands under the diagonal power-of-two scales of ttrnn_f10_dev.h (chosen per
    launch from the cores; the state's scale per SAMPLE and — a GRU's state decays only as fast as z lets it — per STEP while a
    caller's h_0 keeps it outside (-1, 1)): nothing may overflow fp16's range or lose the small entries, whatever the
    magnitudes.  Both modes against the float64 oracle, error relative to the largest state; batch rows independent."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    m = _cfg3_fp32_module()
    torch.manual_seed(17)
    T = 40 if case == "decaying_h0" else 6
    B = 5
    h0 = torch.randn(B, 256) * 0.3
    x = torch.randn(B, T, 1)
    with torch.no_grad():
        cores = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n]
        assert len(cores) == 3
        if case == "tiny_weights":
            for p in cores:
                p.mul_(1e-4)
        elif case == "huge_weights":
            for p in cores:
                p.mul_(40.0)
        elif case == "huge_h0":
            h0 = torch.randn(B, 256) * 300.0
            h0[1] *= 1e-4                                     # one sample inside (-1, 1) next to them: scales are per sample
        elif case == "decaying_h0":
            h0 = torch.randn(B, 256) * 6.0                    # back inside (-1, 1) after 10 ... 20 steps (z ~ 0.5), small ever after
            h0[3] = 0.0
            h0[4] *= 0.25
        elif case == "zero_core":
            cores[1].zero_()
        elif case == "mixed_magnitudes":
            for k, step, f in ((2, 3, 1e-6), (0, 2, 1e-5)):
                w = cores[k].detach().clone().reshape(-1)
                w[::step] *= f
                cores[k].copy_(w.reshape(cores[k].shape))
        elif case == "outlier_entry":
            for k in (2, 1):                                  # ONE entry x 1e4 in core 2 and in core 1: the diagonal scales keep
                w = cores[k].detach().clone().reshape(-1)     # the other rows' / slices' bits
                w[7] *= 1e4
                cores[k].copy_(w.reshape(cores[k].shape))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r64, h64, _ = _oracle_forward("ttgru", sd, 1, x.double(), h0.double())
    scale = max(1e-30, float(r64.abs().max()))
    errs, outs = {}, {}
    for mode in ("exact", "split"):
        with ttrnn_hip.fp32_math(mode), torch.no_grad():
            if mode == "split":
                assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == "fused_core"
            out, hT = m(x.to(dev()), h0.to(dev()))
            if mode == "split":
                sub = m(x[[3, 1]].to(dev()), h0[[3, 1]].to(dev()))[0]
                assert torch.equal(out[[3, 1]], sub)          # a sample's result never depends on its batch
        assert torch.isfinite(out).all(), (case, mode)
        assert torch.equal(out[:, -1], hT)
        errs[mode] = _maxabs(out, r64)
        outs[mode] = out
    # late steps on their own scale: once the state is back inside (-1, 1) its pieces must be fine again
    late = _maxabs(outs["split"][:, -1], r64[:, -1]) / max(1e-30, float(r64[:, -1].abs().max()))
    print(case, "max abs error vs float64 (state scale %.3g):" % scale, errs, "last step relative: %.3g" % late)
    tol = 2e-3 if case in ("huge_weights", "huge_h0", "outlier_entry") else 2e-6
    assert errs["split"] <= tol * max(1.0, scale)
    assert errs["split"] <= 3.0 * errs["exact"] + 2e-7 * max(1.0, scale)
    if case == "decaying_h0":
        assert float(r64[:, -1].abs().max()) < 1.0 and late <= 2e-6


def test_gru_fp32_fused_core_variants_vs_oracle_and_tier():
    """k_gru_fwd_f10vh's template variants — input_size 1 / gin-fed (input_size 40, stacked layers), h_0 given or not, `out`
    skipped (the classifier reads only the last step) — against the fp32 oracle and the runtime-shape tier's kernel (option gru_fwd_on_tier),
    plus the training forward (reserve) feeding the reverse-time kernel k_gru_bwd_f10h: every gradient against the oracle's
    autograd in float64."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    from oracle import ttrnn_oracle as O
    torch.manual_seed(31)
    # (input_size != 1: the same recurrent kernel behind the runtime tier's dense K-in; rank 16: that route only, core 2's S2
    # fragments in LDS)
    for inp, L, B, T, with_h0, rank in ((1, 1, 9, 50, False, 8), (1, 1, 70, 33, True, 8), (40, 2, 6, 21, True, 8), (40, 1, 300, 12, False, 8),
                                        (40, 2, 9, 17, True, 16), (256, 1, 300, 10, False, 16),
                                        (1, 1, 7, 60, True, 16), (1, 1, 66, 30, False, 16)):      # r = 16, input_size 1: behind the tier's unit-row K-in
        m = _cfg3_fp32_module(inp, L, rank)
        x = torch.rand(B, T, inp)
        h0 = (torch.randn(B, 256) * 0.5) if with_h0 else None
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        layers, leaves = O.layers_from_state_dict({k: v.double() for k, v in sd.items()}, L, requires_grad=True, dtype=torch.float64)
        xr = x.double().clone().requires_grad_(True)
        ro, rh = O.gru_forward(layers, xr, h0.double() if with_h0 else None)
        outs = {}
        for name, on in (("fused", 0), ("tier", 1)):
            with ttrnn_hip.option("gru_fwd_on_tier", on), torch.no_grad():
                assert F.rnn_route(m._all_layers[-1]._layer_spec(), B, T) == ("fused_core" if not on else "runtime_mfma")
                outs[name] = m(x.to(dev()), h0.to(dev()) if with_h0 else None)
        assert _maxabs(outs["fused"][0], ro) <= 1e-5 and _maxabs(outs["fused"][1], rh) <= 1e-5
        assert _maxabs(outs["fused"][0], outs["tier"][0]) <= 2e-6
        # training forward + backward
        w = torch.randn(B, T, 256)
        ((ro * w.double()).sum() + 0.5 * rh.sum()).backward()
        m.zero_grad()
        xg = x.to(dev()).requires_grad_(True)
        out, hT = m(xg, h0.to(dev()) if with_h0 else None)
        assert torch.equal(out.detach(), outs["fused"][0])
        ((out * w.to(dev())).sum() + 0.5 * hT.sum()).backward()
        worst = 0.0
        for n, p in m.named_parameters():
            ref = leaves[n].grad
            worst = max(worst, _maxabs(p.grad, ref) / max(float(ref.abs().max()), 1e-30))
        worst = max(worst, _maxabs(xg.grad, xr.grad) / max(float(xr.grad.abs().max()), 1e-30))
        print("TT-GRU fp32 in=%d L=%d B=%d T=%d h0=%s r=%d: max gradient error relative to each tensor's maximum %.3g" % (
            inp, L, B, T, with_h0, rank, worst))
        assert worst <= 1e-4


@pytest.mark.parametrize("inp,B,T,h0_scale", [(256, 5, 30, None), (40, 300, 9, 0.5), (256, 70, 12, 40.0)])
def test_gru_h512_gates_on_accumulators_kernel(inp, B, T, h0_scale):
    """k_gru_fwd_f10g5 (ttrnn_fast_f10g5.hip, round 5): the reference's benchmark defaults with --gru (benchmarking.py:75-83:
    TT-GRU H = 512, d = 3, rank 8 — out modes (8, 12, 16): r, z, n of a unit share a column of the fused core, 32 rows apart), gates on
    the accumulators as in the TT-LSTM kernels, behind the runtime tier's dense K-in.  Against the float64 oracle and the tier's own
    recurrent kernel (option gru_fwd_on_tier); h_0 inside and far outside (-1, 1); final-state-only calls; training forward feeding the
    tier's reverse kernel: every gradient against the oracle's float64 autograd."""
    import ttrnn_hip
    from ttrnn_hip import functional as F
    from oracle import ttrnn_oracle as O
    torch.manual_seed(inp + B)
    m = build_module(dict(kind="ttgru", input_size=inp, hidden_size=512, num_layers=1, n_cores=3, tt_rank=8), dev())
    x = torch.rand(B, T, inp)
    h0 = None if h0_scale is None else torch.randn(B, 512) * h0_scale
    if h0 is not None and h0_scale > 1:
        h0[1] *= 1e-3                                  # a sample inside (-1, 1) next to them: scales are per sample
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr = x.double().clone().requires_grad_(True)
    ro, rh = O.gru_forward(layers, xr, None if h0 is None else h0.double())
    scale = max(1.0, float(ro.abs().max()))
    outs = {}
    for name, on in (("fused", 0), ("tier", 1)):
        with ttrnn_hip.option("gru_fwd_on_tier", on), torch.no_grad():
            assert F.rnn_route(m._all_layers[0]._layer_spec(), B, T) == ("fused_core" if not on else "runtime_mfma")
            outs[name] = m(x.to(dev()), None if h0 is None else h0.to(dev()))
    ef, et = _maxabs(outs["fused"][0], ro), _maxabs(outs["tier"][0], ro)
    print("TT-GRU H=512 in=%d B=%d h0=%s: max abs error vs float64 fused %.3g tier %.3g (state scale %.3g)" % (inp, B, h0_scale, ef, et, scale))
    tol = 1e-3 if (h0_scale or 0) > 1 else 2e-6
    assert ef <= tol * scale and ef <= 3.0 * et + 2e-7 * scale
    assert torch.equal(outs["fused"][0][:, -1], outs["fused"][1])
    with torch.no_grad():
        sub = m(x[[2, 0]].to(dev()), None if h0 is None else h0[[2, 0]].to(dev()))
        fin = m(x.to(dev()), None if h0 is None else h0.to(dev()), need_outputs=False)
    assert torch.equal(sub[0], outs["fused"][0][[2, 0]])
    assert fin[0] is None and torch.equal(fin[1], outs["fused"][1])
    if (h0_scale or 0) > 1:
        return
    w = torch.randn(B, T, 512)
    ((ro * w.double()).sum() + 0.5 * rh.sum()).backward()
    m.zero_grad()
    out, hT = m(x.to(dev()), None if h0 is None else h0.to(dev()))
    assert torch.equal(out.detach(), outs["fused"][0])
    ((out * w.to(dev())).sum() + 0.5 * hT.sum()).backward()
    worst = 0.0
    for n, p in m.named_parameters():
        ref = leaves[n].grad
        worst = max(worst, _maxabs(p.grad, ref) / max(float(ref.abs().max()), 1e-30))
    assert worst <= 1e-4


# ---- (13) repeatability of the gradients ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("meta", [
    dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8),          # fused core, in = 1 sums
    dict(kind="ttlstm", input_size=40, hidden_size=256, num_layers=3, n_cores=3, tt_rank=16),         # fused core, stacked, dense gradients
    dict(kind="ttgru", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8),
    dict(kind="ttlstm", input_size=256, hidden_size=512, num_layers=1, n_cores=3, tt_rank=8),         # runtime-shape tier (reference default)
    dict(kind="ttlstm", input_size=1, hidden_size=1024, num_layers=1, n_cores=2, tt_rank=16),         # runtime tier, in = 1: k_in1_reduce
    dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8, is_naive=True),
    dict(kind="ttlstm", input_size=1, hidden_size=128, num_layers=1, n_cores=2, tt_rank=4),           # cfg1: two-core kernels, dense gradient + k_proj2
    dict(kind="ttlstm", input_size=40, hidden_size=768, num_layers=1, n_cores=4, tt_rank=8),          # d = 4: dense gradients pulled back by the any-shape kernel (fixed-order slabs)
    dict(kind="ttgru", input_size=40, hidden_size=512, num_layers=1, n_cores=3, tt_rank=8),           # runtime tier GRU, resident reverse fragments
    dict(kind="ttgru", input_size=40, hidden_size=64, num_layers=1, n_cores=3, tt_rank=8),            # 3H = 192 columns: a partly filled column tile of the dense gradient (round 5; per-row atomics before)
    dict(kind="ttlstm", input_size=40, hidden_size=768, num_layers=1, n_cores=4, tt_rank=16),         # d = 4, r = 16: 100 KB of LDS accumulators per workgroup, fixed-order slabs on a capped grid (round 5)
], ids=lambda m: "{kind}-{input_size}-{hidden_size}-L{num_layers}-d{n_cores}-r{tt_rank}{n}".format(n="-naive" if m.get("is_naive") else "", **m))
def test_gradients_are_bitwise_repeatable(meta):
    """Three identical backward passes give bit-identical gradients for EVERY parameter.  Round 3 left two families to the order
    of arrival of atomicAdds: the bias gradients of every dense weight gradient (column sums of the gate gradients) and, on the
    runtime-shape tier, the input_size == 1 reduction (k_in1_reduce).  Both now leave per-workgroup partial sums that a second
    kernel adds in a fixed order (ttrnn_fast_gemm.hip: bias_partial / k_dense_bias_reduce; ttrnn_generic.hip: k_in1_finish)."""
    torch.manual_seed(3)
    m = build_module(meta, dev())
    B, T = 96, 64
    x = torch.randn(B, T, meta["input_size"], device=dev())
    w = torch.randn(B, T, meta["hidden_size"], device=dev())
    runs = []
    for _ in range(3):
        m.zero_grad(set_to_none=True)
        out = m(x)[0]                  # the input is data, not differentiated — as in the reference's training loops
        (out * w).sum().backward()     # (benchmarking.py:41-70); a differentiated first-layer input takes per-row kernels whose
        runs.append([p.grad.clone() for p in m.parameters()])          # core-gradient flush still goes through atomics
    names = [n for n, _ in m.named_parameters()]
    differing = [n for n, a, b, c in zip(names, *runs) if not (torch.equal(a, b) and torch.equal(a, c))]
    assert not differing, differing


# ---- (14) two-core reverse-time kernel (ttrnn_fast_f2.hip: k_lstm_bwd_f2) ------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "decades", "sparse_steps", "last_step_only", "outlier_core0", "outlier_core1", "long"])
def test_two_core_reverse_kernel_ranges(case):
    """cfg1's shape (H = 128, d = 2, r = 4; pMNIST's default --ncores 2) in split mode: both transposed stages on two fp16 pieces,
    the weights' rows under their own power-of-two scales, every step's gate gradients scaled from the maximum of their WAVE's 64
    units and T0's results from a bound.  Output gradients over ten decades, steps and samples without gradient, a loss on the last
    step only, one core entry x 1e5 / 1e6 (row scales: no guard needed), a 784-step sequence: every parameter / input /
    initial-state gradient against the float64 oracle next to the stage-wise fp32-MFMA kernel (exact mode) on the same inputs;
    the kernel's own results bitwise repeatable and independent of the rest of the batch."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    from ttrnn_hip import functional as F
    torch.manual_seed(211)
    H, inp = 128, 1
    meta = dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=2, tt_rank=4)
    m = build_module(meta, dev())
    B = 5
    T = 60 if case == "last_step_only" else (784 if case == "long" else 9)
    if case.startswith("outlier"):
        core = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n][int(case[-1])]
        with torch.no_grad():
            flat = core.detach().clone().contiguous().view(-1)
            flat[(5 * flat.numel()) // 11] *= (1e5 if case[-1] == "1" else 1e6)
            core.copy_(flat.view(core.shape))
    x = torch.rand(B, T, inp) if case == "long" else torch.randn(B, T, inp)
    h0, c0 = torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))
    elif case == "sparse_steps":
        w[:, 1:5] = 0.0
        w[2] = 0.0
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r, c0r = (t.double().clone().requires_grad_(True) for t in (x, h0, c0))
    ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r))
    wsum = 0.0 if case in ("sparse_steps", "last_step_only") else 1.0
    ((ro * w.double()).sum() + wsum * (rc.sum() + 0.5 * rh.sum())).backward()

    def run(sel=None):
        m.zero_grad()
        xs, hs, cs, ws = (t if sel is None else t[sel] for t in (x, h0, c0, w))
        xg, h0g, c0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (xs, hs, cs))
        out, (hT, cT) = m(xg, (h0g, c0g))
        ((out * ws.to(dev())).sum() + wsum * (cT.sum() + 0.5 * hT.sum())).backward()
        return {"x": xg.grad.clone(), "h0": h0g.grad.clone(), "c0": c0g.grad.clone(),
                **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}

    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_backward_route(spec, B, T) == "fused_core"
    got = run()
    again = run()
    sub = run([2, 0])
    with ttrnn_hip.fp32_math("exact"):
        assert F.rnn_backward_route(spec, B, T) == "stagewise_mfma"
        exact = run()
    refs = {"x": xr.grad, "h0": h0r.grad, "c0": c0r.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    worst = {"two_fp16": 0.0, "fp32_mfma": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        worst["two_fp16"] = max(worst["two_fp16"], _maxabs(got[n].double(), ref) / sc)
        worst["fp32_mfma"] = max(worst["fp32_mfma"], _maxabs(exact[n].double(), ref) / sc)
    for n in ("h0", "c0"):                                         # the reverse-time kernel's own results
        assert torch.equal(got[n], again[n]), n
        assert torch.equal(got[n][[2, 0]], sub[n]), n
    if case == "sparse_steps":
        assert float(got["h0"][2].abs().max()) == 0.0
    if case == "last_step_only":
        rel = _maxabs(got["h0"].double(), h0r.grad) / max(float(h0r.grad.abs().max()), 1e-300)
        print("d_h0 after 60 steps: max |ref| %.3g, relative error %.3g" % (float(h0r.grad.abs().max()), rel))
        assert rel <= 1e-4
    print(case, "max gradient error relative to each tensor's maximum:", worst)
    assert not torch.equal(got["h0"], exact["h0"])                 # a different kernel did run
    # (outlier forward weights trip the FORWARD kernel's guard: then both runs share the fp32 forward and differ in the reverse only;
    # a core entry x 1e5 makes the gradients themselves ill-conditioned: the fp32-MFMA kernel sits at 5e-5 there, the yardstick)
    assert worst["two_fp16"] <= (1.5 * worst["fp32_mfma"] + 1e-6 if case.startswith("outlier") else 2e-5)
    assert worst["two_fp16"] <= 3.0 * worst["fp32_mfma"] + 1e-6


# ---- (15) H = 512, r = 8: the fused-core forward under the runtime tier's K-in (ttrnn_fast_f10.hip: launch_rnn_fwd_f10_h512) ------------
@pytest.mark.parametrize("B,T,inp,with_state,H", [(3, 9, 256, True, 512), (5, 33, 40, False, 512), (300, 6, 256, True, 512),
                                                   (5, 33, 40, True, 384), (300, 6, 384, False, 384)])
def test_h512_fused_core_forward_route(B, T, inp, with_state, H):
    """The reference's default benchmark shape (benchmarking.py:75-83: TT-LSTM hidden 512, ncores 3, ttrank 8): in split mode the
    forward recurrent kernel is the fused-core kernel as eight-wave workgroups (k_lstm_fwd_f10q<ShpH512R8L>) behind the runtime tier's
    dense K-in; exact mode and option h512_fwd_on_tier keep the runtime-shape / any-shape kernels.  Round 5: the same for --hidden_size 384
    (out modes (8, 12, 16): six S10 tiles = six waves, the 24 S2 tiles dealt out one by one, a 48-slot image row swizzled in blocks
    of sixteen).  Outputs and every gradient (the reverse
    kernel is the runtime tier's, reading this kernel's reserve) against the float64 oracle; the two forward kernels against each
    other; B = 300 > #CUs runs in two rounds of workgroups; batch split, repeat launches and the outputs-not-wanted call bit for bit."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    from ttrnn_hip import functional as F
    torch.manual_seed(97 + B)
    m = build_module(dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=8), dev())
    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_route(spec, B, T) == "fused_core"
    with ttrnn_hip.option("h512_fwd_on_tier", 1):
        assert F.rnn_route(spec, B, T) == "runtime_mfma"
    x = torch.randn(B, T, inp) * 0.5
    h0, c0 = (torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3) if with_state else (None, None)
    nchk = min(B, 4)
    rows = sorted({0, B // 2, B - 1, 1 % B})[:nchk]
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr = x[rows].double().clone().requires_grad_(True)
    init = (h0[rows].double(), c0[rows].double()) if with_state else None
    ro, (rh, rc) = O.lstm_forward(layers, xr, init)
    w = torch.randn(len(rows), T, H)
    ((ro * w.double()).sum() + rc.sum()).backward()

    def run(sel=None, need_out=True):
        xs = x if sel is None else x[sel]
        st = None if not with_state else ((h0 if sel is None else h0[sel]).to(dev()), (c0 if sel is None else c0[sel]).to(dev()))
        with torch.no_grad():
            return m(xs.to(dev()), st) if need_out else m(xs.to(dev()), st, need_outputs=False)

    out, (hT, cT) = run()
    assert _maxabs(out[rows], ro.detach()) <= 2e-6 and _maxabs(cT[rows], rc.detach()) <= 2e-6
    again = run()
    assert torch.equal(out, again[0]) and torch.equal(cT, again[1][1])
    part = run(rows)
    assert torch.equal(out[rows], part[0])
    nout = run(need_out=False)
    assert torch.equal(nout[1][0], hT) and torch.equal(nout[1][1], cT)
    with ttrnn_hip.option("h512_fwd_on_tier", 1):
        g2out = run()[0]
    assert not torch.equal(g2out, out) and _maxabs(g2out, out) <= 2e-6
    # training step through this forward + the runtime tier's reverse kernel (masked loss on `rows`)
    m.zero_grad()
    xg = x.to(dev()).requires_grad_(True)
    st = None if not with_state else (h0.to(dev()), c0.to(dev()))
    o2, (h2, c2) = m(xg, st)
    W = torch.zeros(B, T, H)
    W[rows] = w
    mask = torch.zeros(B, 1)
    mask[rows] = 1.0
    ((o2 * W.to(dev())).sum() + (c2 * mask.to(dev())).sum()).backward()
    assert _maxabs(xg.grad[rows], xr.grad) <= 1e-4 * max(float(xr.grad.abs().max()), 1e-30)
    for n, p in m.named_parameters():
        ref = leaves[n].grad
        assert _maxabs(p.grad, ref) <= 1e-4 * max(float(ref.abs().max()), 1e-30), n


# ---- (16) H = 512, r = 8: the fused-core reverse-time kernel (ttrnn_fast_f10bh.hip: k_lstm_bwd_f10h<ShpH512R8L>) ---------------------
@pytest.mark.parametrize("case", ["plain", "decades", "sparse_steps", "last_step_only", "outlier_core0", "outlier_core2", "two_rounds"])
def test_h512_fused_core_reverse_kernel(case):
    """The reference's default benchmark shape (benchmarking.py:75-83) in split mode: the reverse-time recurrence is the fused-core
    kernel on two fp16 pieces with all eight waves as gate waves (torch autograd through lstm.py:23-32,123-133 and t3nsor/ops.py:78-93
    is what it restates); option h512_bwd_on_tier keeps the runtime tier's kernel, exact mode its own route.  Every parameter / input / initial-state
    gradient against the float64 oracle next to the runtime tier's kernel on the same inputs — output gradients over ten decades,
    steps and samples without gradient, a loss on the last step only, one core entry x 1e5, 300 samples (two rounds of
    workgroups); the kernel's own results bitwise repeatable and independent of the rest of the batch; a request for the
    per-step state gradients still takes the runtime tier."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    from ttrnn_hip import functional as F
    torch.manual_seed(223)
    H, inp = 512, 40
    meta = dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=8)
    m = build_module(meta, dev())
    B = 300 if case == "two_rounds" else 5
    T = 60 if case == "last_step_only" else (4 if case == "two_rounds" else 9)
    if case.startswith("outlier"):
        core = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n][int(case[-1])]
        with torch.no_grad():
            flat = core.detach().clone().contiguous().view(-1)
            flat[(5 * flat.numel()) // 11] *= 1e5
            core.copy_(flat.view(core.shape))
    x = torch.randn(B, T, inp)
    h0, c0 = torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))
    elif case == "sparse_steps":
        w[:, 1:5] = 0.0
        w[2] = 0.0
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    rows = list(range(B)) if B <= 8 else [0, 1, B // 2, B - 1]
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r, c0r = (t[rows].double().clone().requires_grad_(True) for t in (x, h0, c0))
    ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r))
    wsum = 0.0 if case in ("sparse_steps", "last_step_only") else 1.0
    ((ro * w[rows].double()).sum() + wsum * (rc.sum() + 0.5 * rh.sum())).backward()
    mask = torch.zeros(B, 1)
    mask[rows] = 1.0

    def run(sel=None):
        m.zero_grad()
        xs, hs, cs, ws, ms = (t if sel is None else t[sel] for t in (x, h0, c0, w, mask))
        xg, h0g, c0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (xs, hs, cs))
        out, (hT, cT) = m(xg, (h0g, c0g))
        md = ms.to(dev())
        ((out * (ws * ms.unsqueeze(-1)).to(dev())).sum() + wsum * ((cT * md).sum() + 0.5 * (hT * md).sum())).backward()
        return {"x": xg.grad.clone(), "h0": h0g.grad.clone(), "c0": c0g.grad.clone(),
                **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}

    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_backward_route(spec, B, T) == "fused_core"
    assert F.rnn_backward_route(spec, B, T, want_state=True) == "runtime_mfma"
    with ttrnn_hip.fp32_math("exact"):
        assert F.rnn_backward_route(spec, B, T) != "fused_core"
    got = run()
    again = run()
    sub = run([rows[2], rows[0]]) if B <= 8 else None
    with ttrnn_hip.option("h512_bwd_on_tier", 1):
        assert F.rnn_backward_route(spec, B, T) == "runtime_mfma"
        tier = run()
    refs = {"x": xr.grad, "h0": h0r.grad, "c0": c0r.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    worst = {"two_fp16": 0.0, "tier": 0.0}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        assert torch.isfinite(got[n]).all(), n
        g, t = (d[n][rows] if n in ("x", "h0", "c0") else d[n] for d in (got, tier))
        worst["two_fp16"] = max(worst["two_fp16"], _maxabs(g.double(), ref) / sc)
        worst["tier"] = max(worst["tier"], _maxabs(t.double(), ref) / sc)
    for n in ("h0", "c0", "x"):                                    # the reverse-time kernel's own results (x: through d_gates)
        assert torch.equal(got[n], again[n]), n
        if sub is not None:
            assert torch.equal(got[n][[rows[2], rows[0]]], sub[n]), n
    if case == "sparse_steps":
        assert float(got["h0"][2].abs().max()) == 0.0
    if case == "last_step_only":
        rel = _maxabs(got["h0"].double(), h0r.grad) / max(float(h0r.grad.abs().max()), 1e-300)
        print("d_h0 after 60 steps: max |ref| %.3g, relative error %.3g" % (float(h0r.grad.abs().max()), rel))
        assert rel <= 1e-4
    print(case, "max gradient error relative to each tensor's maximum:", worst)
    assert not torch.equal(got["h0"], tier["h0"])                  # a different kernel did run
    assert worst["two_fp16"] <= (1.5 * worst["tier"] + 1e-6 if case.startswith("outlier") else 2e-5)
    assert worst["two_fp16"] <= 3.0 * worst["tier"] + 1e-6


# ---- (17) fused-core reverse LSTM kernel with one wave per 64 units (ttrnn_fast_f10bh.hip: k_lstm_bwd_f10l) at H = 256 ------------
@pytest.mark.parametrize("rank,inp", [(8, 1), (16, 40)])
def test_wave_local_reverse_kernel_h256(rank, inp):
    """H = 256 launches with more samples than CUs run the reverse-time recurrence as four-wave workgroups, two per CU, whose T2 and
    dh hand-off stay inside a wave (two barriers per step); option f10bl_never keeps the eight-wave kernel.  Same arithmetic, another
    summation order in T2 (whole K per wave instead of k-block partial sums): the two agree to rounding, both meet the float64 oracle
    (autograd through lstm.py:23-32,123-133) on sampled rows; the by-products (column maxima; in = 1: the bias / input sums) come out
    of the gate threads of either kernel."""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    from ttrnn_hip import functional as F
    torch.manual_seed(229 + rank)
    H, B, T = 256, 300, 7
    m = build_module(dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=rank), dev())
    x = torch.randn(B, T, inp)
    h0, c0 = torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H) * (10.0 ** (torch.rand(B, T, 1) * 6 - 4))
    rows = [0, 1, 150, 299]
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r, c0r = (t[rows].double().clone().requires_grad_(True) for t in (x, h0, c0))
    ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r))
    ((ro * w[rows].double()).sum() + rc.sum() + 0.5 * rh.sum()).backward()
    mask = torch.zeros(B, 1)
    mask[rows] = 1.0

    def run():
        m.zero_grad()
        xg, h0g, c0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (x, h0, c0))
        out, (hT, cT) = m(xg, (h0g, c0g))
        md = mask.to(dev())
        ((out * (w * mask.unsqueeze(-1)).to(dev())).sum() + (cT * md).sum() + 0.5 * (hT * md).sum()).backward()
        return {"x": xg.grad.clone(), "h0": h0g.grad.clone(), "c0": c0g.grad.clone(),
                **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}

    spec = m._all_layers[0]._layer_spec()
    assert F.rnn_backward_route(spec, B, T) == "fused_core"
    got, again = run(), run()
    with ttrnn_hip.option("f10bl_never", 1):
        wide = run()
    refs = {"x": xr.grad, "h0": h0r.grad, "c0": c0r.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    for n, ref in refs.items():
        sc = max(float(ref.abs().max()), 1e-30)
        g, o = (d[n][rows] if n in ("x", "h0", "c0") else d[n] for d in (got, wide))
        assert torch.isfinite(got[n]).all(), n
        assert _maxabs(g.double(), ref) <= 2e-5 * sc, n
        assert _maxabs(g, o) <= 4e-6 * sc, n
    for n in ("h0", "c0"):
        assert torch.equal(got[n], again[n]), n
        assert float(got[n][[2, 77, 298]].abs().max()) == 0.0, n        # samples outside the loss
    assert not torch.equal(got["h0"], wide["h0"])                  # a different kernel did run


# ---- (18) runtime-shape reverse-time kernel on two fp16 pieces (ttrnn_g2.hip: k_g2_bwd) --------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "decades", "sparse_steps", "last_step_only", "outlier_core0", "outlier_last", "many_samples"])
@pytest.mark.parametrize("meta", [
    dict(kind="ttgru", input_size=40, hidden_size=512, num_layers=1, n_cores=3, tt_rank=8),        # head^T resident (twelve slots)
    dict(kind="ttlstm", input_size=40, hidden_size=768, num_layers=1, n_cores=4, tt_rank=8),       # streamed, several units per thread
], ids=lambda m: "{kind}-H{hidden_size}-d{n_cores}-r{tt_rank}".format(**m))
def test_runtime_reverse_kernel_ranges(meta, case):
    """Both transposed stages of the runtime-shape tier's reverse-time kernel multiply two fp16 pieces per operand (round 4: three bf16
    pieces / the fp32 MFMA before): the merged cores' rows under power-of-two row scales, every step's gate gradients under the scale of
    their exact maximum, T2's results under the bound L1(row) x max|dg_t| (the scheme of ttrnn_fast_f10bh.hip).  Output gradients over
    ten decades, steps and samples without gradient, a loss on the last step only, one core entry x 1e3, more samples than CUs (the
    other workgroup plan): every parameter / input / initial-state gradient against the float64 oracle (torch autograd through
    lstm.py:23-32,123-133 / gru.py:38-44 and t3nsor/ops.py:78-93) within 2e-5 of each tensor's maximum; repeat runs bit for bit.
    An outlier entry makes the problem itself ill-conditioned in fp32 (x 1e5: the any-shape fp32 kernels of `exact` mode miss the
    float64 forward by 6e-4 and the gradients by 6e-3): there the yardstick is `exact` mode on the same inputs.  (Block-diagonal
    heads — naive per-gate sets — have their gradient test in test_naive_per_gate_sets_run_on_the_fused_path.)"""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    from ttrnn_hip import functional as F
    torch.manual_seed(241)
    H, inp = meta["hidden_size"], meta["input_size"]
    lstm = meta["kind"] == "ttlstm"
    m = build_module(meta, dev())
    B = 300 if case == "many_samples" else 5
    T = 40 if case == "last_step_only" else (4 if case == "many_samples" else 9)
    if case.startswith("outlier"):
        cores = [p for n, p in m.named_parameters() if "hidden_weights" in n and p.dim() > 1]
        core = cores[0] if case == "outlier_core0" else cores[-1]
        with torch.no_grad():
            flat = core.detach().clone().contiguous().view(-1)
            flat[(5 * flat.numel()) // 11] *= 1e3
            core.copy_(flat.view(core.shape))
    x = torch.randn(B, T, inp)
    h0, c0 = torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3
    w = torch.randn(B, T, H)
    if case == "decades":
        w = w * (10.0 ** (torch.rand(B, T, 1) * 10 - 6))
    elif case == "sparse_steps":
        w[:, 1:5] = 0.0
        w[2] = 0.0
    elif case == "last_step_only":
        w[:, :-1] = 0.0
    rows = list(range(B)) if B <= 8 else [0, 1, B // 2, B - 1]
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr, h0r, c0r = (t[rows].double().clone().requires_grad_(True) for t in (x, h0, c0))
    wsum = 0.0 if case in ("sparse_steps", "last_step_only") else 1.0
    if lstm:
        ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r))
        ((ro * w[rows].double()).sum() + wsum * (rc.sum() + 0.5 * rh.sum())).backward()
    else:
        ro, rh = O.gru_forward(layers, xr, h0r)
        ((ro * w[rows].double()).sum() + wsum * 0.5 * rh.sum()).backward()
    mask = torch.zeros(B, 1)
    mask[rows] = 1.0

    def run():
        m.zero_grad()
        xg, h0g, c0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (x, h0, c0))
        md = mask.to(dev())
        if lstm:
            out, (hT, cT) = m(xg, (h0g, c0g))
            loss = (out * (w * mask.unsqueeze(-1)).to(dev())).sum() + wsum * ((cT * md).sum() + 0.5 * (hT * md).sum())
        else:
            out, hT = m(xg, h0g)
            loss = (out * (w * mask.unsqueeze(-1)).to(dev())).sum() + wsum * 0.5 * (hT * md).sum()
        loss.backward()
        got = {"x": xg.grad.clone(), "h0": h0g.grad.clone(), **{n: p.grad.detach().clone() for n, p in m.named_parameters()}}
        if lstm:
            got["c0"] = c0g.grad.clone()
        return got

    spec = m._all_layers[0]._layer_spec()
    # (round 6: the TT-GRU of H = 512 has a fused-core reverse-time kernel of its own; option gru_h512_bwd_on_tier keeps it on the tier's kernel,
    # which this test is about — the fused route runs the same cases further down)
    import contextlib
    tier = ttrnn_hip.option("gru_h512_bwd_on_tier", 1) if not lstm else contextlib.nullcontext()
    with tier:
        assert F.rnn_backward_route(spec, B, T) == "runtime_mfma"
        got, again = run(), run()
    refs = {"x": xr.grad, "h0": h0r.grad, **{n: leaves[n].grad for n, _ in m.named_parameters()}}
    if lstm:
        refs["c0"] = c0r.grad
    def worst_of(res):
        wv = 0.0
        for n, ref in refs.items():
            sc = max(float(ref.abs().max()), 1e-30)
            assert torch.isfinite(res[n]).all(), n
            g = res[n][rows] if n in ("x", "h0", "c0") else res[n]
            wv = max(wv, _maxabs(g.double(), ref) / sc)
        return wv
    worst = worst_of(got)
    for n in ("h0", "x"):
        assert torch.equal(got[n], again[n]), n
    if case == "sparse_steps":
        assert float(got["h0"][2].abs().max()) == 0.0
    if case == "last_step_only":
        rel = _maxabs(got["h0"].double(), h0r.grad) / max(float(h0r.grad.abs().max()), 1e-300)
        print("d_h0 after 40 steps: max |ref| %.3g, relative error %.3g" % (float(h0r.grad.abs().max()), rel))
        assert rel <= 1e-4
    print(meta["kind"], H, case, "max gradient error relative to each tensor's maximum: %.3g" % worst)
    exact = None
    if case.startswith("outlier"):
        with ttrnn_hip.fp32_math("exact"):
            exact = worst_of(run())
        print("   exact mode on the same inputs: %.3g" % exact)
        assert worst <= max(10.0 * exact, 2e-5) and worst <= 5e-3
    else:
        assert worst <= 2e-5
    if not lstm:
        assert F.rnn_backward_route(spec, B, T) == "fused_core"
        fused, fused2 = run(), run()
        wf = worst_of(fused)
        print("   fused-core reverse kernel (k_gru_bwd_f10h<ShpH512R8G>): %.3g" % wf)
        for n in ("h0", "x"):
            assert torch.equal(fused[n], fused2[n]), n
        if case == "sparse_steps":
            assert float(fused["h0"][2].abs().max()) == 0.0
        assert wf <= (max(10.0 * exact, 2e-5) if exact is not None else 2e-5)


# ---- (19) the round-4 reverse-time kernels at the corners -------------------------------------------------------------------------------
@pytest.mark.parametrize("meta", [
    dict(kind="ttlstm", input_size=40, hidden_size=512, num_layers=1, n_cores=3, tt_rank=8),       # fused core, one wave per 64 units
    dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8),        # fused core, eight-wave kernel
    dict(kind="ttgru", input_size=40, hidden_size=512, num_layers=1, n_cores=3, tt_rank=8),        # runtime tier, resident fragments
    dict(kind="ttlstm", input_size=40, hidden_size=768, num_layers=1, n_cores=4, tt_rank=8),       # runtime tier, streamed fragments
    dict(kind="ttgru", input_size=40, hidden_size=96, num_layers=1, n_cores=2, tt_rank=3),         # runtime tier, padded rank, H < 128
], ids=lambda m: "{kind}-H{hidden_size}-d{n_cores}-r{tt_rank}".format(**m))
def test_reverse_kernels_edge_cases_vs_oracle(meta):
    """B = 1, T = 1 ... 4 (the rotating record registers of the fused-core kernels, the one-step-ahead record request of the runtime
    tier's: first and last steps are their special cases), explicit and absent initial state, a loss that uses the final states only:
    every gradient against the float64 oracle (autograd through lstm.py:101-135 / gru.py:101-130)."""
    from oracle import ttrnn_oracle as O
    torch.manual_seed(307)
    H, inp = meta["hidden_size"], meta["input_size"]
    lstm = meta["kind"] == "ttlstm"
    m = build_module(meta, dev())
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    for B, T, with_init, final_only in [(1, 1, False, False), (1, 2, True, False), (3, 1, True, True), (2, 3, False, False),
                                        (2, 4, True, True), (5, 7, True, False)]:
        x = torch.randn(B, T, inp)
        h0, c0 = torch.randn(B, H) * 0.3, torch.randn(B, H) * 0.3
        w = torch.zeros(B, T, H) if final_only else torch.randn(B, T, H)
        layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
        xr, h0r, c0r = (t.double().clone().requires_grad_(True) for t in (x, h0, c0))
        if lstm:
            ro, (rh, rc) = O.lstm_forward(layers, xr, (h0r, c0r) if with_init else None)
            ((ro * w.double()).sum() + rc.sum() + 0.5 * rh.sum()).backward()
        else:
            ro, rh = O.gru_forward(layers, xr, h0r if with_init else None)
            ((ro * w.double()).sum() + 0.5 * rh.sum()).backward()
        m.zero_grad()
        xg, h0g, c0g = (t.to(dev()).contiguous().requires_grad_(True) for t in (x, h0, c0))
        if lstm:
            out, (hT, cT) = m(xg, (h0g, c0g) if with_init else None)
            ((out * w.to(dev())).sum() + cT.sum() + 0.5 * hT.sum()).backward()
        else:
            out, hT = m(xg, h0g if with_init else None)
            ((out * w.to(dev())).sum() + 0.5 * hT.sum()).backward()
        assert _maxabs(out.detach(), ro.detach()) <= 1e-5, (B, T)
        refs = {"x": (xg.grad, xr.grad), **{n: (p.grad, leaves[n].grad) for n, p in m.named_parameters()}}
        if with_init:
            refs["h0"] = (h0g.grad, h0r.grad)
            if lstm:
                refs["c0"] = (c0g.grad, c0r.grad)
        for n, (g, ref) in refs.items():
            assert g is not None and torch.isfinite(g).all(), (n, B, T)
            assert _maxabs(g.double(), ref) <= 2e-5 * max(float(ref.abs().max()), 1e-30), (n, B, T, with_init, final_only)

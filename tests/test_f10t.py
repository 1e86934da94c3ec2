"""k_lstm_fwd_f10t (ttrnn_fast_f10t.hip): the fused-core TT-LSTM forward of H = 256, d = 3, r = 8 with cores 0·1 contracted first and
the stage hand-off in registers — the default for that shape in split mode while a sample has a CU of its own; option
f10t_off keeps k_lstm_fwd_f10q (core 2 first).  Through the module API, against the float64 oracle and against k_lstm_fwd_f10q:
    out / h_T within 2e-6 and c_T within 4e-6 of float64 (the bounds of the single-barrier kernel's test), never more than twice
    k_lstm_fwd_f10q's own error + 1e-7, and within 5e-7 of k_lstm_fwd_f10q on out;
    repeat runs and batch subsets bit for bit; the final-state-only call; training forward = eval forward; gradients through the
    reverse-time kernel within 1e-4 of each gradient's maximum; the operand-range and outlier weight sets of
    test_gpu_parity.py in BOTH routes (bounds as there: the split mode within the exact mode's class against float64);
    one capture-and-replay of a forward.
Sizes: in in {1, 40}, B in {1, 3, 5}, T in {1, 2, 5, 33}, with / without (h_0, c_0) — h_0 = 0.5 randn leaves (-1, 1) — and biases.
"""
import contextlib
import functools

import pytest
import torch

from golden_io import build_module

pytestmark = pytest.mark.gpu

H = 256
BS = (1, 3, 5)
TS = (1, 2, 5, 33)
F10Q = "f10t_off"    # option: k_lstm_fwd_f10q for the calls k_lstm_fwd_f10t would take


def dev():
    return torch.device("cuda:0")


def _maxabs(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


@functools.lru_cache(maxsize=None)
def _module(inp, bias):
    torch.manual_seed(1000 + inp + (7 if bias else 0))
    m = build_module(dict(kind="ttlstm", input_size=inp, hidden_size=H, num_layers=1, n_cores=3, tt_rank=8, bias=bias), dev())
    if bias:      # (fresh biases may be constant: make every unit's differ)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("bias"):
                    p.copy_(0.1 * torch.randn_like(p))
    return m


@functools.lru_cache(maxsize=None)
def _data(inp, with_state):
    g = torch.Generator().manual_seed(5 + inp + (3 if with_state else 0))
    x = torch.rand(max(BS), max(TS), inp, generator=g)
    init = (0.5 * torch.randn(max(BS), H, generator=g), torch.randn(max(BS), H, generator=g)) if with_state else None
    return x, init


@functools.lru_cache(maxsize=None)
def _oracle(inp, with_state, bias, T):
    """float64 oracle on the largest batch, the first T steps (computed once per size, shared, never modified)"""
    from oracle import ttrnn_oracle as O
    m = _module(inp, bias)
    x, init = _data(inp, with_state)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, _ = O.layers_from_state_dict(sd, 1, dtype=torch.float64)
    with torch.no_grad():
        ro, (rh, rc) = O.lstm_forward(layers, x[:, :T].double(), None if init is None else tuple(t.double() for t in init))
    return ro, rh, rc


def _spec(m):
    return m._all_layers[0]._layer_spec()


def _assert_routes(m, B, T):
    import ttrnn_hip
    from ttrnn_hip import functional as F
    assert F.rnn_route(_spec(m), B, T) == "fused_core"
    assert F.rnn_cores01_first(_spec(m), B, T)
    with ttrnn_hip.option(F10Q, 1):
        assert F.rnn_route(_spec(m), B, T) == "fused_core"
        assert not F.rnn_cores01_first(_spec(m), B, T)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("inp", [1, 40])
def test_forward_against_oracle_and_f10q(inp, with_state, bias, T):
    import ttrnn_hip
    m = _module(inp, bias)
    x, init = _data(inp, with_state)
    ro, rh, rc = _oracle(inp, with_state, bias, T)
    full = None
    for B in sorted(BS, reverse=True):
        _assert_routes(m, B, T)
        xb = x[:B, :T].to(dev())
        ib = None if init is None else tuple(t[:B].to(dev()) for t in init)
        with torch.no_grad():
            new = m(xb, ib)
            again = m(xb, ib)
            with ttrnn_hip.option(F10Q, 1):
                old = m(xb, ib)
            last = m(xb, ib, need_outputs=False)              # OUT = false: the caller consumes only the final state
        en, eo = _maxabs(new[0], ro[:B]), _maxabs(old[0], ro[:B])
        eh, ec = _maxabs(new[1][0], rh[:B]), _maxabs(new[1][1], rc[:B])
        dq = _maxabs(new[0], old[0])
        print("in=%d state=%d bias=%d T=%d B=%d: vs float64 out %.3g (f10q %.3g) h_T %.3g c_T %.3g; |f10t - f10q| %.3g"
              % (inp, with_state, bias, T, B, en, eo, eh, ec, dq))
        assert torch.isfinite(new[0]).all()
        assert en <= 2e-6 and eh <= 2e-6 and ec <= 4e-6
        assert en <= 2.0 * eo + 1e-7
        assert dq <= 5e-7
        assert torch.equal(new[0], again[0]) and torch.equal(new[1][0], again[1][0]) and torch.equal(new[1][1], again[1][1])
        assert torch.equal(new[1][0], new[0][:, -1])
        assert torch.equal(last[1][0], new[0][:, -1]) and torch.equal(last[1][1], new[1][1])
        # the training forward (reserve written) equals the eval forward bit for bit
        tr = m(xb, ib)
        assert tr[0].requires_grad and torch.equal(tr[0].detach(), new[0]) and torch.equal(tr[1][1].detach(), new[1][1])
        if full is None:
            full = new
        else:      # a batch subset: samples never interact
            assert torch.equal(new[0], full[0][:B]) and torch.equal(new[1][1], full[1][1][:B])
    if max(BS) > 2:
        idx = [2, 0]
        with torch.no_grad():
            sub = m(x[idx, :T].to(dev()), None if init is None else tuple(t[idx].to(dev()) for t in init))
        assert torch.equal(sub[0], full[0][idx])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("inp", [1, 40])
def test_gradients_through_reverse_kernel(inp, with_state, bias):
    from oracle import ttrnn_oracle as O
    m = _module(inp, bias)
    B, T = max(BS), max(TS)
    x, init = _data(inp, with_state)
    _assert_routes(m, B, T)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, leaves = O.layers_from_state_dict(sd, 1, requires_grad=True, dtype=torch.float64)
    xr = x.double().clone().requires_grad_(True)
    ir = None if init is None else tuple(t.double().clone().requires_grad_(True) for t in init)
    ro, (rh, rc) = O.lstm_forward(layers, xr, ir)
    w = torch.randn(B, T, H, generator=torch.Generator().manual_seed(11))
    ((ro * w.double()).sum() + 0.5 * rh.sum() + 0.25 * rc.sum()).backward()
    m.zero_grad()
    xg = x.to(dev()).requires_grad_(True)
    ig = None if init is None else tuple(t.to(dev()).requires_grad_(True) for t in init)
    out, (hT, cT) = m(xg, ig)
    ((out * w.to(dev())).sum() + 0.5 * hT.sum() + 0.25 * cT.sum()).backward()
    pairs = [(n, p.grad, leaves[n].grad) for n, p in m.named_parameters()] + [("x", xg.grad, xr.grad)]
    if init is not None:
        pairs += [("h0", ig[0].grad, ir[0].grad), ("c0", ig[1].grad, ir[1].grad)]
    worst = 0.0
    for n, got, ref in pairs:
        e = _maxabs(got, ref) / max(float(ref.abs().max()), 1e-30)
        worst = max(worst, e)
        assert e <= 1e-4, (n, e)
    print("in=%d state=%d bias=%d: worst gradient error relative to its maximum %.3g" % (inp, with_state, bias, worst))
    m.zero_grad()


def _cfg2_module():
    torch.manual_seed(1111)
    return build_module(dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), dev())


def _both_routes_vs_exact(m, x, h0, c0, label):
    """errors of the exact mode and of the split mode in both routes against the float64 oracle + the state's scale"""
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    B, T = x.shape[0], x.shape[1]
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    layers, _ = O.layers_from_state_dict(sd, 1, dtype=torch.float64)
    with torch.no_grad():
        r64, (_, c64) = O.lstm_forward(layers, x.double(), (h0.double(), c0.double()))
    errs = {}
    for name, mode, f10q in (("exact", "exact", 0), ("f10t", "split", 0), ("f10q", "split", 1)):
        with contextlib.ExitStack() as stack:
            stack.enter_context(ttrnn_hip.fp32_math(mode))
            stack.enter_context(ttrnn_hip.option(F10Q, f10q))
            if name == "f10t":
                _assert_routes(m, B, T)
            with torch.no_grad():
                out, (hT, cT) = m(x.to(dev()), (h0.to(dev()), c0.to(dev())))
        assert torch.isfinite(out).all() and torch.isfinite(cT).all(), (label, name)
        errs[name] = max(_maxabs(out, r64), _maxabs(cT, c64))
    return errs, r64, c64


@pytest.mark.parametrize("case", ["tiny_weights", "huge_weights", "huge_h0", "zero_core", "mixed_magnitudes"])
def test_operand_ranges_both_routes(case):
    """the weight sets and bounds of test_gpu_parity.py::test_split_math_operand_ranges"""
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
                p.mul_(1e-4)
        elif case == "huge_weights":
            for p in cores:
                p.mul_(40.0)
        elif case == "huge_h0":
            h0 = torch.randn(3, 256) * 300.0
        elif case == "zero_core":
            cores[1].zero_()
        elif case == "mixed_magnitudes":
            for k, step, f in ((2, 3, 1e-6), (0, 2, 1e-5)):
                w = cores[k].detach().clone().reshape(-1)
                w[::step] *= f
                cores[k].copy_(w.reshape(cores[k].shape))
    errs, r64, c64 = _both_routes_vs_exact(m, x, h0, c0, case)
    scale = max(1e-30, float(c64.abs().max()), float(r64.abs().max()))
    print(case, "max abs error vs float64 (state scale %.3g):" % scale, errs)
    tol = 2e-3 if case in ("huge_weights", "huge_h0") else 2e-6
    for route in ("f10t", "f10q"):
        assert errs[route] <= tol * max(1.0, scale), route
        assert errs[route] <= 3.0 * errs["exact"] + 2e-7 * max(1.0, scale), route


@pytest.mark.parametrize("case", ["hid_core0_1e3", "hid_core1_1e5", "hid_corelast_1e7", "hid_corelast_1e5", "h0_unit_1e4"])
def test_outlier_up_both_routes(case):
    """the weight sets and bounds of test_gpu_parity.py::test_split_math_outlier_up (shape fused_core_r8)"""
    B, T = 3, 5
    torch.manual_seed(41)
    m = build_module(dict(kind="ttlstm", input_size=1, hidden_size=256, num_layers=1, n_cores=3, tt_rank=8), dev())
    g = torch.Generator().manual_seed(43)
    x = torch.randn(B, T, 1, generator=g)
    h0 = torch.randn(B, H, generator=g) * 0.1
    c0 = torch.randn(B, H, generator=g) * 0.3
    hid = [p for n, p in m.named_parameters() if "hidden_weights.parameters" in n]

    def bump(core, factor, pos=(7, 13)):
        with torch.no_grad():
            flat = core.detach().clone().contiguous().view(-1)
            flat[(pos[0] * flat.numel()) // pos[1]] *= factor
            core.copy_(flat.view(core.shape))

    if case == "hid_core0_1e3":
        bump(hid[0], 1e3)
    elif case == "hid_core1_1e5":
        bump(hid[1], 1e5)
    elif case == "hid_corelast_1e7":
        bump(hid[-1], 1e7)
    elif case == "hid_corelast_1e5":
        bump(hid[-1], 1e5, (5, 11))
    elif case == "h0_unit_1e4":
        h0[:, 77] *= 1e4
    errs, r64, c64 = _both_routes_vs_exact(m, x, h0, c0, case)
    scale = max(1.0, float(r64.abs().max()), float(c64.abs().max()))
    print(case, "max abs error vs float64 (state scale %.3g):" % scale, errs)
    factor = 8.0 if case == "h0_unit_1e4" else 3.0
    for route in ("f10t", "f10q"):
        assert errs[route] <= factor * errs["exact"] + 4e-7 * scale, route


def test_captured_forward_replays_bit_equal():
    m = _module(1, True)
    x, init = _data(1, True)
    B, T = max(BS), max(TS)
    _assert_routes(m, B, T)
    xs = x.to(dev())
    ib = tuple(t.to(dev()) for t in init)
    with torch.no_grad():
        eager = m(xs, ib)
        side = torch.cuda.Stream(device=dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            m(xs, ib)
        torch.cuda.current_stream(dev()).wait_stream(side)
        torch.cuda.synchronize(dev())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = m(xs, ib)
        graph.replay()
        torch.cuda.synchronize(dev())
    assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1][0], eager[1][0]) and torch.equal(cap[1][1], eager[1][1])

"""k_lstm_fwd_f10t's two time loops (ttrnn_fast_f10t.hip): the default — a unit's two fp16 pieces on adjacent rows of stage 1's A
operand, fold inside the lane — against round 7's loop (pieces eight rows apart, fold across the wave's halves), which option
f10t_r7_loop keeps selectable in the same library.  Stage 2 sums in another k order, so the two are not bit-equal; the bounds are the
ones tests/test_f10t.py uses between the two forward kernels:
    out / h_T within 2e-6 and c_T within 4e-6 of the float64 oracle, for BOTH loops;
    the default loop's error never more than twice round 7's + 1e-7; the two within 5e-7 of each other on out;
    repeat runs and batch subsets bit for bit; the final-state-only call; training forward = eval forward bit for bit.
Sizes: in in {1, 40}, B in {1, 3}, T in {1, 2, 5, 33} (both image parities, the first step's own h_0 scale, the refill of the x
chunk), with / without (h_0, c_0) and biases.  Modules, inputs and oracles are test_f10t.py's (computed once, shared, read only).
"""
import pytest
import torch

from test_f10t import TS, _assert_routes, _data, _maxabs, _module, _oracle, dev

pytestmark = pytest.mark.gpu

BS = (1, 3)
R7_LOOP = "f10t_r7_loop"       # option: round 7's time loop of k_lstm_fwd_f10t


def _eq(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("inp", [1, 40])
def test_default_loop_against_round7_loop(inp, with_state, bias, T):
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
            last = m(xb, ib, need_outputs=False)              # OUT = false: the caller consumes only the final state
            with ttrnn_hip.option(R7_LOOP, 1):
                _assert_routes(m, B, T)                       # still k_lstm_fwd_f10t
                old = m(xb, ib)
                old_again = m(xb, ib)
                old_last = m(xb, ib, need_outputs=False)
        en, eo = _maxabs(new[0], ro[:B]), _maxabs(old[0], ro[:B])
        eh, ec = _maxabs(new[1][0], rh[:B]), _maxabs(new[1][1], rc[:B])
        oh, oc = _maxabs(old[1][0], rh[:B]), _maxabs(old[1][1], rc[:B])
        dq = _maxabs(new[0], old[0])
        print("in=%d state=%d bias=%d T=%d B=%d: vs float64 out %.3g (round 7 %.3g) h_T %.3g (%.3g) c_T %.3g (%.3g); |new - round 7| %.3g"
              % (inp, with_state, bias, T, B, en, eo, eh, oh, ec, oc, dq))
        assert torch.isfinite(new[0]).all() and torch.isfinite(old[0]).all()
        assert en <= 2e-6 and eh <= 2e-6 and ec <= 4e-6
        assert eo <= 2e-6 and oh <= 2e-6 and oc <= 4e-6
        assert en <= 2.0 * eo + 1e-7
        assert dq <= 5e-7
        assert _eq(new, again) and _eq(old, old_again)
        assert torch.equal(new[1][0], new[0][:, -1]) and torch.equal(old[1][0], old[0][:, -1])
        assert torch.equal(last[1][0], new[0][:, -1]) and torch.equal(last[1][1], new[1][1])
        assert torch.equal(old_last[1][0], old[0][:, -1]) and torch.equal(old_last[1][1], old[1][1])
        # the training forward (reserve written) equals the eval forward bit for bit, in both loops
        tr = m(xb, ib)
        assert tr[0].requires_grad and torch.equal(tr[0].detach(), new[0]) and torch.equal(tr[1][1].detach(), new[1][1])
        with ttrnn_hip.option(R7_LOOP, 1):
            tr = m(xb, ib)
        assert tr[0].requires_grad and torch.equal(tr[0].detach(), old[0]) and torch.equal(tr[1][1].detach(), old[1][1])
        if full is None:
            full = (new, old)
        else:      # a batch subset: samples never interact
            for got, ref in ((new, full[0]), (old, full[1])):
                assert torch.equal(got[0], ref[0][:B]) and torch.equal(got[1][1], ref[1][1][:B])
    idx = [2, 0]
    with torch.no_grad():
        sub = m(x[idx, :T].to(dev()), None if init is None else tuple(t[idx].to(dev()) for t in init))
    assert torch.equal(sub[0], full[0][0][idx])

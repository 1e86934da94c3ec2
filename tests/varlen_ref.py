"""Expected results for calls with per-sample sequence lengths: the oracle (oracle/ttrnn_oracle.py) run PER SAMPLE on the
truncated input x[b:b+1, :len_b], losses summed, autograd for the gradients — the one definition of the semantics
(include/ttrnn.h, TTRNN_HAS_VARLEN).  Shared by tests/test_varlen_host.py (which checks this harness against the reference's
own numbers, tests/golden/g11_varlen_*.npz) and tests/test_varlen.py (which checks the GPU against it)."""
import torch

from oracle import ttrnn_oracle as O


def oracle_varlen(kind, sd, num_layers, x, lengths, h0=None, c0=None, w_out=None, w_h=None, w_c=None, dtype=torch.float32):
    """kind: 'ttlstm' / 'lstm' / 'ttgru' / 'gru'; sd: state_dict (CPU); x [B, T, in]; lengths: B ints.
    Loss: sum_b [ sum_{t < len_b} w_out[b, t] . out[b, t] + w_h[b] . hT[b] + w_c[b] . cT[b] ] over the weights that are given
    (none given: forward only).  Returns a dict: out (zero past each length), hT, cT (LSTM), and — with a loss — grads
    {parameter name: tensor}, grad_x (zero past each length), grad_h0 / grad_c0 where initial states were given."""
    lstm = kind in ("ttlstm", "lstm")
    want_grads = any(w is not None for w in (w_out, w_h, w_c))
    layers, leaves = O.layers_from_state_dict(sd, num_layers, requires_grad=want_grads, dtype=dtype)
    B, T, _ = x.shape
    assert len(lengths) == B and all(1 <= int(n) <= T for n in lengths)
    H = O._hidden_size(layers[0][1])
    res = dict(out=torch.zeros(B, T, H, dtype=dtype), hT=torch.zeros(B, H, dtype=dtype))
    if lstm:
        res["cT"] = torch.zeros(B, H, dtype=dtype)
    if want_grads:
        res["grad_x"] = torch.zeros(x.shape, dtype=dtype)
        if h0 is not None:
            res["grad_h0"] = torch.zeros(B, H, dtype=dtype)
        if lstm and c0 is not None:
            res["grad_c0"] = torch.zeros(B, H, dtype=dtype)
    for b, n in enumerate(int(v) for v in lengths):
        xb = x[b:b + 1, :n].to(dtype).clone().requires_grad_(want_grads)
        hb = None if h0 is None else h0[b:b + 1].to(dtype).clone().requires_grad_(want_grads)
        cb = None if (c0 is None or not lstm) else c0[b:b + 1].to(dtype).clone().requires_grad_(want_grads)
        with torch.set_grad_enabled(want_grads):
            if lstm:
                init = None
                if hb is not None or cb is not None:
                    zero = torch.zeros(1, H, dtype=dtype)
                    init = (hb if hb is not None else zero, cb if cb is not None else zero)
                o, (h, c) = O.lstm_forward(layers, xb, init)
            else:
                o, h = O.gru_forward(layers, xb, hb)
                c = None
        res["out"][b, :n] = o.detach()[0]
        res["hT"][b] = h.detach()[0]
        if lstm:
            res["cT"][b] = c.detach()[0]
        if not want_grads:
            continue
        loss = 0.0
        if w_out is not None:
            loss = loss + (o * w_out[b:b + 1, :n].to(dtype)).sum()
        if w_h is not None:
            loss = loss + (h * w_h[b:b + 1].to(dtype)).sum()
        if lstm and w_c is not None:
            loss = loss + (c * w_c[b:b + 1].to(dtype)).sum()
        loss.backward()              # leaf gradients accumulate over the samples
        res["grad_x"][b, :n] = xb.grad[0]
        if hb is not None and hb.grad is not None:
            res["grad_h0"][b] = hb.grad[0]
        if cb is not None and cb.grad is not None:
            res["grad_c0"][b] = cb.grad[0]
    if want_grads:
        res["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return res


def grad_bound(ref):
    """The project's gradient tolerance (tests/test_w2.py): 1e-4 of the tensor's maximum, floor 1e-3."""
    return 1e-4 * max(1e-3, float(ref.abs().max()))

"""Scale rehearsal for k_lstm_fwd_f10t (cores 0·1 contracted first) against k_lstm_fwd_f10q's order, on the CPU.

One step of the hidden-to-hidden product of cfg2's TT-LSTM (H = 256, d = 3, r = 8) is emulated in both contraction orders with the
kernels' own operand formats — two fp16 pieces per operand, fp32 accumulation, the diagonal power-of-two scales of ttrnn_f10_dev.h
(eu per i2, ev per r2, ep / ept per row of the fused core) — and compared with float64, for the weight sets of
tests/test_gpu_parity.py::test_split_math_operand_ranges and ::test_split_math_outlier_up: fresh, tiny / huge / mixed magnitudes, a
zero core, single core entries x 1e3 / 1e5 / 1e7, a huge h_0 (which the kernels bring back into (-1, 1) per sample: f10h_h0_expo).

Printed per weight set: the error of both orders relative to the largest pre-activation, max |D'| of the new order (must stay below
65 504, fp16's largest number) and the share of the fused core's second pieces that are subnormal in fp16.

    python tools/f10t_scale_sim.py

CPU only; needs nothing but numpy, torch and this repo's modules (parameters of a freshly initialised TTLSTM).
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorized-rnn_amd"))
from tensorized_rnn.tt_lstm import TTLSTM  # noqa: E402

HS_OLD, HS_NEW, ROW_EXP, G2_EXP = 6, 4, 10, 12      # F10H_HSC, F10T_HSC, F10T_ROW_EXP, core 2's 2^12 (ttrnn_f10_dev.h)
GF = np.array([-1.4426950408889634, -1.4426950408889634, 2.8853900817779268, -1.4426950408889634])      # gates i, f, g, o


def expo(x):      # f10h_expo
    if not x > 0:
        return 0
    if not x < 3e38:
        return 40
    return int(min(40, max(-40, np.frexp(np.float32(x))[1])))


def split2h(v):      # two fp16 pieces of fp32 values
    v = v.astype(np.float32)
    with np.errstate(over="ignore"):
        p0 = v.astype(np.float16)
        p1 = (v - p0.astype(np.float32)).astype(np.float16)
    return p0.astype(np.float64), p1.astype(np.float64)


def mm32(a, b):      # exact products, fp32 accumulation
    return (a.astype(np.float32) @ b.astype(np.float32)).astype(np.float64)


def cores(mod):
    sd = {k: v.detach().double().numpy() for k, v in mod.state_dict().items()}
    return [sd["cell0.hidden_weights.parameters.%d" % k].copy() for k in range(3)]      # (R_k, I_k, J_k, R_{k+1})


def evaluate(G, h):
    """G: the three cores; h [B][256] with |h| < 1.  Returns (err_new, err_old, max |D'|, subnormal share)."""
    G0, G1, G2 = [g.astype(np.float32).astype(np.float64) for g in G]
    I0, J0, I1, J1, I2, J2 = G0.shape[1], G0.shape[2], G1.shape[1], G1.shape[2], G2.shape[1], G2.shape[2]
    R2 = G2.shape[0]
    W = np.einsum("aijb,bklc->ikjlc", G0, G1).reshape(I0 * I1, J0 * J1, R2)      # [m][k = (j0, j1)][r2]
    W = W.astype(np.float32).astype(np.float64)
    G2m = G2[:, :, :, 0]                                                           # [r2][i2][j2]
    hh = h.reshape(-1, J0 * J1, J2)                                                # [b][k][j2]
    ref = np.einsum("mkr,bkj,rij->bmi", W, hh, G2m)                                # float64 pre-activations (hidden part)
    big = max(np.abs(ref).max(), 1e-300)
    gate = np.repeat(GF, I0 * I1 // 4)                                             # rows m = 16 gate + ...
    eu = np.array([-expo(np.abs(G2m[:, i, :]).max()) for i in range(I2)])
    ev = np.array([-expo((np.abs(G2m[r]) * 2.0 ** eu[:, None]).max()) for r in range(R2)])
    # ---- old order: S2 (core 2 x h), then the fused core --------------------------------------------------------------------
    ep = np.array([12 - expo((np.abs(W[m]) * 2.0 ** -ev[None, :]).max()) for m in range(W.shape[0])])
    g0, g1 = split2h(G2m * 2.0 ** (HS_OLD + eu[None, :, None] + ev[:, None, None]))
    h0, h1 = split2h(hh * 2.0 ** HS_OLD)
    X = sum(np.einsum("rij,bkj->bkri", a, b) for a, b in ((g0, h0), (g0, h1), (g1, h0), (g1, h1)))
    X = X.astype(np.float32)
    x0, x1 = split2h(X.reshape(X.shape[0], -1, I2))
    w0, w1 = split2h(W * gate[:, None, None] * 2.0 ** (ep[:, None, None] - ev[None, None, :]))
    w0, w1 = w0.reshape(W.shape[0], -1), w1.reshape(W.shape[0], -1)
    lo = np.stack([mm32(w1, a) + mm32(w0, b) for a, b in zip(x0, x1)]).astype(np.float32)
    hi = np.stack([mm32(w0, a) for a in x0])
    un = 2.0 ** -(ep[:, None] + eu[None, :] + 12.0)
    old = (hi * un + lo * un) / gate[:, None]
    # ---- new order: the fused core x h, then core 2 ---------------------------------------------------------------------------
    l1 = (np.abs(W).astype(np.float32).sum(axis=1) * 2.0 ** -ev[None, :]).max(axis=1)
    ept = np.array([ROW_EXP - expo(v) for v in l1])
    w0, w1 = split2h(W * gate[:, None, None] * 2.0 ** (ept[:, None, None] - ev[None, None, :]))
    sub = float(np.mean((np.abs(w1) < 2.0 ** -14) & (w1 != 0)))
    h0, h1 = split2h(hh * 2.0 ** HS_NEW)
    D = sum(np.einsum("mkr,bkj->bmrj", a, b) for a, b in ((w0, h0), (w1, h0), (w0, h1), (w1, h1))).astype(np.float32)
    dmax = float(np.abs(D).max())
    d0, d1 = split2h(D)
    g0, g1 = split2h(G2m * 2.0 ** (G2_EXP + eu[None, :, None] + ev[:, None, None]))
    lo = (np.einsum("bmrj,rij->bmi", d0, g1) + np.einsum("bmrj,rij->bmi", d1, g0)).astype(np.float32)
    hi = np.einsum("bmrj,rij->bmi", d0, g0).astype(np.float32)
    un = 2.0 ** -(ept[:, None] + eu[None, :] + HS_NEW + G2_EXP + 0.0)
    new = (hi * un + lo * un) / gate[:, None]
    return np.abs(new - ref).max() / big, np.abs(old - ref).max() / big, dmax, sub


def bump(core, factor, pos=(7, 13)):
    flat = core.reshape(-1)
    flat[(pos[0] * flat.size) // pos[1]] *= factor


def main():
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        mod = TTLSTM(1, 256, 1, torch.device("cpu"), n_cores=3, tt_rank=8)
    rng = np.random.default_rng(1)
    # 50 random h over four decades (|h_t| < 1), plus saturated states
    h = np.tanh(rng.standard_normal((50, 256)) * 10.0 ** rng.uniform(-4, 0, (50, 1)))
    h[-1] = np.sign(h[-1]) * (1 - 2.0 ** -24)
    sets = {}
    sets["fresh"] = cores(mod)
    sets["tiny_weights"] = [g * 1e-4 for g in cores(mod)]
    sets["huge_weights"] = [g * 40.0 for g in cores(mod)]
    z = cores(mod); z[1][:] = 0; sets["zero_core"] = z
    mx = cores(mod)
    for k, step, f in ((2, 3, 1e-6), (0, 2, 1e-5)):
        mx[k].reshape(-1)[::step] *= f
    sets["mixed_magnitudes"] = mx
    for name, k, f, pos in (("hid_core0_1e3", 0, 1e3, (7, 13)), ("hid_core1_1e5", 1, 1e5, (7, 13)),
                            ("hid_corelast_1e7", 2, 1e7, (7, 13)), ("hid_corelast_1e5", 2, 1e5, (5, 11))):
        g = cores(mod); bump(g[k], f, pos); sets[name] = g
    print("%-18s %10s %10s %10s %10s" % ("weight set", "err new", "err old", "max |D'|", "subnormal"))
    worst = 0.0
    for name, g in sets.items():
        en, eo, dmax, sub = evaluate(g, h)
        worst = max(worst, dmax)
        print("%-18s %10.3g %10.3g %10.0f %9.2f%%" % (name, en, eo, dmax, 100 * sub))
    # a huge h_0 reaches the product as 2^-e0 h_0, |.| < 1, and the accumulators are multiplied back (exact): same operands as above
    h0 = rng.standard_normal((3, 256)) * 300.0
    e0 = max(0, expo(np.abs(h0).max()))
    en, eo, dmax, sub = evaluate(sets["fresh"], h0 * 2.0 ** -e0)
    print("%-18s %10.3g %10.3g %10.0f %9.2f%%" % ("huge_h0 (2^-%d)" % e0, en, eo, dmax, 100 * sub))
    assert max(worst, dmax) < 65504.0, "stage-1 result leaves fp16"


if __name__ == "__main__":
    main()

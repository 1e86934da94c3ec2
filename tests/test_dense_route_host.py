"""Route TTRNN_ROUTE_DENSE_STEP (include/ttrnn.h, csrc/ttrnn_fast_dense.hip) without a GPU: the host-side answers of the
library for dense (nn.Linear, d = 1) LSTM / GRU descriptors, and a numpy rehearsal of the step kernels' index maps
(csrc/ttrnn_dense.h) in the manner of tests/test_f10t_layout.py.

What the rehearsal is: a second, Python statement of the maps as ttrnn_dense.h documents them, shown to be CONSISTENT — row
permutation, slot layout, K padding, plane order and the MFMA fragment layout together reproduce the plain contraction.  It reads
nothing from the .hip file and so pins nothing in it: a kernel whose indexing diverges from the documented maps is caught by the
GPU tests (tests/test_dense_route.py), not here."""
import ctypes

import numpy as np
import pytest

from ttrnn_hip import _lib
from ttrnn_hip.functional import RnnLayerSpec, TTSpec

DENSE_STEP = 5


def dense_spec(cell, inp, H, bias_in=None, bias_hid=True):
    G = 4 if cell == "lstm" else 3
    if bias_in is None:
        bias_in = cell == "gru"          # lstm.py:18,21: no bias on the input weights; gru.py:31-34: on both
    return RnnLayerSpec(cell, inp, H, TTSpec([inp], [G * H], [1, 1]), TTSpec([H], [G * H], [1, 1]), bias_in, bias_hid)


def routes(lib, d, want_state=0):
    return lib.ttrnn_rnn_forward_route(ctypes.byref(d)), lib.ttrnn_rnn_backward_route(ctypes.byref(d), want_state)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("inp,H", [(28, 128), (1, 256), (40, 768), (40, 160), (192, 192), (1, 512)])
def test_dense_descriptors_take_the_step_route(cell, inp, H):
    lib = _lib.load()
    assert _lib.ROUTES[DENSE_STEP] == "dense_step"
    d = dense_spec(cell, inp, H).desc(64, 9, 0)
    assert routes(lib, d) == (DENSE_STEP, DENSE_STEP)
    assert lib.ttrnn_rnn_backward_stats(ctypes.byref(d)) == 0
    assert lib.ttrnn_rnn_out_optional(ctypes.byref(d)) == 1
    assert lib.ttrnn_rnn_prepare_supported(ctypes.byref(d)) == 0 and lib.ttrnn_rnn_forward_cores_fused(ctypes.byref(d)) == 0


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_everything_else_keeps_its_route(cell):
    """A d = 1 descriptor outside the new route's set runs where it ran before: on the any-shape kernels, with their workspaces
    (what force_generic selects; no other family takes one-core matrices)."""
    lib = _lib.load()

    def generic_answers(d):
        with _lib.option("force_generic", 1):
            return (routes(lib, d), lib.ttrnn_rnn_workspace(ctypes.byref(d)), lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 0),
                    lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 1))

    def answers(d):
        return (routes(lib, d), lib.ttrnn_rnn_workspace(ctypes.byref(d)), lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 0),
                lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 1))

    for H in (64, 136, 96, 144):                              # below 128 / no multiple of the unit tile
        d = dense_spec(cell, 28, H).desc(3, 6, 0)
        assert answers(d) == generic_answers(d) and routes(lib, d) == (0, 0)
    d = dense_spec(cell, 28, 128).desc(3, 6, 1)               # bf16 storage
    assert answers(d) == generic_answers(d) and routes(lib, d) == (0, 0)
    d = dense_spec(cell, 28, 128).desc(3, 6, 0)
    assert routes(lib, d) == (DENSE_STEP, DENSE_STEP)
    with _lib.fp32_math("exact"):
        assert answers(d) == generic_answers(d) and routes(lib, d) == (0, 0)
    with _lib.option("force_generic", 1):
        assert routes(lib, d) == (0, 0)
    # a d_state request and a call with lengths keep their kernels
    assert lib.ttrnn_rnn_backward_route(ctypes.byref(d), 1) == 0
    with _lib.option("force_generic", 1):
        ws_state = lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 1)
        ws_varlen = lib.ttrnn_rnn_varlen_workspace(ctypes.byref(d))
    assert lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 1) == ws_state
    assert lib.ttrnn_rnn_forward_varlen_route(ctypes.byref(d)) == 0
    assert lib.ttrnn_rnn_varlen_workspace(ctypes.byref(d)) == ws_varlen
    # hid_blocks > 1 is a promise about a multi-core train: not this route
    spec = dense_spec(cell, 28, 128)
    spec.hid_blocks = 4 if cell == "lstm" else 3
    assert routes(lib, spec.desc(3, 6, 0)) == (0, 0)


def test_tt_descriptors_do_not_move():
    """d >= 2: cfg2, the speaker encoder's shape and the `tiny` descriptor of tests/test_host_api.py answer as before."""
    lib = _lib.load()
    cfg2 = RnnLayerSpec("lstm", 1, 256, TTSpec([1, 1, 1], [8, 8, 16], [1, 8, 8, 1]), TTSpec([4, 8, 8], [8, 8, 16], [1, 8, 8, 1]),
                        True, True).desc(64, 784, 0)
    assert routes(lib, cfg2) == (2, 2)
    assert lib.ttrnn_rnn_workspace(ctypes.byref(cfg2)) == 2 * 256 * 4 * 4 + 256 + 4 * 8 * 3 * 1024
    enc = RnnLayerSpec("lstm", 40, 768, TTSpec([5, 8], [48, 64], [1, 2, 1]), TTSpec([24, 32], [48, 64], [1, 2, 1]),
                       True, True).desc(64, 160, 0)
    assert routes(lib, enc) == (2, 2)
    assert lib.ttrnn_rnn_forward_varlen_route(ctypes.byref(enc)) == 2
    tiny = RnnLayerSpec("gru", 28, 64, TTSpec([4, 7], [12, 16], [1, 3, 1]), TTSpec([8, 8], [12, 16], [1, 3, 1]),
                        True, True).desc(3, 6, 0)
    assert routes(lib, tiny) == (4, 4)
    # a TT layer of a dense-eligible H stays a TT layer
    tt128 = RnnLayerSpec("lstm", 28, 128, TTSpec([4, 7], [16, 32], [1, 4, 1]), TTSpec([8, 16], [16, 32], [1, 4, 1]),
                         True, True).desc(3, 6, 0)
    assert DENSE_STEP not in routes(lib, tt128)


@pytest.mark.parametrize("cell,G", [("lstm", 4), ("gru", 3)])
@pytest.mark.parametrize("inp,H,B", [(28, 128, 3), (1, 256, 64), (40, 768, 512), (33, 160, 70)])
def test_workspace_formulas(cell, G, inp, H, B):
    """include/ttrnn.h: 24 (Kxp + H) H + 24 Bp H forward, 6 G H H + 12 Bp G H + 4 Bp H reverse."""
    lib = _lib.load()
    d = dense_spec(cell, inp, H).desc(B, 7, 0)
    Bp, Kxp = (B + 31) // 32 * 32, (inp + 31) // 32 * 32
    fwd = lib.ttrnn_rnn_workspace(ctypes.byref(d))
    bwd = lib.ttrnn_rnn_backward_workspace_ex(ctypes.byref(d), 0)
    assert fwd == 24 * (Kxp + H) * H + 24 * Bp * H > 0
    assert bwd == 6 * G * H * H + 12 * Bp * G * H + 4 * Bp * H > 0
    assert lib.ttrnn_rnn_backward_workspace(ctypes.byref(d)) >= bwd
    # too small a workspace and NULL operands are refused before anything is launched
    assert lib.ttrnn_rnn_forward(ctypes.byref(d), *([None] * 12), 0, None) == -2


# ---- numpy rehearsal of the index maps (csrc/ttrnn_dense.h) ---------------------------------------------------------------------
LSTM_GATE_OF_SLOT = (0, 2, 1, 3)      # slots i, g, f, o of gates i, f, g, o


def pieces(v):
    """Three float64 'pieces' with v = p0 + p1 + p2 exactly enough for the test: the kernels' bf16 pieces differ in size by 2^-8
    per level, here by ~1e-3."""
    p0 = np.round(v, 3)
    p1 = np.round(v - p0, 6)
    return [p0, p1, v - p0 - p1]


SIX_TERMS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))      # (activation piece, weight piece)


def mfma(a_frag, b_frag):
    """v_mfma_f32_16x16x32: lane (n, q) = n + 16 q holds A[row n][k = 8 q + e] and B[k = 8 q + e][col n]; D[m][n]."""
    A = a_frag.reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)      # [row][k]
    Bm = b_frag.reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)     # [col][k]
    return A @ Bm.T


def wcat(cell, slot, unit, k, inp, H, Kxp, Win, Whh):
    """column k of [W_in ; W_hh] for (slot, unit); Win [G H][in], Whh [G H][H] as nn.Linear stores them"""
    xseg = k < Kxp
    if cell == "gru":
        if (slot == 2 and not xseg) or (slot == 3 and xseg):
            return 0.0
        gate = 2 if slot == 3 else slot
    else:
        gate = LSTM_GATE_OF_SLOT[slot]
    col = gate * H + unit
    if xseg:
        return Win[col, k] if k < inp else 0.0
    return Whh[col, k - Kxp]


def wf_planes(cell, inp, H, Win, Whh):
    Kxp = (inp + 31) // 32 * 32
    nkb = (Kxp + H) // 32
    dense = np.zeros((H // 16, nkb, 4, 64, 8))
    for ut in range(H // 16):
        for kb in range(nkb):
            for slot in range(4):
                for lane in range(64):
                    n, q = lane & 15, lane >> 4
                    for e in range(8):
                        dense[ut, kb, slot, lane, e] = wcat(cell, slot, 16 * ut + n, 32 * kb + 8 * q + e, inp, H, Kxp, Win, Whh)
    p = pieces(dense)
    return np.stack(p, axis=3)            # [ut][kb][slot][piece][lane][8]


def a_fragment(plane, row0, col0):
    """lane (n, q) reads 8 consecutive elements of row row0 + n at column col0 + 8 q of a row-major plane"""
    return plane[row0:row0 + 16, col0:col0 + 32].reshape(16, 4, 8).transpose(1, 0, 2).reshape(64, 8)


def fwd_step_rehearsal(cell, inp, H, B, x_t, hprev, Win, Whh):
    """returns the gate-slot accumulators [B][H][4] the epilogue sees"""
    Kxp = (inp + 31) // 32 * 32
    nkx, nkb = Kxp // 32, (Kxp + H) // 32
    Bp = (B + 31) // 32 * 32
    WF = wf_planes(cell, inp, H, Win, Whh)
    xpad = np.zeros((Bp, Kxp))
    xpad[:B, :inp] = x_t
    xp = pieces(xpad)
    hp = [np.full((Bp, H), np.nan) for _ in range(3)]          # rows >= B are never initialised
    for k, p in enumerate(pieces(hprev)):
        hp[k][:B] = p
    acc = np.zeros((B, H, 4))
    for by in range(Bp // 32):
        for bx in range(H // 32):
            for wave in range(4):
                ut = bx * 2 + (wave >> 1)
                row0 = by * 32 + 16 * (wave & 1)
                D = np.zeros((4, 16, 16))
                for kb in range(nkb):
                    xseg = kb < nkx
                    for slot in range(4):
                        if cell == "gru" and ((xseg and slot == 3) or (not xseg and slot == 2)):
                            continue
                        for (pa, pw) in SIX_TERMS:
                            a = a_fragment(xp[pa], row0, 32 * kb) if xseg else a_fragment(hp[pa], row0, 32 * (kb - nkx))
                            D[slot] += mfma(a, WF[ut, kb, slot, pw])
                for lane in range(64):          # D layout: lane (n, q), register i <-> row 4 q + i, column n
                    n, q = lane & 15, lane >> 4
                    for i in range(4):
                        r = row0 + 4 * q + i
                        if r < B:
                            acc[r, 16 * ut + n] = D[:, 4 * q + i, n]
    return acc


def six_term(a_pieces, w_pieces):
    return sum(a_pieces[pa] @ w_pieces[pw] for (pa, pw) in SIX_TERMS)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("inp,H,B", [(1, 128, 3), (28, 160, 5), (40, 128, 33)])
def test_forward_step_index_maps(cell, inp, H, B):
    rng = np.random.default_rng(inp + H)
    G = 4 if cell == "lstm" else 3
    Win, Whh = rng.standard_normal((G * H, inp)), rng.standard_normal((G * H, H))
    x_t, hprev = rng.standard_normal((B, inp)), rng.standard_normal((B, H))
    acc = fwd_step_rehearsal(cell, inp, H, B, x_t, hprev, Win, Whh)
    assert np.isfinite(acc).all()           # the uninitialised rows never reach a stored element
    xs, hs = pieces(x_t), pieces(hprev)
    gi = six_term(xs, [p.T for p in pieces(Win)])          # [B][G H] in the reference's gate order
    gh = six_term(hs, [p.T for p in pieces(Whh)])
    if cell == "lstm":
        want = np.stack([(gi + gh)[:, g * H:(g + 1) * H] for g in LSTM_GATE_OF_SLOT], axis=2)      # record order i, g, f, o
    else:
        want = np.stack([(gi + gh)[:, :H], (gi + gh)[:, H:2 * H], gi[:, 2 * H:], gh[:, 2 * H:]], axis=2)
    assert np.abs(acc - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # and the six terms are the product to the pieces' third order
    full = x_t @ Win.T + hprev @ Whh.T
    assert np.abs((gi + gh) - full).max() <= 1e-5 * np.abs(full).max()


def wr_planes(H, G, Whh):
    nkr = G * H // 32
    dense = np.zeros((H // 16, nkr, 64, 8))
    for ut in range(H // 16):
        for kb in range(nkr):
            for lane in range(64):
                n, q = lane & 15, lane >> 4
                for e in range(8):
                    dense[ut, kb, lane, e] = Whh[32 * kb + 8 * q + e, 16 * ut + n]       # the transposed half Wt[c][j]
    return np.stack(pieces(dense), axis=2)       # [ut][kb][piece][lane][8]


@pytest.mark.parametrize("G", [4, 3])
@pytest.mark.parametrize("H,B", [(128, 3), (160, 33)])
def test_reverse_step_index_maps(G, H, B):
    """dh[b][u] = sum_c dg_hid[b][c] W_hh[c][u]: K = G H in k-blocks of 32 (G H / 32 is odd at G = 3, H = 160)."""
    rng = np.random.default_rng(G * H)
    Whh = rng.standard_normal((G * H, H))
    dg = rng.standard_normal((B, G * H))
    Bp = (B + 31) // 32 * 32
    WR = wr_planes(H, G, Whh)
    dp = [np.full((Bp, G * H), np.nan) for _ in range(3)]
    for k, p in enumerate(pieces(dg)):
        dp[k][:B] = p
    dh = np.zeros((B, H))
    for by in range(Bp // 32):
        for bx in range(H // 32):
            for wave in range(4):
                ut, row0 = bx * 2 + (wave >> 1), by * 32 + 16 * (wave & 1)
                D = np.zeros((16, 16))
                for kb in range(G * H // 32):
                    for (pa, pw) in SIX_TERMS:
                        D += mfma(a_fragment(dp[pa], row0, 32 * kb), WR[ut, kb, pw])
                for lane in range(64):
                    n, q = lane & 15, lane >> 4
                    for i in range(4):
                        if row0 + 4 * q + i < B:
                            dh[row0 + 4 * q + i, 16 * ut + n] = D[4 * q + i, n]
    want = six_term(pieces(dg), pieces(Whh))
    assert np.isfinite(dh).all()
    assert np.abs(dh - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(want - dg @ Whh).max() <= 1e-5 * np.abs(dg @ Whh).max()


# ---- fixtures generated from the reference (tests/golden/gen_golden_dense.py) ----------------------------------------------------
@pytest.mark.parametrize("name", ["g11_dense_lstm", "g11_dense_gru"])
def test_oracle_reproduces_the_dense_fixtures(name):
    """the project's fixture rule (tests/test_oracle_golden.py): forward <= 1e-6 abs, gradients <= 1e-5 of the tensor's maximum"""
    import os

    import test_oracle_golden as rule
    from golden_io import GOLDEN, Case
    case = Case(name)
    assert case.meta["input_size"] == 28 and case.meta["hidden_size"] == 128 and (case.meta["B"], case.meta["T"]) == (3, 6)
    for key in ("out", "hT", "grad_x", "grad_h0", "grad/cell0.input_weights.weight", "grad/cell0.hidden_weights.weight",
                "grad/cell0.hidden_weights.bias"):
        assert key in case.arr, key
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz") and "g11_dense" not in f)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < largest
    rule.test_torch_oracle_gradients(name)

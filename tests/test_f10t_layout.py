"""Host-side rehearsal of k_lstm_fwd_f10t's time loop with a unit's two pieces on adjacent MFMA rows (ttrnn_fast_f10t.hip, ADJ):
a numpy emulation of the v_mfma_f32_16x16x32_f16 lane maps applied to the h image in LDS, the fold inside the lane and core 2's
fragment order, for one step on random float64 data, against the dense contraction
    out[m][i2] = sum_{k, r2, j2} W10[m][k][r2] h[k][j2] G2[r2][j2][i2].
float64 throughout (the pieces are an arbitrary exact two-term split of h), so agreement is to rounding of float64: the bound is
64 x 32 x 2 terms' worth of eps relative to the sum of the terms' magnitudes.  Also: every (r2, j2) exactly once over stage 2's
k index, every image slot written exactly once, the 16-byte alignment of the fragment read, and the bank-conflict degree of the row
read and of the piece writes by the LDS rules (ds_read_b128: four 16-lane groups over 64 banks; ds_write_b16: the wave's two halves
over 32 banks; accesses to one dword do not conflict).  No GPU."""
import numpy as np
import pytest

J2, R2, I2, K, M = 8, 8, 16, 32, 64       # H = 256, d = 3, r = 8: h[k = (j0, j1)][j2], fused core W10[m][k][r2], core 2 G2[r2][j2][i2]
ROW = 48                                  # F10T_ROW: halves from one image row to the next
PAR = 16 * ROW                            # halves per parity


# ---- the index formulas of the device code, restated ------------------------------------------------------------------------------
def img_off(row, k):
    """f10t_img_off (ttrnn_f10_dev.h): halves from the parity's base to (row = 2 j2 + piece, k)"""
    return row * ROW + 8 * ((k >> 3) ^ ((row >> 2) & 3)) + (k & 7)


def unit_of(wave, lane):
    """k_lstm_fwd_f10t: hd = (4 wave + q) I2 + c, the hidden unit whose gates and state lane (c, q) of the wave owns"""
    return (4 * wave + (lane >> 4)) * I2 + (lane & 15)


def unit_store_off(hd):
    """k_lstm_fwd_f10t, hoff: the unit's first piece at (row 2 j2, k) with (j2, k) = (hd & 7, hd >> 3); second piece: + ROW"""
    return img_off(2 * (hd & 7), hd >> 3)


def frag_read_off(lane):
    """k_lstm_fwd_f10t, aoff: the lane's stage-1 A fragment = eight halves at (row c, k = 8 q)"""
    return img_off(lane & 15, 8 * (lane >> 4))


def w10_row(wave, c):
    """f10t_build_w10: the row m of the fused core in column c of the wave's stage-1 B operand"""
    return 16 * (c & 3) + 4 * wave + (c >> 2)


def g2_index(kb, q, j):
    """f10t_load_g2<S, true>: (r2, j2) of element j of k-block kb in lane group q"""
    return 4 * kb + (j >> 1), 2 * q + (j & 1)


def fold_slot(r2):
    """k_lstm_fwd_f10t, the fold: tile r2 fills dword r2 & 3 (elements 2 (r2 & 3), + 1) of k-block r2 >> 2 of stage 2's A operand"""
    return r2 >> 2, 2 * (r2 & 3)


# ---- v_mfma_f32_16x16x32_f16: A[row = lane & 15][k = 8 (lane >> 4) + e], B[k = 8 (lane >> 4) + e][col = lane & 15],
#      D[row = 4 (lane >> 4) + reg][col = lane & 15] --------------------------------------------------------------------------------
def mfma(a_frag, b_frag, acc):
    """a_frag, b_frag: [64 lanes][8]; acc: [64 lanes][4]"""
    A = np.zeros((16, 32))
    B = np.zeros((32, 16))
    for lane in range(64):
        for e in range(8):
            A[lane & 15, 8 * (lane >> 4) + e] = a_frag[lane, e]
            B[8 * (lane >> 4) + e, lane & 15] = b_frag[lane, e]
    D = A @ B
    out = acc.copy()
    for lane in range(64):
        for reg in range(4):
            out[lane, reg] += D[4 * (lane >> 4) + reg, lane & 15]
    return out


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(8)
    h = rng.standard_normal((K, J2))
    p0 = np.round(h * 64.0) / 64.0            # an exact two-term split: p0 + p1 == h
    p1 = h - p0
    assert np.array_equal(p0 + p1, h)
    W10 = rng.standard_normal((M, K, R2))
    G2 = rng.standard_normal((R2, J2, I2))
    return h, p0, p1, W10, G2


def _image(p0, p1):
    img = np.full(PAR, np.nan)
    written = np.zeros(PAR, dtype=int)
    for wave in range(4):
        for lane in range(64):
            hd = unit_of(wave, lane)
            j2, k = hd & 7, hd >> 3
            off = unit_store_off(hd)
            assert off + ROW == img_off(2 * j2 + 1, k)
            img[off], img[off + ROW] = p0[k, j2], p1[k, j2]
            written[off] += 1
            written[off + ROW] += 1
    return img, written


def test_image_slots():
    p = np.arange(K * J2, dtype=float).reshape(K, J2)
    _, written = _image(p, p)
    assert written.max() == 1 and written.sum() == 2 * K * J2          # 512 slots, each once; the rest is padding
    used = {img_off(row, k) for row in range(16) for k in range(K)}
    assert used == set(np.nonzero(written)[0]) and max(used) < PAR
    for lane in range(64):
        assert (2 * frag_read_off(lane)) % 16 == 0                        # ds_read_b128 on its natural alignment
        row, q = lane & 15, lane >> 4
        assert [frag_read_off(lane) + e for e in range(8)] == [img_off(row, 8 * q + e) for e in range(8)]


def test_every_r2_j2_once():
    seen = {}
    for kb in range(2):
        for q in range(4):
            for j in range(8):
                seen.setdefault(g2_index(kb, q, j), []).append((kb, q, j))
    assert sorted(seen) == [(r2, j2) for r2 in range(R2) for j2 in range(J2)]
    assert all(len(v) == 1 for v in seen.values())
    # and the fold delivers exactly that pair to that element: tile r2, lane group q, registers (0, 1) -> j2 = 2 q, (2, 3) -> 2 q + 1
    for r2 in range(R2):
        kb, j = fold_slot(r2)
        for q in range(4):
            assert g2_index(kb, q, j) == (r2, 2 * q) and g2_index(kb, q, j + 1) == (r2, 2 * q + 1)


def test_one_step_against_dense(data):
    h, p0, p1, W10, G2 = data
    img, _ = _image(p0, p1)
    dense = np.einsum("mkr,kj,rji->mi", W10, h, G2)
    mag = np.einsum("mkr,kj,rji->mi", np.abs(W10), np.abs(p0) + np.abs(p1), np.abs(G2))
    got = np.full((M, I2), np.nan)
    for wave in range(4):
        ha = np.array([[img[frag_read_off(lane) + e] for e in range(8)] for lane in range(64)])
        a2 = np.zeros((2, 64, 8))                                          # stage 2's A operand [k-block][lane][element]
        for r2 in range(R2):
            wb = np.array([[W10[w10_row(wave, lane & 15), 8 * (lane >> 4) + e, r2] for e in range(8)] for lane in range(64)])
            d = mfma(ha, wb, np.zeros((64, 4)))
            # rows of the tile: register 0/1 = first / second piece of j2 = 2 q, 2/3 of j2 = 2 q + 1
            for lane in range(64):
                q, m = lane >> 4, w10_row(wave, lane & 15)
                for reg in range(4):
                    j2, piece = 2 * q + (reg >> 1), reg & 1
                    want = W10[m, :, r2] @ (p0, p1)[piece][:, j2]
                    assert abs(d[lane, reg] - want) <= 1e-13 * (np.abs(W10[m, :, r2]) @ np.abs(h[:, j2]) + 1.0)
            kb, j = fold_slot(r2)
            a2[kb, :, j] = d[:, 0] + d[:, 1]
            a2[kb, :, j + 1] = d[:, 2] + d[:, 3]
        acc = np.zeros((64, 4))
        for kb in range(2):
            gb = np.zeros((64, 8))
            for lane in range(64):
                for j in range(8):
                    r2, j2 = g2_index(kb, lane >> 4, j)
                    gb[lane, j] = G2[r2, j2, lane & 15]
            acc = mfma(a2[kb], gb, acc)
        # result rows = stage 1's columns: lane (c, q), register g <- column 4 q + g = row m = 16 g + 4 wave + q: gate g of unit hd
        for lane in range(64):
            c, q = lane & 15, lane >> 4
            for g in range(4):
                m = w10_row(wave, 4 * q + g)
                assert m == 16 * g + unit_of(wave, lane) // I2 and c == unit_of(wave, lane) % I2
                assert np.isnan(got[m, c])
                got[m, c] = acc[lane, g]
    assert not np.isnan(got).any()
    eps = np.finfo(np.float64).eps
    assert (np.abs(got - dense) <= 2 * K * R2 * J2 * eps * mag).all()


# ---- bank conflicts by the LDS rules ------------------------------------------------------------------------------------------------
READ_B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
READ_B128_GROUPS += [[l + 32 for l in g] for g in READ_B128_GROUPS]
WRITE_GROUPS = [list(range(32)), list(range(32, 64))]


def _degree(groups, byte_addr, width, banks):
    worst = 1
    for g in groups:
        per_bank = {}
        for lane in g:
            a = byte_addr(lane)
            for dword in range(a // 4, (a + width + 3) // 4):
                per_bank.setdefault(dword % banks, set()).add(dword)
        worst = max(worst, max(len(s) for s in per_bank.values()))
    return worst


def test_lds_conflict_degree():
    assert _degree(READ_B128_GROUPS, lambda lane: 2 * frag_read_off(lane), 16, 64) == 1
    for wave in range(4):
        for piece in range(2):
            assert _degree(WRITE_GROUPS, lambda lane: 2 * (unit_store_off(unit_of(wave, lane)) + piece * ROW), 2, 32) == 1
    # what the padding and the XOR buy: 64-byte rows, chunks in place
    flat = lambda row, k: row * 32 + k
    assert _degree(READ_B128_GROUPS, lambda lane: 2 * flat(lane & 15, 8 * (lane >> 4)), 16, 64) == 2
    assert _degree(WRITE_GROUPS, lambda lane: 2 * flat(2 * (unit_of(0, lane) & 7), unit_of(0, lane) >> 3), 2, 32) == 8

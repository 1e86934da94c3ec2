"""Shared by tests/test_ge2e_eer_host.py and tests/test_ge2e_eer.py: the oracle `eer_exact` (a numpy / Fraction restatement of the
EER's definition on exact integers that shares no code with tensorized-rnn_amd/csrc/ttrnn_eer.h), the seeded score builders, the
shapes, and the three assertions every route is held to."""
import functools
import math
from fractions import Fraction

import numpy as np

# the smallest shapes at which a mechanism can break
SHAPES = [
    (2, 1),        # smallest legal shape; U = 1
    (3, 7),        # row length below a wave
    (65, 3),       # one past 64
    (16, 32),      # the reference's training batch
    (64, 10),      # the README's GE2E layout
    (40, 32),      # the reference's validation batch
    (300, 2),      # S > 256
]
LARGE = (2048, 2)  # the S limit; 8.4 M scores; Nn P > 2^32: the 64-bit products
BUILDERS = ["clustered", "ties_half", "ties_int", "all_equal", "separated", "inverted", "signed_zeros", "negatives", "wide",
            "subnormal", "low_byte", "nan_last"]
NO_HOST_ROUTE = ("wide", "nan_last")      # +-inf / NaN: roc_curve refuses them
CASES = [(b, sh) for sh in SHAPES for b in BUILDERS]
LARGE_CASE = ("clustered", LARGE)
MAX_WORKGROUPS = 256                      # the cap include/ttrnn.h states for ttrnn_eer_desc.workgroups
EER_TOL = 2.0 ** -50                      # four double roundings of at most 2^-53 on values at most 1, with a factor 2
HOST_TOL = 4e-12                          # twice brentq's default xtol


def case_id(case):
    return "%s-S%d-U%d" % (case[0], case[1][0], case[1][1])


def positives(S, U):
    """bool [S, U, S]: element [s, u, j] is a positive iff j == s."""
    return np.broadcast_to(np.eye(S, dtype=bool)[:, None, :], (S, U, S))


def _canonical(flat):
    """float32 with -0 as +0, by bits (never through arithmetic, which a flush-to-zero mode would bend)."""
    bits = np.ascontiguousarray(flat, dtype=np.float32).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    return bits.view(np.float32)


def eer_exact(sim):
    """(eer float64, theta float32, (tp', fp', tp, fp)) of a float32 [S, U, S] matrix.  Distinct values by np.unique (+0 and -0
    are one value, reported as +0), counts as Python ints, the final expression as a Fraction rounded once to float64.  A NaN
    anywhere: (nan, nan, (-1, -1, -1, -1))."""
    S, U, _ = sim.shape
    flat = _canonical(sim.reshape(-1))
    if np.isnan(flat).any():
        return float("nan"), np.float32("nan"), (-1, -1, -1, -1)
    lab = positives(S, U).reshape(-1)
    P, Nn = S * U, S * U * (S - 1)
    vals, inv = np.unique(flat, return_inverse=True)
    inv = inv.reshape(-1)
    hp = np.bincount(inv[lab], minlength=len(vals))[::-1]
    hn = np.bincount(inv[~lab], minlength=len(vals))[::-1]
    ctp, cfp = np.cumsum(hp, dtype=np.int64), np.cumsum(hn, dtype=np.int64)      # at or above the k-th largest value

    def holds(k):
        return int(cfp[k]) * P + int(ctp[k]) * Nn >= Nn * P

    lo, hi = 0, len(vals) - 1      # the left side grows with k and holds at the smallest value: first k that holds
    assert holds(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        if holds(mid):
            hi = mid
        else:
            lo = mid + 1
    k = lo
    tp, fp = int(ctp[k]), int(cfp[k])
    tp0, fp0 = (int(ctp[k - 1]), int(cfp[k - 1])) if k else (0, 0)
    a = Nn * P - (fp0 * P + tp0 * Nn)
    b = (fp - fp0) * P + (tp - tp0) * Nn
    e = (fp0 + Fraction(a, b) * (fp - fp0)) / Nn
    return float(e), np.float32(vals[::-1][k]), (tp0, fp0, tp, fp)


def _clustered(S, U, rng):
    x = rng.normal(0.2, 0.2, size=(S, U, S))
    return np.where(positives(S, U), x + 0.4, x)


def build(name, S, U):
    """float32 [S, U, S], seeded per (builder, shape)."""
    rng = np.random.default_rng([BUILDERS.index(name), S, U])
    pos = positives(S, U)
    if name in ("clustered", "nan_last"):
        x = _clustered(S, U, rng)
    elif name == "ties_half":
        x = np.clip(np.round(2 * (rng.normal(0, 1, size=(S, U, S)) + pos)) / 2, -3, 4)
    elif name == "ties_int":
        x = np.clip(np.round(rng.normal(0, 1, size=(S, U, S)) + pos), -3, 4)
    elif name == "all_equal":
        x = np.full((S, U, S), 0.25)
    elif name == "separated":
        x = rng.random((S, U, S)) + 2 * pos
    elif name == "inverted":
        x = rng.random((S, U, S)) + 2 * ~pos
    elif name == "signed_zeros":
        x = np.where(rng.random((S, U, S)) < 0.5, 0.0, -0.0)
    elif name == "negatives":
        x = _clustered(S, U, rng) - 3.0
    elif name == "wide":
        x = np.where(rng.random((S, U, S)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-30, 30, size=(S, U, S))
        x.reshape(-1)[1] = np.inf
        x.reshape(-1)[2] = -np.inf
    elif name == "subnormal":       # k 2^-149, k = 1 .. 3000: by bits
        k = rng.integers(1, 2000, size=(S, U, S)) + 1000 * pos
        return k.astype(np.uint32).view(np.float32)
    elif name == "low_byte":        # 1 + k 2^-23, k = 0 .. 255
        k = np.minimum(rng.integers(0, 226, size=(S, U, S)) + 30 * pos, 255)
        return (np.uint32(0x3f800000) + k.astype(np.uint32)).view(np.float32)
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if name == "nan_last":
        x.reshape(-1)[-1] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """(sim, exact) of one case, computed once and shared (callers must not modify either); asserts first that the case is
    what it claims to be."""
    S, U = shape
    sim = build(name, S, U)
    assert sim.dtype == np.float32 and sim.shape == (S, U, S) and sim.flags.c_contiguous
    sim.setflags(write=False)
    exact = eer_exact(sim)
    e, theta, (tp0, fp0, tp, fp) = exact
    P, Nn, N = S * U, S * U * (S - 1), S * U * S
    flat, bits = sim.reshape(-1), sim.reshape(-1).view(np.uint32)
    if name in ("ties_half", "ties_int"):
        bound = 15 if name == "ties_half" else 8
        assert len(np.unique(flat)) <= bound
        assert len(np.unique(flat)) < N or N <= bound
    elif name == "all_equal":
        assert e == 0.5 and (tp0, fp0, tp, fp) == (0, 0, P, Nn)
    elif name == "separated":
        assert e == 0.0 and fp == 0 and tp == P
    elif name == "inverted":
        assert e == 1.0 and tp == 0 and fp == Nn
    elif name == "signed_zeros":
        assert not flat.any() and e == 0.5 and theta == 0 and (tp0, fp0, tp, fp) == (0, 0, P, Nn)
        assert (bits == 0).any() and (bits == 0x80000000).any()
    elif name == "negatives":
        assert (flat < 0).all()
    elif name == "wide":
        assert np.isposinf(flat).sum() == 1 and np.isneginf(flat).sum() == 1
        for sh in (24, 16, 8, 0):
            assert len(np.unique((bits >> sh) & 255)) > 1
    elif name == "subnormal":
        assert ((bits > 0) & (bits < 0x00800000)).all() and (len(np.unique(bits)) > 1 or N < 8)
    elif name == "low_byte":
        assert len(np.unique(bits >> 8)) == 1
    elif name == "nan_last":
        assert np.isnan(flat[-1]) and not np.isnan(flat[:-1]).any() and math.isnan(e)
    if shape == LARGE:
        assert Nn * P > 2 ** 32
    return sim, exact


def check(got, exact, label):
    """got = (eer float, theta float32 scalar, counts of 4 ints): theta bit for bit (NaN for NaN), counts exactly, the EER to
    2^-50.  Prints the figures before asserting."""
    e, theta, counts = got
    xe, xtheta, xcounts = exact
    print("%s: eer %.17g exact %.17g diff %.3e  theta %r exact %r  counts %s exact %s" % (
        label, e, xe, abs(e - xe), float(theta), float(xtheta), tuple(counts), tuple(xcounts)))
    assert tuple(int(c) for c in counts) == tuple(xcounts), label
    if math.isnan(xe):
        assert math.isnan(e) and np.isnan(theta), label
        return
    assert np.float32(theta).view(np.uint32) == np.float32(xtheta).view(np.uint32), label
    assert abs(e - xe) <= EER_TOL, label


def grid_counts(S, U):
    """route 2's workgroup counts for one shape: 1, 2, 3, 7, a count that does not divide the S U S scores and — where the cap
    of 256 workgroups allows it — more workgroups than the matrix has rows."""
    N, rows = S * U * S, S * U
    out = [1, 2, 3, 7, next(g for g in (5, 11, 13, 3) if N % g)]
    if rows + 1 <= MAX_WORKGROUPS:
        out.append(rows + 1)
    return out

"""Shared by tests/test_optim_host.py and tests/test_optim.py: the tables and cases of the fused gradient scaling / norm clipping /
Adam step (include/ttrnn.h, TTRNN_HAS_OPTIM), a float64 evaluation of the header's formulas on the same fp32 inputs, torch's own
fp32 path (clip_grad_norm_ + torch.optim.Adam) on them, and the project's accuracy rule:

    max |err| <= max(4 x the error of torch's fp32 path on the same inputs, 2^-19 x max |reference|)

for each of p, m, v, the written-back g and total_norm.  Every hyper-parameter is a float32 value (the descriptor holds floats),
handed to torch as the same number, so both paths and the oracle start from identical inputs."""
import functools
import os
import re

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def header_define(name):
    text = open(os.path.join(ROOT, "include", "ttrnn.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


CHUNK = header_define("TTRNN_OPTIM_CHUNK")
GROUP = header_define("TTRNN_OPTIM_GROUP")


def f32(x):
    return float(np.float32(x))


BETA1, BETA2, EPS = f32(0.9), f32(0.999), f32(1e-8)
SCALE = f32(0.01)


@functools.lru_cache(maxsize=None)
def table(name):
    """T1: chunk edges, one-element tensors, a tensor of three chunks.  T2: one tensor more than an argument group holds, sizes
    cycling 1 .. 7 with one of 1025.  T3: the reference's encoder layer (TTLSTM(40, 768, 1, n_cores=2, tt_rank=2)), its head and
    the two similarity scalars."""
    if name == "T1":
        return (1, 1, 3, 1023, 1024, 1025, 2049, 1)
    if name == "T2":
        return tuple(1025 if i == 77 else 1 + i % 7 for i in range(GROUP + 1))
    if name == "T3":
        return tuple(p.numel() for p in encoder("cpu").parameters())
    raise KeyError(name)


def encoder(device, seed=3):
    import contextlib
    import io
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from models import SpeakerEncoder
    torch.manual_seed(seed)
    dev = torch.device(device)
    with contextlib.redirect_stdout(io.StringIO()):
        return SpeakerEncoder(40, 768, 1, 256, dev, n_cores=2, rank=2).to(dev)


TABLES = ("T1", "T2", "T3")

# name: max_norm (None = off), grad_scale on the last two tensors, weight decay, lr, steps, counter on entry, gradient magnitude
CASES = {
    "below": dict(max_norm=3.0, gmag=1e-3),                       # the norm stays below max_norm: coef is exactly 1
    "above": dict(max_norm=0.5, gmag=1e2),
    "clip_off": dict(max_norm=None),
    "scales": dict(max_norm=3.0, scales=True),
    "decay": dict(max_norm=3.0, wd=f32(1e-2), lr=f32(1e-2)),
    "steps2": dict(max_norm=3.0, steps=2),
    "steps50": dict(max_norm=3.0, steps=50, scales=True),
    "counter1000": dict(max_norm=3.0, step0=1000),
    "counter1e6": dict(max_norm=3.0, step0=10 ** 6),
}
SPECIALS = ("zero", "inf", "nan")


class Problem(object):
    """One case on one table: the fp32 inputs (per tensor), and — computed once, never modified — the float64 reference and
    torch's fp32 results after the last step."""

    def __init__(self, tname, cname, special=None):
        spec = dict(max_norm=3.0, scales=False, wd=0.0, lr=f32(1e-3), steps=1, step0=0, gmag=1.0)
        spec.update(CASES[cname])
        self.name = "%s-%s%s" % (tname, cname, "-" + special if special else "")
        self.numel = table(tname)
        n = len(self.numel)
        self.max_norm, self.wd, self.lr, self.steps, self.step0 = spec["max_norm"], spec["wd"], spec["lr"], spec["steps"], spec["step0"]
        self.scales = [SCALE if (spec["scales"] and i >= n - 2) else 1.0 for i in range(n)]
        rng = np.random.default_rng(sum(map(ord, tname + cname)))      # (hash() of a string changes from process to process)
        self.P0 = [(0.3 * rng.standard_normal(k)).astype(np.float32) for k in self.numel]
        # gradients of mixed magnitudes: two decades below gmag
        self.grads = [[(spec["gmag"] * rng.standard_normal(k) * 10.0 ** rng.uniform(-2, 0, k)).astype(np.float32) for k in self.numel]
                      for _ in range(self.steps)]
        if self.step0:       # a run in progress: moments of the gradients' size
            self.M0 = [(0.1 * spec["gmag"] * rng.standard_normal(k)).astype(np.float32) for k in self.numel]
            self.V0 = [(0.01 * spec["gmag"] ** 2 * rng.uniform(0.01, 1, k)).astype(np.float32) for k in self.numel]
        else:
            self.M0 = [np.zeros(k, np.float32) for k in self.numel]
            self.V0 = [np.zeros(k, np.float32) for k in self.numel]
        if special == "zero":
            self.grads = [[np.zeros(k, np.float32) for k in self.numel] for _ in range(self.steps)]
        elif special in ("inf", "nan"):
            big = int(np.argmax(self.numel))
            self.grads[0][big][self.numel[big] // 2] = np.inf if special == "inf" else np.nan
        self.special = special
        self._finish()

    def _finish(self):
        with np.errstate(all="ignore"):
            self.ref = oracle(self)
        self.torch = torch_path(self)

    @classmethod
    def from_arrays(cls, name, P0, grads, M0, V0, step0, scales, max_norm, lr, wd=0.0):
        """One step from a state in progress: flat fp32 arrays per tensor, in memory order."""
        pr = cls.__new__(cls)
        pr.name, pr.special = name, None
        pr.numel = tuple(int(x.size) for x in P0)
        pr.max_norm, pr.wd, pr.lr, pr.steps, pr.step0 = max_norm, wd, f32(lr), 1, int(step0)
        pr.scales = [f32(s) for s in scales]
        pr.P0, pr.grads, pr.M0, pr.V0 = list(P0), [list(grads)], list(M0), list(V0)
        pr._finish()
        return pr


@functools.lru_cache(maxsize=None)
def problem(tname, cname, special=None):
    return Problem(tname, cname, special)


def oracle(pr):
    """The header's formulas in float64 from the fp32 inputs: dict p, g, m, v (lists), norm, step."""
    P = [x.astype(np.float64) for x in pr.P0]
    M = [x.astype(np.float64) for x in pr.M0]
    V = [x.astype(np.float64) for x in pr.V0]
    t = pr.step0
    for grads in pr.grads:
        G = [s * g.astype(np.float64) for s, g in zip(pr.scales, grads)]
        norm = np.sqrt(sum(float((g * g).sum()) for g in G))
        coef = 1.0
        if pr.max_norm is not None and pr.max_norm > 0:
            coef = pr.max_norm / (norm + 1e-6)
            coef = 1.0 if coef > 1.0 else coef
        G = [coef * g for g in G]
        t += 1
        bc1, bc2 = 1.0 - BETA1 ** t, 1.0 - BETA2 ** t
        for i, g in enumerate(G):
            gd = g + pr.wd * P[i]
            M[i] = BETA1 * M[i] + (1.0 - BETA1) * gd
            V[i] = BETA2 * V[i] + (1.0 - BETA2) * gd * gd
            P[i] = P[i] - (pr.lr / bc1) * M[i] / (np.sqrt(V[i]) / np.sqrt(bc2) + EPS)
    return dict(p=P, g=G, m=M, v=V, norm=float(norm), step=t)


def torch_path(pr):
    """do_gradient_ops-style scaling + clip_grad_norm_ + torch.optim.Adam in fp32 on the CPU: the same dict."""
    ps = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in pr.P0]
    opt = torch.optim.Adam(ps, lr=pr.lr, betas=(BETA1, BETA2), eps=EPS, weight_decay=pr.wd)
    for p, m0, v0 in zip(ps, pr.M0, pr.V0):
        opt.state[p] = {"step": torch.tensor(float(pr.step0)), "exp_avg": torch.from_numpy(m0.copy()),
                        "exp_avg_sq": torch.from_numpy(v0.copy())}
    for grads in pr.grads:
        for p, g, s in zip(ps, grads, pr.scales):
            p.grad = torch.from_numpy(g.copy())
            if s != 1.0:
                p.grad *= s
        if pr.max_norm:
            norm = torch.nn.utils.clip_grad_norm_(ps, pr.max_norm, norm_type=2)
        else:       # clipping off: the norm alone, as clip_grad_norm_ forms it (the norm of the tensors' norms)
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad, 2) for p in ps]), 2)
        opt.step()
    return dict(p=[p.detach().numpy() for p in ps], g=[p.grad.numpy() for p in ps], m=[opt.state[p]["exp_avg"].numpy() for p in ps],
                v=[opt.state[p]["exp_avg_sq"].numpy() for p in ps], norm=float(norm), step=int(opt.state[ps[0]]["step"]))


def segments(numel):
    offs, o = [], 0
    for k in numel:
        offs.append(o)
        o += -(-k // CHUNK) * CHUNK
    return offs, o


def pack(parts, numel, fill=0.0):
    """Per-tensor arrays -> the flat, chunk-padded moments layout of the library."""
    offs, total = segments(numel)
    flat = np.full(total, fill, np.float32)
    for o, x in zip(offs, parts):
        flat[o:o + x.size] = x
    return flat


def unpack(flat, numel):
    offs, _ = segments(numel)
    return [flat[o:o + k].copy() for o, k in zip(offs, numel)]


def _cat(parts):
    return np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in parts])


def rule(what, got, ref, tor, label):
    """The accuracy rule on one quantity (flat float64 arrays); where the reference is not finite the positions and kinds of the
    non-finite values must be torch's, and the finite entries obey the rule."""
    got, ref, tor = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (got, ref, tor))
    fin = np.isfinite(tor)
    assert np.array_equal(np.isnan(got), np.isnan(tor)), "%s %s: NaN positions differ from torch's" % (label, what)
    assert np.array_equal(got[~fin & ~np.isnan(tor)], tor[~fin & ~np.isnan(tor)]), "%s %s: infinities differ" % (label, what)
    if not fin.any():
        return
    fin &= np.isfinite(ref)
    err = float(np.abs(got[fin] - ref[fin]).max())
    terr = float(np.abs(tor[fin] - ref[fin]).max())
    bound = max(4.0 * terr, 2.0 ** -19 * float(np.abs(ref[fin]).max()))
    print("%-28s %-5s err %.3e torch %.3e bound %.3e" % (label, what, err, terr, bound))
    assert err <= bound, "%s %s: error %.3e > bound %.3e (torch's own %.3e)" % (label, what, err, bound, terr)


def check(pr, got, label="", grads_written=True):
    """got: dict p, g, m, v (per-tensor fp32 arrays), norm (or None), step."""
    label = label or pr.name
    assert got["step"] == pr.ref["step"] == pr.torch["step"], (label, got["step"], pr.ref["step"])
    for what in ("p", "m", "v") + (("g",) if grads_written else ()):
        rule(what, _cat(got[what]), _cat(pr.ref[what]), _cat(pr.torch[what]), label)
    if got.get("norm") is not None:
        rule("norm", got["norm"], pr.ref["norm"], pr.torch["norm"], label)


def bits(got):
    """Everything a call wrote, as one uint32 array: for the same-bits comparisons."""
    parts = [np.concatenate([np.asarray(x, np.float32).ravel() for x in got[k]]) for k in ("p", "g", "m", "v")]
    parts.append(np.asarray([got["norm"] if got.get("norm") is not None else 0.0], np.float32))
    return np.concatenate(parts).view(np.uint32)

"""Shared by tests/test_ge2e_fused_host.py and tests/test_ge2e_fused.py: the shape list, the seeded inputs, the float64 reference
(the tensor-op ge2e.similarity_matrix / ge2e_loss with torch autograd on the CPU — code the fused kernels do not share) and
the tolerance rule."""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (S, U, D, U_enroll): the smallest shapes at which each mechanism of the kernels can go wrong
SHAPES = [
    (1, 2, 8, 0),        # one class: loss and every gradient exactly 0
    (5, 2, 32, 0),       # U = 2: the exclusive centroid is the other utterance
    (3, 7, 30, 0),       # D not a multiple of 4, S below a tile
    (65, 3, 256, 0),     # one speaker past a 64 tile; rows spread over several workgroups
    (16, 32, 256, 0),    # the reference's training batch (params_model.py)
    (64, 10, 256, 0),    # the README's GE2E layout
    (7, 3, 36, 2),       # enrollment form
    (40, 32, 256, 32),   # ... the reference's validation batch
]
# (w, b, g) per case: the reference's initial values everywhere, one case with other values; upstream gradient 1 and 3.5
SCALARS = [(10.0, -5.0, 1.0), (10.0, -5.0, 3.5)]
EXTRA = [((3, 7, 30, 0), (3.7, 0.4, 3.5))]
CASES = [(sh, sc) for sh in SHAPES for sc in SCALARS] + EXTRA


# the loops that take more than one pass, the tile carries of phase 3 and the descriptors at the plan's limits
LOOP_SHAPES = [
    (3, 2, 300, 0),      # D just past one pass of the 256 threads: every `d = tid; d < D; d += nthr` loop runs twice for 44 threads
    (2, 3, 4096, 0),     # D at the limit: sixteen passes, the largest LDS of the centroid phase
    (300, 2, 5, 0),      # S > 256: R = P = 1 and npair = 300 > 256, the pair loops of the row phase take two passes
    (2048, 2, 8, 0),     # S at the limit: 36 KB of LDS in the row phase, eight passes of its pair loops
    (5, 3, 3, 0),        # D < P: DC = 1 and the split threads c >= D have an empty component range
    (17, 257, 20, 0),    # N = 4369: CH = 274, two tiles in ge2e_cgrad_body; U = 257: two tiles in ge2e_asum_body
    (3, 300, 12, 2),     # enrollment form with U > 256 verification rows per speaker, U_enroll = 2
    (6, 2, 40, 300),     # enrollment form, the centroid sum runs over 300 enrollment rows
]
LOOP_CASES = [(sh, (10.0, -5.0, 3.5)) for sh in LOOP_SHAPES]
# many rows per speaker: the sums over U (centroids, slabs, asum) must hold the accuracy rule up to the row limit
LONG_SHAPES = [
    (4, 20000, 8, 0),    # 79 tiles per chunk in ge2e_cgrad_body, 79 in ge2e_asum_body
    (4, 3, 16, 100000),  # enrollment form: a centroid sum of 100000 rows
    (2, 1 << 21, 4, 0),  # the row limit, 2^22 rows: 1024 tiles per chunk, 8192 per speaker
]
LONG_CASES = [(sh, (10.0, -5.0, 1.0)) for sh in LONG_SHAPES]


def case_id(case):
    (S, U, D, Ue), (w, b, g) = case
    return "S%d-U%d-D%d-Ue%d-w%g-b%g-g%g" % (S, U, D, Ue, w, b, g)


loop_id = long_id = case_id

# (input builder, (w, b, g)): values of w, b and of the embeddings at which a softmax without max-subtraction overflows and at
# which both arms of the two eps clamps are taken
RANGE_CASES = [
    ("unclustered", (300.0, -100.0, 1.0)),        # exp(out) overflows fp32 without the subtraction (|out| up to ~400)
    ("unclustered", (-300.0, 50.0, 1.0)),         # negative w: the row maximum is the LEAST similar centroid
    ("unclustered", (1000.0, 0.0, 1.0)),          # |out| up to ~1000
    ("unclustered_enroll", (300.0, -100.0, 1.0)),  # the same through the enrollment form
    ("zero_rows", (10.0, -5.0, 1.0)),             # exact zeros: an exclusive and an inclusive centroid of norm 0 (fl == 0 arms)
    ("eps_straddle", (1e12, -5.0, 1.0)),          # centroid norms on both sides of eps = 1e-12
]
EPS = 1e-12


def range_id(case):
    name, (w, b, g) = case
    return "%s-w%g-b%g-g%g" % (name, w, b, g)


@functools.lru_cache(maxsize=None)
def range_inputs(name):
    """(E, A or None) of a RANGE_CASES builder, float32, CPU; shared, callers must not modify them."""
    if name.startswith("unclustered"):
        gen = torch.Generator().manual_seed(20240611)

        def draw(n):
            x = torch.randn(6, n, 24, generator=gen)
            x = x / x.norm(dim=2, keepdim=True)
            return (x * (0.5 + 1.5 * torch.rand(6, n, 1, generator=gen))).float().contiguous()

        E = draw(3)
        return E, (draw(2) if name == "unclustered_enroll" else None)
    if name == "zero_rows":
        E = inputs(4, 2, 16, 0)[0].clone()
        E[1, 1] = 0      # the exclusive centroid of row (1, 0) is exactly 0, and row (1, 1) is a zero embedding
        E[2] = 0         # a speaker whose inclusive centroid is exactly 0
        return E, None
    if name == "eps_straddle":
        return (inputs(4, 3, 16, 0)[0] * 1e-12).contiguous(), None
    raise KeyError(name)


def centroid_norms(E):
    """float64 norms of the inclusive centroids [S] and of the exclusive centroids [S, U] (training form)."""
    e = E.double()
    U = e.shape[1]
    return e.mean(dim=1).norm(dim=1).numpy(), ((e.sum(dim=1, keepdim=True) - e) / (U - 1)).norm(dim=2).numpy()


@functools.lru_cache(maxsize=None)
def range_reference(case):
    """float64 on the CPU, once per range case; asserts first that the case exercises what it is there for."""
    name, (w, b, g) = case
    E, A = range_inputs(name)
    ref = evaluate(E, A, w, b, g, torch.float64)
    S, U, _ = E.shape
    if name.startswith("unclustered"):
        assert ref["loss"] > 1 and np.abs(ref["d_E"]).max() > 1e-3, (ref["loss"], np.abs(ref["d_E"]).max())
        own = ref["sim"][np.arange(S), :, np.arange(S)]                  # [S, U]: every row's true-class entry
        assert (own < ref["sim"].max(axis=2)).any()
        assert np.abs(ref["sim"]).max() > 89                             # exp overflows fp32 above 88.7
    elif name == "zero_rows":
        incl, excl = centroid_norms(E)
        assert incl[2] == 0 and excl[1, 0] == 0 and not E[1, 1].any() and not E[2].any()
        assert (np.delete(incl, 2) > 0.1).all() and excl[0].min() > 0.1
    elif name == "eps_straddle":
        for n in centroid_norms(E):
            assert (n < EPS).any() and (n > EPS).any(), n
            assert np.abs(n / EPS - 1).min() > 1e-3, n
        assert np.abs(ref["d_E"]).max() > 1e-3
    return ref


@functools.lru_cache(maxsize=None)
def inputs(S, U, D, Ue):
    """Seeded embeddings clustered per speaker (so the loss is neither 0 nor log S), every row rescaled by a factor in
    [0.5, 2] (so the normalisation Jacobians matter) -> (E [S, U, D], A [S, Ue, D] or None), float32, CPU."""
    gen = torch.Generator().manual_seed(1000 * S + 10 * U + D + Ue)
    centers = torch.randn(S, 1, D, generator=gen)

    def draw(n):
        x = centers + 0.9 * torch.randn(S, n, D, generator=gen)
        x = x / x.norm(dim=2, keepdim=True)
        return (x * (0.5 + 1.5 * torch.rand(S, n, 1, generator=gen))).float().contiguous()

    return draw(U), (draw(Ue) if Ue else None)


def evaluate(E, A, w, b, g, dtype, device="cpu"):
    """The tensor-op path in `dtype` on `device` -> dict of float64 numpy arrays: sim, loss, d_E, d_w, d_b."""
    from ttrnn_hip import ge2e
    e = E.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
    a = A.to(device=device, dtype=dtype) if A is not None else None
    wt = torch.tensor(w, dtype=dtype, device=device, requires_grad=True)
    bt = torch.tensor(b, dtype=dtype, device=device, requires_grad=True)
    sim = ge2e.similarity_matrix(e, wt, bt, a)
    loss, _ = ge2e.ge2e_loss(e, wt, bt, a, with_eer=False)
    (g * loss).backward()
    return {"sim": sim.detach().double().cpu().numpy(), "loss": np.float64(loss.item()), "d_E": e.grad.double().cpu().numpy(),
            "d_w": np.float64(wt.grad.item()), "d_b": np.float64(bt.grad.item())}


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64 on the CPU, computed once per case and shared (callers must not modify it)."""
    (S, U, D, Ue), (w, b, g) = case
    E, A = inputs(S, U, D, Ue)
    return evaluate(E, A, w, b, g, torch.float64)


def check(got, ref, torch32, label):
    """err <= max(4 x the fp32 tensor-op path's own error, 2^-19 x max|reference|) for each of sim, loss, d_E, d_w, d_b.  The
    factor 4 allows for another summation order; the floor is 32 fp32 ulps of the largest magnitude (D-term fp32 dot products).
    d_b is 0 in exact arithmetic: its scale is 2, the bound on sum |d_out|.  Prints every figure before asserting."""
    bad = []
    for key in ("sim", "loss", "d_E", "d_w", "d_b"):
        r = np.asarray(ref[key], dtype=np.float64)
        err = float(np.max(np.abs(np.asarray(got[key], dtype=np.float64) - r)))
        err_t = float(np.max(np.abs(np.asarray(torch32[key], dtype=np.float64) - r)))
        scale = 2.0 if key == "d_b" else float(np.max(np.abs(r)))
        bound = max(4.0 * err_t, 2.0 ** -19 * scale)
        print("%s %-4s err %.3e  torch-op fp32 err %.3e  scale %.3e  bound %.3e" % (label, key, err, err_t, scale, bound))
        if not err <= bound:
            bad.append((key, err, bound))
    assert not bad, "%s: %s" % (label, bad)


def fixture_names():
    import glob
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "g9_ge2e_*.npz")))


def load_fixture(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    enr = torch.from_numpy(d["enroll"]) if d["enroll"].size else None
    return d, torch.from_numpy(d["embeds"]), enr

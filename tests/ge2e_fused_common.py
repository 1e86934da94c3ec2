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


def case_id(case):
    (S, U, D, Ue), (w, b, g) = case
    return "S%d-U%d-D%d-Ue%d-w%g-b%g-g%g" % (S, U, D, Ue, w, b, g)


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

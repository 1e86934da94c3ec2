"""GE2E similarity matrix and softmax loss for the speaker-verification caller of the hot path.

The reference builds the [S, U, S] similarity matrix on the CPU with a Python loop over speakers
(experiments/speaker_verification/encoder/speaker_encoder.py:109-127; main.py moves the embeddings to `loss_device`
first).  Here the whole thing is a handful of device-side tensor ops — inclusive centroids, leave-one-out centroids for the
diagonal, one [S*U, D] x [D, S] product — so it stays on the GPU next to the encoder, and under data parallelism every
rank contributes its utterances through one all-gather of the [S_local, U, D] embeddings (gradients flow back to the
local slice only; the loss is the mean over ALL utterances, as on a single device)."""
import contextlib
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib


def similarity_matrix(verification, weight, bias, enrollment=None):
    """verification [S, U, D] L2-normalised embeddings -> scaled cosine similarities [S, U, S] (speaker_encoder.py:93-140)."""
    S, U, _ = verification.shape
    if enrollment is not None:
        cen = F.normalize(enrollment.mean(dim=1), dim=1)                           # [S, D]
        sim = torch.einsum("sud,jd->suj", verification, cen)
        return sim * weight + bias
    incl = F.normalize(verification.mean(dim=1), dim=1)                            # [S, D]
    excl = F.normalize((verification.sum(dim=1, keepdim=True) - verification) / (U - 1), dim=2)   # [S, U, D]
    sim = torch.einsum("sud,jd->suj", verification, incl)
    own = (verification * excl).sum(dim=2)                                         # [S, U]: speaker against its own rest
    eye = torch.eye(S, dtype=torch.bool, device=verification.device).unsqueeze(1)  # [S, 1, S]
    sim = torch.where(eye, own.unsqueeze(2), sim)
    return sim * weight + bias


def eer(sim2d, S, U):
    """Equal error rate of a [S*U, S] similarity matrix (speaker_encoder.py:160-168); host side, not back-propagated."""
    from scipy.interpolate import interp1d
    from scipy.optimize import brentq
    from sklearn.metrics import roc_curve
    truth = np.repeat(np.arange(S), U)
    labels = np.eye(S, dtype=np.int64)[truth]
    fpr, tpr, _ = roc_curve(labels.flatten(), np.asarray(sim2d, dtype=np.float64).flatten())
    return float(brentq(lambda v: 1. - v - interp1d(fpr, tpr)(v), 0., 1.))


def ge2e_loss(verification, weight, bias, enrollment=None, with_eer=True):
    """(softmax loss over all S*U utterances, EER or None) — speaker_encoder.py:142-170.  with_eer="device": the EER as a 0-d
    float64 device tensor from eer_fused (fp32 GPU similarities only; TtrnnError otherwise), with no synchronisation."""
    S, U, _ = verification.shape
    sim = similarity_matrix(verification, weight, bias, enrollment).reshape(S * U, S)
    target = torch.arange(S, device=sim.device).repeat_interleave(U)
    loss = F.cross_entropy(sim, target)
    if _on_device(with_eer):
        return loss, eer_fused(sim.detach(), S, U)
    e = eer(sim.detach().float().cpu().numpy(), S, U) if with_eer else None
    return loss, e


def _on_device(with_eer):
    """with_eer is True / False / None (the host-side EER, or none) or the string "device"."""
    if isinstance(with_eer, str):
        if with_eer != "device":
            raise ValueError('with_eer must be True, False, None or "device", got {!r}'.format(with_eer))
        return True
    return False


class _GatherSpeakers(torch.autograd.Function):
    """all_gather along the speaker axis; backward hands every rank the gradient slice of its own speakers."""

    @staticmethod
    def forward(ctx, local, group):
        import torch.distributed as dist
        world = dist.get_world_size(group)
        parts = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(parts, local.contiguous(), group=group)
        ctx.rank, ctx.n, ctx.world = dist.get_rank(group), local.shape[0], world
        return torch.cat(parts, dim=0)

    @staticmethod
    def backward(ctx, grad):
        # Every rank evaluates the FULL loss, so rank r's slice of d(loss)/d(embeds) is already the single-device
        # gradient of its own utterances; the data-parallel step then takes the MEAN over ranks of every parameter
        # gradient.  The encoder's gradient flows through this slice only (the other ranks contribute zero for these
        # utterances), so it is scaled by `world` here to survive that mean.  The replicated similarity weight / bias
        # receive their full gradient on every rank, the mean leaves them exact, and the loss value stays unscaled.
        return grad[ctx.rank * ctx.n:(ctx.rank + 1) * ctx.n].contiguous() * ctx.world, None


# ---- the same loss as library calls (include/ttrnn.h, TTRNN_HAS_GE2E): centroids, rows, centroid gradients, d_E ----------------

def _desc(S, U, D, U_enroll=0):
    d = _lib.Ge2eDesc()
    d.S, d.U, d.D, d.U_enroll = int(S), int(U), int(D), int(U_enroll)
    return d


def fused_supported(S, U, D, dtype, device, U_enroll=0):
    """True when ge2e_loss_fused / similarity_matrix_fused take this call: fp32 embeddings on a GPU and a shape the kernels
    accept (training form U >= 2; S <= 2048, D <= 4096, at most 2^22 rows)."""
    if dtype != torch.float32 or torch.device(device).type != "cuda":
        return False
    return _plan(int(S), int(U), int(D), int(U_enroll))[1] > 0


@functools.lru_cache(maxsize=64)
def _plan(S, U, D, U_enroll):
    """(descriptor, workspace bytes; 0 = refused) of one shape — pure host arithmetic in the library, cached per shape."""
    desc = _desc(S, U, D, U_enroll)
    return desc, int(_lib.load().ttrnn_ge2e_workspace(ctypes.byref(desc)))


def _on(device):
    """The launches go to the CURRENT device's copy of the kernels: switch only when the tensors live elsewhere."""
    return contextlib.nullcontext() if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _scalar(name, t, like):
    if not torch.is_tensor(t) or t.numel() != 1:
        raise _lib.TtrnnError("{} must be a one-element tensor (the kernels read it on the device)".format(name))
    if t.device != like.device or t.dtype != torch.float32:
        raise _lib.TtrnnError("{} is {} on {}: the fused GE2E loss needs float32 on {}".format(name, t.dtype, t.device, like.device))
    return t.detach().contiguous()


def _fused_operands(verification, weight, bias, enrollment):
    if verification.dim() != 3:
        raise _lib.TtrnnError("verification embeddings must be [S, U, D], got {}".format(tuple(verification.shape)))
    S, U, D = verification.shape
    if not verification.is_cuda or verification.dtype != torch.float32:
        raise _lib.TtrnnError("the fused GE2E loss runs on float32 GPU tensors only (got {} on {}); there is no fallback — "
                              "call ge2e_loss for the tensor-op path".format(verification.dtype, verification.device))
    Ue = 0
    if enrollment is not None:
        if (enrollment.dim() != 3 or enrollment.shape[0] != S or enrollment.shape[2] != D or enrollment.shape[1] < 1
                or enrollment.device != verification.device or enrollment.dtype != torch.float32):
            raise _lib.TtrnnError("enrollment embeddings must be float32 [S, U_enroll, D] on the verification embeddings' device")
        Ue = enrollment.shape[1]
    desc, nbytes = _plan(S, U, D, Ue)
    if nbytes == 0:
        raise _lib.TtrnnError("the fused GE2E kernels do not take S={} U={} D={} U_enroll={}".format(S, U, D, Ue))
    E = verification.detach().contiguous()
    A = enrollment.detach().contiguous() if enrollment is not None else None
    return desc, nbytes, E, A, _scalar("weight", weight, E), _scalar("bias", bias, E)


def _fused_forward(verification, weight, bias, enrollment=None, want_sim=False, need_grad=False, workspace=None):
    """ttrnn_ge2e_forward on torch tensors -> (loss [], sim [S, U, S] or None, state for _fused_backward).  `workspace`: a uint8
    tensor of at least ttrnn_ge2e_workspace bytes to use instead of a fresh one (its contents do not matter)."""
    desc, nbytes, E, A, w, b = _fused_operands(verification, weight, bias, enrollment)
    S, U, _ = E.shape
    with _on(E.device):
        ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=E.device)
        loss = torch.empty((), dtype=torch.float32, device=E.device)
        sim = torch.empty((S, U, S), dtype=torch.float32, device=E.device) if want_sim else None
        _lib.check(_lib.load().ttrnn_ge2e_forward(ctypes.byref(desc), _ptr(E), _ptr(A), _ptr(w), _ptr(b), _ptr(loss), _ptr(sim),
                                                  1 if need_grad else 0, _ptr(ws), ws.numel(), _stream(E)), "ttrnn_ge2e_forward")
    return loss, sim, (desc, E, w, ws)


def _fused_backward(state, grad=None, want=(True, True, True)):
    """ttrnn_ge2e_backward -> (d_E, d_w, d_b), None where not wanted; grad: upstream gradient of the loss (device scalar) or None = 1."""
    desc, E, w, ws = state
    with _on(E.device):
        g = grad.detach().to(torch.float32).contiguous() if grad is not None else None
        d_E = torch.empty_like(E) if want[0] else None
        d_w = torch.empty((), dtype=torch.float32, device=E.device) if want[1] else None
        d_b = torch.empty((), dtype=torch.float32, device=E.device) if want[2] else None
        _lib.check(_lib.load().ttrnn_ge2e_backward(ctypes.byref(desc), _ptr(E), _ptr(w), _ptr(g), _ptr(d_E), _ptr(d_w), _ptr(d_b),
                                                   _ptr(ws), ws.numel(), _stream(E)), "ttrnn_ge2e_backward")
    return d_E, d_w, d_b


class _FusedGE2E(torch.autograd.Function):
    """loss (and the scaled similarity matrix, not differentiable) from ttrnn_ge2e_forward; backward = ttrnn_ge2e_backward."""

    @staticmethod
    def forward(ctx, verification, weight, bias, enrollment, want_sim):
        need = any(ctx.needs_input_grad[:3])
        loss, sim, state = _fused_forward(verification, weight, bias, enrollment, want_sim, need)
        ctx.state, ctx.need = state, need
        ctx.w_shape, ctx.b_shape = weight.shape, bias.shape
        if sim is None:
            return loss
        ctx.mark_non_differentiable(sim)
        return loss, sim

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        want = tuple(ctx.needs_input_grad[:3])
        d_E, d_w, d_b = _fused_backward(ctx.state, grad_loss, want)
        return (d_E, d_w.reshape(ctx.w_shape) if d_w is not None else None,
                d_b.reshape(ctx.b_shape) if d_b is not None else None, None, None)


def similarity_matrix_fused(verification, weight, bias, enrollment=None):
    """similarity_matrix as one library call (forward only; the inputs are treated as detached) -> [S, U, S]."""
    return _fused_forward(verification, weight, bias, enrollment, want_sim=True, need_grad=False)[1]


def ge2e_loss_fused(verification, weight, bias, enrollment=None, with_eer=False):
    """ge2e_loss through the library's GE2E kernels: (loss, EER or None).  Gradients reach verification, weight and bias (four
    launches for loss plus all gradients); the enrollment embeddings are a constant.  Raises TtrnnError on CPU tensors,
    non-fp32 or shapes the kernels refuse — there is no fallback to the tensor-op path."""
    if enrollment is not None and enrollment.requires_grad:
        raise _lib.TtrnnError("the fused GE2E loss has no gradient to the enrollment embeddings (detach them)")
    S, U, _ = verification.shape
    device_eer = _on_device(with_eer)
    if not with_eer:
        return _FusedGE2E.apply(verification, weight, bias, enrollment, False), None
    loss, sim = _FusedGE2E.apply(verification, weight, bias, enrollment, True)
    if device_eer:      # two more launches at most, on the same stream; nothing is read on the host
        return loss, eer_fused(sim, S, U)
    return loss, eer(sim.reshape(S * U, S).cpu().numpy(), S, U)


# ---- the equal error rate of the similarity matrix as a library call (include/ttrnn.h, TTRNN_HAS_GE2E_EER) -----------------------

EER_ROUTES = {"auto": 0, "one": 1, "grid": 2}      # ttrnn_eer_desc.route
EER_MAX_WORKGROUPS = 256


@functools.lru_cache(maxsize=64)
def _eer_plan(S, U, route, workgroups):
    """(descriptor, workspace bytes; 0 = refused) — pure host arithmetic in the library, cached per shape and route."""
    desc = _lib.EerDesc(S, U, route, workgroups)
    return desc, int(_lib.load().ttrnn_ge2e_eer_workspace(ctypes.byref(desc)))


def eer_supported(S, U, dtype, device):
    """True when eer_fused takes a [S, U, S] similarity matrix of this dtype on this device: fp32 on a GPU, 2 <= S <= 2048,
    S U <= 2^22, S U S <= 2^30."""
    if dtype != torch.float32 or torch.device(device).type != "cuda":
        return False
    S, U = int(S), int(U)
    if not (0 <= S < 2 ** 31 and 0 <= U < 2 ** 31):
        return False
    return _eer_plan(S, U, 0, 0)[1] > 0


def eer_fused(sim, S=None, U=None, want_aux=False, route="auto", workgroups=0):
    """Equal error rate of a similarity matrix, [S, U, S] or [S U, S] fp32 on a GPU, as one library call: what `eer` returns
    (to within brentq's tolerance) as a 0-d float64 tensor on sim's device, with no synchronisation and nothing read on the host,
    so it can be captured.  want_aux: (eer, threshold 0-d float32, counts int64 [4] = tp', fp', tp, fp around the threshold).
    route: "auto", "one" (one workgroup, one launch) or "grid" (`workgroups` workgroups, 0 = the library's choice; five launches);
    every route returns the same bits.  A NaN score gives eer = threshold = NaN and counts of -1 (the host route raises there).
    Raises TtrnnError on CPU tensors, other dtypes and shapes the kernels refuse — there is no fallback to the host route."""
    if not torch.is_tensor(sim) or not sim.is_cuda or sim.dtype != torch.float32:
        raise _lib.TtrnnError("eer_fused runs on float32 GPU tensors only (got {} on {}); there is no fallback — call eer for the "
                              "host route".format(getattr(sim, "dtype", type(sim)), getattr(sim, "device", "the host")))
    if sim.dim() == 3 and sim.shape[0] == sim.shape[2]:
        s_, u_ = sim.shape[0], sim.shape[1]
    elif sim.dim() == 2 and sim.shape[1] > 0 and sim.shape[0] % sim.shape[1] == 0:
        s_, u_ = sim.shape[1], sim.shape[0] // sim.shape[1]
    else:
        raise _lib.TtrnnError("the similarity matrix must be [S, U, S] or [S U, S], got {}".format(tuple(sim.shape)))
    if (S is not None and int(S) != s_) or (U is not None and int(U) != u_):
        raise _lib.TtrnnError("a similarity matrix of shape {} is not S={} U={}".format(tuple(sim.shape), S, U))
    if route not in EER_ROUTES and route not in EER_ROUTES.values():
        raise ValueError("route must be one of {}".format(sorted(EER_ROUTES)))
    desc, nbytes = _eer_plan(s_, u_, EER_ROUTES.get(route, route), int(workgroups))
    if nbytes == 0:
        raise _lib.TtrnnError("the EER kernels do not take S={} U={} route={} workgroups={}".format(s_, u_, route, workgroups))
    x = sim.detach().contiguous()
    with _on(x.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        out = torch.empty((), dtype=torch.float64, device=x.device)
        thr = torch.empty((), dtype=torch.float32, device=x.device) if want_aux else None
        cnt = torch.empty(4, dtype=torch.int64, device=x.device) if want_aux else None
        _lib.check(_lib.load().ttrnn_ge2e_eer(ctypes.byref(desc), _ptr(x), _ptr(out), _ptr(thr), _ptr(cnt), _ptr(ws), ws.numel(),
                                              _stream(x)), "ttrnn_ge2e_eer")
    return (out, thr, cnt) if want_aux else out


def ge2e_loss_data_parallel(local_embeds, weight, bias, group=None, with_eer=False, force_gather=False, fused=False):
    """Every rank holds [S_local, U, D] embeddings of its own speakers.  The similarity matrix needs all centroids: one
    all-gather (cfg4: 512 x 256 floats), then each rank evaluates the FULL loss (identical on every rank, returned
    unscaled) and back-propagates into its slice.  After the gradient all-reduce (MEAN) of the data-parallel step
    (ttrnn_hip.dist.FlatGradAllReduce) every parameter holds its single-device gradient: the slice gradient is scaled by
    the world size in _GatherSpeakers.backward, the replicated similarity weight / bias are left alone.
    (The reference computes the loss on one CPU, main.py:280.)  fused=True: the full loss after the gather is ge2e_loss_fused.
    with_eer="device": the EER of the full matrix as a device scalar (eer_fused), the same on every rank."""
    import os
    import torch.distributed as dist
    loss_fn = ge2e_loss_fused if fused else ge2e_loss
    if not (dist.is_available() and dist.is_initialized()):
        return loss_fn(local_embeds, weight, bias, None, with_eer)
    # force_gather / TTRNN_FORCE_COLLECTIVES=1: take the all-gather even in a one-rank group (drives RCCL on a 1-GPU box)
    if dist.get_world_size(group) == 1 and not (force_gather or os.environ.get("TTRNN_FORCE_COLLECTIVES") == "1"):
        return loss_fn(local_embeds, weight, bias, None, with_eer)
    full = _GatherSpeakers.apply(local_embeds, group)
    return loss_fn(full, weight, bias, None, with_eer)

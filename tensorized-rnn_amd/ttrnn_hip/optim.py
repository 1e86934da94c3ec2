"""Gradient scaling, global-norm clipping and the Adam step as one library call (include/ttrnn.h, TTRNN_HAS_OPTIM).

The tail of the reference's training steps after ``loss.backward()`` — speaker_encoder.py:61-67 (the similarity parameters'
gradients x 0.01, ``clip_grad_norm_(3.0)``) and ``optimizer.step()`` of main.py:77-78,252; pmnist_test.py:139,160-163 (Adam,
optional --clip, StepLR); benchmarking.py:43,56 — is two in-place multiplies, a foreach norm, a stack, a second norm, a clamp, a
foreach multiply and torch.optim.Adam's own launches.  ``ClipAdam`` does all of it in ``ttrnn_optim_step`` (one launch for the
small tables, two per 128 tensors on the grid route), bitwise repeatable and capture-safe:

    opt = ClipAdam(model.parameters(), lr=1e-3, max_norm=3.0,
                   grad_scales={model.similarity_weight: 0.01, model.similarity_bias: 0.01})
    loss.backward(); opt.step()            # no do_gradient_ops(): p.grad holds the scaled, clipped gradients afterwards

``state_dict()`` / ``load_state_dict()`` speak torch.optim.Adam's format in both directions (the reference checkpoints
``optimizer_state``, main.py:95-103, and resumes from it, :257-267).  Opt-in: nothing uses it unless asked to.
There is no fallback: what the kernels do not take raises TtrnnError."""
import ctypes

import torch

from . import _lib

ROUTES = {"auto": 0, "one": 1, "grid": 2}          # ttrnn_optim_desc.route


def _dense_order(t):
    """True when t's elements fill numel consecutive words with no overlap (any permutation of a contiguous layout)."""
    dims = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz > 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _same_layout(a, b):
    return a.shape == b.shape and all(sa == sb for sz, sa, sb in zip(a.shape, a.stride(), b.stride()) if sz > 1)


def _segments(numels):
    """Offsets of the tensors' segments in the flat moments: every tensor is padded to whole chunks (include/ttrnn.h)."""
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += -(-n // _lib.OPTIM_CHUNK) * _lib.OPTIM_CHUNK
    return offs, o


def _desc(n, mode, route, workgroups, write_grads, betas, eps, weight_decay, max_norm):
    if route not in ROUTES and route not in ROUTES.values():
        raise ValueError("route must be one of {}".format(sorted(ROUTES)))
    return _lib.OptimDesc(n, mode, ROUTES.get(route, route), int(workgroups), 1 if write_grads else 0, float(betas[0]),
                          float(betas[1]), float(eps), float(weight_decay), float(max_norm) if max_norm is not None else 0.0)


def _on(device):
    import contextlib
    return contextlib.nullcontext() if torch.cuda.current_device() == device.index else torch.cuda.device(device)


class ClipAdam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay, no amsgrad) with the gradient scaling and global-norm clipping that precede it in the
    reference folded into the same library call.

    grad_scales: {parameter: factor} applied to that parameter's gradient before the norm is taken (the encoder's 0.01).
    max_norm: clip_grad_norm_'s bound on the 2-norm of all (scaled) gradients; None = no clipping.
    write_grads: after step() p.grad holds the scaled and clipped gradient, as it does in the reference (False saves the store).
    route: "auto", "one" (one workgroup) or "grid" — every route gives the same bits.

    One parameter group of fp32 parameters, each filling its memory densely in any dimension order (the reference's transposed
    TT cores do); every parameter needs a gradient with its parameter's strides at every step.  The moments are two flat fp32
    buffers; state[p]["exp_avg"] / ["exp_avg_sq"] are views of p's segment with p's sizes and strides.  The step counter and
    the learning rate are device scalars: param_groups[0]["lr"] (what StepLR changes) is compared with a cached host value at
    each step() and written to the device when it changed.  A CAPTURED step does not run that comparison: set the learning
    rate between replays with set_lr().  last_total_norm: 0-d device tensor, the norm before clipping (None without max_norm).
    Construction, state_dict() and load_state_dict() work for CPU parameters; step() needs the GPU."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_norm=None, grad_scales=None,
                 write_grads=True, route="auto", workgroups=0, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise _lib.TtrnnError("ClipAdam has no amsgrad / maximize variant; there is no fallback — use torch.optim.Adam")
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise _lib.TtrnnError("ClipAdam takes one parameter group, got {}".format(len(params)))
        template = torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults
        super().__init__(params, dict(template))
        ps = self.param_groups[0]["params"]
        self._check_group(self.param_groups[0])
        for p in ps:
            if p.dtype != torch.float32:
                raise _lib.TtrnnError("ClipAdam takes float32 parameters only, got {}; there is no fallback".format(p.dtype))
            if p.numel() < 1 or not _dense_order(p):
                raise _lib.TtrnnError("ClipAdam needs non-empty parameters that fill their memory densely without overlap; got "
                                      "sizes {} strides {}".format(tuple(p.shape), p.stride()))
            if p.device != ps[0].device:
                raise _lib.TtrnnError("ClipAdam needs all parameters on one device")
        if len(ps) > 4096 or sum(p.numel() for p in ps) >= 2 ** 31:
            raise _lib.TtrnnError("ClipAdam takes at most 4096 tensors and fewer than 2^31 elements")
        scales = dict(grad_scales or {})
        unknown = [k for k in scales if not any(k is p for p in ps)]
        if unknown:
            raise _lib.TtrnnError("grad_scales names {} tensor(s) that are not parameters of this optimizer".format(len(unknown)))
        self.max_norm = None if max_norm is None else float(max_norm)
        self.write_grads, self.route, self.workgroups = bool(write_grads), route, int(workgroups)
        _desc(len(ps), 0, route, workgroups, write_grads, betas, eps, weight_decay, max_norm)      # validates `route`
        dev = ps[0].device
        self._numel = [p.numel() for p in ps]
        self._strides = [p.stride() for p in ps]
        offs, total = _segments(self._numel)
        self._m = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._step = torch.zeros((), dtype=torch.int64, device=dev)
        self._lr = torch.full((), float(lr), dtype=torch.float32, device=dev)
        self._lr_host = float(lr)
        self.last_total_norm = torch.zeros((), dtype=torch.float32, device=dev) if self.max_norm is not None else None
        for p, o in zip(ps, offs):
            self.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32),
                             "exp_avg": self._m.as_strided(p.shape, p.stride(), o),
                             "exp_avg_sq": self._v.as_strided(p.shape, p.stride(), o)}
        n = len(ps)
        self._c_numel = (ctypes.c_int64 * n)(*self._numel)
        self._c_scale = (ctypes.c_float * n)(*[float(next((v for k, v in scales.items() if k is p), 1.0)) for p in ps])
        self._c_params = (ctypes.c_void_p * n)()
        self._c_grads = (ctypes.c_void_p * n)()
        self._ws = None

    @staticmethod
    def _check_group(group):
        if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
            raise _lib.TtrnnError("ClipAdam has no amsgrad / maximize / decoupled weight decay variant; there is no fallback")

    def add_param_group(self, param_group):
        if len(self.param_groups) >= 1:
            raise _lib.TtrnnError("ClipAdam takes one parameter group")
        super().add_param_group(param_group)

    def set_lr(self, lr):
        """Set the learning rate: param_groups[0]["lr"] and the device scalar a captured step reads."""
        self.param_groups[0]["lr"] = float(lr)
        self._lr_host = float(lr)
        self._lr.fill_(float(lr))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        ps = group["params"]
        dev = ps[0].device
        if dev.type != "cuda":
            raise _lib.TtrnnError("ClipAdam.step runs on GPU parameters only (got {}); there is no fallback".format(dev))
        self._check_group(group)
        lr = float(group["lr"])
        if lr != self._lr_host:
            self._lr.fill_(lr)
            self._lr_host = lr
        for i, p in enumerate(ps):
            g = p.grad
            if g is None:
                raise _lib.TtrnnError("ClipAdam.step needs a gradient for every parameter (parameter {} has none)".format(i))
            if g.dtype is not torch.float32 or g.is_sparse or g.device != dev:
                raise _lib.TtrnnError("ClipAdam takes dense float32 gradients on the parameters' device")
            # (the common case first: equal strides; size-1 dimensions may differ)
            if g.stride() != self._strides[i] and not (p.stride() == self._strides[i] and _same_layout(g, p)):
                raise _lib.TtrnnError("the gradient of parameter {} has strides {} but its parameter {} (sizes {}): the kernels walk "
                                      "both in memory order".format(i, g.stride(), p.stride(), tuple(p.shape)))
            self._c_params[i] = p.data_ptr()
            self._c_grads[i] = g.data_ptr()
        desc = _desc(len(ps), _lib.OPTIM_ADAM, self.route, self.workgroups, self.write_grads, group["betas"], group["eps"],
                     group["weight_decay"], self.max_norm)
        lib = _lib.load()
        with _on(dev):
            if self._ws is None:
                nbytes = int(lib.ttrnn_optim_workspace(ctypes.byref(desc), self._c_numel))
                if nbytes == 0:
                    raise _lib.TtrnnError("the optimizer kernels refuse this descriptor (betas {}, eps {}, weight_decay {})".format(
                        group["betas"], group["eps"], group["weight_decay"]))
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            norm = self.last_total_norm
            _lib.check(lib.ttrnn_optim_step(ctypes.byref(desc), self._c_numel, self._c_params, self._c_grads, self._c_scale,
                                            self._m.data_ptr(), self._v.data_ptr(), self._step.data_ptr(), self._lr.data_ptr(),
                                            norm.data_ptr() if norm is not None else None, self._ws.data_ptr(), self._ws.numel(),
                                            torch.cuda.current_stream(dev).cuda_stream), "ttrnn_optim_step")
        return loss

    def step_count(self):
        """The counter as a host integer (synchronises)."""
        return int(self._step.item())

    def state_dict(self):
        """torch.optim.Adam's format: every parameter's `step` is the one counter (read from the device here)."""
        t = float(self.step_count())
        for st in self.state.values():
            st["step"] = torch.tensor(t, dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Takes a torch.optim.Adam (or ClipAdam) state_dict: the moments are copied INTO the flat buffers, so the state
        tensors stay views of them; the parameters' `step` values must agree."""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise _lib.TtrnnError("ClipAdam takes one parameter group, the state_dict has {}".format(len(groups)))
        self._check_group(groups[0])
        steps = {float(st["step"]) for st in state_dict["state"].values() if "step" in st}
        if len(steps) > 1:
            raise _lib.TtrnnError("the parameters of this state_dict are at different steps ({}): ClipAdam keeps one counter".format(
                sorted(steps)))
        if any("max_exp_avg_sq" in st for st in state_dict["state"].values()):
            raise _lib.TtrnnError("the state_dict holds amsgrad state; ClipAdam has no amsgrad variant")
        views = {p: (st["exp_avg"], st["exp_avg_sq"]) for p, st in self.state.items()}
        super().load_state_dict(state_dict)
        ps = self.param_groups[0]["params"]
        t = steps.pop() if steps else 0.0
        with torch.no_grad():
            for p in ps:
                m_view, v_view = views[p]
                loaded = self.state.get(p, {})
                if "exp_avg" in loaded:
                    m_view.copy_(loaded["exp_avg"])
                    v_view.copy_(loaded["exp_avg_sq"])
                else:
                    m_view.zero_()
                    v_view.zero_()
                self.state[p] = {"step": torch.tensor(t, dtype=torch.float32), "exp_avg": m_view, "exp_avg_sq": v_view}
            self._step.fill_(int(t))
            self._lr_host = float(self.param_groups[0]["lr"])
            self._lr.fill_(self._lr_host)


def clip_grad_norm_fused(params, max_norm, grad_scales=None, route="auto", workgroups=0):
    """torch.nn.utils.clip_grad_norm_(params, max_norm) — after multiplying the gradients named in grad_scales ({parameter:
    factor}) — as one library call (mode TTRNN_OPTIM_CLIP_ONLY), for callers with another optimizer.  The gradients are scaled in
    place; returns the norm before clipping as a 0-d float32 DEVICE tensor (nothing is read on the host).  Parameters without a
    gradient are skipped.  Raises TtrnnError on CPU tensors, other dtypes, or gradients that do not fill their memory densely."""
    if torch.is_tensor(params):
        params = [params]
    scales = dict(grad_scales or {})
    grads, sc = [], []
    for p in params:
        g = p.grad
        if g is None:
            continue
        if not g.is_cuda or g.is_sparse or g.dtype != torch.float32 or g.numel() < 1 or not _dense_order(g):
            raise _lib.TtrnnError("clip_grad_norm_fused takes dense, non-empty float32 GPU gradients; there is no fallback — call "
                                  "torch.nn.utils.clip_grad_norm_")
        grads.append(g)
        sc.append(float(next((v for k, v in scales.items() if k is p), 1.0)))
    if not grads:
        raise _lib.TtrnnError("clip_grad_norm_fused: no parameter has a gradient")
    dev = grads[0].device
    if any(g.device != dev for g in grads):
        raise _lib.TtrnnError("clip_grad_norm_fused needs all gradients on one device")
    n = len(grads)
    desc = _desc(n, _lib.OPTIM_CLIP_ONLY, route, workgroups, True, (0.9, 0.999), 1e-8, 0.0, max_norm)
    numel = (ctypes.c_int64 * n)(*[g.numel() for g in grads])
    ptrs = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    lib = _lib.load()
    nbytes = int(lib.ttrnn_optim_workspace(ctypes.byref(desc), numel))
    if nbytes == 0:
        raise _lib.TtrnnError("the optimizer kernels refuse this table ({} tensors, max_norm {})".format(n, max_norm))
    with _on(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        norm = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(lib.ttrnn_optim_step(ctypes.byref(desc), numel, None, ptrs, (ctypes.c_float * n)(*sc), None, None, None, None,
                                        norm.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream),
                   "ttrnn_optim_step")
    return norm

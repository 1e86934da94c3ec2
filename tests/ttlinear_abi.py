"""TEST INFRASTRUCTURE ONLY — one TT-matrix driven through the C ABI (ttrnn_ttlinear_* / ttrnn_head_*) with caller-owned
buffers, its float64 reference (oracle.ttrnn_oracle.ttlinear + autograd) and the error rule the route tests share
(tests/test_ttlinear_routes.py, tests/test_heads.py).

The rule, per tensor (that of tests/test_dense_route.py):
    err <= max(4 x the error of the yardstick on the same input, floor x max|reference|)
with floor = 2^-19 for fp32 storage and 2^-8 (one bf16 ulp of the largest stored value) for bf16 storage.  The yardstick is
never the code under test: the any-shape route (option force_generic = 1) for TTLinear, the unfused path for the heads.
"""
import ctypes

import torch

TAIL = 4096                 # bytes behind every workspace that no call may touch
TAIL_BYTE = 0x5A
FLOOR = {"fp32": 2.0 ** -19, "bf16": 2.0 ** -8}
REQUESTS = [("dx", "dw", "db"), ("dw",), ("dx",), ("db",), ("dx", "dw"), ("dx", "db"), ("dw", "db")]


def dev():
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def make_cores(in_modes, out_modes, rank, gen, zero_core=None):
    """fp32 cores (R_k, I_k, J_k, R_{k+1}) whose dense matrix has entries of variance 1 / in: y = O(1) for x = O(1)."""
    d = len(in_modes)
    ranks = [1] + [rank] * (d - 1) + [1]
    cores = []
    for k in range(d):
        std = (in_modes[k] * ranks[k + 1]) ** -0.5
        cores.append(torch.randn(ranks[k], out_modes[k], in_modes[k], ranks[k + 1], generator=gen) * std)
    if zero_core is not None:
        cores[zero_core].zero_()
    return ranks, cores


class Lin(object):
    """storage: "fp32" | "bf16" (cores, bias, x, y, dx); the float64 copies are what the device holds, rounded once."""

    def __init__(self, in_modes, out_modes, rank, storage="fp32", seed=0, bias=True, zero_core=None, bias_values=None):
        from ttrnn_hip import _lib
        from ttrnn_hip.functional import TTSpec
        self.lib = _lib.load()
        self.storage = storage
        self.dt = torch.float32 if storage == "fp32" else torch.bfloat16
        self.code = 0 if storage == "fp32" else 1
        g = torch.Generator().manual_seed(seed)
        ranks, cores = make_cores(in_modes, out_modes, rank, g, zero_core)
        self.spec = TTSpec(in_modes, out_modes, ranks)
        self.in_f, self.out_f = self.spec.in_features, self.spec.out_features
        self.cores = [c.to(self.dt).to(dev()) for c in cores]
        b = torch.randn(self.out_f, generator=g) * 0.1 if bias_values is None else bias_values.float()
        self.bias = b.to(self.dt).to(dev()) if bias else None
        self.packed = self.spec.pack(self.cores)
        self.like = [c.float() for c in self.cores]
        self.cores64 = [c.cpu().double() for c in self.cores]
        self.bias64 = None if self.bias is None else self.bias.cpu().double()
        self.pe = self.spec.packed_elems
        # what d_packed / d_bias hold before a call: the gradients are ACCUMULATED into them
        self.r_packed = (torch.randn(self.pe, generator=g) * 0.5).to(dev())
        self.r_bias = (torch.randn(self.out_f, generator=g) * 0.5).to(dev())
        self.r_cores64 = [t.cpu().double() for t in self.spec.unpack_grads(self.r_packed, self.like)]

    # ---- operands ------------------------------------------------------------------------------------------------------------
    def rows(self, n, seed, x_scale=1.0, dy_bf16=False, dy_decades=False, dy_zero_col=None):
        """(x, dy) on the device in their storage types."""
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn(n, self.in_f, generator=g) * x_scale).to(self.dt)
        dy = torch.randn(n, self.out_f, generator=g)
        if dy_decades:
            dy = dy * (10.0 ** torch.linspace(-5, 5, n)).view(n, 1)
        if dy_zero_col is not None:
            dy[:, dy_zero_col] = 0.0
        dy = dy.to(torch.bfloat16 if dy_bf16 else torch.float32)
        return x.to(dev()), dy.to(dev())

    def reference(self, x, dy=None):
        """float64: y and, with dy, the gradients of sum(y * dy) — the tensors a backward call leaves, r included."""
        from oracle import ttrnn_oracle as O
        cores = [c.clone().requires_grad_(True) for c in self.cores64]
        b = None if self.bias64 is None else self.bias64.clone().requires_grad_(True)
        xr = x.cpu().double().requires_grad_(True)
        y = O.ttlinear(cores, b, xr)
        ref = {"y": y.detach()}
        if dy is not None:
            (y * dy.cpu().double()).sum().backward()
            ref["dx"] = xr.grad
            ref["db"] = self.r_bias.cpu().double() + (b.grad if b is not None else dy.cpu().double().sum(0))
            for k, c in enumerate(cores):
                ref["dcore%d" % k] = self.r_cores64[k] + c.grad
        return ref

    # ---- calls ---------------------------------------------------------------------------------------------------------------
    def _ws(self, nbytes, nan):
        ws = torch.empty(int(nbytes) + TAIL, dtype=torch.uint8, device=dev())
        ws[:int(nbytes)].fill_(0xFF if nan else 0)          # 0xFFFFFFFF / 0xFFFF: NaN as fp32 and as bf16
        ws[int(nbytes):].fill_(TAIL_BYTE)
        return ws

    def _tail_ok(self, ws, nbytes, what):
        torch.cuda.synchronize()
        assert bool((ws[int(nbytes):] == TAIL_BYTE).all()), "%s wrote behind its workspace of %d bytes" % (what, nbytes)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self, x, nan_ws=True):
        n = x.shape[0]
        w = ctypes.byref(self.spec.desc)
        wsb = int(self.lib.ttrnn_ttlinear_workspace(w, n))
        ws = self._ws(wsb, nan_ws)
        y = torch.full((n, self.out_f), float("nan"), dtype=self.dt, device=dev())
        st = self.lib.ttrnn_ttlinear_forward(w, self.code, n, _p(self.packed), _p(self.bias), _p(x), _p(y), _p(ws), wsb, self._stream())
        assert st == 0, st
        self._tail_ok(ws, wsb, "ttrnn_ttlinear_forward")
        return y

    def backward(self, x, dy, req, nan_ws=True, hints=None):
        """req: subset of ("dx", "dw", "db"); hints: dict of fp32 device tensors (x_colmax / dy_colmax / xdy_sum) -> the
        _hinted entry point, None -> ttrnn_ttlinear_backward.  Returns the raw buffers {"dx", "dpk", "db"} (None = not asked)."""
        from ttrnn_hip._lib import LinHints
        n = x.shape[0]
        w = ctypes.byref(self.spec.desc)
        wsb = int(self.lib.ttrnn_ttlinear_workspace(w, n))
        ws = self._ws(wsb, nan_ws)
        dx = torch.full((n, self.in_f), float("nan"), dtype=self.dt, device=dev()) if "dx" in req else None
        dpk = self.r_packed.clone() if "dw" in req else None
        db = self.r_bias.clone() if "db" in req else None
        dyc = 1 if dy.dtype == torch.bfloat16 else 0
        if hints is None:
            st = self.lib.ttrnn_ttlinear_backward(w, self.code, dyc, n, _p(self.packed), _p(x), _p(dy), _p(dx), _p(dpk), _p(db),
                                                  _p(ws), wsb, self._stream())
        else:
            hs = LinHints(_p(hints.get("x_colmax")), _p(hints.get("dy_colmax")), _p(hints.get("xdy_sum")), 0, _p(None), _p(None))
            st = self.lib.ttrnn_ttlinear_backward_hinted(w, self.code, dyc, n, _p(self.packed), _p(x), _p(dy), _p(dx), _p(dpk),
                                                         _p(db), ctypes.byref(hs), _p(ws), wsb, self._stream())
        assert st == 0, "request %s over %d rows: status %d" % ("+".join(req), n, st)
        self._tail_ok(ws, wsb, "ttrnn_ttlinear_backward")
        if dpk is not None:
            h = self.pe // 2
            assert torch.equal(dpk[h:], self.r_packed[h:]), "the second half of d_packed changed"
        return {"dx": dx, "dpk": dpk, "db": db}

    def head_forward(self, x, epi, want_aux=True, nan_ws=True):
        n = x.shape[0]
        w = ctypes.byref(self.spec.desc)
        wsb = int(self.lib.ttrnn_head_workspace(w, n))
        ws = self._ws(wsb, nan_ws)
        y = torch.full((n, self.out_f), float("nan"), dtype=self.dt, device=dev())
        aux = torch.full((n,), float("nan"), device=dev()) if want_aux else None
        st = self.lib.ttrnn_head_forward(w, self.code, epi, n, _p(self.packed), _p(self.bias), _p(x), _p(y), _p(aux), _p(ws), wsb,
                                         self._stream())
        assert st == 0, st
        self._tail_ok(ws, wsb, "ttrnn_head_forward")
        return y, aux

    def tensors(self, res):
        """raw buffers of a backward call -> {name: float64 CPU tensor} under the names of reference()."""
        out = {}
        if res.get("dx") is not None:
            out["dx"] = res["dx"].cpu().double()
        if res.get("db") is not None:
            out["db"] = res["db"].cpu().double()
        if res.get("dpk") is not None:
            for k, g in enumerate(self.spec.unpack_grads(res["dpk"], self.like)):
                out["dcore%d" % k] = g.cpu().double()
        return out


def same_bits(a, b, keys=("dx", "dpk", "db")):
    """every asked-for buffer bit-identical (NaN anywhere fails too)"""
    return all(a[k] is None or torch.equal(a[k], b[k]) for k in keys)


def judge(tag, got, yard, ref, storage, bad, names=("route", "any-shape"), design2=None):
    """Print one line per tensor and collect the misses of the rule above in `bad`.  design2: DESIGN.md section 2 on top, the
    factor of the tensor's maximum (1e-4 for gradients; the forward is 1e-5 x max(1, max|ref|)): fp32 cases only."""
    for k in sorted(got):
        r = ref[k]
        scale = float(r.abs().max()) if r.numel() else 0.0
        e = float((got[k] - r).abs().max()) if r.numel() else 0.0
        ey = float((yard[k] - r).abs().max()) if r.numel() else 0.0
        bound = max(4.0 * ey, FLOOR[storage] * scale)
        print("%-58s %-7s max|ref| %.3e  %s %.3e  %s %.3e  bound %.3e" % (tag, k, scale, names[0], e, names[1], ey, bound))
        if not e <= bound:
            bad.append((tag, k, e, bound))
        if design2 is not None and storage == "fp32":
            lim = 1e-5 * max(1.0, scale) if k in ("y", "aux") else design2 * scale
            if not e <= lim:
                bad.append((tag, k, "DESIGN.md section 2", e, lim))

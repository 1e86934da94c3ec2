"""The fused gradient scaling / norm clipping / Adam step (ttrnn_fast_optim.hip, include/ttrnn.h TTRNN_HAS_OPTIM) on the device:
the C entry point on the tables and cases of optim_common against float64 by the accuracy rule, the same bits on every route and
workspace, the ClipAdam wrapper on the reference's encoder next to do_gradient_ops + torch.optim.Adam, a captured training step,
and the example's --fused_optim flag."""
import contextlib
import copy
import ctypes
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_common as C

sys.path.insert(0, os.path.join(C.ROOT, "examples"))

pytestmark = pytest.mark.gpu
ADAM, CLIP_ONLY = 0, 1


def dev():
    return torch.device("cuda", 0)


def arena(numel):
    """One float32 buffer for all tensors; every third tensor starts one word off a 16-byte boundary (the scalar path)."""
    offs, o = [], 0
    for i, k in enumerate(numel):
        o = (o + 3) & ~3
        if i % 3 == 1:
            o += 1
        offs.append(o)
        o += k
    return offs, o + 4


def run_dev(pr, route=1, workgroups=0, ws_fill=0x5a, write_grads=1, mode=ADAM, want_norm=True):
    """All of the problem's steps through ttrnn_optim_step -> dict p, g, m, v (per tensor), norm, step: one host read, at the end."""
    from ttrnn_hip import _lib
    lib = _lib.load()
    n = len(pr.numel)
    desc = _lib.OptimDesc(n, mode, route, workgroups, write_grads, C.BETA1, C.BETA2, C.EPS, pr.wd,
                          pr.max_norm if pr.max_norm is not None else 0.0)
    numel = (ctypes.c_int64 * n)(*pr.numel)
    nbytes = lib.ttrnn_optim_workspace(ctypes.byref(desc), numel)
    assert nbytes > 0 and lib.ttrnn_optim_state_elems(ctypes.byref(desc), numel) == C.segments(pr.numel)[1]
    offs, words = arena(pr.numel)
    host_p = np.full(words, 7.0, np.float32)
    host_g = np.full((len(pr.grads), words), 7.0, np.float32)
    for o, x in zip(offs, pr.P0):
        host_p[o:o + x.size] = x
    for s, grads in enumerate(pr.grads):
        for o, x in zip(offs, grads):
            host_g[s, o:o + x.size] = x
    P, Gall = torch.from_numpy(host_p).to(dev()), torch.from_numpy(host_g).to(dev())
    G = torch.empty(words, dtype=torch.float32, device=dev())
    M, V = (torch.from_numpy(C.pack(x, pr.numel, 7.0)).to(dev()) for x in (pr.M0, pr.V0))
    assert P.data_ptr() % 16 == 0 and G.data_ptr() % 16 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    step = torch.tensor(pr.step0, dtype=torch.int64, device=dev())
    lr = torch.tensor(pr.lr, dtype=torch.float32, device=dev())
    norm = torch.full((), -7.0, dtype=torch.float32, device=dev())
    pp = (ctypes.c_void_p * n)(*[P.data_ptr() + 4 * o for o in offs])
    gp = (ctypes.c_void_p * n)(*[G.data_ptr() + 4 * o for o in offs])
    sc = (ctypes.c_float * n)(*pr.scales)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)
    for s in range(len(pr.grads)):
        G.copy_(Gall[s])
        ws.fill_(ws_fill)
        _lib.check(lib.ttrnn_optim_step(ctypes.byref(desc), numel, pp, gp, sc, M.data_ptr(), V.data_ptr(), step.data_ptr(),
                                        lr.data_ptr(), norm.data_ptr() if want_norm else None, ws.data_ptr(), nbytes, stream),
                   "ttrnn_optim_step")
    P, G, M, V = (x.cpu().numpy() for x in (P, G, M, V))
    mask = np.ones(words, bool)
    for o, k in zip(offs, pr.numel):
        mask[o:o + k] = False
    assert (P[mask] == 7.0).all() and (G[mask] == 7.0).all()          # nothing outside the tensors is written
    pad = np.ones(M.size, bool)
    for o, k in zip(C.segments(pr.numel)[0], pr.numel):
        pad[o:o + k] = False
    assert (M[pad] == 7.0).all() and (V[pad] == 7.0).all()
    return dict(p=[P[o:o + k].copy() for o, k in zip(offs, pr.numel)], g=[G[o:o + k].copy() for o, k in zip(offs, pr.numel)],
                m=C.unpack(M, pr.numel), v=C.unpack(V, pr.numel), norm=float(norm.cpu()) if want_norm else None, step=int(step.cpu()))


@pytest.mark.parametrize("cname", sorted(C.CASES))
@pytest.mark.parametrize("tname", C.TABLES)
def test_device_cases_obey_the_rule(tname, cname):
    """T1 / T2 / T3 x every case through the C entry point: p, m, v, g and total_norm against float64 by the accuracy rule; the
    same bits from route 1, from the grid with 1, 3 and 5 workgroups and from the library's choice, on a workspace of NaN bytes
    as on any other."""
    pr = C.problem(tname, cname)
    one = run_dev(pr, 1)
    C.check(pr, one)
    first = C.bits(one)
    for route, w, fill in ((1, 0, 0xff), (2, 1, 0x5a), (2, 3, 0xff), (2, 5, 0x00), (0, 0, 0xff)):
        assert np.array_equal(C.bits(run_dev(pr, route, w, ws_fill=fill)), first), (route, w, fill)


@pytest.mark.parametrize("tname", C.TABLES)
def test_device_write_grads_off_clip_only_and_no_norm(tname):
    pr = C.problem(tname, "scales")
    full = run_dev(pr, 1)
    for route, w in ((1, 0), (2, 3)):
        quiet = run_dev(pr, route, w, write_grads=0)
        for k in ("p", "m", "v"):
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(quiet[k], full[k])), k
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(quiet["g"], pr.grads[-1]))
        silent = run_dev(pr, route, w, want_norm=False)
        assert np.array_equal(C.bits(dict(silent, norm=full["norm"])), C.bits(full))
        clip = run_dev(pr, route, w, mode=CLIP_ONLY)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(clip["g"], full["g"]))
        assert all(np.array_equal(a, b) for a, b in zip(clip["p"], pr.P0)) and clip["step"] == 0 and clip["norm"] == full["norm"]
    off = C.problem(tname, "clip_off")
    want = run_dev(off, 1)
    for route, w in ((1, 0), (2, 3)):      # no clipping, no norm wanted: the first launches shrink to the counter's workgroup
        got = run_dev(off, route, w, want_norm=False)
        assert np.array_equal(C.bits(dict(got, norm=want["norm"])), C.bits(want)) and got["step"] == 1


@pytest.mark.parametrize("special", C.SPECIALS)
@pytest.mark.parametrize("tname", C.TABLES)
def test_device_zero_and_non_finite_gradients(tname, special):
    for cname in ("scales", "clip_off"):
        pr = C.problem(tname, cname, special)
        one = run_dev(pr, 1)
        C.check(pr, one)
        assert np.array_equal(C.bits(run_dev(pr, 2, 3, ws_fill=0xff)), C.bits(one))
        if special == "zero" and cname == "clip_off":
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(one["p"], pr.P0))


def memory_order(t):
    """A dense tensor's words in memory order, as a float32 numpy array."""
    t = t.detach()
    return t.as_strided((t.numel(),), (1,), t.storage_offset()).cpu().numpy().copy()


def test_encoder_steps_next_to_do_gradient_ops_and_adam():
    """The reference's encoder layer, three training steps on the fused GE2E loss: copy A as the reference runs it
    (do_gradient_ops + torch.optim.Adam), copy B with ClipAdam.  After each step B's parameters, gradients and moments obey the
    rule against the float64 update of B's own state and fp32 gradients, and the strides stay."""
    from ttrnn_hip import ClipAdam, clip_grad_norm_fused
    a = C.encoder(dev())
    b = copy.deepcopy(a)
    S, U = 4, 3
    torch.manual_seed(9)
    x = torch.rand(S * U, 20, 40, device=dev())
    opt_a = torch.optim.Adam(a.parameters(), lr=1e-3)
    opt_b = ClipAdam(b.parameters(), lr=1e-3, max_norm=3.0, grad_scales={b.similarity_weight: 0.01, b.similarity_bias: 0.01})
    ps = list(b.parameters())
    assert tuple(p.numel() for p in ps) == C.table("T3") and any(not p.is_contiguous() for p in ps)
    strides = [p.stride() for p in ps]
    scales = [0.01 if (p is b.similarity_weight or p is b.similarity_bias) else 1.0 for p in ps]
    assert scales.count(0.01) == 2 and scales.count(1.0) == len(ps) - 2
    losses = []
    for it in range(3):
        opt_a.zero_grad(set_to_none=True)
        la, _ = a.loss(a(x).view(S, U, -1), fused=True, with_eer=False)
        la.backward()
        a.do_gradient_ops()
        opt_a.step()
        opt_b.zero_grad(set_to_none=True)
        lb, _ = b.loss(b(x).view(S, U, -1), fused=True, with_eer=False)
        lb.backward()
        before = [[memory_order(t) for t in ts] for ts in (ps, [p.grad for p in ps], [opt_b.state[p]["exp_avg"] for p in ps],
                                                          [opt_b.state[p]["exp_avg_sq"] for p in ps])]
        # the clip-only call on a copy of the gradients gives the same gradients and norm
        twins = [torch.nn.Parameter(torch.empty_like(p)) for p in ps]
        for q, p in zip(twins, ps):
            q.grad = p.grad.clone()
        norm_only = clip_grad_norm_fused(twins, 3.0, {q: s for q, s in zip(twins, scales) if s != 1.0})
        opt_b.step()
        pr = C.Problem.from_arrays("encoder step %d" % it, before[0], before[1], before[2], before[3], it, scales, 3.0, 1e-3)
        got = dict(p=[memory_order(p) for p in ps], g=[memory_order(p.grad) for p in ps],
                   m=[memory_order(opt_b.state[p]["exp_avg"]) for p in ps], v=[memory_order(opt_b.state[p]["exp_avg_sq"]) for p in ps],
                   norm=float(opt_b.last_total_norm.cpu()), step=opt_b.step_count())
        C.check(pr, got)
        assert [p.stride() for p in ps] == strides and all(p.grad.stride() == p.stride() or p.numel() == 1 for p in ps)
        assert float(norm_only.cpu()) == got["norm"]
        assert all(np.array_equal(memory_order(q.grad).view(np.uint32), g.view(np.uint32)) for q, g in zip(twins, got["g"]))
        losses.append((float(la), float(lb)))
    # the first losses are one forward on equal parameters; the later ones are printed, not asserted: Adam divides by sqrt(v), so
    # an element whose gradient is last-bit noise of the atomically summed bias gradients moves by +-lr in either copy
    print(losses)
    assert losses[0][0] == losses[0][1]


def test_captured_step_with_clip_adam():
    """CapturedTrainStep takes a ClipAdam with no after_backward: replays track eager ClipAdam steps (the comparison of
    test_graph_capture.py), the counter advances by one per replay, set_lr() between replays changes the next update."""
    import test_graph_capture as TG
    import ttrnn_hip
    from models import MNISTClassifier
    kw, B, T = TG.CASES["runtime_tier_small"]
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        a = MNISTClassifier(device=dev(), **kw).to(dev()).train()
    b = copy.deepcopy(a)
    x = torch.rand(B, T, kw["input_size"], device=dev())
    t = torch.randint(0, kw["output_size"], (B,), device=dev())
    start = copy.deepcopy(a.state_dict())
    opt_b = ttrnn_hip.ClipAdam(b.parameters(), lr=1e-3, max_norm=3.0)
    fresh = copy.deepcopy(opt_b.state_dict())
    cap = ttrnn_hip.CapturedTrainStep(b, opt_b, TG._loss, (x, t))
    b.load_state_dict(start)
    opt_b.load_state_dict(fresh)                                      # in place: the graph holds the flat buffers
    assert opt_b.step_count() == 0 and float(opt_b._m.abs().max()) == 0.0
    opt_a = ttrnn_hip.ClipAdam(a.parameters(), lr=1e-3, max_norm=3.0)
    losses_c, losses_a = [], []
    for _ in range(3):
        losses_c.append(float(cap(x, t)))
        opt_a.zero_grad(set_to_none=True)
        la = TG._loss(a, x, t)
        la.backward()
        opt_a.step()
        losses_a.append(float(la))
    torch.cuda.synchronize()
    with torch.no_grad():
        fa, fb = float(TG._loss(a, x, t)), float(TG._loss(b, x, t))
    assert losses_c[0] == losses_a[0]
    assert all(abs(u - v) <= 2e-5 * abs(v) for u, v in zip(losses_c, losses_a)), (losses_c, losses_a)
    assert abs(fa - fb) <= 2e-5 * abs(fa), (fa, fb)
    assert opt_b.step_count() == 3 == opt_a.step_count()
    assert abs(float(opt_b.last_total_norm) - float(opt_a.last_total_norm)) <= 2e-5 * float(opt_a.last_total_norm)
    # a learning rate of zero between replays: the next replay leaves every parameter as it is, and still counts
    opt_b.set_lr(0.0)
    held = [p.detach().clone() for p in b.parameters()]
    cap(x, t)
    assert all(torch.equal(p, q) for p, q in zip(b.parameters(), held)) and opt_b.step_count() == 4
    opt_b.set_lr(1e-2)
    cap(x, t)
    moved = max(float((p - q).abs().max()) for p, q in zip(b.parameters(), held))
    assert moved > 0.0 and opt_b.step_count() == 5 and float(opt_b._lr) == np.float32(1e-2)
    assert ttrnn_hip.device_status()["pair_timeouts"] == 0


def test_speaker_step_example_with_fused_optim():
    out = subprocess.run([sys.executable, os.path.join(C.ROOT, "examples", "speaker_step.py"), "--fused_optim", "--speakers", "4",
                          "--utterances", "3", "--frames", "20", "-n", "2"], cwd=os.path.join(C.ROOT, "examples"),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0
    found = re.search(r"fused optimizer.*loss ([-0-9.einfa]+),", out.stdout)
    assert found and math.isfinite(float(found.group(1)))

"""The device-side equal error rate (ttrnn_fast_eer.hip, include/ttrnn.h TTRNN_HAS_GE2E_EER) on the device: both routes against
the exact-integer oracle of ge2e_eer_common, repeatability on any workspace contents, the reference-made fixtures, the callers
(ge2e_loss_fused, ge2e_loss, SpeakerEncoder.loss with with_eer="device") and graph capture."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

import ge2e_eer_common as C
import ge2e_fused_common as F

sys.path.insert(0, os.path.join(F.ROOT, "examples"))

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def run(sim_dev, route, workgroups=0):
    """eer_fused with its auxiliary outputs -> (eer float, theta float32, counts tuple): one host read, after the call."""
    from ttrnn_hip import ge2e
    e, theta, counts = ge2e.eer_fused(sim_dev, want_aux=True, route=route, workgroups=workgroups)
    assert e.dtype == torch.float64 and e.dim() == 0 and e.device == sim_dev.device
    assert theta.dtype == torch.float32 and theta.dim() == 0 and counts.dtype == torch.int64 and counts.shape == (4,)
    return float(e.cpu().numpy()), theta.cpu().numpy()[()], tuple(int(c) for c in counts.cpu().numpy())


def bits_of(got):
    return (np.float64(got[0]).view(np.uint64), np.float32(got[1]).view(np.uint32), got[2])


def device_configs(S, U):
    out = [("one", 0), ("auto", 0), ("grid", 1), ("grid", 3), ("grid", 7)]
    if S * U + 1 <= C.MAX_WORKGROUPS:
        out.append(("grid", S * U + 1))
    return out


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_device_matches_exact(case):
    """Every builder x every shape: route 1, route 2 with 1, 3, 7 and (where 256 workgroups allow it) more workgroups than rows,
    and the library's choice: theta bit for bit, counts exactly, the EER to 2^-50; sim is left as it was."""
    name, (S, U) = case
    sim, exact = C.case(name, (S, U))
    x = torch.from_numpy(sim.copy()).to(dev())
    first = None
    for route, g in device_configs(S, U):
        got = run(x, route, g)
        C.check(got, exact, "%s route %s workgroups %d" % (C.case_id(case), route, g))
        first = first or got
        assert bits_of(got) == bits_of(first)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), sim.view(np.uint32))


def test_device_at_the_workgroup_cap():
    sim, exact = C.case("clustered", (16, 32))
    C.check(run(torch.from_numpy(sim.copy()).to(dev()), "grid", C.MAX_WORKGROUPS), exact, "workgroups 256")


def test_device_large_shape():
    """S at its limit, 8.4 M scores, Nn P > 2^32: once per route."""
    sim, exact = C.case(*C.LARGE_CASE)
    x = torch.from_numpy(sim.copy()).to(dev())
    for route in ("one", "grid", "auto"):
        C.check(run(x, route), exact, "large route %s" % route)


@pytest.mark.parametrize("route,workgroups", [(1, 0), (2, 5)])
def test_repeatable_on_any_workspace_and_null_outputs(route, workgroups):
    """The C entry point on a NaN-filled and on a zero-filled workspace: identical bits; threshold and counts may be NULL."""
    from ttrnn_hip import _lib
    lib = _lib.load()
    sim, exact = C.case("ties_half", (65, 3))
    x = torch.from_numpy(sim.copy()).to(dev())
    desc = _lib.EerDesc(65, 3, route, workgroups)
    n = lib.ttrnn_ge2e_eer_workspace(ctypes.byref(desc))
    assert n > 0
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)
    results = []
    for fill in (0xff, 0x00, None):       # None: threshold = counts = NULL
        ws = torch.full((n,), fill if fill is not None else 0x5a, dtype=torch.uint8, device=dev())
        e = torch.full((), -7.0, dtype=torch.float64, device=dev())
        theta = torch.full((), -7.0, dtype=torch.float32, device=dev())
        counts = torch.full((4,), -7, dtype=torch.int64, device=dev())
        aux = fill is not None
        _lib.check(lib.ttrnn_ge2e_eer(ctypes.byref(desc), x.data_ptr(), e.data_ptr(), theta.data_ptr() if aux else None,
                                      counts.data_ptr() if aux else None, ws.data_ptr(), n, stream), "ttrnn_ge2e_eer")
        got = (float(e.cpu().numpy()), theta.cpu().numpy()[()], tuple(int(c) for c in counts.cpu().numpy()))
        if aux:
            C.check(got, exact, "workspace filled with %#x" % fill)
            results.append(bits_of(got))
        else:
            assert np.float64(got[0]).view(np.uint64) == results[0][0] and got[1] == -7.0 and got[2] == (-7,) * 4
    assert results[0] == results[1]
    assert np.array_equal(x.cpu().numpy().view(np.uint32), sim.view(np.uint32))


def test_two_dimensional_and_non_contiguous_views():
    from ttrnn_hip import TtrnnError, ge2e
    sim, exact = C.case("clustered", (16, 32))
    x = torch.from_numpy(sim.copy()).to(dev())
    want = float(ge2e.eer_fused(x).cpu().numpy())
    assert abs(want - exact[0]) <= C.EER_TOL
    assert float(ge2e.eer_fused(x.reshape(16 * 32, 16)).cpu().numpy()) == want
    assert float(ge2e.eer_fused(x.reshape(16 * 32, 16), 16, 32).cpu().numpy()) == want
    wide = torch.zeros(16, 32, 32, device=dev())
    wide[:, :, ::2] = x
    assert float(ge2e.eer_fused(wide[:, :, ::2]).cpu().numpy()) == want
    with pytest.raises(TtrnnError):
        ge2e.eer_fused(x, 32, 16)
    with pytest.raises(TtrnnError):
        ge2e.eer_fused(x.double())
    with pytest.raises(TtrnnError):
        ge2e.eer_fused(x, route="grid", workgroups=C.MAX_WORKGROUPS + 1)


@pytest.mark.parametrize("name", F.fixture_names())
def test_device_matches_reference_fixture(name):
    from ttrnn_hip import ge2e
    d = np.load(os.path.join(F.ROOT, "tests", "golden", name + ".npz"))
    x = torch.from_numpy(np.ascontiguousarray(d["sim"], dtype=np.float32)).to(dev())
    x = x.reshape(-1, x.shape[-1])
    for route in ("one", "grid"):
        got = float(ge2e.eer_fused(x, route=route).cpu().numpy())
        print("%s route %s: device %.17g stored %.17g" % (name, route, got, float(d["eer"])))
        assert abs(got - float(d["eer"])) <= C.HOST_TOL


@pytest.mark.parametrize("shape", [sh for sh in F.SHAPES if sh[0] >= 2], ids=lambda sh: "S%d-U%d-D%d-Ue%d" % sh)
def test_fused_loss_with_device_eer(shape):
    """ge2e_loss_fused(with_eer="device"): loss and gradients bit for bit those of with_eer=False; the EER is the exact EER of
    the kernels' own similarity matrix (not of the tensor-op one: a one-ulp difference in a score may swap two ranks)."""
    from ttrnn_hip import ge2e
    S, U, D, Ue = shape
    E, A = F.inputs(S, U, D, Ue)
    a = A.to(dev()) if A is not None else None
    res = []
    for with_eer in ("device", False):
        e = E.to(dev()).requires_grad_(True)
        w = torch.tensor(10.0, device=dev(), requires_grad=True)
        b = torch.tensor(-5.0, device=dev(), requires_grad=True)
        loss, eer = ge2e.ge2e_loss_fused(e, w, b, a, with_eer=with_eer)
        loss.backward()
        res.append((loss.detach(), e.grad, w.grad, b.grad))
        if with_eer:
            assert torch.is_tensor(eer) and eer.dtype == torch.float64 and eer.dim() == 0 and eer.is_cuda and not eer.requires_grad
            got = float(eer.cpu().numpy())
            sim = ge2e.similarity_matrix_fused(e, w, b, a).cpu().numpy()
            exact = C.eer_exact(sim)[0]
            print("S %d U %d D %d Ue %d: device %.17g exact %.17g" % (S, U, D, Ue, got, exact))
            assert abs(got - exact) <= C.EER_TOL
        else:
            assert eer is None
    for x, y in zip(*res):
        assert torch.equal(x, y) and np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))


def test_tensor_op_loss_with_device_eer():
    from ttrnn_hip import ge2e
    E, _ = F.inputs(16, 32, 256, 0)
    e = E.to(dev())
    w, b = torch.tensor(10.0, device=dev()), torch.tensor(-5.0, device=dev())
    loss, eer = ge2e.ge2e_loss(e, w, b, with_eer="device")
    sim = ge2e.similarity_matrix(e, w, b).cpu().numpy()
    assert torch.is_tensor(eer) and eer.dtype == torch.float64 and eer.is_cuda
    assert abs(float(eer.cpu().numpy()) - C.eer_exact(sim)[0]) <= C.EER_TOL
    assert torch.equal(loss, ge2e.ge2e_loss(e, w, b, with_eer=False)[0])
    _, eer_dp = ge2e.ge2e_loss_data_parallel(e, w, b, with_eer="device", fused=True)
    _, eer_f = ge2e.ge2e_loss_fused(e, w, b, with_eer="device")
    assert torch.is_tensor(eer_dp) and torch.equal(eer_dp, eer_f)


def test_speaker_encoder_loss_with_device_eer():
    """SpeakerEncoder.loss forwards with_eer: "device" returns a device tensor, and today's with_eer=True float (the host route
    on the same matrix) agrees with it to twice brentq's tolerance."""
    from models import SpeakerEncoder
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = SpeakerEncoder(40, 64, 1, 32, dev(), n_cores=2, rank=2).to(dev())
    S, U = 4, 3
    x = torch.rand(S * U, 12, 40, device=dev())
    with torch.no_grad():
        emb = enc(x).view(S, U, -1)
    for fused in (True, False):
        loss_d, eer_d = enc.loss(emb, fused=fused, with_eer="device")
        loss_h, eer_h = enc.loss(emb, fused=fused, with_eer=True)
        assert torch.is_tensor(eer_d) and eer_d.is_cuda and eer_d.dtype == torch.float64 and isinstance(eer_h, float)
        print("fused %s: device %.17g host %.17g" % (fused, float(eer_d.cpu().numpy()), eer_h))
        assert abs(float(eer_d.cpu().numpy()) - eer_h) <= C.HOST_TOL
        assert torch.equal(loss_d, loss_h)


@pytest.mark.parametrize("route,workgroups", [("one", 0), ("grid", 3)])
def test_graph_capture_replays_on_new_scores(route, workgroups):
    """eer_fused recorded on one stream; every replay reads the static buffer's current contents and matches the eager call."""
    from ttrnn_hip import ge2e
    S, U = 16, 32
    names = ("clustered", "ties_half", "low_byte")
    static = torch.zeros(S, U, S, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ge2e.eer_fused(static, want_aux=True, route=route, workgroups=workgroups)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge2e.eer_fused(static, want_aux=True, route=route, workgroups=workgroups)
    for name in names:
        sim, exact = C.case(name, (S, U))
        x = torch.from_numpy(sim.copy()).to(dev())
        with torch.no_grad():
            static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        replayed = (float(out[0].cpu().numpy()), out[1].cpu().numpy()[()], tuple(int(v) for v in out[2].cpu().numpy()))
        eager = run(x, route, workgroups)
        assert bits_of(replayed) == bits_of(eager), name
        C.check(replayed, exact, "replay of " + name)

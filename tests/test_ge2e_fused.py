"""The fused GE2E similarity / loss / gradient kernels (ttrnn_fast_ge2e.hip, include/ttrnn.h TTRNN_HAS_GE2E) on the device:
against float64 under a bound tied to the tensor-op path's own fp32 error, against the reference-made fixtures, bitwise
repeatability, graph capture, and the callers (SpeakerEncoder.loss, ge2e_loss_data_parallel)."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

import ge2e_fused_common as C

sys.path.insert(0, os.path.join(C.ROOT, "examples"))

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def scalars(w, b):
    return (torch.tensor(w, device=dev(), requires_grad=True), torch.tensor(b, device=dev(), requires_grad=True))


def run_fused(E, A, w, b, g, want_sim=True):
    """ge2e_loss_fused + backward of g * loss (+ similarity_matrix_fused) -> dict of device tensors."""
    from ttrnn_hip import ge2e
    e = E.to(dev()).requires_grad_(True)
    a = A.to(dev()) if A is not None else None
    wt, bt = scalars(w, b)
    loss, _ = ge2e.ge2e_loss_fused(e, wt, bt, a)
    (g * loss).backward()
    out = {"loss": loss.detach(), "d_E": e.grad, "d_w": wt.grad, "d_b": bt.grad}
    if want_sim:
        out["sim"] = ge2e.similarity_matrix_fused(e, wt, bt, a)
    return out


def to_np(res):
    return {k: v.double().cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_fused_matches_float64(case):
    (S, U, D, Ue), (w, b, g) = case
    E, A = C.inputs(S, U, D, Ue)
    got = to_np(run_fused(E, A, w, b, g))
    C.check(got, C.reference(case), C.evaluate(E, A, w, b, g, torch.float32, dev()), C.case_id(case))
    if S == 1:
        assert got["loss"] == 0 and got["d_w"] == 0 and got["d_b"] == 0 and not got["d_E"].any()


@pytest.mark.parametrize("case", C.LOOP_CASES, ids=C.loop_id)
def test_fused_multi_pass_loops_match_float64(case):
    """Strided loops of more than one pass, two tiles in both tile loops of phase 3, the descriptors at the plan's limits."""
    (S, U, D, Ue), (w, b, g) = case
    E, A = C.inputs(S, U, D, Ue)
    got = to_np(run_fused(E, A, w, b, g))
    C.check(got, C.reference(case), C.evaluate(E, A, w, b, g, torch.float32, dev()), C.loop_id(case))


@pytest.mark.parametrize("case", C.RANGE_CASES, ids=C.range_id)
def test_fused_value_ranges_match_float64(case):
    """Large and negative w (the softmax's max-subtraction), exact zero centroids and centroid norms on both sides of eps."""
    name, (w, b, g) = case
    E, A = C.range_inputs(name)
    ref = C.range_reference(case)
    got = to_np(run_fused(E, A, w, b, g))
    assert all(np.isfinite(v).all() for v in got.values())
    C.check(got, ref, C.evaluate(E, A, w, b, g, torch.float32, dev()), C.range_id(case))


@pytest.mark.parametrize("case", C.LONG_CASES, ids=C.long_id)
def test_fused_long_sums_match_float64(case):
    """Many rows per speaker, up to the row limit of 2^22: the sums over U of phases 1 and 3 under the same rule."""
    (S, U, D, Ue), (w, b, g) = case
    E, A = C.inputs(S, U, D, Ue)
    got = to_np(run_fused(E, A, w, b, g))
    C.check(got, C.reference(case), C.evaluate(E, A, w, b, g, torch.float32, dev()), C.long_id(case))


@pytest.mark.parametrize("name", C.fixture_names())
def test_fused_matches_reference_fixture(name):
    d, emb, enr = C.load_fixture(name)
    got = to_np(run_fused(emb, enr, float(d["weight"]), float(d["bias"]), 1.0))
    assert float(np.abs(got["sim"] - d["sim"]).max()) <= 1e-5
    assert abs(float(got["loss"]) - float(d["loss"])) <= 2e-5
    assert float(np.abs(got["d_E"] - d["d_embeds"]).max()) <= 2e-6


@pytest.mark.parametrize("shape", [(65, 3, 256, 0), (16, 32, 256, 0), (7, 3, 36, 2), (17, 257, 20, 0), (300, 2, 5, 0), (3, 2, 300, 0)],
                         ids=str)
def test_bitwise_repeatable(shape):
    """Two calls; a workspace filled with NaN before the call (nothing is read that the call did not write); and the
    similarity matrix requested or not: identical bits every time."""
    from ttrnn_hip import ge2e
    E, A = C.inputs(*shape)
    E, A = E.to(dev()), (A.to(dev()) if A is not None else None)
    w, b = torch.tensor(10.0, device=dev()), torch.tensor(-5.0, device=dev())
    g = torch.tensor(3.5, device=dev())

    def call(want_sim, workspace=None):
        loss, sim, state = ge2e._fused_forward(E, w, b, A, want_sim=want_sim, need_grad=True, workspace=workspace)
        return (loss, sim) + ge2e._fused_backward(state, g)

    first = call(True)
    again = call(True)
    ws = torch.full_like(ge2e._fused_forward(E, w, b, A)[2][3].view(torch.float32), float("nan")).view(torch.uint8)
    poisoned = call(True, ws)
    no_sim = call(False)
    for other in (again, poisoned):
        assert all(torch.equal(x, y) for x, y in zip(first, other))
    assert no_sim[1] is None and all(torch.equal(first[i], no_sim[i]) for i in (0, 2, 3, 4))
    assert all(bool(torch.isfinite(t).all()) for t in first)
    # gradients asked of a forward-only workspace are NaN, never stale
    state = ge2e._fused_forward(E, w, b, A, need_grad=False, workspace=ws)[2]
    assert all(bool(torch.isnan(t).all()) for t in ge2e._fused_backward(state, g))


def raw_call(E, A, w, b, g, with_loss=True, with_sim=True, want=(True, True, True)):
    """ttrnn_ge2e_forward + ttrnn_ge2e_backward through ctypes with NULL for every output not asked for; every buffer (outputs
    and workspace) holds NaN before the call, so an element the kernels do not write shows.  g: device scalar or None (NULL)."""
    import ctypes
    from ttrnn_hip import _lib, ge2e
    desc, nbytes, E, A, wd, bd = ge2e._fused_operands(E, w, b, A)
    S, U, _ = E.shape

    def nan(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())

    ws = nan(nbytes // 4)
    out = {"loss": nan() if with_loss else None, "sim": nan(S, U, S) if with_sim else None, "d_E": nan(*E.shape) if want[0] else None,
           "d_w": nan() if want[1] else None, "d_b": nan() if want[2] else None}
    lib, p = _lib.load(), ge2e._ptr
    _lib.check(lib.ttrnn_ge2e_forward(ctypes.byref(desc), p(E), p(A), p(wd), p(bd), p(out["loss"]), p(out["sim"]), 1, p(ws), nbytes,
                                      ge2e._stream(E)), "ttrnn_ge2e_forward")
    _lib.check(lib.ttrnn_ge2e_backward(ctypes.byref(desc), p(E), p(wd), p(g), p(out["d_E"]), p(out["d_w"]), p(out["d_b"]), p(ws),
                                       nbytes, ge2e._stream(E)), "ttrnn_ge2e_backward")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", [(7, 3, 36, 0), (7, 3, 36, 2)], ids=str)
def test_nullable_outputs(shape):
    """Every output the header allows to be NULL, left out: what is delivered has the bits of the call that asks for everything
    (with d_E == NULL the backward is a one-workgroup grid), and no delivered element is left unwritten."""
    E, A = C.inputs(*shape)
    E, A = E.to(dev()), (A.to(dev()) if A is not None else None)
    w, b = torch.tensor(10.0, device=dev()), torch.tensor(-5.0, device=dev())
    g = torch.tensor(3.5, device=dev())
    full = raw_call(E, A, w, b, g)
    assert all(bool(torch.isfinite(t).all()) for t in full.values())
    assert float(full["d_E"].abs().max()) > 0 and float(full["d_w"].abs()) > 0

    def same(got, ref, keys):
        assert {k for k, v in got.items() if v is not None} == set(keys)
        for k in keys:
            assert torch.equal(got[k], ref[k]), k      # NaN never compares equal: an unwritten element fails here too

    same(raw_call(E, A, w, b, g, with_loss=False), full, ("sim", "d_E", "d_w", "d_b"))
    same(raw_call(E, A, w, b, g, with_loss=False, with_sim=False), full, ("d_E", "d_w", "d_b"))
    same(raw_call(E, A, w, b, g, want=(False, True, True)), full, ("loss", "sim", "d_w", "d_b"))
    same(raw_call(E, A, w, b, g, want=(True, False, False)), full, ("loss", "sim", "d_E"))
    same(raw_call(E, A, w, b, g, want=(False, False, True)), full, ("loss", "sim", "d_b"))
    one = raw_call(E, A, w, b, torch.tensor(1.0, device=dev()))
    same(raw_call(E, A, w, b, None), one, ("loss", "sim", "d_E", "d_w", "d_b"))
    assert not torch.equal(one["d_E"], full["d_E"])


def test_graph_capture_replays_on_new_values():
    """Loss + backward recorded on one stream; the replay reads the embeddings, w, b and the upstream gradient on the device."""
    capture_and_replay(16, 32, 256)


def test_graph_capture_replays_through_tile_carries():
    """The same at two tiles per chunk in ge2e_cgrad_body and two per speaker in ge2e_asum_body."""
    capture_and_replay(17, 257, 20)


def capture_and_replay(S, U, D):
    from ttrnn_hip import ge2e
    E0, _ = C.inputs(S, U, D, 0)
    e = E0.to(dev()).requires_grad_(True)
    w, b = scalars(10.0, -5.0)
    up = torch.tensor(1.0, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss, _ = ge2e.ge2e_loss_fused(e, w, b)
        torch.autograd.grad(loss * up, [e, w, b])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, _ = ge2e.ge2e_loss_fused(e, w, b)
        grads = torch.autograd.grad(loss * up, [e, w, b])
    E1 = torch.roll(E0, 3, dims=0).mul(1.25).to(dev())
    with torch.no_grad():
        e.copy_(E1)
        w.fill_(3.7)
        b.fill_(0.4)
        up.fill_(3.5)
    graph.replay()
    torch.cuda.synchronize()
    eager = run_fused(E1.cpu(), None, 3.7, 0.4, 3.5, want_sim=False)
    assert torch.equal(loss.detach(), eager["loss"])
    for got, ref in zip(grads, (eager["d_E"], eager["d_w"], eager["d_b"])):
        assert torch.equal(got, ref)
    assert float(eager["d_E"].abs().max()) > 0


def test_speaker_encoder_loss_fused_vs_torch_ops():
    from models import SpeakerEncoder
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = SpeakerEncoder(40, 64, 1, 32, dev(), n_cores=2, rank=2).to(dev())
    S, U = 4, 3
    x = torch.rand(S * U, 12, 40, device=dev())
    grads, losses = [], []
    for fused in (True, False):
        enc.zero_grad(set_to_none=True)
        loss, _ = enc.loss(enc(x).view(S, U, -1), fused=fused, with_eer=False)
        loss.backward()
        losses.append(loss.item())
        grads.append({n: p.grad.clone() for n, p in enc.named_parameters()})
    assert abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[1]))
    assert set(grads[0]) == set(grads[1])
    # the encoder's own parameters (recurrent layers, head): 1e-5 of each gradient's maximum.  The similarity weight / bias are
    # not compared this way — d_b is 0 in exact arithmetic, so "its maximum" is either path's rounding error, and d_w is a sum
    # of cancelling terms: they get the float64 rule of test_fused_matches_float64 on these very embeddings instead.
    encoder = [n for n in grads[1] if not n.startswith("similarity_")]
    assert len(encoder) >= 8
    for name in encoder:
        ref = grads[1][name]
        scale = float(ref.abs().max())
        assert scale > 0, name
        assert float((grads[0][name] - ref).abs().max()) <= 1e-5 * scale, name
    emb = enc(x).view(S, U, -1).detach().cpu()
    C.check(to_np(run_fused(emb, None, 10.0, -5.0, 1.0)), C.evaluate(emb, None, 10.0, -5.0, 1.0, torch.float64),
            C.evaluate(emb, None, 10.0, -5.0, 1.0, torch.float32, dev()), "encoder embeddings")
    # the default picks the kernels where they take the call, and the validation form runs through them too
    with torch.no_grad():
        emb = enc(x).view(S, U, -1)
        auto, eer = enc.loss(emb)
        ref, eer_ref = enc.loss(emb, fused=False)
        val, _ = enc.loss(emb, emb[:, :2], with_eer=False)
        val_ref, _ = enc.loss(emb, emb[:, :2], fused=False, with_eer=False)
    assert abs(auto.item() - ref.item()) <= 1e-5 and abs(eer - eer_ref) <= 1e-4
    assert abs(val.item() - val_ref.item()) <= 1e-5


def test_data_parallel_fused_one_rank(tmp_path):
    """ge2e_loss_data_parallel(fused=True) through the all-gather of a one-rank group = the single-process fused loss."""
    import torch.distributed as dist
    from ttrnn_hip import ge2e
    E, _ = C.inputs(5, 2, 32, 0)
    single = run_fused(E, None, 10.0, -5.0, 1.0, want_sim=False)
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        e = E.to(dev()).requires_grad_(True)
        w, b = scalars(10.0, -5.0)
        loss, _ = ge2e.ge2e_loss_data_parallel(e, w, b, with_eer=False, force_gather=True, fused=True)
        loss.backward()
    finally:
        dist.destroy_process_group()
    assert torch.equal(loss.detach(), single["loss"]) and torch.equal(e.grad, single["d_E"])
    assert torch.equal(w.grad, single["d_w"]) and torch.equal(b.grad, single["d_b"])

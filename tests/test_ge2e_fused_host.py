"""The fused GE2E loss without a GPU: the phase bodies of tensorized-rnn_amd/csrc/ttrnn_ge2e.h — the arithmetic of the four
kernels of ttrnn_fast_ge2e.hip — through the serial host executor tests/hostemu/hostemu_ge2e.cpp against the reference-made
fixtures and against float64, and the host-side logic of the library's entry points (descriptor checks, workspace query)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import ge2e_fused_common as C
from ttrnn_hip import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "hostemu", "libttrnn_hostemu_ge2e.so")


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(HERE, "hostemu", "hostemu_ge2e.cpp")
    csrc = os.path.join(ROOT, "tensorized-rnn_amd", "csrc")
    deps = [src, os.path.join(csrc, "ttrnn_ge2e.h"), os.path.join(csrc, "ttrnn_core.h"), os.path.join(ROOT, "include", "ttrnn.h")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                               "-o", SO, src])
    lib = ctypes.CDLL(SO)
    lib.hostemu_ge2e_workspace_floats.restype = ctypes.c_long
    lib.hostemu_ge2e.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else ctypes.c_void_p(0)


FORWARD, REVERSE = 0, 1      # hostemu_ge2e's thread orders; any other value seeds a permutation


def run_emu(emu, E, A, w, b, g, order=FORWARD):
    """All four phases on numpy copies of the torch inputs -> dict as ge2e_fused_common.evaluate."""
    S, U, D = E.shape
    desc = _lib.Ge2eDesc(S, U, D, A.shape[1] if A is not None else 0)
    n = emu.hostemu_ge2e_workspace_floats(ctypes.byref(desc))
    assert n > 0
    e = np.ascontiguousarray(E.numpy(), dtype=np.float32)
    a = np.ascontiguousarray(A.numpy(), dtype=np.float32) if A is not None else None
    ws = np.empty(n, dtype=np.float32)
    sim, d_E = np.full((S, U, S), np.nan, np.float32), np.full((S, U, D), np.nan, np.float32)
    sc = {k: np.full(1, v, np.float32) for k, v in (("w", w), ("b", b), ("g", g), ("loss", np.nan), ("dw", np.nan), ("db", np.nan))}
    st = emu.hostemu_ge2e(ctypes.byref(desc), _p(e), _p(a), _p(sc["w"]), _p(sc["b"]), _p(sc["g"]), _p(sc["loss"]), _p(sim), 1,
                          _p(d_E), _p(sc["dw"]), _p(sc["db"]), _p(ws), ctypes.c_int(order))
    assert st == 0
    return {"sim": sim, "loss": sc["loss"][0], "d_E": d_E, "d_w": sc["dw"][0], "d_b": sc["db"][0]}


@pytest.mark.parametrize("name", C.fixture_names())
def test_host_bodies_match_reference_fixture(emu, name):
    d, emb, enr = C.load_fixture(name)
    got = run_emu(emu, emb, enr, float(d["weight"]), float(d["bias"]), 1.0)
    assert float(np.abs(got["sim"] - d["sim"]).max()) <= 1e-5
    assert abs(float(got["loss"]) - float(d["loss"])) <= 1e-5
    assert float(np.abs(got["d_E"] - d["d_embeds"]).max()) <= 1e-6


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_host_bodies_match_float64(emu, case):
    (S, U, D, Ue), (w, b, g) = case
    E, A = C.inputs(S, U, D, Ue)
    got = run_emu(emu, E, A, w, b, g)
    C.check(got, C.reference(case), C.evaluate(E, A, w, b, g, torch.float32), C.case_id(case))
    if S == 1:
        assert got["loss"] == 0 and got["d_w"] == 0 and got["d_b"] == 0 and not got["d_E"].any()


@pytest.mark.parametrize("case", C.LOOP_CASES, ids=C.loop_id)
def test_host_bodies_multi_pass_loops_match_float64(emu, case):
    """Strided loops of more than one pass, two tiles in both tile loops of phase 3, the descriptors at the plan's limits."""
    (S, U, D, Ue), (w, b, g) = case
    E, A = C.inputs(S, U, D, Ue)
    C.check(run_emu(emu, E, A, w, b, g), C.reference(case), C.evaluate(E, A, w, b, g, torch.float32), C.loop_id(case))


@pytest.mark.parametrize("case", C.LONG_CASES, ids=C.long_id)
def test_host_bodies_long_sums_match_float64(emu, case):
    """Many rows per speaker, up to the row limit: the sums over U of phases 1 and 3 under the same rule as every other shape."""
    (S, U, D, Ue), (w, b, g) = case
    E, A = C.inputs(S, U, D, Ue)
    C.check(run_emu(emu, E, A, w, b, g), C.reference(case), C.evaluate(E, A, w, b, g, torch.float32), C.long_id(case))


@pytest.mark.parametrize("case", C.RANGE_CASES, ids=C.range_id)
def test_host_bodies_value_ranges_match_float64(emu, case):
    """Large and negative w (the softmax's max-subtraction), exact zero centroids and centroid norms on both sides of eps."""
    name, (w, b, g) = case
    E, A = C.range_inputs(name)
    ref = C.range_reference(case)
    got = run_emu(emu, E, A, w, b, g)
    assert all(np.isfinite(np.asarray(v)).all() for v in got.values())
    C.check(got, ref, C.evaluate(E, A, w, b, g, torch.float32), C.range_id(case))


@pytest.mark.parametrize("case", C.CASES + C.LOOP_CASES + C.RANGE_CASES, ids=lambda c: (C.range_id if isinstance(c[0], str) else C.case_id)(c))
def test_thread_order_does_not_matter(emu, case):
    """The threads of every par in forward, reverse and one shuffled order: identical bits.  A value written and read inside one
    par without a barrier between would differ here, as it would race on the device."""
    E, A = C.range_inputs(case[0]) if isinstance(case[0], str) else C.inputs(*case[0])
    w, b, g = case[1]
    first = run_emu(emu, E, A, w, b, g, FORWARD)
    assert all(np.isfinite(np.asarray(v)).all() for v in first.values())
    for order in (REVERSE, 4711):
        other = run_emu(emu, E, A, w, b, g, order)
        for key in ("sim", "loss", "d_E", "d_w", "d_b"):
            assert np.array_equal(np.asarray(first[key]).view(np.uint32), np.asarray(other[key]).view(np.uint32)), (key, order)


def test_entry_points_host_logic():
    """What the library decides before it launches anything; it loads without a device."""
    lib = _lib.load()
    ws = lib.ttrnn_ge2e_workspace

    def desc(*a):
        return ctypes.byref(_lib.Ge2eDesc(*a))

    assert ws(desc(16, 32, 256, 0)) > 0 and ws(desc(40, 32, 256, 32)) > 0 and ws(desc(128, 5, 512, 0)) > 0
    assert ws(desc(7, 1, 36, 2)) > 0                     # one verification utterance is fine against enrollment centroids
    one = ctypes.c_void_p(8)                             # any non-NULL pointer: refused calls launch nothing
    for bad in ((4, 1, 8, 0), (0, 2, 8, 0), (4, 0, 8, 0), (4, 2, 0, 0), (4, 2, 8, -1), (-1, 2, 8, 0)):
        assert ws(desc(*bad)) == 0
        assert lib.ttrnn_ge2e_forward(desc(*bad), one, one, one, one, one, None, 1, one, 1 << 30, None) == -1
        assert lib.ttrnn_ge2e_backward(desc(*bad), one, one, None, one, one, one, one, 1 << 30, None) == -1
    for big in ((4096, 2, 8, 0), (4, 2, 8192, 0)):       # beyond the plan: refused, never a wrong answer
        assert ws(desc(*big)) == 0
        assert lib.ttrnn_ge2e_forward(desc(*big), one, one, one, one, one, None, 1, one, 1 << 30, None) == -3
    good, n = desc(4, 2, 8, 0), ws(desc(4, 2, 8, 0))
    assert lib.ttrnn_ge2e_forward(None, one, one, one, one, one, None, 1, one, n, None) == -2
    assert lib.ttrnn_ge2e_forward(good, None, None, one, one, one, None, 1, one, n, None) == -2       # E
    assert lib.ttrnn_ge2e_forward(good, one, None, None, one, one, None, 1, one, n, None) == -2       # w
    assert lib.ttrnn_ge2e_forward(good, one, None, one, None, one, None, 1, one, n, None) == -2       # b
    assert lib.ttrnn_ge2e_forward(good, one, None, one, one, one, None, 1, None, n, None) == -2       # workspace
    assert lib.ttrnn_ge2e_forward(desc(4, 2, 8, 3), one, None, one, one, one, None, 1, one, 1 << 30, None) == -2   # A
    assert lib.ttrnn_ge2e_forward(good, one, None, one, one, one, None, 1, one, n - 1, None) == -4
    assert lib.ttrnn_ge2e_backward(good, None, one, None, one, one, one, one, n, None) == -2
    assert lib.ttrnn_ge2e_backward(good, one, None, None, one, one, one, one, n, None) == -2
    assert lib.ttrnn_ge2e_backward(good, one, one, None, one, one, one, None, n, None) == -2
    assert lib.ttrnn_ge2e_backward(good, one, one, None, one, one, one, one, n - 1, None) == -4
    assert lib.ttrnn_abi_version() == 7


def test_fused_supported_and_no_fallback():
    from ttrnn_hip import TtrnnError, ge2e
    assert not ge2e.fused_supported(16, 32, 256, torch.float32, torch.device("cpu"))
    assert not ge2e.fused_supported(16, 32, 256, torch.bfloat16, torch.device("cuda", 0))
    assert not ge2e.fused_supported(16, 1, 256, torch.float32, torch.device("cuda", 0))
    assert ge2e.fused_supported(16, 32, 256, torch.float32, torch.device("cuda", 0))
    assert ge2e.fused_supported(16, 1, 256, torch.float32, torch.device("cuda", 0), U_enroll=4)
    E = torch.randn(4, 3, 8, requires_grad=True)
    w, b = torch.tensor(10.0), torch.tensor(-5.0)
    with pytest.raises(TtrnnError):
        ge2e.ge2e_loss_fused(E, w, b)
    with pytest.raises(TtrnnError):
        ge2e.similarity_matrix_fused(E, w, b)
    with pytest.raises(TtrnnError):
        ge2e.ge2e_loss_fused(E, w, b, torch.randn(4, 2, 8, requires_grad=True))
    with pytest.raises(TtrnnError):
        ge2e.ge2e_loss_data_parallel(E, w, b, fused=True)

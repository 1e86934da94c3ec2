"""The device-side equal error rate without a GPU: the phase bodies of tensorized-rnn_amd/csrc/ttrnn_eer.h — the arithmetic of
the kernels of ttrnn_fast_eer.hip — through the serial host executor tests/hostemu/hostemu_eer.cpp against the exact-integer
oracle of ge2e_eer_common, that oracle against the host route (ge2e.eer: roc_curve + interp1d + brentq) and the reference-made
fixtures, and what the library's entry points and the Python wrappers decide before anything is launched."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import ge2e_eer_common as C
import ge2e_fused_common as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "hostemu", "libttrnn_hostemu_eer.so")

FORWARD, REVERSE, SHUFFLED = 0, 1, 4711      # hostemu_eer's thread / workgroup orders; any other value seeds a permutation
ORDERS = [(FORWARD, FORWARD), (REVERSE, REVERSE), (SHUFFLED, 1234), (FORWARD, REVERSE)]


class EerDesc(ctypes.Structure):
    """struct ttrnn_eer_desc of include/ttrnn.h, restated here so that this file needs nothing of the binding"""
    _fields_ = [("S", ctypes.c_int32), ("U", ctypes.c_int32), ("route", ctypes.c_int32), ("workgroups", ctypes.c_int32)]


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(HERE, "hostemu", "hostemu_eer.cpp")
    csrc = os.path.join(ROOT, "tensorized-rnn_amd", "csrc")
    deps = [src, os.path.join(csrc, "ttrnn_eer.h"), os.path.join(csrc, "ttrnn_core.h"), os.path.join(ROOT, "include", "ttrnn.h")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                               "-o", SO, src])
    lib = ctypes.CDLL(SO)
    lib.hostemu_eer_plan.restype = ctypes.c_int
    lib.hostemu_eer.restype = ctypes.c_int
    return lib


def run_emu(emu, sim, route, workgroups=0, thread_order=FORWARD, wg_order=FORWARD, aux=True):
    """The whole call on a float32 [S, U, S] numpy matrix -> (eer, theta, counts); outputs start as poison."""
    S, U, _ = sim.shape
    desc = EerDesc(S, U, route, workgroups)
    words = ctypes.c_long(0)
    assert emu.hostemu_eer_plan(ctypes.byref(desc), ctypes.byref(words), None, None) == 0
    ws = np.empty(max(words.value, 1), dtype=np.uint32)
    eer = np.full(1, -7.0, np.float64)
    theta = np.full(1, -7.0, np.float32)
    counts = np.full(4, -7, np.int64)
    before = sim.copy()
    st = emu.hostemu_eer(ctypes.byref(desc), sim.ctypes.data_as(ctypes.c_void_p), eer.ctypes.data_as(ctypes.c_void_p),
                         theta.ctypes.data_as(ctypes.c_void_p) if aux else None,
                         counts.ctypes.data_as(ctypes.c_void_p) if aux else None, ws.ctypes.data_as(ctypes.c_void_p),
                         ctypes.c_int(thread_order), ctypes.c_int(wg_order))
    assert st == 0
    assert np.array_equal(before.view(np.uint32), sim.view(np.uint32))
    return float(eer[0]), theta[0], tuple(int(c) for c in counts)


def bits_of(got):
    return (np.float64(got[0]).view(np.uint64), np.float32(got[1]).view(np.uint32), got[2])


def configs(S, U):
    return [(1, 0), (0, 0)] + [(2, g) for g in C.grid_counts(S, U)]


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_host_bodies_match_exact(emu, case):
    """Every builder x every shape, both routes, route 2 with 1, 2, 3, 7, a non-dividing count and (where 256 workgroups allow
    it) more workgroups than rows: theta bit for bit, counts exactly, the EER to 2^-50 — and the same bits under every order of
    threads and workgroups."""
    name, (S, U) = case
    sim, exact = C.case(name, (S, U))
    for route, g in configs(S, U):
        first = run_emu(emu, sim, route, g)
        C.check(first, exact, "%s route %d workgroups %d" % (C.case_id(case), route, g))
        for t_order, w_order in ORDERS[1:]:
            other = run_emu(emu, sim, route, g, t_order, w_order)
            assert bits_of(other) == bits_of(first), (route, g, t_order, w_order)


def test_host_bodies_at_the_workgroup_cap(emu):
    """Shapes with more rows than the cap cannot have more workgroups than rows; the cap itself, at the training batch."""
    sim, exact = C.case("clustered", (16, 32))
    C.check(run_emu(emu, sim, 2, C.MAX_WORKGROUPS), exact, "workgroups 256")
    C.check(run_emu(emu, sim, 2, C.MAX_WORKGROUPS, REVERSE, SHUFFLED), exact, "workgroups 256, other order")


def test_host_bodies_large_shape(emu):
    """S at its limit, 8.4 M scores, Nn P > 2^32: route 1, route 2 with a count that does not divide, and the library's choice
    (a grid)."""
    sim, exact = C.case(*C.LARGE_CASE)
    first = run_emu(emu, sim, 1)
    C.check(first, exact, "large route 1")
    for route, g, t_order, w_order in ((2, 7, REVERSE, SHUFFLED), (0, 0, FORWARD, REVERSE)):
        other = run_emu(emu, sim, route, g, t_order, w_order)
        C.check(other, exact, "large route %d workgroups %d" % (route, g))
        assert bits_of(other) == bits_of(first)


def test_null_outputs(emu):
    sim, exact = C.case("clustered", (3, 7))
    for route, g in ((1, 0), (2, 3)):
        assert run_emu(emu, sim, route, g, aux=False)[0] == run_emu(emu, sim, route, g)[0]


@pytest.mark.parametrize("case", [c for c in C.CASES if c[0] not in C.NO_HOST_ROUTE], ids=C.case_id)
def test_exact_matches_host_route(case):
    """The oracle against ge2e.eer (sklearn's roc_curve, scipy's interp1d and brentq): if the host route stopped meaning what
    the kernels compute, this would show it."""
    from ttrnn_hip import ge2e
    name, (S, U) = case
    sim, exact = C.case(name, (S, U))
    host = ge2e.eer(sim.reshape(S * U, S), S, U)
    print("%s: exact %.17g host %.17g diff %.3e" % (C.case_id(case), exact[0], host, abs(exact[0] - host)))
    assert abs(exact[0] - host) <= C.HOST_TOL


@pytest.mark.parametrize("name", F.fixture_names())
def test_exact_and_host_bodies_match_reference_fixture(emu, name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    sim = np.ascontiguousarray(d["sim"], dtype=np.float32)
    S = sim.shape[-1]
    sim = sim.reshape(S, -1, S)
    exact = C.eer_exact(sim)
    print("%s: exact %.17g stored %.17g" % (name, exact[0], float(d["eer"])))
    assert abs(exact[0] - float(d["eer"])) <= C.HOST_TOL
    for route, g in ((1, 0), (2, 3)):
        C.check(run_emu(emu, sim, route, g), exact, "%s route %d" % (name, route))


def test_entry_points_host_logic(emu):
    """Every refusal is decided before any launch: the listed code with no GPU, and a workspace query of 0."""
    from ttrnn_hip import _lib
    _lib.load()                                          # raises if libttrnn.so is not built
    lib = ctypes.CDLL(_lib.LIB_PATH)                     # a handle of this test's own: its signatures use the structure above
    ws = lib.ttrnn_ge2e_eer_workspace
    ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.POINTER(EerDesc)]
    call = lib.ttrnn_ge2e_eer
    call.restype = ctypes.c_int
    call.argtypes = [ctypes.POINTER(EerDesc)] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
    one = ctypes.c_void_p(8)                             # any non-NULL pointer: refused calls launch nothing

    def desc(*a):
        return ctypes.byref(EerDesc(*a))

    bad = [(1, 4, 0, 0), (0, 4, 0, 0), (-1, 4, 0, 0),                       # S < 2: no negatives
           (4, 0, 0, 0), (4, -3, 0, 0),                                     # U < 1
           (4, 2, -1, 0), (4, 2, 3, 0),                                     # route outside 0 .. 2
           (4, 2, 2, -1), (4, 2, 2, C.MAX_WORKGROUPS + 1),                  # workgroups negative / above the cap
           (4, 2, 0, 2), (4, 2, 1, 1)]                                      # workgroups without route 2
    for b in bad:
        assert ws(desc(*b)) == 0, b
        assert call(desc(*b), one, one, one, one, one, 1 << 30, None) == -1, b
        assert emu.hostemu_eer_plan(desc(*b), None, None, None) == -1, b
    big = [(2049, 1, 0, 0), (2, (1 << 21) + 1, 0, 0), (2048, 257, 0, 0), (2048, 2048, 2, 4)]
    assert 2048 * 257 <= 1 << 22 and 2048 * 257 * 2048 > 1 << 30          # the third is refused for its element count alone
    for b in big:
        assert ws(desc(*b)) == 0, b
        assert call(desc(*b), one, one, one, one, one, 1 << 30, None) == -3, b
    # the limits themselves are taken
    for ok in ((2, 1, 0, 0), (2048, 2, 0, 0), (2, 1 << 21, 0, 0), (2048, 256, 0, 0), (16, 32, 2, C.MAX_WORKGROUPS), (16, 32, 2, 1)):
        assert ws(desc(*ok)) > 0, ok
    for d in ((16, 32, 1, 0), (16, 32, 2, 5), (16, 32, 0, 0)):
        n = ws(desc(*d))
        assert call(None, one, one, one, one, one, n, None) == -2
        assert call(desc(*d), None, one, one, one, one, n, None) == -2       # sim
        assert call(desc(*d), one, None, one, one, one, n, None) == -2       # eer
        assert call(desc(*d), one, one, one, one, None, n, None) == -2       # workspace
        assert call(desc(*d), one, one, None, None, one, n - 1, None) == -4
    # the grid's workspace holds its partial histograms: it grows with the workgroup count, and the emulator's plan is the library's
    assert ws(desc(16, 32, 2, 8)) > ws(desc(16, 32, 2, 2))
    words, route, g = ctypes.c_long(0), ctypes.c_int(0), ctypes.c_int(0)
    assert emu.hostemu_eer_plan(desc(16, 32, 2, 8), ctypes.byref(words), ctypes.byref(route), ctypes.byref(g)) == 0
    assert words.value * 4 == ws(desc(16, 32, 2, 8)) and (route.value, g.value) == (2, 8)
    assert lib.ttrnn_abi_version() == 7


def test_wrappers_refuse_without_fallback_and_keep_host_route():
    from ttrnn_hip import TtrnnError, ge2e
    assert not ge2e.eer_supported(16, 32, torch.float32, torch.device("cpu"))
    assert not ge2e.eer_supported(16, 32, torch.bfloat16, torch.device("cuda", 0))
    assert not ge2e.eer_supported(1, 32, torch.float32, torch.device("cuda", 0))
    assert not ge2e.eer_supported(4096, 2, torch.float32, torch.device("cuda", 0))
    assert ge2e.eer_supported(16, 32, torch.float32, torch.device("cuda", 0))
    assert ge2e.eer_supported(40, 32, torch.float32, "cuda")
    sim = torch.from_numpy(C.case("clustered", (3, 7))[0].copy())
    with pytest.raises(TtrnnError):
        ge2e.eer_fused(sim)
    with pytest.raises(TtrnnError):
        ge2e.eer_fused(sim.to(torch.bfloat16))
    with pytest.raises(TtrnnError):
        ge2e.eer_fused(sim.reshape(21, 3), want_aux=True)
    E, _ = F.inputs(5, 2, 32, 0)
    w, b = torch.tensor(10.0), torch.tensor(-5.0)
    with pytest.raises(TtrnnError):
        ge2e.ge2e_loss(E, w, b, with_eer="device")
    with pytest.raises(TtrnnError):
        ge2e.ge2e_loss_fused(E, w, b, with_eer="device")
    with pytest.raises(TtrnnError):
        ge2e.ge2e_loss_data_parallel(E, w, b, with_eer="device")
    with pytest.raises(ValueError):
        ge2e.ge2e_loss(E, w, b, with_eer="host")
    # True / False / None are today's: a float from the host route, or None
    loss, e = ge2e.ge2e_loss(E, w, b, with_eer=True)
    sim2d = ge2e.similarity_matrix(E, w, b).reshape(10, 5)
    assert isinstance(e, float) and e == ge2e.eer(sim2d.numpy(), 5, 2)
    assert abs(e - C.eer_exact(sim2d.numpy().reshape(5, 2, 5))[0]) <= C.HOST_TOL
    assert ge2e.ge2e_loss(E, w, b, with_eer=False)[1] is None and ge2e.ge2e_loss(E, w, b, with_eer=None)[1] is None
    assert ge2e.ge2e_loss_data_parallel(E, w, b, with_eer=True)[1] == e
    for name in F.fixture_names():
        d, emb, enr = F.load_fixture(name)
        wt, bt = torch.tensor(float(d["weight"])), torch.tensor(float(d["bias"]))
        assert abs(ge2e.ge2e_loss(emb, wt, bt, enr, with_eer=True)[1] - float(d["eer"])) <= C.HOST_TOL


def test_stand_alone_program_builds_and_agrees(tmp_path):
    """-DHOSTEMU_EER_MAIN: one case per builder through both routes under all orders; exit status 0 = every result independent of
    route and order.  (The form a sanitizer build takes: add -fsanitize=address,undefined.)"""
    exe = str(tmp_path / "hostemu_eer")
    csrc = os.path.join(ROOT, "tensorized-rnn_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHOSTEMU_EER_MAIN", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-o", exe,
                           os.path.join(HERE, "hostemu", "hostemu_eer.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 11 and lines[-1].startswith("nan_last") and lines[-1].endswith("eer nan theta nan counts -1 -1 -1 -1")

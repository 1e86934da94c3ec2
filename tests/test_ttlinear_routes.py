"""ttrnn_ttlinear_forward / _backward / _backward_hinted on every route `lin_backward` (csrc/ttrnn_api.hip) can choose, through
the C ABI with caller-owned buffers, against a float64 evaluation of the oracle.

`expected_route` below restates the dispatch of lin_backward as a table: per shape class, row count, request set, storage and
math mode the route a call takes, the option(s) that switch that route off, and whether it sums in a fixed order.  Every case
proves its row of the table on the device: under each named option at least one requested buffer must change bitwise; a case
that claims the any-shape chain kernel must give the bits of force_generic = 1.  A stale table fails — nothing is skipped.

Per case:
  values         per tensor  err <= max(4 x err of the any-shape route, floor x max|ref|)  (tests/ttlinear_abi.py), and for
                 fp32 storage DESIGN.md section 2 on top (forward 1e-5 x max(1, max|ref|), gradients 1e-4 of the maximum)
  writes         dx starts NaN-filled and comes back finite; a NULL output does not fail the call
  accumulation   d_packed / d_bias start from seeded values r: the result is r + gradient; the second half of d_packed
                 keeps its bits
  workspace      NaN-filled, with a 4 KiB tail that must keep its pattern; a second run on a zero-filled workspace gives the
                 same bits
  repeatability  the second run is bit-identical for the routes that sum in a fixed order (dense gradients, proj*, in1)

Where a route flushes partial sums with float atomics (launch_ttlinear_bwd_fast, the fused-core weight-gradient kernel, the
merged-core kernel, and the any-shape kernel as soon as it runs more than one workgroup) the bits of d_packed / d_bias depend
on the order of arrival, so for those the second run must give the same bits of dx and meet the value bound in d_packed /
d_bias; the bitwise comparison with force_generic = 1 of a chain case covers dx at every row count and every buffer at one
row (one workgroup, one flush).
"""
import collections
import contextlib

import pytest
import torch

from ttlinear_abi import REQUESTS, Lin, dev, judge, same_bits

pytestmark = pytest.mark.gpu

# fwd_nb / bwd_nb: rows per tile of the shape-specialised kernels (TT_LIN_SHAPES in csrc/ttrnn_fast_lin.hip, TT_LINB_SHAPES in
# csrc/ttrnn_fast_bwd.hip); f10: a fused-core weight-gradient kernel exists (fp32 storage), f10_dx: and it produces dx
Shape = collections.namedtuple("Shape", "name in_modes out_modes rank fwd_nb bwd_nb f10 f10_dx big")
SHAPES = [
    Shape("ShpH256R8L", [4, 8, 8], [8, 8, 16], 8, 4, 2, True, True, False),
    Shape("ShpI40R16L", [2, 4, 5], [8, 8, 16], 16, 4, 2, True, False, False),
    Shape("ShpI1R8L", [1, 1, 1], [8, 8, 16], 8, 16, 8, False, False, False),
    Shape("ShpH256R16G", [4, 8, 8], [8, 8, 12], 16, 2, 1, False, False, False),
    Shape("ShpH128R4L", [8, 16], [16, 32], 4, 16, 8, False, False, False),
    Shape("ShpHd256R16", [4, 8, 8], [4, 8, 8], 16, 4, 2, False, False, False),
    Shape("cfg5", [4, 4, 8, 8], [8, 8, 8, 8], 32, 0, 0, False, False, True),
    Shape("gen128x64", [4, 4, 8], [4, 4, 4], 3, 0, 0, False, False, False),
    Shape("gen32x24d4", [2, 2, 2, 4], [2, 3, 2, 2], 3, 0, 0, False, False, False),
    Shape("gen12x20d1", [12], [20], 1, 0, 0, False, False, False),
    Shape("gen28x30", [4, 7], [5, 6], 3, 0, 0, False, False, False),
    Shape("gen1x60", [1, 1], [6, 10], 3, 0, 0, False, False, False),
]
BY_NAME = {s.name: s for s in SHAPES}
Route = collections.namedtuple("Route", "name off fixed_order")


def _prod(v):
    r = 1
    for a in v:
        r *= a
    return r


def expected_route(shp, n, req, storage="fp32", dy_bf16=False, exact=False):
    """lin_backward, restated.  `off`: options that each move the call to another kernel; () = the any-shape chain kernel."""
    dx, dw, db = "dx" in req, "dw" in req, "db" in req
    f32 = storage == "fp32"
    split = storage == "bf16" or not exact                      # fp32_math() == TTRNN_MATH_SPLIT || dtype == TTRNN_BF16
    inn, out, d = _prod(shp.in_modes), _prod(shp.out_modes), len(shp.in_modes)
    many = n >= 4 * inn
    dense_ok = inn >= 4 and inn % 4 == 0 and out >= 4 and out % 4 == 0      # gen_dense().ok / dense_wgrad_ok
    dx_gemm = out % 8 == 0 and inn % 128 == 0                               # gemm_split_ok(out, in)
    proj = d in (2, 3, 4)                                                   # proj3_workspace_bytes > 0
    proj_off = (["no_proj3"] if proj else []) + (["no_proj4"] if d == 4 else [])
    table = shp.fwd_nb > 0
    if table:
        if inn == 1 and not dx and dw:
            return Route("in1", ("no_in1",), True)
        f10 = shp.f10 and f32 and not dy_bf16
        if split and dw and f10 and dense_ok and many and (not dx or (f32 and not exact and dx_gemm)):
            return Route("fused_core_dense", ("no_gemm", "no_proj3"), True)
        if split and dw and f10 and (not dx or shp.f10_dx):
            return Route("wgrad_f10", ("no_f10",), False)
        gdf_ok = dense_ok and proj and dw and not dy_bf16 and many and (not dx or (dx_gemm and f32 and not exact))
        if not gdf_ok:
            return Route("bwd_fast", ("force_generic",), False)
    if shp.big and (dw or (dx and not db)) and not dy_bf16:
        return Route("bwd_big", ("no_bigb",), False)
    if inn == 1 and not dx and dw:
        return Route("gen_in1", ("no_in1", "no_gemm"), True)
    if dense_ok and dw and not dy_bf16 and many and (not dx or (dx_gemm and f32 and split)):
        return Route("gdf" if table else "gd", tuple(["no_gemm"] + proj_off), True)
    return Route("chain", (), False)


def row_counts(shp):
    if shp.big:
        return [5, 70]
    t = 4 * _prod(shp.in_modes)
    c = {1, t - 1, t, t + 3}
    for nb in (shp.fwd_nb, shp.bwd_nb):
        if nb:
            c |= {nb - 1, nb + 1}
    return sorted(v for v in c if v >= 1)


def threshold_counts(shp):
    t = 4 * _prod(shp.in_modes)
    return [5, 70] if shp.big else [t - 1, t]


def _options(**kw):
    import ttrnn_hip
    st = contextlib.ExitStack()
    for k, v in kw.items():
        st.enter_context(ttrnn_hip.option(k, v))
    return st


def check_backward(tag, lin, shp, x, dy, req, ref, bad, exact=False, hints=None, routes=None):
    n = x.shape[0]
    route = expected_route(shp, n, req, lin.storage, dy.dtype == torch.bfloat16, exact)
    if routes is not None:
        routes[route.name] += 1
    tag = "%s %-11s %s" % (tag, "+".join(req), route.name)
    a = lin.backward(x, dy, req, nan_ws=True, hints=hints)
    b = lin.backward(x, dy, req, nan_ws=False, hints=hints)
    with _options(force_generic=1):
        gen = lin.backward(x, dy, req, nan_ws=True)
    ta, tg = lin.tensors(a), lin.tensors(gen)
    judge(tag, ta, tg, ref, lin.storage, bad, design2=1e-4)
    # the second run, on a zero-filled workspace
    if route.fixed_order:
        if not same_bits(a, b):
            bad.append((tag, "a second run on a zero-filled workspace gives other bits"))
    else:
        if not same_bits(a, b, ("dx",)):
            bad.append((tag, "dx of a second run on a zero-filled workspace has other bits"))
        judge(tag + " (2nd)", lin.tensors(b), tg, ref, lin.storage, bad, design2=1e-4)
    # the route ran
    if route.name == "chain":
        keys = ("dx", "dpk", "db") if n == 1 else ("dx",)
        if not same_bits(a, gen, keys):
            bad.append((tag, "claims the any-shape kernel but differs from force_generic = 1"))
    for opt in route.off:
        if opt == "force_generic":
            other = gen
        else:
            with _options(**{opt: 1}):
                other = lin.backward(x, dy, req, nan_ws=True, hints=hints)
        if same_bits(a, other):
            bad.append((tag, "option %s changes no bit: the route table is stale" % opt))


def check_forward(tag, lin, shp, x, ref, bad, kernel_check=True):
    y1 = lin.forward(x, nan_ws=True)
    y2 = lin.forward(x, nan_ws=False)
    with _options(force_generic=1):
        yg = lin.forward(x, nan_ws=True)
    judge(tag + " forward", {"y": y1.cpu().double()}, {"y": yg.cpu().double()}, ref, lin.storage, bad, design2=1e-5)
    if not torch.equal(y1, y2):
        bad.append((tag, "forward: a second run on a zero-filled workspace gives other bits"))
    # table shapes run k_ttlinear_fwd_fast, every other the any-shape kernel (bf16 outputs round the difference away)
    if kernel_check and lin.storage == "fp32" and (shp.fwd_nb > 0) == torch.equal(y1, yg):
        bad.append((tag, "forward: the kernel is not the one the table names"))


def _case(shp, n, requests, storage="fp32", dy_bf16=False, exact=False, forward=True, seed=0, routes=None, **knobs):
    import ttrnn_hip
    lin_kw = {k: knobs.pop(k) for k in ("zero_core",) if k in knobs}
    lin = Lin(shp.in_modes, shp.out_modes, shp.rank, storage, seed=100 + seed, **lin_kw)
    x, dy = lin.rows(n, 7 * n + seed, dy_bf16=dy_bf16, **knobs)
    ref = lin.reference(x, dy)
    tag = "%-11s n=%-4d %s%s%s" % (shp.name, n, storage, "/dy16" if dy_bf16 else "", " exact" if exact else "")
    bad = []
    with ttrnn_hip.fp32_math("exact" if exact else "split"):
        if forward:
            check_forward(tag, lin, shp, x, ref, bad, kernel_check="zero_core" not in lin_kw)      # (W = 0: y is the bias on any kernel)
        for req in requests:
            check_backward(tag, lin, shp, x, dy, req, ref, bad, exact=exact, routes=routes)
    assert not bad, bad


CASES = [(s.name, n) for s in SHAPES for n in row_counts(s)]


@pytest.mark.parametrize("name,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_fp32(name, n):
    shp = BY_NAME[name]
    _case(shp, n, REQUESTS if n in threshold_counts(shp) else REQUESTS[:2])


@pytest.mark.parametrize("name", [s.name for s in SHAPES])
def test_fp32_exact_math(name):
    """TTRNN_MATH_EXACT: the fused-core kernels and every GEMM on fp16 / bf16 pieces are off; the dense gradient stays (fp32 MFMA)."""
    shp = BY_NAME[name]
    _case(shp, threshold_counts(shp)[-1] if not shp.big else 5, [REQUESTS[0], REQUESTS[1], REQUESTS[2]], exact=True)


@pytest.mark.parametrize("dy_bf16", [False, True], ids=["dy_fp32", "dy_bf16"])
@pytest.mark.parametrize("name", [s.name for s in SHAPES])
def test_bf16_storage(name, dy_bf16):
    """bf16 x / cores / bias / dx with fp32 dy (what the recurrent backward hands over) and with bf16 dy (a stand-alone module).
    Request sets with d_packed only: the proof that the route ran needs an fp32 buffer — two kernels' dx, rounded to bf16, agree
    in every bit more often than not."""
    shp = BY_NAME[name]
    for n in ([5] if shp.big else threshold_counts(shp)):
        _case(shp, n, REQUESTS[:2], storage="bf16", dy_bf16=dy_bf16)


def test_route_table_is_covered():
    """The table sends the cases above to every route at least once, every non-empty request set reaches a fast-table shape,
    a non-table shape and the cfg5 matrix on each side of the row threshold, and each intended route of the issue's table is
    the one expected_route names."""
    seen = collections.Counter()
    for s in SHAPES:
        for n in row_counts(s):
            for req in (REQUESTS if n in threshold_counts(s) else REQUESTS[:2]):
                seen[expected_route(s, n, req).name] += 1
    assert set(seen) == {"in1", "fused_core_dense", "wgrad_f10", "bwd_fast", "bwd_big", "gen_in1", "gdf", "gd", "chain"}, seen
    full, dw, dxo, dbo, dxdw, dxdb, dwdb = REQUESTS
    E = lambda name, n, req, **kw: expected_route(BY_NAME[name], n, req, **kw).name
    assert E("ShpH256R8L", 1023, full) == "wgrad_f10" and E("ShpH256R8L", 1024, full) == "fused_core_dense"
    assert E("ShpH256R8L", 1024, dxdb) == "bwd_fast" and E("ShpH256R8L", 1024, dbo) == "bwd_fast"
    assert E("ShpI40R16L", 159, dw) == "wgrad_f10" and E("ShpI40R16L", 160, dw) == "fused_core_dense"
    assert E("ShpI40R16L", 160, full) == "bwd_fast" and E("ShpI40R16L", 159, dxdw) == "bwd_fast"
    assert E("ShpI1R8L", 7, dw) == "in1" and E("ShpI1R8L", 7, dwdb) == "in1" and E("ShpI1R8L", 7, full) == "bwd_fast"
    assert E("ShpH256R16G", 1023, full) == "bwd_fast" and E("ShpH256R16G", 1024, full) == "gdf"
    assert E("ShpH128R4L", 511, dw) == "bwd_fast" and E("ShpH128R4L", 512, dw) == "gdf"
    assert E("ShpHd256R16", 1024, full) == "gdf"
    assert E("cfg5", 70, full) == "bwd_big" and E("cfg5", 70, dxo) == "bwd_big" and E("cfg5", 5, dxdb) == "chain" and E("cfg5", 5, dbo) == "chain"
    assert E("gen128x64", 511, full) == "chain" and E("gen128x64", 512, full) == "gd" and E("gen128x64", 512, full, exact=True) == "chain"
    assert E("gen32x24d4", 128, dw) == "gd" and E("gen32x24d4", 128, full) == "chain"
    assert E("gen12x20d1", 48, dw) == "gd" and E("gen12x20d1", 47, dw) == "chain"
    assert all(E("gen28x30", n, r) == "chain" for n in (1, 111, 112, 115) for r in REQUESTS)
    assert E("gen1x60", 3, dw) == "gen_in1" and E("gen1x60", 3, dxdw) == "chain"


# ---- operand ranges ---------------------------------------------------------------------------------------------------------------
RANGES = [dict(x_scale=1e-4), dict(x_scale=1e4), dict(dy_decades=True), dict(dy_zero_col=5), dict(zero_core=1)]


@pytest.mark.parametrize("knobs", RANGES, ids=["-".join("%s=%s" % kv for kv in d.items()) for d in RANGES])
@pytest.mark.parametrize("name,n", [("ShpH256R8L", 1024), ("gen128x64", 512)])
def test_operand_ranges(name, n, knobs):
    _case(BY_NAME[name], n, REQUESTS[:2], seed=3, **dict(knobs))


@pytest.mark.parametrize("loose", [1.0, 8.0], ids=["exact_bounds", "bounds_x8"])
def test_hinted_column_bounds(loose):
    """hints x_colmax / dy_colmax (UPPER BOUNDS of the column maxima, include/ttrnn.h): the dense weight gradient then runs on two
    fp16 pieces under per-column scales.  Exact and eight times too large: the same bound as the unhinted call."""
    shp = BY_NAME["ShpH256R8L"]
    lin = Lin(shp.in_modes, shp.out_modes, shp.rank, seed=41)
    x, dy = lin.rows(1024, 43)
    ref = lin.reference(x, dy)
    hints = {"x_colmax": (x.abs().max(0).values * loose).contiguous(), "dy_colmax": (dy.abs().max(0).values * loose).contiguous()}
    bad = []
    for req in REQUESTS[:2]:
        check_backward("%-11s n=1024 hinted x%g" % (shp.name, loose), lin, shp, x, dy, req, ref, bad, hints=hints)
    assert not bad, bad


def test_in1_with_the_row_sums_as_a_hint():
    """hints.xdy_sum with d_bias == NULL (in_size == 1, dx == NULL): the weight gradient from sum_n x[n] dy[n][:] alone."""
    shp = BY_NAME["ShpI1R8L"]
    lin = Lin(shp.in_modes, shp.out_modes, shp.rank, seed=47)
    bad = []
    for n in (1, 9, 70):
        x, dy = lin.rows(n, 53 + n)
        ref = lin.reference(x, dy)
        xdy = (x.double().t() @ dy.double()).float().view(-1).contiguous()
        check_backward("%-11s n=%-4d xdy_sum" % (shp.name, n), lin, shp, x, dy, ("dw",), ref, bad, hints={"xdy_sum": xdy})
        hinted = lin.backward(x, dy, ("dw",), hints={"xdy_sum": xdy})
        poisoned = lin.backward(x, torch.full_like(dy, float("nan")), ("dw",), hints={"xdy_sum": xdy})
        if not torch.equal(hinted["dpk"], poisoned["dpk"]):
            bad.append((n, "dy was read although the hint carries its row sums"))
    assert not bad, bad

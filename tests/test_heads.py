"""The callers either side of the path: TTLinear heads with their fused row-wise
epilogues, pinned by fixtures generated from the reference's own MNIST_Classifier / SpeakerEncoder classes
(tests/golden/gen_golden_heads.py), and the harness scripts under examples/."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tensorized-rnn_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "g9_head_*.npz")))


def _load(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    meta = json.loads(str(d["meta"]))
    sd = {}
    for k in d.files:
        if k.startswith("sd/"):
            key = k[3:]
            t = torch.from_numpy(d[k])
            st = tuple(int(v) for v in d["stride/" + key])
            if t.dim() > 0 and st != t.stride():
                buf = torch.empty_strided(t.shape, st, dtype=t.dtype)
                buf.copy_(t)
                t = buf
            sd[key] = t
    return d, meta, sd


def _oracle(meta, sd, x):
    """The reference's forward restated with the oracle's pieces (CPU, fp32)."""
    from oracle import ttrnn_oracle as O
    L = meta["num_layers"]
    rnn_sd = {k[4:]: v for k, v in sd.items() if k.startswith("rnn.")}
    layers, leaves = O.layers_from_state_dict(rnn_sd, L, requires_grad=True)
    gru = meta.get("gru", meta.get("use_gru", False))
    ncore = len([k for k in sd if k.startswith("linear.parameters.")])
    head = [sd["linear.parameters.%d" % k].clone().requires_grad_(True) for k in range(ncore)]
    hb = sd["linear.bias"].clone().requires_grad_(True)
    if gru:
        out, hT = O.gru_forward(layers, x)
    else:
        out, (hT, _) = O.lstm_forward(layers, x)
    if meta["model"] == "MNIST_Classifier":
        y = torch.log_softmax(O.ttlinear(head, hb, out[:, -1, :]), dim=1)
    else:
        raw = torch.relu(O.ttlinear(head, hb, hT))
        y = raw / torch.norm(raw, dim=1, keepdim=True)
    grads = {"rnn." + k: v for k, v in leaves.items()}
    for k in range(ncore):
        grads["linear.parameters.%d" % k] = head[k]
    grads["linear.bias"] = hb
    return y, grads


def _loss(meta, d, y):
    if meta["model"] == "MNIST_Classifier":
        return torch.nn.functional.nll_loss(y, torch.from_numpy(d["target"]).to(y.device))
    return (y * torch.from_numpy(d["w"]).to(y.device)).sum()


@pytest.mark.parametrize("name", CASES)
def test_oracle_restates_reference_models(name):
    d, meta, sd = _load(name)
    y, leaves = _oracle(meta, sd, torch.from_numpy(d["x"]))
    assert float((y.detach() - torch.from_numpy(d["out"])).abs().max()) <= 1e-6
    _loss(meta, d, y).backward()
    for key, leaf in leaves.items():
        ref = torch.from_numpy(d["grad/" + key])
        assert float((leaf.grad - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-6), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_product_models_match_reference_fixtures(name):
    """examples/models.py (drop-in packages + the fused head call) loads the reference's state_dict strictly and reproduces
    its outputs (1e-5 abs) and every gradient (1e-4 of the tensor max) on the device."""
    import contextlib
    import io
    import models
    d, meta, sd = _load(name)
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(io.StringIO()):
        if meta["model"] == "MNIST_Classifier":
            m = models.MNISTClassifier(meta["input_size"], meta["output_size"], meta["hidden_size"], meta["num_layers"], dev,
                                       gru=meta["gru"], n_cores=meta["n_cores"], tt_rank=meta["tt_rank"]).to(dev)
        else:
            m = models.SpeakerEncoder(meta["mel_n_channels"], meta["hidden_size"], meta["num_layers"], meta["embedding_size"], dev,
                                      n_cores=meta["n_cores"], rank=meta["rank"], use_gru=meta["use_gru"]).to(dev)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    y = m(torch.from_numpy(d["x"]).to(dev))
    assert float((y.detach().cpu() - torch.from_numpy(d["out"])).abs().max()) <= 1e-5
    loss = _loss(meta, d, y)
    assert abs(loss.item() - float(d["loss"])) <= 1e-4 * max(1.0, abs(float(d["loss"])))
    loss.backward()
    for key, p in m.named_parameters():
        if "grad/" + key not in d.files:
            continue
        ref = torch.from_numpy(d["grad/" + key])
        assert float((p.grad.cpu() - ref).abs().max()) <= 1e-4 * max(float(ref.abs().max()), 1e-6), key


@pytest.mark.gpu
@pytest.mark.parametrize("epilogue,out_f", [("log_softmax", 10), ("relu_l2norm", 256), ("log_softmax", 300)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_head_equals_unfused_ops(epilogue, out_f, dtype):
    """ttrnn_head_forward / _backward against TTLinear followed by the ATen ops the reference's callers use."""
    import contextlib
    import io
    from t3nsor.layers import TTLinear
    dev = torch.device("cuda:0")
    torch.manual_seed(9)
    with contextlib.redirect_stdout(io.StringIO()):
        lin = TTLinear(in_features=256, out_features=out_f, bias=True, auto_shapes=True, d=3, tt_rank=8).to(dev).to(dtype)
    x = torch.randn(37, 256, device=dev).to(dtype)
    w = torch.randn(37, out_f, device=dev)

    def run(fused):
        lin.zero_grad()
        xg = x.clone().requires_grad_(True)
        if fused:
            y = lin.forward_head(xg, epilogue)
        elif epilogue == "log_softmax":
            y = torch.log_softmax(lin(xg), dim=1)
        else:
            raw = torch.relu(lin(xg))
            y = raw / torch.norm(raw, dim=1, keepdim=True)
        (y.float() * w).sum().backward()
        return y.detach().float(), xg.grad.float(), [p.grad.float().clone() for p in lin.parameters()]

    a, b = run(True), run(False)
    tol = 2e-6 if dtype == torch.float32 else 3e-2
    assert float((a[0] - b[0]).abs().max()) <= tol * max(1.0, float(b[0].abs().max()))
    assert float((a[1] - b[1]).abs().max()) <= (1e-4 if dtype == torch.float32 else 6e-2) * max(float(b[1].abs().max()), 1e-6)
    for ga, gb in zip(a[2], b[2]):
        assert float((ga - gb).abs().max()) <= (1e-4 if dtype == torch.float32 else 6e-2) * max(float(gb.abs().max()), 1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("script,args", [
    # H2: pmnist_test.py flags of BASELINE configs[0] (+ the GRU / extra-core / naive variants), a few steps
    ("pmnist_synthetic.py", ["--tt", "--ncores", "2", "--ttrank", "4", "--hidden_size", "128", "--batch_size", "32", "--permute",
                             "--steps", "3"]),
    ("pmnist_synthetic.py", ["--tt", "--gru", "--ncores", "3", "--ttrank", "2", "--hidden_size", "64", "--batch_size", "8",
                             "--extra_core", "first", "--clip", "1.0", "--steps", "2"]),
    ("pmnist_synthetic.py", ["--tt", "--naive_tt", "--ncores", "2", "--ttrank", "3", "--hidden_size", "64", "--batch_size", "4",
                             "--steps", "1"]),
    # H1: benchmarking.py (eval and train modes: zero_grad + forward + nll_loss + backward + Adam)
    ("benchmarking.py", ["--tt", "--batch_size", "32", "--in_size", "64", "--hidden_size", "128", "--seq_len", "20", "-n", "3"]),
    ("benchmarking.py", ["--tt", "--train", "--batch_size", "32", "--in_size", "64", "--hidden_size", "128", "--seq_len", "20",
                         "-n", "3"]),
    # H3: the speaker-verification step (encoder, GE2E loss, gradient scaling / clipping, Adam)
    ("speaker_step.py", ["--speakers", "4", "--utterances", "5", "--frames", "20", "--n_layers", "2", "-n", "2"]),
])
def test_harness_scripts_run(script, args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script)] + args, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=600, cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-3000:]
    assert "nan" not in res.stdout.lower(), res.stdout[-2000:]


# ---- the fused heads against a float64 evaluation (tests/ttlinear_abi.py has the rule) ------------------------------------------------
# width -> (in modes, out modes, rank).  out <= 32: chain + epilogue in ONE launch of the any-shape kernel (one thread per row;
# option head_split_epilogue = 1: the separate wave-per-row launch); 36 is the first width on the wave-per-row kernel, 256 is the
# speaker head's own matrix (a shape-specialised forward), 300 needs more than four passes per lane.
HEAD_SHAPES = {2: ([4, 8, 8], [1, 1, 2], 8), 10: ([4, 8, 8], [1, 2, 5], 8), 32: ([4, 8, 8], [2, 4, 4], 8),
               36: ([4, 8, 8], [3, 3, 4], 8), 64: ([4, 8, 8], [4, 4, 4], 8), 256: ([4, 8, 8], [4, 8, 8], 16),
               300: ([4, 8, 8], [5, 6, 10], 8)}
EPI_CODE = {"log_softmax": 1, "relu_l2norm": 2}


def _epilogue(z, epi):
    if epi == "log_softmax":
        return torch.log_softmax(z, dim=1)
    raw = torch.relu(z)
    return raw / torch.norm(raw, dim=1, keepdim=True)


def _head_reference(lin, x, w, epi):
    """float64: y, aux and every gradient of sum(y * w)."""
    from oracle import ttrnn_oracle as O
    cores = [c.clone().requires_grad_(True) for c in lin.cores64]
    b = None if lin.bias64 is None else lin.bias64.clone().requires_grad_(True)
    xr = x.cpu().double().requires_grad_(True)
    z = O.ttlinear(cores, b, xr)
    y = _epilogue(z, epi)
    aux = torch.logsumexp(z, dim=1) if epi == "log_softmax" else torch.relu(z).norm(dim=1)
    (y * w.cpu().double()).sum().backward()
    ref = {"y": y.detach(), "aux": aux.detach(), "z": z.detach(), "dx": xr.grad}
    if b is not None:
        ref["db"] = b.grad
    for k, c in enumerate(cores):
        ref["dcore%d" % k] = c.grad
    return ref


def _head_product(lin, x, w, epi, fused):
    """forward + backward through the autograd functions of ttrnn_hip.functional; aux through the C ABI (fused) or the
    float32 ATen ops on the unfused TTLinear output."""
    from ttrnn_hip import functional as F
    xg = x.clone().requires_grad_(True)
    cores = [c.clone().requires_grad_(True) for c in lin.cores]
    b = None if lin.bias is None else lin.bias.clone().requires_grad_(True)
    if fused:
        y = F.tt_linear_head(xg, cores, b, lin.spec, epi)
        aux = lin.head_forward(x, EPI_CODE[epi])[1]
    else:
        z = F.tt_linear(xg, cores, b, lin.spec)
        y = _epilogue(z, epi)
        zf = z.detach().float()
        aux = torch.logsumexp(zf, dim=1) if epi == "log_softmax" else torch.relu(zf).norm(dim=1)
    (y.float() * w).sum().backward()
    torch.cuda.synchronize()
    res = {"y": y.detach().cpu().double(), "aux": aux.cpu().double(), "dx": xg.grad.cpu().double()}
    if b is not None:
        res["db"] = b.grad.cpu().double()
    for k, c in enumerate(cores):
        res["dcore%d" % k] = c.grad.cpu().double()
    return res


def _head_check(tag, lin, x, w, epi, bad, ref=None, keep=None):
    """The fused head (both forward paths where the width has two) against the unfused path, per tensor.  keep: the rows whose
    values are compared (the gradients then belong to a reference over those rows alone)."""
    import ttrnn_hip
    from ttlinear_abi import FLOOR, judge
    if ref is None:
        ref = _head_reference(lin, x, w, epi)
    ref = {k: v for k, v in ref.items() if k != "z"}
    sel = (lambda d: d) if keep is None else (lambda d: dict(d, y=d["y"][keep], aux=d["aux"][keep], dx=d["dx"][keep]))
    yard = _head_product(lin, x, w, epi, False) if keep is None else _head_product(lin, x[keep].contiguous(), w[keep].contiguous(), epi, False)
    got = {"one launch" if lin.out_f <= 32 else "two launches": sel(_head_product(lin, x, w, epi, True))}
    if lin.out_f <= 32:
        with ttrnn_hip.option("head_split_epilogue", 1):
            got["two launches"] = sel(_head_product(lin, x, w, epi, True))
    for path, res in got.items():
        judge("%s %s" % (tag, path), res, yard, ref, lin.storage, bad, names=("fused", "unfused"), design2=1e-4)
    if len(got) == 2:
        a, b = got["one launch"], got["two launches"]
        for k in sorted(ref):
            scale = float(ref[k].abs().max())
            bound = max(4.0 * float((yard[k] - ref[k]).abs().max()), FLOOR[lin.storage] * scale)
            e = float((a[k] - b[k]).abs().max())
            if not e <= bound:
                bad.append((tag, k, "the two forward paths differ by", e, bound))
    return got


def _ordinary_rows(lin, n, g):
    """n random rows whose pre-activation has two entries well above zero, in every storage type.  A ReLU row without one is
    0 / 0, and one with a single positive entry is a unit vector whose gradients are exactly zero — a narrow head has both
    by chance, and a batch of them leaves a reference of float64 rounding noise around 0 (test_head_relu_l2norm_edge_rows has
    the two cases on purpose)."""
    from oracle import ttrnn_oracle as O
    cand = torch.randn(16 * n + 64, lin.in_f, generator=g).to(lin.dt)
    z = O.ttlinear(lin.cores64, lin.bias64, cand.double())
    ok = ((z > 0.1).sum(dim=1) >= 2).nonzero().view(-1)[:n]
    assert len(ok) == n
    return cand[ok].contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("epi", ["log_softmax", "relu_l2norm"])
@pytest.mark.parametrize("width", sorted(HEAD_SHAPES))
def test_fused_head_against_float64(width, epi, storage):
    """Rows 1 ... 5 end inside the last workgroup of either epilogue kernel (four rows each); with and without a bias."""
    from ttlinear_abi import Lin, dev
    jm, im, r = HEAD_SHAPES[width]
    bad = []
    for bias in (True, False):
        lin = Lin(jm, im, r, storage, seed=300 + width, bias=bias)
        for n in (1, 3, 4, 5, 37):
            g = torch.Generator().manual_seed(17 * n + width)
            x = _ordinary_rows(lin, n, g).to(dev())
            w = torch.randn(n, width, generator=g).to(lin.dt).float().to(dev())
            _head_check("head %3d %-11s %s %-6s n=%-2d" % (width, epi, storage, "bias" if bias else "nobias", n), lin, x, w, epi, bad)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("width", [10, 300])
def test_head_inference_without_aux(width):
    """aux == NULL (include/ttrnn.h: inference with LOG_SOFTMAX): the same y, on both forward paths."""
    import ttrnn_hip
    from ttlinear_abi import Lin, dev
    jm, im, r = HEAD_SHAPES[width]
    lin = Lin(jm, im, r, seed=5)
    for n in (1, 5, 37):
        x = torch.randn(n, lin.in_f, generator=torch.Generator().manual_seed(n)).to(dev())
        for split in (0, 1):
            with ttrnn_hip.option("head_split_epilogue", split):
                y, aux = lin.head_forward(x, 1)
                y0, none = lin.head_forward(x, 1, want_aux=False, nan_ws=False)
            assert none is None and torch.isfinite(aux).all() and torch.equal(y, y0)


def _edge_lin(width, bias_values, seed=0):
    from ttlinear_abi import Lin
    jm, im, r = HEAD_SHAPES[width]
    return Lin(jm, im, r, seed=900 + seed + width, bias_values=bias_values)


def _edge_rows(lin, n=6, seed=0, scale=0.5):
    """row 0 is all zero, so that its pre-activation is the bias itself; the others are ordinary"""
    from ttlinear_abi import dev
    g = torch.Generator().manual_seed(1234 + seed)
    x = torch.randn(n, lin.in_f, generator=g) * scale
    x[0] = 0.0
    return x.to(dev()), torch.randn(n, lin.out_f, generator=g).to(dev())


@pytest.mark.gpu
@pytest.mark.parametrize("width", [10, 32, 300])
def test_head_log_softmax_edge_rows(width):
    bad = []
    g = torch.Generator().manual_seed(width)
    # logits spread over +-80 around +300: exp() of them overflows fp32 without the max-subtraction
    b = 300.0 + 80.0 * torch.linspace(-1, 1, width)[torch.randperm(width, generator=g)]
    lin = _edge_lin(width, b)
    x, w = _edge_rows(lin)
    ref = _head_reference(lin, x, w, "log_softmax")
    z0 = ref["z"][0]
    assert float(z0.max() - z0.min()) == 160.0 and float(z0.min()) == 220.0 and float(z0.max()) > 88.8
    got = _head_check("head %3d log_softmax spread" % width, lin, x, w, "log_softmax", bad, ref=ref)
    assert all(torch.isfinite(r["y"]).all() and torch.isfinite(r["aux"]).all() for r in got.values())
    # a row whose maximum occurs twice
    b = torch.randn(width, generator=g)
    b[1] = b[width - 1] = float(b.max()) + 1.0
    lin = _edge_lin(width, b, seed=1)
    x, w = _edge_rows(lin, seed=1)
    ref = _head_reference(lin, x, w, "log_softmax")
    assert int((ref["z"][0] == ref["z"][0].max()).sum()) == 2
    _head_check("head %3d log_softmax double max" % width, lin, x, w, "log_softmax", bad, ref=ref)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("width", [10, 32, 300])
def test_head_relu_l2norm_edge_rows(width):
    import ttrnn_hip
    bad = []
    g = torch.Generator().manual_seed(width + 1)
    # exactly one positive entry: y is that unit vector, and the pre-activation gradient of the row is exactly zero
    # (dz_k = (dy_k - y_k * (y . dy)) / norm with y_k = 1; dz = 0 wherever y = 0) — so is its row of dx
    b = -torch.rand(width, generator=g) - 0.1
    b[3 % width] = 0.7
    lin = _edge_lin(width, b)
    x, w = _edge_rows(lin)
    ref = _head_reference(lin, x, w, "relu_l2norm")
    assert int((ref["z"][0] > 0).sum()) == 1 and abs(float(ref["y"][0, 3 % width]) - 1.0) < 1e-15 and float(ref["dx"][0].abs().max()) < 1e-12
    got = _head_check("head %3d relu_l2norm one positive" % width, lin, x, w, "relu_l2norm", bad, ref=ref)
    for path, r in got.items():
        assert float(r["y"][0, 3 % width]) == 1.0 and int((r["y"][0] != 0).sum()) == 1, path
        assert not r["dx"][0].any(), (path, "dx of the unit-vector row", float(r["dx"][0].abs().max()))
    # norms of 1e-15 and 1e15 (row 0; with the large bias every row)
    for s in (1e-15, 1e15):
        b = torch.rand(width, generator=g) * s
        b[::2] = -b[::2]
        lin = _edge_lin(width, b, seed=2)
        x, w = _edge_rows(lin, seed=2)
        ref = _head_reference(lin, x, w, "relu_l2norm")
        assert 0.1 * s <= float(ref["aux"][0]) <= 100.0 * s
        got = _head_check("head %3d relu_l2norm norm %g" % (width, s), lin, x, w, "relu_l2norm", bad, ref=ref)
        assert all(torch.isfinite(r["y"]).all() and torch.isfinite(r["dx"]).all() for r in got.values())
    # no positive entry in row 0: y = 0 / 0 = NaN there, exactly where float32 torch.norm + divide gives NaN; the kernel's
    # `y > 0 ? ... : 0` rule (csrc/ttrnn_head.hip: k_head_epilogue_bwd) then gives dz = 0 for the row, so it adds nothing
    # to any gradient: the other rows and the parameter gradients are those of the batch without it
    b = -torch.rand(width, generator=g) - 0.1
    lin = _edge_lin(width, b, seed=3)
    x, w = _edge_rows(lin, seed=3, scale=4.0)
    full = _head_reference(lin, x, w, "relu_l2norm")
    assert int((full["z"][0] > 0).sum()) == 0 and all(int((full["z"][i] > 0).sum()) > 0 for i in range(1, x.shape[0]))
    keep = slice(1, None)
    ref = _head_reference(lin, x[keep], w[keep], "relu_l2norm")
    from ttrnn_hip import functional as F
    with torch.no_grad():
        y_aten = _epilogue(F.tt_linear(x, lin.cores, lin.bias, lin.spec), "relu_l2norm")
    assert torch.isnan(y_aten[0]).all() and not torch.isnan(y_aten[1:]).any()
    for split in ((0, 1) if width <= 32 else (0,)):
        with ttrnn_hip.option("head_split_epilogue", split):
            r = _head_product(lin, x, w, "relu_l2norm", True)
        assert torch.equal(torch.isnan(r["y"]), torch.isnan(y_aten).cpu()), split
        assert float(r["aux"][0]) == 0.0 and not r["dx"][0].any(), split
    _head_check("head %3d relu_l2norm no positive" % width, lin, x, w, "relu_l2norm", bad, ref=ref, keep=keep)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["forward", "log_softmax", "relu_l2norm"])
def test_ttlinear_module_autograd_subsets(path):
    """TTLinear.forward / .forward_head under every requires_grad subset of (x, cores, bias): a frozen tensor ends with
    grad None (its gradient is a NULL output of the library call), the others match the float64 reference."""
    import contextlib
    import io
    import itertools
    import ttrnn_hip
    from oracle import ttrnn_oracle as O
    from t3nsor.layers import TTLinear
    from ttlinear_abi import judge
    dev = torch.device("cuda:0")
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        lin = TTLinear(in_features=256, out_features=10, bias=True, auto_shapes=True, d=3, tt_rank=8).to(dev)
    cores = list(lin.weight_t.tt_cores)
    rc = [c.detach().cpu().double().requires_grad_(True) for c in cores]
    rb = lin.bias.detach().cpu().double().requires_grad_(True)
    cand = torch.randn(120, 256)
    with torch.no_grad():      # (rows with an entry well above zero: a ReLU row without one is 0 / 0)
        x = cand[(O.ttlinear(rc, rb, cand.double()).max(dim=1).values > 0.1).nonzero().view(-1)[:37]].to(dev)
    assert x.shape[0] == 37
    w = torch.randn(37, 10, device=dev)
    rx = x.cpu().double().requires_grad_(True)
    z = O.ttlinear(rc, rb, rx)
    ry = z if path == "forward" else _epilogue(z, path)
    (ry * w.cpu().double()).sum().backward()
    ref = {"y": ry.detach(), "dx": rx.grad, "db": rb.grad}
    ref.update(("dcore%d" % k, c.grad) for k, c in enumerate(rc))

    def run(fused):
        lin.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(need_x)
        if path == "forward":
            y = lin(xg)
        elif fused:
            y = lin.forward_head(xg, path)
        else:
            y = _epilogue(lin(xg), path)
        (y * w).sum().backward()
        res = {"y": y.detach().cpu().double()}
        for name, t, need in [("dx", xg, need_x), ("db", lin.bias, need_b)] + [("dcore%d" % k, c, need_w) for k, c in enumerate(cores)]:
            if need:
                assert t.grad is not None and t.grad.shape == t.shape, name
                res[name] = t.grad.cpu().double()
            else:
                assert t.grad is None, "%s is frozen but has a gradient" % name
        return res

    bad = []
    try:
        for need_x, need_w, need_b in itertools.product((False, True), repeat=3):
            if not (need_x or need_w or need_b):
                continue
            for c in cores:
                c.requires_grad_(need_w)
            lin.bias.requires_grad_(need_b)
            got = run(True)
            if path == "forward":      # the yardstick: the any-shape route
                with ttrnn_hip.option("force_generic", 1):
                    yard = run(True)
            else:                      # the unfused path
                yard = run(False)
            judge("TTLinear %-11s x=%d cores=%d bias=%d" % (path, need_x, need_w, need_b), got, yard, ref, "fp32", bad,
                  names=("module", "yardstick"), design2=1e-4)
    finally:
        for p in lin.parameters():
            p.requires_grad_(True)
    assert not bad, bad

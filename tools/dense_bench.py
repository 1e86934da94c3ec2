#!/usr/bin/env python3
"""Times the uncompressed (nn.Linear) baselines of BASELINE.md on one GPU: eval forward and training step of
  pmnist      dense LSTM H = 256, in = 1, B = 64, T = 784           (291 840-parameter baseline)
  spk_lstm    dense LSTM H = 768, in = 40, B = 512, T = 160          (2 682 112-parameter baseline)
  spk_gru     dense GRU of the same shape
  bench       examples/benchmarking.py's defaults with --dense (in = 256, H = 512, B = 512, T = 160, classifier head)
and, with --tt, the tensor-train layer of the same (in, H, B, T) beside them (n_cores = 3, rank = 8; spk: the reference's
encoder layer, n_cores = 2, rank = 2), so that the dense-vs-TT ratio is a measured one.

One process times one library under one setting: per configuration `--blocks` blocks of `--iters` steps, each block timed as a
whole between two device synchronisations; printed are the median of the blocks' per-step times and their spread (min .. max).

    python tools/dense_bench.py                          the in-tree build, default routes
    python tools/dense_bench.py --force_generic          ... on the any-shape kernels (the A/B switch)
    python tools/dense_bench.py --lib other/libttrnn.so  another build of the library (e.g. the parent commit's)
    python tools/dense_bench.py --alternate other/libttrnn.so --rounds 3
        one session: other build / this build / this build with force_generic, in turn, `--rounds` times — the per-configuration
        medians of every visit are printed, so drift of the machine between visits shows
"""
import argparse
import contextlib
import io
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    # name: (kind, in, H, B, T, tt kwargs)
    "pmnist": ("lstm", 1, 256, 64, 784, dict(n_cores=3, tt_rank=8)),
    "spk_lstm": ("lstm", 40, 768, 512, 160, dict(n_cores=2, tt_rank=2)),
    "spk_gru": ("gru", 40, 768, 512, 160, dict(n_cores=2, tt_rank=2)),
    "bench": ("lstm", 256, 512, 512, 160, dict(n_cores=3, tt_rank=8)),
}


def build(name, tt, dev):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from models import MNISTClassifier
    from tensorized_rnn.gru import GRU, TTGRU
    from tensorized_rnn.lstm import LSTM
    from tensorized_rnn.tt_lstm import TTLSTM
    kind, inp, H, B, T, ttkw = CONFIGS[name]
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        if name == "bench":
            model = MNISTClassifier(inp, 256, H, 1, dev, gru=False, tt=tt, **ttkw).to(dev)
            rnn = model.rnn
        elif tt:
            model = rnn = (TTLSTM if kind == "lstm" else TTGRU)(inp, H, 1, dev, **ttkw)
        else:
            model = rnn = (LSTM if kind == "lstm" else GRU)(inp, H, 1, dev)
    x = torch.rand(B, T, inp, device=dev)
    target = torch.randint(0, 256, (B,), device=dev)
    return model, rnn, x, target


def time_config(name, tt, train, blocks, iters):
    import torch
    import torch.nn.functional as F
    from ttrnn_hip import functional as TF
    dev = torch.device("cuda:0")
    model, rnn, x, target = build(name, tt, dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    B, T = x.shape[0], x.shape[1]
    spec = rnn.cell0._layer_spec()
    route = "%s/%s" % (TF.rnn_route(spec, B, T), TF.rnn_backward_route(spec, B, T))

    def step():
        if not train:
            with torch.no_grad():
                return model(x) if name == "bench" else model(x, need_outputs=False)
        opt.zero_grad(set_to_none=True)
        if name == "bench":
            loss = F.nll_loss(model(x), target)
        else:
            res = model(x)
            h = res[1] if isinstance(res[1], torch.Tensor) else res[1][0]
            loss = (res[0] * res[0]).mean() + h.sum()
        loss.backward()
        opt.step()
        return loss

    step()
    torch.cuda.synchronize()
    per_step = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        per_step.append((time.perf_counter() - t0) / iters * 1e3)
    return route, per_step


def run_here(args):
    if args.force_generic:
        import ttrnn_hip
        ttrnn_hip.set_option("force_generic", 1)
    label = args.label or ("force_generic" if args.force_generic else "default")
    for name in args.configs:
        for tt in ([False, True] if args.tt else [False]):
            if tt and args.force_generic:
                continue
            for train in (False, True):
                iters = args.iters
                if args.force_generic or args.slow:      # the any-shape kernels take up to a second per step on these shapes
                    iters = 1
                route, ms = time_config(name, tt, train, args.blocks, iters)
                print("%-14s %-9s %-5s %-5s route %-24s median %9.3f ms  spread %9.3f .. %9.3f  (%d blocks x %d)" % (
                    label, name, "tt" if tt else "dense", "train" if train else "eval", route, statistics.median(ms), min(ms),
                    max(ms), args.blocks, iters), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tt", action="store_true", help="also time the TT layer of the same (in, H, B, T)")
    ap.add_argument("--force_generic", action="store_true")
    ap.add_argument("--slow", action="store_true", help="one step per block (a build whose dense layers run on the any-shape kernels)")
    ap.add_argument("--lib", help="path of another libttrnn.so to time instead of the in-tree build")
    ap.add_argument("--label")
    ap.add_argument("--alternate", metavar="LIB", help="alternate LIB / this build / this build with force_generic in one session")
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.alternate:
        common = [sys.executable, os.path.abspath(__file__), "--configs"] + args.configs + ["--blocks", str(args.blocks), "--iters",
                                                                                              str(args.iters)]
        for r in range(args.rounds):
            visits = [(["--lib", args.alternate, "--slow", "--label", "other[%d]" % r]),
                      (["--label", "this[%d]" % r] + (["--tt"] if args.tt and r == 0 else [])),
                      (["--force_generic", "--label", "this_generic[%d]" % r])]
            for extra in visits:
                rc = subprocess.call(common + extra)      # a fresh process per visit: one library per process
                if rc != 0:
                    sys.exit(rc)
        return
    if args.lib:
        os.environ["TTRNN_LIB_PATH"] = os.path.abspath(args.lib)
    sys.path.insert(0, os.path.join(ROOT, "tensorized-rnn_amd"))
    run_here(args)


if __name__ == "__main__":
    main()

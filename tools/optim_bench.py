#!/usr/bin/env python3
"""The tail of a training step after loss.backward() — gradient scaling, norm clipping, Adam — as torch runs it against
ttrnn_hip.ClipAdam (one library call).

  optim_bench.py call [--calls 200 --blocks 5]  on synthetic gradients, per eager call: do_gradient_ops + torch.optim.Adam as it
                                                is, with fused=True, with capturable=True, fused=True, and ClipAdam on route
                                                "auto", "one" and "grid" — all variants alternate in blocks of --calls calls in
                                                one process; median of the blocks and spread (max - min), as device-event span
                                                and as host wall time.  Tables: the reference encoder's one-layer model, the
                                                3-layer default's, the dense H = 768 baseline's (2.68 M elements).  Then route
                                                "one" against "grid" by chunk count: where route "auto" should switch
  optim_bench.py steps [-n 20]                 examples/speaker_step.py at the H = 768 one-layer shape and at its defaults,
                                                each with and without --fused_optim, one child process per run under its own
                                                time limit; stops at the first run that fails
  optim_bench.py count TRACE.csv                launches after the last backward kernel of each step in a kernel trace
                                                (rocprofv3 --kernel-trace --stats --output-format csv -- python
                                                examples/speaker_step.py ... [--fused_optim])
Each sub-command prints plain text; redirect it into profiles/."""
import argparse
import contextlib
import copy
import csv
import io
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorized-rnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def _blocks(fns, calls, blocks):
    """The callables of `fns` (name -> f) alternate in blocks of `calls` calls; per block the host wall time per call around a
    final synchronise, and the device-event span per call.  -> {name: (median wall us, spread, median device us, spread)}"""
    import torch
    sync = torch.cuda.synchronize
    for f in fns.values():
        for _ in range(5):
            f()
    sync()
    res = {name: ([], []) for name in fns}
    for _ in range(blocks):
        for name, f in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            t0 = time.perf_counter()
            start.record()
            for _ in range(calls):
                f()
            stop.record()
            sync()
            res[name][0].append(1e6 * (time.perf_counter() - t0) / calls)
            res[name][1].append(1e3 * start.elapsed_time(stop) / calls)
    return {name: (statistics.median(w), max(w) - min(w), statistics.median(g), max(g) - min(g)) for name, (w, g) in res.items()}


def _show(label, r):
    for name, (wall, wspread, gpu, gspread) in r.items():
        print("%-30s %-34s host wall %8.1f us/call (spread %5.1f)   device span %8.1f us/call (spread %5.1f)" % (
            label, name, wall, wspread, gpu, gspread), flush=True)


def _synthetic_grads(model, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.empty_like(p).copy_(0.05 * torch.randn(p.shape, generator=gen))      # empty_like keeps p's strides


def cmd_call(args):
    import torch
    import ttrnn_hip
    from models import SpeakerEncoder
    dev = torch.device("cuda", 0)
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| calls per block", args.calls, "| blocks", args.blocks)
    print("every time is per eager call on static synthetic gradients: host wall = perf_counter around a block ending in a "
          "synchronise; device span = events around it")
    tables = (("encoder 1 layer H=768 r2", dict(hidden_size=768, num_layers=1, n_cores=2, rank=2)),
              ("3-layer default H=256 r16", dict(hidden_size=256, num_layers=3, n_cores=3, rank=16)),
              ("dense H=768 baseline", dict(hidden_size=768, num_layers=1, compression=None)))
    for label, kw in tables:
        torch.manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            base = SpeakerEncoder(40, embedding_size=256, device=dev, **kw).to(dev)
        ps = list(base.parameters())
        label = "%s: %d tensors, %d elements" % (label, len(ps), sum(p.numel() for p in ps))
        fns = {}

        def torch_variant(name, **adam_kw):
            m = copy.deepcopy(base)
            _synthetic_grads(m, 2)
            opt = torch.optim.Adam(m.parameters(), lr=1e-3, **adam_kw)

            def f():
                m.do_gradient_ops()
                opt.step()
            fns[name] = f

        def ours(name, route):
            m = copy.deepcopy(base)
            _synthetic_grads(m, 2)
            opt = ttrnn_hip.ClipAdam(m.parameters(), lr=1e-3, max_norm=3.0, route=route,
                                     grad_scales={m.similarity_weight: 0.01, m.similarity_bias: 0.01})
            fns[name] = opt.step

        torch_variant("do_gradient_ops + Adam")
        torch_variant("do_gradient_ops + Adam(fused)", fused=True)
        torch_variant("do_gradient_ops + Adam(capt,fused)", capturable=True, fused=True)
        for route in ("auto", "one", "grid"):
            ours("ClipAdam route=%s" % route, route)
        r = _blocks(fns, args.calls, args.blocks)
        _show(label, r)
        for col, what in ((0, "host wall"), (2, "device span")):
            best = min((v[col], v[col + 1], k) for k, v in r.items() if "ClipAdam" not in k)
            mine = r["ClipAdam route=auto"]
            faster = best[0] - mine[col] > max(best[1], mine[col + 1])
            print("%-30s %s: ClipAdam (auto) %.1f us against the fastest torch variant (%s) %.1f us: %s" % (
                label, what, mine[col], best[2], best[0],
                "faster by more than the blocks' spread" if faster else "NOT separated by the blocks' spread"), flush=True)
    print("\n-- route \"one\" against \"grid\" by chunk count (8 equal tensors; clipping on) --")
    for chunks in (8, 16, 32, 64, 96, 128, 192, 256, 512, 1024, 2624):
        fns = {}
        for route in ("one", "grid"):
            ps = [torch.nn.Parameter(torch.randn(chunks // 8 * 1024, device=dev)) for _ in range(8)]
            for p in ps:
                p.grad = 0.05 * torch.randn_like(p)
            fns["ClipAdam route=%s" % route] = ttrnn_hip.ClipAdam(ps, lr=1e-3, max_norm=3.0, route=route).step
        _show("%d chunks" % chunks, _blocks(fns, args.calls, args.blocks))
    return 0


def cmd_steps(args):
    step = os.path.join(ROOT, "examples", "speaker_step.py")
    shapes = (["--hidden_size", "768", "--n_layers", "1", "--ncores", "2", "--ttrank", "2"], [])
    for shape in shapes:
        for extra in ([], ["--fused_optim"]):
            cmd = [sys.executable, step, "-n", str(args.n)] + shape + extra
            print("$ python examples/speaker_step.py", " ".join(cmd[2:]), flush=True)
            try:
                res = subprocess.run(cmd, cwd=os.path.join(ROOT, "examples"), timeout=args.limit, stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT, universal_newlines=True)
            except subprocess.TimeoutExpired:
                print("time limit of %d s reached: stopping" % args.limit)
                return 124
            print(res.stdout.strip()[-600:], flush=True)
            if res.returncode != 0:
                print("exit status %d: stopping" % res.returncode)
                return res.returncode
    return 0


OPTIMIZER_MARKS = ("k_optim_", "adam", "Adam", "multi_tensor_apply")


def cmd_count(args):
    rows = list(csv.DictReader(open(args.trace)))
    key = next(k for k in ("Kernel_Name", "KernelName", "Name") if k in rows[0])
    t0 = next(k for k in ("Start_Timestamp", "BeginNs", "Start") if k in rows[0])
    rows.sort(key=lambda r: int(r[t0]))
    names = [r[key] for r in rows]

    def is_opt(n):
        return any(m in n for m in OPTIMIZER_MARKS)

    def is_lib(n):       # a kernel of the library's forward / backward: every one is named k_<something>
        return re.search(r"\bk_[a-z]", n) is not None and "k_optim_" not in n

    print("kernel launches in the trace:", len(names), "| optimizer kernels:", sum(is_opt(n) for n in names))
    # a step's tail: everything after the last forward / backward kernel of the library up to the last optimizer kernel that
    # precedes the next such kernel
    tails, last_lib, last_opt = [], None, None
    for i, n in enumerate(names + ["k_end"]):
        if is_lib(n):
            if last_opt is not None and last_lib is not None:
                tails.append(names[last_lib + 1:last_opt + 1])
            last_lib, last_opt = i, None
        elif is_opt(n):
            last_opt = i
    if not tails:
        print("no optimizer kernel after a library kernel in the trace")
        return 1
    print("steps found:", len(tails), "| launches after the last backward kernel, per step:", " ".join(str(len(t)) for t in tails))
    short = [n.replace("(anonymous namespace)::", "").split("(")[0][:110] for n in tails[-1]]
    for k in sorted(set(short)):
        print("   %5d  %s" % (short.count(k), k))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("call")
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--blocks", type=int, default=5)
    p = sub.add_parser("steps")
    p.add_argument("-n", type=int, default=20)
    p.add_argument("--limit", type=int, default=240, help="seconds per child process")
    p = sub.add_parser("count")
    p.add_argument("trace")
    args = ap.parse_args()
    return {"call": cmd_call, "steps": cmd_steps, "count": cmd_count}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())

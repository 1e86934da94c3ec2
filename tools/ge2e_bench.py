#!/usr/bin/env python3
"""Fused GE2E loss (ttrnn_hip.ge2e.ge2e_loss_fused: four launches) against the tensor-op loss (ge2e.ge2e_loss + autograd).

  ge2e_bench.py loss [--calls 200 --blocks 5]   loss forward + backward alone at (16,32,256), (64,10,256) and the (40,32,256)
                                                enrollment forward: both paths alternate in blocks inside one process; per
                                                block the device-event time and the host wall time (final synchronise) per call
  ge2e_bench.py steps [-n 20]                   examples/speaker_step.py at its defaults and at the H = 768 first-tier shape,
                                                each with and without --torch_loss, one child process per run under its own
                                                time limit; stops at the first run that fails
  ge2e_bench.py count TRACE.csv                 launches of a kernel trace (rocprofv3 --kernel-trace --stats --output-format
                                                csv -- python examples/speaker_step.py ...): the GE2E kernels' own launches and
                                                what lies between the head's forward kernel and the head's backward kernel
Each sub-command prints plain text; redirect it into profiles/."""
import argparse
import csv
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorized-rnn_amd"))


def _inputs(S, U, D, Ue, dev):
    import torch
    gen = torch.Generator().manual_seed(S * 100 + U)
    def draw(n):
        x = torch.randn(S, 1, D, generator=gen) + 0.9 * torch.randn(S, n, D, generator=gen)
        return torch.nn.functional.normalize(torch.relu(x), dim=2).to(dev)
    return draw(U), (draw(Ue) if Ue else None)


def cmd_loss(args):
    import torch
    from ttrnn_hip import ge2e
    dev = torch.device("cuda", 0)
    print("device:", torch.cuda.get_device_name(0), "| calls per block", args.calls, "| blocks", args.blocks)
    for S, U, D, Ue in ((16, 32, 256, 0), (64, 10, 256, 0), (40, 32, 256, 32)):
        E, A = _inputs(S, U, D, Ue, dev)
        w = torch.tensor([10.0], device=dev, requires_grad=True)
        b = torch.tensor([-5.0], device=dev, requires_grad=True)
        e = E.clone().requires_grad_(Ue == 0)

        def call(fn):
            if Ue:                      # validation: forward only, no gradients
                with torch.no_grad():
                    return fn(e, w, b, A, with_eer=False)[0]
            e.grad = w.grad = b.grad = None
            loss = fn(e, w, b, None, with_eer=False)[0]
            loss.backward()
            return loss

        paths = (("torch-op", ge2e.ge2e_loss), ("fused", ge2e.ge2e_loss_fused))
        for _, fn in paths:
            for _ in range(20):
                call(fn)
        torch.cuda.synchronize()
        res = {name: ([], []) for name, _ in paths}
        for _ in range(args.blocks):
            for name, fn in paths:
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                start.record()
                for _ in range(args.calls):
                    call(fn)
                stop.record()
                torch.cuda.synchronize()
                res[name][1].append(1e6 * (time.perf_counter() - t0) / args.calls)
                res[name][0].append(1e3 * start.elapsed_time(stop) / args.calls)
        what = "enrollment forward" if Ue else "forward + backward"
        for name, (gpu, wall) in res.items():
            print("(%d,%d,%d)%s %-8s %s: device span %7.1f us/call (blocks %s; spread %.1f)  host wall %7.1f us/call (spread %.1f)" % (
                S, U, D, " U_e=%d" % Ue if Ue else "", name, what, statistics.median(gpu), " ".join("%.1f" % v for v in gpu),
                max(gpu) - min(gpu), statistics.median(wall), max(wall) - min(wall)))
    return 0


def cmd_steps(args):
    step = os.path.join(ROOT, "examples", "speaker_step.py")
    shapes = ([], ["--hidden_size", "768", "--n_layers", "1", "--ncores", "2", "--ttrank", "2"])
    for shape in shapes:
        for extra in ([], ["--torch_loss"]):
            cmd = [sys.executable, step, "-n", str(args.n)] + shape + extra
            print("$", " ".join(cmd[1:]), flush=True)
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


def cmd_count(args):
    rows = list(csv.DictReader(open(args.trace)))
    key = next(k for k in ("Kernel_Name", "KernelName", "Name") if k in rows[0])
    t0 = next(k for k in ("Start_Timestamp", "BeginNs", "Start") if k in rows[0])
    rows.sort(key=lambda r: int(r[t0]))
    names = [r[key] for r in rows]
    ge2e_n = ["k_ge2e_" + n.split("k_ge2e_")[1].split("(")[0] for n in names if "k_ge2e_" in n]
    print("kernel launches in the trace:", len(names), "| GE2E kernels:", len(ge2e_n))
    for k in sorted(set(ge2e_n)):
        print("   %5d  %s" % (ge2e_n.count(k), k))
    # the step's tail: from a head forward kernel (epilogue relu_l2norm: the name carries `head`) to the next head backward kernel
    gaps, a = [], None
    for i, n in enumerate(names):
        if "k_head_epilogue_bwd" in n:
            if a is not None:
                gaps.append(names[a + 1:i])
            a = None
        elif "k_head_epilogue" in n:
            a = i
    if not gaps:
        print("no k_head_epilogue ... k_head_epilogue_bwd pair in the trace")
    for g in gaps[-3:]:
        print("launches between the head's forward and backward kernels: %d (GE2E kernels among them: %d)" % (
            len(g), sum("k_ge2e_" in n for n in g)))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("loss")
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--blocks", type=int, default=5)
    p = sub.add_parser("steps")
    p.add_argument("-n", type=int, default=20)
    p.add_argument("--limit", type=int, default=240, help="seconds per child process")
    p = sub.add_parser("count")
    p.add_argument("trace")
    args = ap.parse_args()
    return {"loss": cmd_loss, "steps": cmd_steps, "count": cmd_count}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())

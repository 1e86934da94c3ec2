#!/usr/bin/env python3
"""Fused GE2E loss (ttrnn_hip.ge2e.ge2e_loss_fused: four launches) against the tensor-op loss (ge2e.ge2e_loss + autograd).

  ge2e_bench.py loss [--calls 200 --blocks 5]   loss forward + backward alone at (16,32,256), (64,10,256) and the (40,32,256)
                                                enrollment forward: both paths alternate in blocks inside one process; per
                                                block the device-event time and the host wall time (final synchronise) per call
  ge2e_bench.py eer [--calls 200 --blocks 5]    equal error rate per eager call: ge2e.eer_fused (library's choice, one workgroup,
                                                a grid with the workgroup count swept) against the host route (sim.cpu() +
                                                ge2e.eer) at (16,32), (64,10), (40,32) with ttrnn_ge2e_forward with / without
                                                sim_out alongside, then route 1 against route 2 from 65 K to 8.4 M scores; exit
                                                status 1 unless route 0 beats the host route at the three reference shapes
  ge2e_bench.py steps [-n 20]                  examples/speaker_step.py at its defaults and at the H = 768 first-tier shape,
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


def _blocks(fns, calls, blocks, sync):
    """The callables of `fns` (name -> f) alternate in blocks of `calls` calls; per block the host wall time per call around a
    final synchronise, and the device-event span per call.  -> {name: (median wall us, spread, median device us, spread)}"""
    import torch
    for f in fns.values():
        for _ in range(3):
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
        print("%-22s %-24s host wall %9.1f us/call (spread %.1f)   device span %9.1f us/call (spread %.1f)" % (
            label, name, wall, wspread, gpu, gspread), flush=True)


def cmd_eer(args):
    """Equal error rate: the device routes (ge2e.eer_fused) against the host route (sim.cpu() + ge2e.eer), per eager call."""
    import torch
    from ttrnn_hip import ge2e
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    print("device:", torch.cuda.get_device_name(0), "| calls per block", args.calls, "| blocks", args.blocks)
    print("every time is per eager call: host wall = perf_counter around a block ending in a synchronise; device span = events around it")
    verdicts = []
    print("\n-- the reference's shapes: library's choice, both routes, the host route (its result is a host float: it synchronises) --")
    for S, U, Ue in ((16, 32, 0), (64, 10, 0), (40, 32, 32)):
        E, A = _inputs(S, U, 256, Ue, dev)
        w, b = torch.tensor([10.0], device=dev), torch.tensor([-5.0], device=dev)
        sim = ge2e.similarity_matrix_fused(E, w, b, A)
        host = ge2e.eer(sim.reshape(S * U, S).cpu().numpy(), S, U)
        got = float(ge2e.eer_fused(sim))
        fns = {"device route=0": lambda: ge2e.eer_fused(sim), "device route=1": lambda: ge2e.eer_fused(sim, route="one")}
        for g in (1, 2, 4, 8, 16, 64):
            fns["device route=2 wg=%d" % g] = (lambda g=g: ge2e.eer_fused(sim, route="grid", workgroups=g))
        fns["host sim.cpu()+eer"] = lambda: ge2e.eer(sim.reshape(S * U, S).cpu().numpy(), S, U)
        r = _blocks(fns, args.calls, args.blocks, sync)
        label = "(%d,%d)%s %d scores" % (S, U, " U_e=%d" % Ue if Ue else "", S * U * S)
        _show(label, r)
        ok = r["device route=0"][0] < r["host sim.cpu()+eer"][0]
        verdicts.append(ok)
        print("%-22s EER device %.12f host %.12f (difference %.2e);  route=0 faster than the host route: %s (%.1fx)" % (
            label, got, host, abs(got - host), "PASS" if ok else "FAIL", r["host sim.cpu()+eer"][0] / r["device route=0"][0]))
        fwd = {"ge2e forward, no sim_out": lambda: ge2e._fused_forward(E, w, b, A, want_sim=False),
               "ge2e forward + sim_out": lambda: ge2e._fused_forward(E, w, b, A, want_sim=True),
               "... + sim_out + EER": lambda: ge2e.eer_fused(ge2e._fused_forward(E, w, b, A, want_sim=True)[1])}
        _show(label, _blocks(fwd, args.calls, args.blocks, sync))
    print("\n-- where the routes cross: route 1 against route 2 by score count (random scores; the host route once per shape) --")
    gen = torch.Generator().manual_seed(5)
    for S, U in ((128, 4), (128, 16), (256, 8), (256, 16), (512, 8), (1024, 4), (2048, 2)):
        sim = torch.randn(S, U, S, generator=gen).to(dev)
        fns = {"device route=1": lambda: ge2e.eer_fused(sim, route="one")}
        for g in (4, 16, 64, 128, 256):
            fns["device route=2 wg=%d" % g] = (lambda g=g: ge2e.eer_fused(sim, route="grid", workgroups=g))
        fns["device route=2 wg=0"] = lambda: ge2e.eer_fused(sim, route="grid")
        fns["device route=0"] = lambda: ge2e.eer_fused(sim)
        label = "(%d,%d) %d scores" % (S, U, S * U * S)
        r = _blocks(fns, max(args.calls // 4, 5), args.blocks, sync)
        _show(label, r)
        best = min((v[0], k) for k, v in r.items() if "route=2" in k)
        print("%-22s route 1 %.1f us, best grid %s %.1f us" % (label, r["device route=1"][0], best[1], best[0]), flush=True)
        if S * U * S <= 1 << 21:
            t0 = time.perf_counter()
            host = ge2e.eer(sim.reshape(S * U, S).cpu().numpy(), S, U)
            print("%-22s host route, one call: %.1f ms; EER host %.12f device %.12f" % (
                label, 1e3 * (time.perf_counter() - t0), host, float(ge2e.eer_fused(sim))), flush=True)
    print("\nroute=0 faster than the host route at the three reference shapes:", "PASS" if all(verdicts) else "FAIL")
    return 0 if all(verdicts) else 1


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
    p = sub.add_parser("eer")
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--blocks", type=int, default=5)
    p = sub.add_parser("steps")
    p.add_argument("-n", type=int, default=20)
    p.add_argument("--limit", type=int, default=240, help="seconds per child process")
    p = sub.add_parser("count")
    p.add_argument("trace")
    args = ap.parse_args()
    return {"loss": cmd_loss, "eer": cmd_eer, "steps": cmd_steps, "count": cmd_count}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())

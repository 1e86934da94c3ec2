#!/usr/bin/env python3
"""One speaker-verification training step on synthetic data with the semantics of the reference's
experiments/speaker_verification/main.py:65-78,257-290 (cfg4): utterances [speakers*utterances, 160, 40] -> 3-layer
TT-LSTM -> TTLinear -> ReLU -> L2 norm -> GE2E loss on [speakers, utterances, 256] -> backward -> gradient scaling /
clipping -> Adam(1e-3).  Everything, the loss included, stays on the GPU (the reference moves the embeddings to the CPU
for its per-speaker loop).  Example:  python examples/speaker_step.py --speakers 16 --utterances 32 -n 10"""
import argparse
import contextlib
import io
import time

import torch

from models import SpeakerEncoder


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, default=16)
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--mels", type=int, default=40)
    ap.add_argument("--hidden_size", type=int, default=256)
    ap.add_argument("--n_layers", type=int, default=3)
    ap.add_argument("--emb_size", type=int, default=256)
    ap.add_argument("--ncores", type=int, default=3)
    ap.add_argument("--ttrank", type=int, default=16)
    ap.add_argument("--gru", action="store_true")
    ap.add_argument("--dense", action="store_true",
                    help="the uncompressed baseline (the reference's compression=None): dense LSTM / GRU stack + nn.Linear")
    ap.add_argument("-n", "--nruns", type=int, default=10)
    ap.add_argument("--torch_loss", action="store_true",
                    help="GE2E loss as torch tensor ops + autograd instead of the library's GE2E kernels (A/B)")
    ap.add_argument("--eer", action="store_true",
                    help="also time the step with the EER computed every step on the device (with_eer=\"device\": no host "
                         "round trip; the value is read once, after the loop), as the reference's step reports loss and EER")
    ap.add_argument("--fused_optim", action="store_true",
                    help="gradient scaling, norm clipping and the Adam step as one library call (ttrnn_hip.ClipAdam) instead of "
                         "do_gradient_ops() + torch.optim.Adam (A/B)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        model = SpeakerEncoder(args.mels, args.hidden_size, args.n_layers, args.emb_size, dev, n_cores=args.ncores,
                               rank=args.ttrank, use_gru=args.gru, compression=None if args.dense else 'tt').to(dev)
    if args.fused_optim:
        import ttrnn_hip
        opt = ttrnn_hip.ClipAdam(model.parameters(), lr=1e-3, max_norm=3.0,
                                 grad_scales={model.similarity_weight: 0.01, model.similarity_bias: 0.01})
    else:
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    S, U = args.speakers, args.utterances
    x = torch.rand(S * U, args.frames, args.mels, device=dev)

    def step(with_eer=False):
        opt.zero_grad(set_to_none=True)
        embeds = model(x).view(S, U, -1)
        loss, eer = model.loss(embeds, fused=False if args.torch_loss else None, with_eer=with_eer)
        loss.backward()
        if not args.fused_optim:
            model.do_gradient_ops()
        opt.step()
        return loss, eer

    def timed(with_eer):
        out = step(with_eer)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.nruns):
            t0 = time.perf_counter()
            out = step(with_eer)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return times, out

    times, (loss, _) = timed(False)
    if args.eer:
        times_eer, (loss_eer, eer_dev) = timed("device")
    with torch.no_grad():
        embeds = model(x).view(S, U, -1)
        _, eer = model.loss(embeds)
    ms = 1e3 * sum(times) / len(times)
    print("speaker-encoder train step (%s GE2E loss%s): %.2f ms (min %.2f) for %d utterances x %d frames; loss %.4f, EER %.3f" % (
        "torch-op" if args.torch_loss else "fused", ", fused optimizer" if args.fused_optim else "", ms, 1e3 * min(times), S * U,
        args.frames, float(loss), eer))
    if args.eer:
        ms_eer = 1e3 * sum(times_eer) / len(times_eer)
        print("... with the EER on the device every step: %.2f ms (min %.2f), %+.3f ms against the step without it; "
              "loss %.4f, EER of the last step %.3f" % (ms_eer, 1e3 * min(times_eer), ms_eer - ms, float(loss_eer), float(eer_dev)))
    if args.dense:
        from ttrnn_hip import functional as TF
        spec = model.rnn.cell0._layer_spec()
        print("recurrent kernels: forward {}, reverse {}".format(TF.rnn_route(spec, S * U, args.frames),
                                                                 TF.rnn_backward_route(spec, S * U, args.frames)))


if __name__ == "__main__":
    main()

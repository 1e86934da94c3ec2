#!/usr/bin/env python3
"""Embed a LIST of utterances of different lengths in one call — the batched counterpart of the reference's
experiments/speaker_verification/encoder/inference.py:110-154 (`embed_utterance`, which takes one waveform per call and
carries "TODO: handle multiple wavs to benefit from batching on GPU"; `embed_speaker` there raises NotImplemented).

Input here is the mel spectrogram of every utterance ([n_frames_i, 40]; the reference computes it from the waveform with
librosa, which is outside the hot path), synthetic from a seed.
  using_partials=False  the whole spectrogram of every utterance through the network: ONE variable-length forward
                        (SpeakerEncoder.forward(batch, lengths) -> LSTM.forward(..., lengths=...)): utterance i's embedding is
                        exactly that of the call on utterance i alone;
  using_partials=True   every utterance is cut into partial utterances of 160 frames, half overlapping (the last one kept, zero
                        padded, when at least 75 % of it is there); the partials of ALL utterances form one fixed-length batch;
                        an utterance's embedding is the L2-normalised mean of its partials' embeddings.
Example:  python examples/embed_utterances.py --utterances 64 --min_frames 40 --max_frames 400 --check"""
import argparse
import contextlib
import io
import time

import torch

from models import SpeakerEncoder

PARTIAL_FRAMES = 160          # params_data.py:11 (1600 ms)


def partial_starts(n_frames, partial_frames=PARTIAL_FRAMES, min_coverage=0.75, overlap=0.5):
    """First frames of the partial utterances of an n_frames long spectrogram: a step of (1 - overlap) partials; a last
    partial that reaches past the end is kept (to be zero padded) when at least min_coverage of it exists — always at least one."""
    step = max(int(round(partial_frames * (1.0 - overlap))), 1)
    starts = list(range(0, max(1, n_frames - partial_frames + step + 1), step))
    while len(starts) > 1 and (n_frames - starts[-1]) / float(partial_frames) < min_coverage:
        starts.pop()
    return starts


def pad_batch(mels):
    """list of [n_i, C] tensors -> ([N, max n_i, C] zero padded, lengths)."""
    lengths = [int(m.shape[0]) for m in mels]
    batch = mels[0].new_zeros(len(mels), max(lengths), mels[0].shape[1])
    for i, m in enumerate(mels):
        batch[i, :lengths[i]] = m
    return batch, lengths


@torch.no_grad()
def embed_utterances(model, mels, using_partials=False, partial_frames=PARTIAL_FRAMES):
    """Embeddings [N, D] (unit L2 norm) of N mel spectrograms of different lengths, all on the model's device."""
    if not using_partials:
        batch, lengths = pad_batch(mels)
        return model(batch, lengths=lengths)
    parts, owner = [], []
    for i, m in enumerate(mels):
        for s in partial_starts(m.shape[0], partial_frames):
            p = m.new_zeros(partial_frames, m.shape[1])
            n = min(partial_frames, m.shape[0] - s)
            p[:n] = m[s:s + n]
            parts.append(p)
            owner.append(i)
    embeds = model(torch.stack(parts))                                   # one fixed-length batch of all partials
    owner = torch.tensor(owner, device=embeds.device)
    sums = torch.zeros(len(mels), embeds.shape[1], dtype=embeds.dtype, device=embeds.device).index_add_(0, owner, embeds)
    counts = torch.bincount(owner, minlength=len(mels)).clamp(min=1).unsqueeze(1)
    mean = sums / counts
    return mean / mean.norm(dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--min_frames", type=int, default=40)
    ap.add_argument("--max_frames", type=int, default=400)
    ap.add_argument("--mels", type=int, default=40)
    ap.add_argument("--hidden_size", type=int, default=768)
    ap.add_argument("--n_layers", type=int, default=1)
    ap.add_argument("--emb_size", type=int, default=256)
    ap.add_argument("--ncores", type=int, default=2)
    ap.add_argument("--ttrank", type=int, default=2)
    ap.add_argument("--gru", action="store_true")
    ap.add_argument("--partials", action="store_true", help="using_partials=True")
    ap.add_argument("--check", action="store_true", help="compare with one call per utterance at batch 1")
    ap.add_argument("--seed", type=int, default=11)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        model = SpeakerEncoder(args.mels, args.hidden_size, args.n_layers, args.emb_size, dev, n_cores=args.ncores,
                               rank=args.ttrank, use_gru=args.gru).to(dev).eval()
    g = torch.Generator().manual_seed(args.seed + 1)
    frames = torch.randint(args.min_frames, args.max_frames + 1, (args.utterances,), generator=g).tolist()
    mels = [torch.rand(n, args.mels, generator=g).to(dev) for n in frames]
    embed_utterances(model, mels, args.partials)                         # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    embeds = embed_utterances(model, mels, args.partials)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    print("%d utterances of %d ... %d frames, using_partials=%s: %.2f ms in one call; embeddings %s" % (
        len(mels), min(frames), max(frames), args.partials, ms, tuple(embeds.shape)))
    if args.check:
        t0 = time.perf_counter()
        with torch.no_grad():
            single = torch.cat([embed_utterances(model, [m], args.partials) for m in mels])
        torch.cuda.synchronize()
        ms1 = 1e3 * (time.perf_counter() - t0)
        print("one call per utterance: %.2f ms; max |difference| %.3g" % (ms1, float((single - embeds).abs().max())))


if __name__ == "__main__":
    main()

"""Latency of forced alignment as served, and of the MAS kernel's durations
epilogue: base config, fp16 EmoVITS, deterministic-fill weights.

Serving: 500-frame recordings with 100 tokens of text, B = 1 and B = 8.  Two
figures per batch size, each a host clock around the whole call from the
samples on the host to the durations on the host, taken in turn within each
of ``--reps`` rounds after warm-up (median, p10, p90):

  align    EmoVITS.align (B = 8: align_batch): upload, ONE graph replay (STFT,
           posterior encoder, forward flow, text encoder, neg_cent, MAS with
           the durations epilogue), one copy back
  eager    the composition it replaces: spectrogram on the host (torch.stft,
           the data loader's), upload, the eager SynthesizerTrn.align,
           durations and scores back

Kernel: ops.maximum_path_durations (durations and scores) against what a user
had before, ops.maximum_path_lengths + path.sum(1), on random fp32 neg_cent at
B = 64, 500 x 100 and B = 8, 4096 x 512, full lengths; HIP events around
``--kernel-iters`` back-to-back calls, sides in turn, median of ``--reps``
rounds.  The results are compared before anything is timed.

There is no parent to compare with and no pass bar.  Prints the table and one
JSON line; ``--out`` also writes the table to a file.

    python tools/align_bench.py [--reps 30] [--warmup 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bench import BASE_MODEL, HOP, SR, build_model
from vits_amd import ops, utils
from vits_amd.infer import EmoVITS

N_FFT, WIN = 1024, 768
FRAMES, TOKENS = 500, 100
KERNEL_SHAPES = ((64, 500, 100), (8, 4096, 512))


def host_spectrogram(wav):
    """mel_processing.spectrogram_torch on the host: wav float32 [B, L]."""
    pad = (N_FFT - HOP) // 2
    y = torch.nn.functional.pad(wav.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, N_FFT, hop_length=HOP, win_length=WIN, window=torch.hann_window(WIN),
                      center=False, return_complex=True)
    return torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-6)


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
            "p90": float(np.percentile(a, 90))}


def serving(args, dev, lines, result):
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": N_FFT, "hop_length": HOP,
                 "win_length": WIN, "n_speakers": 2048, "sampling_rate": SR,
                 "noise_scale": 0.707},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=64)
    n = FRAMES * HOP + HOP // 2
    rs = np.random.RandomState(1)
    recs16 = [((rs.randn(n) * 0.2).clip(-1, 1) * 32767).astype(np.int16) for _ in range(8)]
    texts = [rs.randn(TOKENS, 256).astype(np.float32) for _ in range(8)]
    emo = torch.zeros(1, 1024)

    def align(B):
        if B == 1:
            return tts.align(recs16[0], 7, texts[0], emo)[0]
        return tts.align_batch([(r, 7, t, emo) for r, t in zip(recs16[:B], texts[:B])])[0][0]

    def eager(B):
        wav = torch.from_numpy(np.stack(recs16[:B]).astype(np.float32) / 32768.0)
        spec = host_spectrogram(wav).to(dev)
        x = torch.from_numpy(np.stack(texts[:B])).half().to(dev)
        dur, sc, _ = tts.model.align(
            x, torch.full((B,), TOKENS, device=dev), spec, torch.full((B,), spec.shape[2],
                                                                      device=dev),
            emo.half().to(dev).repeat(B, 1), torch.full((B,), 7, device=dev))
        sc.cpu()
        return dur.cpu().numpy()[0]

    sides = (("align", align), ("eager", eager))
    lines.append(f"forced alignment latency: {FRAMES}-frame recordings ({n} samples) x {TOKENS} "
                 f"tokens, base config, fp16 EmoVITS, {torch.cuda.get_device_name(0)}; host "
                 f"clock around each call, median of {args.reps} rounds (sides in turn) after "
                 f"{args.warmup} warm-up rounds")
    for B in (1, 8):
        ms = {name: [] for name, _ in sides}
        got = {}
        for rep in range(args.warmup + args.reps):
            for name, fn in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[name] = fn(B)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    ms[name].append(dt)
        same = bool(np.array_equal(got["align"], got["eager"]))
        result["serving"][str(B)] = {"row0_durations_equal": same}
        for name, _ in sides:
            s = stats(ms[name])
            result["serving"][str(B)][name] = s
            lines.append(f"B={B} {name:6s}: {s['median']:8.3f} ms per call (p10 {s['p10']:.3f}, "
                         f"p90 {s['p90']:.3f}), {s['median'] / B:7.3f} ms per recording")
        a, e = (result["serving"][str(B)][k]["median"] for k in ("align", "eager"))
        lines.append(f"B={B} align / eager (medians) {a / e:.3f}; row 0 durations equal: {same}")


def kernel(args, dev, lines, result):
    lines.append(f"MAS kernel: maximum_path_durations (durations + scores) against "
                 f"maximum_path_lengths + path.sum(1), random fp32 neg_cent, full lengths; HIP "
                 f"events around {args.kernel_iters} calls, median of {args.reps} rounds (sides "
                 f"in turn) after {args.warmup} warm-up rounds")
    for B, Tt, Ts in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(Tt)
        nc = (torch.randn(B, Tt, Ts, generator=g) * 3.0).to(dev)
        tt = torch.full((B,), Tt, dtype=torch.int32, device=dev)
        ts = torch.full((B,), Ts, dtype=torch.int32, device=dev)

        def new():
            return ops.maximum_path_durations(nc, tt, ts)[0]

        def old():
            return ops.maximum_path_lengths(nc, tt, ts, dtype=torch.int32).sum(1)

        assert torch.equal(new().long(), old().long()), "the two sides disagree"
        sides = (("durations", new), ("path+sum", old))
        us = {name: [] for name, _ in sides}
        for rep in range(args.warmup + args.reps):
            for name, fn in sides:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.kernel_iters):
                    fn()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / args.kernel_iters)
        key = f"{B}x{Tt}x{Ts}"
        result["kernel"][key] = {}
        for name, _ in sides:
            s = stats(us[name])
            result["kernel"][key][name] = s
            lines.append(f"B={B} {Tt} x {Ts} {name:9s}: {s['median']:9.1f} us per call (p10 "
                         f"{s['p10']:.1f}, p90 {s['p90']:.1f})")
        a, b = (result["kernel"][key][k]["median"] for k in ("durations", "path+sum"))
        lines.append(f"B={B} {Tt} x {Ts} durations / path+sum (medians) {a / b:.3f}; path tensor "
                     f"not written: {B * Tt * Ts * 4 / 1e6:.1f} MB")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("align_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    lines = []
    result = {"tool": "align_bench", "frames": FRAMES, "tokens": TOKENS, "reps": args.reps,
              "serving": {}, "kernel": {}}
    serving(args, dev, lines, result)
    kernel(args, dev, lines, result)
    text_out = "\n".join(lines)
    print(text_out)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text_out + "\n")


if __name__ == "__main__":
    main()

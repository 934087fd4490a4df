"""Latency of voice conversion as served: a 6 s recording (B = 1) and eight of
them (B = 8), base config, fp16 EmoVITS, deterministic-fill weights.

Three figures per batch size, each a host clock around the whole call from
the samples on the host to the result on the host (the ``time_used_backend``
of VITSWrap), taken in turn within each of ``--reps`` rounds after warm-up
(median, p10, p90):

  convert_pcm    EmoVITS.convert_pcm (B = 8: convert_pcm_batch): upload, ONE
                 graph replay (STFT, posterior encoder, both flows, decoder),
                 the int16 stage, one copy back
  eager          the composition it replaces: spectrogram on the host
                 (torch.stft, the data loader's), upload, the eager
                 SynthesizerTrn.voice_conversion, float waveform back, int16
                 on the host
  infer_pcm      text-to-speech of (about) the same number of frames, for
                 scale (B = 8: infer_pcm_batch); its frame count is printed

There is no parent to compare with and no pass bar.  Prints the table and one
JSON line; ``--out`` also writes the table to a file.

    python tools/vc_bench.py [--reps 30] [--warmup 4] [--seconds 6] [--out FILE]
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
from vits_amd import utils
from vits_amd.infer import EmoVITS

N_FFT, WIN = 1024, 768


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vc_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": N_FFT, "hop_length": HOP,
                 "win_length": WIN, "n_speakers": 2048, "sampling_rate": SR,
                 "noise_scale": 0.707},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        np.random.RandomState(0).randn(4, 1024).astype(np.float32).tofile(
            os.path.join(root, "1.emo"))
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=64)
    n = int(args.seconds * SR)
    frames = n // HOP
    rs = np.random.RandomState(1)
    recs = [(rs.randn(n) * 0.2).clip(-1, 1).astype(np.float32) for _ in range(8)]
    recs16 = [(r * 32767).astype(np.int16) for r in recs]
    emo = torch.zeros(1, 1024)
    # text whose synthesis has about as many frames as the recording
    probe = rs.randn(100, 256).astype(np.float32)
    np.random.seed(3)
    _, _, n100 = tts.infer_pcm(1, probe, emo)
    tokens = max(8, int(round(100 * frames / max(1, n100 // HOP))))
    text = rs.randn(tokens, 256).astype(np.float32)

    def convert(B):
        if B == 1:
            return tts.convert_pcm(recs16[0], 7, 1500)[1] // HOP
        return tts.convert_pcm_batch([(r, 7, 1500) for r in recs16[:B]])[2][0] // HOP

    def eager(B):
        wav = torch.from_numpy(np.stack(recs16[:B]).astype(np.float32) / 32768.0)
        spec = host_spectrogram(wav).to(dev)
        yl = torch.full((B,), spec.shape[2], device=dev)
        o, _, _ = tts.model.voice_conversion(spec, yl, torch.full((B,), 7, device=dev),
                                             torch.full((B,), 1500, device=dev))
        o = o[:, 0].float().cpu().numpy()
        np.clip(o * 32767, -32768, 32767).astype(np.int16)
        return spec.shape[2]

    def tts_call(B):
        np.random.seed(3)
        if B == 1:
            return tts.infer_pcm(1, text, emo)[2] // HOP
        return tts.infer_pcm_batch([(1, text, emo)] * B)[3][0] // HOP

    sides = (("convert_pcm", convert), ("eager", eager), ("infer_pcm", tts_call))
    lines = [f"voice conversion latency: {args.seconds:g} s recordings ({n} samples, {frames} "
             f"frames), base config, fp16 EmoVITS, {torch.cuda.get_device_name(0)}; host clock "
             f"around each call, median of {args.reps} rounds (sides in turn) after "
             f"{args.warmup} warm-up rounds"]
    result = {"tool": "vc_bench", "seconds": args.seconds, "frames": frames, "reps": args.reps,
              "b": {}}
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
        result["b"][str(B)] = {}
        for name, _ in sides:
            s = stats(ms[name])
            result["b"][str(B)][name] = dict(s, frames=int(got[name]))
            lines.append(f"B={B} {name:12s}: {s['median']:8.3f} ms per call (p10 {s['p10']:.3f}, "
                         f"p90 {s['p90']:.3f}), {s['median'] / B:7.3f} ms per recording, "
                         f"{got[name]} frames per row")
        c, e = (result["b"][str(B)][k]["median"] for k in ("convert_pcm", "eager"))
        lines.append(f"B={B} convert_pcm / eager (medians) {c / e:.3f}")
    text_out = "\n".join(lines)
    print(text_out)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text_out + "\n")


if __name__ == "__main__":
    main()

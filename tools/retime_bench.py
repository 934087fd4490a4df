"""Latency of retiming a recording (EmoVITS.retime_pcm): base
config, fp16 EmoVITS, a seeded recording of 500 frames and a text of 100
tokens.

Each call is timed with a host clock from the int16 samples on the host to
the int16 PCM on the host, the sides taking turns round by round; medians of
``--rounds`` rounds after warm-up (the graphs are captured by then):

  retime_pcm without text at speed 1.1
  retime_pcm with the text (alignment in the graph) and a token_scale
  retime_pcm with durations_old given (no alignment in the graph)
  retime_pcm with neutral controls, against
  convert_pcm of the same recording: the overhead of the plan and the warp

Then one round trip, the only evidence this tool can give about the audio:
the retimed waveform is aligned against its text again (EmoVITS.align) and the
recovered per-token durations are set against the dur_new that was asked for;
the alignment's score per frame stands next to that of the plain conversion.
There is no pass bar; the report records what was measured.

    python tools/retime_bench.py [--rounds 30] [--out profiles/retime_latency.txt]
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

SPK = 7
FRAMES, TOKENS = 500, 100


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
            "p90": float(np.percentile(a, 90))}


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("retime_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": 1024, "hop_length": HOP, "win_length": 768,
                 "n_speakers": 2048, "sampling_rate": SR, "noise_scale": 0.667},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"))
    g = torch.Generator().manual_seed(77)
    rec = (torch.randn(FRAMES * HOP + 57, generator=g) * 0.25).clamp(-1, 1).mul(32767).to(
        torch.int16).numpy()
    text = torch.randn(TOKENS, 256, generator=g).numpy()
    emo = torch.randn(1, 1024, generator=g)
    scale = np.ones(TOKENS, np.float32)
    scale[40:60] = 1.5  # twenty tokens half as long again
    d_old = tts.align(rec, SPK, text, emo)[0]
    assert int(d_old.sum()) == FRAMES

    calls = {
        "speed": lambda: tts.retime_pcm(rec, SPK, SPK, speed=1.1),
        "text": lambda: tts.retime_pcm(rec, SPK, SPK, text=text, emo=emo, token_scale=scale),
        "given": lambda: tts.retime_pcm(rec, SPK, SPK, text=text, durations_old=d_old,
                                        token_scale=scale),
        "neutral": lambda: tts.retime_pcm(rec, SPK, SPK),
        "convert_pcm": lambda: tts.convert_pcm(rec, SPK, SPK),
    }
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):  # the sides take turns
        for k, fn in calls.items():
            ms[k].append(clocked(fn)[1])
    t = {k: stats(v) for k, v in ms.items()}
    same = np.array_equal(calls["neutral"]()[0], calls["convert_pcm"]()[0])

    # the round trip
    wav_t, d_o, d_new, _ = tts.retime(rec, SPK, SPK, text=text, emo=emo, token_scale=scale,
                                      return_durations=True)
    y_new = len(wav_t) // HOP
    back, sc_back = tts.align(wav_t, SPK, text, emo)[:2]
    conv = tts.convert(rec, SPK, SPK)
    d_conv, sc_conv = tts.align(conv, SPK, text, emo)[:2]
    sc_rec = tts.align(rec, SPK, text, emo)[1]
    off = np.abs(back.astype(np.int64) - d_new.astype(np.int64))
    off_conv = np.abs(d_conv.astype(np.int64) - d_o.astype(np.int64))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"retime_bench: base config, fp16, {torch.cuda.get_device_name(0)}; a recording of "
        f"{FRAMES} frames, {TOKENS} tokens, token_scale 1.5 on tokens 40..59")
    say(f"host clock, int16 samples on the host -> int16 PCM on the host; medians of "
        f"{args.rounds} rounds after {args.warmup}, the sides taking turns")
    for k, name in (("speed", "retime_pcm no text, speed 1.1     "),
                    ("text", "retime_pcm text + token_scale     "),
                    ("given", "retime_pcm durations_old given    "),
                    ("neutral", "retime_pcm neutral controls       "),
                    ("convert_pcm", "convert_pcm (scale)               ")):
        say(f"  {name}: {t[k]['median']:8.2f} ms (p10 {t[k]['p10']:.2f}, p90 {t[k]['p90']:.2f})")
    say(f"  plan + warp + the copy back (neutral - convert_pcm): "
        f"{t['neutral']['median'] - t['convert_pcm']['median']:.2f} ms; neutral retime_pcm "
        f"{'==' if same else '!='} convert_pcm byte for byte; alignment in the graph (text - "
        f"given): {t['text']['median'] - t['given']['median']:.2f} ms")
    say(f"round trip: {FRAMES} -> {y_new} frames (asked: {int(d_new.sum())}); the retimed audio "
        f"aligned against its text again: |recovered - dur_new| per token median "
        f"{np.median(off):.1f}, max {int(off.max())} frames; for scale, the plain conversion "
        f"aligned against dur_old: median {np.median(off_conv):.1f}, max {int(off_conv.max())}")
    say(f"alignment score per frame: retimed {sc_back.sum() / max(y_new, 1):.3f}, plain "
        f"conversion {sc_conv.sum() / FRAMES:.3f}, the recording itself {sc_rec.sum() / FRAMES:.3f}"
        " (seeded weights and a noise recording: the scores compare paths, they say nothing "
        "about speech)")
    say("not measured: how a linearly interpolated latent sounds (no listening test, no trained "
        "checkpoint), kernel times (no trace taken), other lengths, inputs at another rate, "
        "batches")
    print(json.dumps({"tool": "retime_bench", "frames": FRAMES, "tokens": TOKENS, "ms": t,
                      "round_trip": {"median": float(np.median(off)), "max": int(off.max()),
                                     "y_new": y_new}}))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Latency of speech editing (EmoVITS.edit_pcm): base config,
fp16 EmoVITS, a seeded recording of 500 frames with a text of 100 tokens of
which a span of 10 is replaced by 10 new ones.

The call is timed with a host clock from the int16 samples on the host to the
int16 PCM on the host, with ``graph=True`` (one replay of the cached edit
graph) against ``graph=False`` (the same edit_bucketed call, eagerly), the
two sides taking turns round by round; medians of ``--rounds`` rounds after
warm-up (the graph is captured by then).  ``convert_pcm`` of the same
recording is timed the same way, for scale: it is the audio side plus reverse
flow and decoder without the two text encoders, the alignment and the plan.
There is no pass bar; the report records what was measured.

    python tools/edit_bench.py [--rounds 30] [--out profiles/edit_latency.txt]
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
FRAMES, TOKENS, SPAN = 500, 100, (45, 55, 55)


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
        sys.exit("edit_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
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
    old = torch.randn(TOKENS, 256, generator=g).numpy()
    a, b_old, b_new = SPAN
    new = np.concatenate([old[:a], torch.randn(b_new - a, 256, generator=g).numpy(), old[b_old:]])
    emo = torch.randn(1, 1024, generator=g)
    assert EmoVITS.edit_span(old, new) == SPAN

    def edit(graph):
        tts.graph = graph
        return tts.edit_pcm(rec, SPK, old, new, emo, span_frames="keep")

    def convert():
        tts.graph = True
        return tts.convert_pcm(rec, SPK, SPK)

    for _ in range(args.warmup):
        ref, _, _ = edit(True), edit(False), convert()
    ms = {"graph": [], "eager": [], "convert_pcm": []}
    for _ in range(args.rounds):  # the sides take turns
        ms["graph"].append(clocked(lambda: edit(True))[1])
        ms["eager"].append(clocked(lambda: edit(False))[1])
        ms["convert_pcm"].append(clocked(convert)[1])
    tts.graph = True
    pcm, n_model, dur, (f0, n_new, f1), scores = ref
    assert n_model == FRAMES * HOP and int(dur.sum()) == FRAMES and n_new == f1 - f0
    t = {k: stats(v) for k, v in ms.items()}
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"edit_bench: base config, fp16, {torch.cuda.get_device_name(0)}; a recording of "
        f"{FRAMES} frames, {TOKENS} tokens, span {SPAN} (10 tokens re-spoken, "
        f"span_frames='keep': frames [{f0}, {f1}) of the recording), patch on, alignment in "
        "the graph")
    say(f"host clock, int16 samples on the host -> int16 PCM on the host; medians of "
        f"{args.rounds} rounds after {args.warmup}, the sides taking turns")
    for k, name in (("graph", "edit_pcm graph=True "), ("eager", "edit_pcm graph=False"),
                    ("convert_pcm", "convert_pcm (scale) ")):
        say(f"  {name}: {t[k]['median']:8.2f} ms (p10 {t[k]['p10']:.2f}, p90 {t[k]['p90']:.2f})")
    say(f"  graph=False / graph=True: {t['eager']['median'] / t['graph']['median']:.2f}x; "
        f"edit / convert: {t['graph']['median'] / t['convert_pcm']['median']:.2f}x; RTF of the "
        f"edit {t['graph']['median'] / 1e3 / (FRAMES * HOP / SR):.4f}")
    say("not measured: other lengths and spans, durations_old given (no alignment in the "
        "graph), a re-run after an output-bucket overflow, inputs at another rate")
    print(json.dumps({"tool": "edit_bench", "frames": FRAMES, "tokens": TOKENS, "span": SPAN,
                      "ms": t}))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

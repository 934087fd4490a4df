"""Latency of duration control as served: base config, fp16 EmoVITS,
deterministic-fill weights, 100 tokens of text.

Synthesis: ``infer_pcm`` (B = 8: ``infer_pcm_batch``) with all three controls
(a pin every tenth token, a scale on every token, a target) against the same
call without them at the same text and frame count: the uncontrolled side runs
first, its frame count is the controlled side's target, and the pins are what
the uncontrolled call gave those tokens.  A host clock around each whole call,
text on the host to PCM on the host, sides in turn within each of ``--reps``
rounds after warm-up (median, p10, p90).  The uncontrolled call is the
yardstick: it is what the parent commit serves.

Timing of a recording: ``VITSWrap.speaking_like`` (alignment replay, durations
device to device, synthesis replay) against ``aligning`` followed by
``speaking(durations=...)`` (the durations cross the host), a 500-frame
recording; the two results are compared before anything is timed.

There is no pass bar.  Prints the table and one JSON line; ``--out`` also
writes the table to a file.

    python tools/duration_bench.py [--reps 30] [--warmup 4] [--out FILE]
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
from vits_amd import utils, vits_wrap
from vits_amd.infer import EmoVITS

N_FFT, WIN = 1024, 768
TOKENS, FRAMES = 100, 500


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
            "p90": float(np.percentile(a, 90))}


def timed(sides, reps, warmup):
    ms = {name: [] for name, _ in sides}
    for rep in range(warmup + reps):
        for name, fn in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= warmup:
                ms[name].append(dt)
    return {name: stats(v) for name, v in ms.items()}


class Front:
    max_utt_length = 4 * TOKENS

    def __call__(self, uid, txt):
        rs = np.random.RandomState(len(txt))
        return uid, txt, rs.randn(len(txt), 256).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": N_FFT, "hop_length": HOP,
                 "win_length": WIN, "n_speakers": 2048, "sampling_rate": SR,
                 "noise_scale": 0.707},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=64)
    rs = np.random.RandomState(1)
    texts = [rs.randn(TOKENS, 256).astype(np.float32) for _ in range(8)]
    emo = torch.zeros(1, 1024)
    scale = np.ones(TOKENS, np.float32)
    scale[::3] = 1.25
    lines = [f"duration control latency: {TOKENS} tokens, base config, fp16 EmoVITS, "
             f"{torch.cuda.get_device_name(0)}; host clock around each call, median of "
             f"{args.reps} rounds (sides in turn) after {args.warmup} warm-up rounds"]
    result = {"synthesis": {}, "speaking_like": {}}

    # the uncontrolled call fixes the frame count and the pins of the controlled one
    plain = [tts.infer_pcm(7, t, emo, return_durations=True) for t in texts]
    pins, targets = [], []
    for _, _, n, d in plain:
        g = np.full(TOKENS, -1, np.int32)
        g[::10] = d[::10]
        pins.append(g)
        targets.append(n // HOP)
    for B in (1, 8):
        if B == 1:
            sides = (("plain", lambda: tts.infer_pcm(7, texts[0], emo)),
                     ("controlled", lambda: tts.infer_pcm(
                         7, texts[0], emo, durations=pins[0], token_scale=scale,
                         target_frames=targets[0])))
        else:
            items = [(7, t, emo) for t in texts]
            sides = (("plain", lambda: tts.infer_pcm_batch(items)),
                     ("controlled", lambda: tts.infer_pcm_batch(
                         items, durations=pins, token_scale=[scale] * 8,
                         target_frames=targets)))
        frames = [len(fn()[0]) for _, fn in sides]
        st = timed(sides, args.reps, args.warmup)
        result["synthesis"][str(B)] = dict(st, pcm_samples=frames)
        for name, _ in sides:
            s = st[name]
            lines.append(f"B={B} {name:10s}: {s['median']:8.3f} ms per call (p10 {s['p10']:.3f}, "
                         f"p90 {s['p90']:.3f}), {s['median'] / B:7.3f} ms per utterance")
        lines.append(f"B={B} controlled / plain (medians) "
                     f"{st['controlled']['median'] / st['plain']['median']:.3f}; PCM samples "
                     f"{frames[1]} / {frames[0]}")

    wrap = vits_wrap.VITSWrap(textparser=Front(), speecher=tts, device_post=True)
    n = FRAMES * HOP + HOP // 2
    rec = ((rs.randn(n) * 0.2).clip(-1, 1) * 32767).astype(np.int16)
    text = "a" * TOKENS

    def like():
        return wrap.speaking_like({"wav": rec, "text": text, "spkid_src": 7, "spkid": 11,
                                   "emotion": emo})

    def composed():
        al = wrap.aligning({"wav": rec, "text": text, "spkid": 7, "emotion": emo})
        return wrap.speaking({"text": text, "spkid": 11, "emotion": emo,
                              "durations": al["durations"]})

    np.random.seed(0)
    a = like()
    np.random.seed(0)
    b = composed()
    same = a["wav"] == b["wav"]
    st = timed((("speaking_like", like), ("align+speak", composed)), args.reps, args.warmup)
    result["speaking_like"] = dict(st, equal=bool(same))
    for name, s in st.items():
        lines.append(f"{name:13s}: {s['median']:8.3f} ms per call (p10 {s['p10']:.3f}, p90 "
                     f"{s['p90']:.3f}), {FRAMES}-frame recording")
    lines.append(f"speaking_like / align+speak (medians) "
                 f"{st['speaking_like']['median'] / st['align+speak']['median']:.3f}; results "
                 f"equal: {same}")
    print("\n".join(lines))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

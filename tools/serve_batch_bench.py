"""A/B of VITSWrap.speaking on a request of N segments: one after another
(device_post=True: N B=1 graph replays, N copies, N host syncs) against
batch_segments=True (one batched graph replay, one copy, one sync), base
config, fp16 EmoVITS, every segment Tx = 100 tokens.

Both wrappers share one EmoVITS (same graphs, same noise), alternate call by
call in one process after warm-up, and see the same seed before every call,
so each pair synthesises the same request; the two results are compared byte
for byte before the timing.  The figure is ``time_used_backend`` (ms) of the
returned dict: a host clock from the end of the text front-end to the int16
PCM of the whole request on the host.  BATCH_MIN_SEGMENTS is set to 2 for the
run, so that N = 2 is measured batched whatever the class attribute says.
Prints one line per N with the medians per request and per segment, the share
of pairs batching wins, the smallest N at which batching wins, then one JSON
line.

    python tools/serve_batch_bench.py [--reps 30] [--warmup 4] [--tokens 100]
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bench import BASE_MODEL, HOP, SR, build_model
from vits_amd import utils
from vits_amd.infer import EmoVITS
from vits_amd.vits_wrap import VITSWrap

SEGMENTS = (1, 2, 4, 8, 16)


class FixedParser:
    """Front-end stand-in: one character per segment, the same text vectors
    for every segment."""
    max_utt_length = 1

    def __init__(self, vec):
        self.vec = vec

    def __call__(self, utt_id, text):
        return utt_id, text, self.vec


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
            "p90": float(np.percentile(a, 90)), "min": float(a.min())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("serve_batch_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": 1024, "hop_length": HOP,
                 "n_speakers": 2048, "sampling_rate": SR, "noise_scale": 0.707},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        np.random.RandomState(0).randn(4, 1024).astype(np.float32).tofile(os.path.join(root, "1.emo"))
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=32)
    vec = np.random.RandomState(2).randn(args.tokens, 256).astype(np.float32)
    VITSWrap.BATCH_MIN_SEGMENTS = 2
    wraps = {False: VITSWrap(textparser=FixedParser(vec), speecher=tts, device_post=True),
             True: VITSWrap(textparser=FixedParser(vec), speecher=tts, batch_segments=True)}

    def call(on, n):
        np.random.seed(3)
        return wraps[on].speaking(dict(text="x" * n, spkid=1, id="u"))

    result = {"tool": "serve_batch_bench", "tokens": args.tokens, "reps": args.reps, "n": {}}
    crossover = None
    for n in SEGMENTS:
        for _ in range(args.warmup):
            outs = {on: call(on, n) for on in (False, True)}
        assert outs[False]["wav"] == outs[True]["wav"], n
        assert len(outs[True]["segment_info"]) == n
        seconds = (len(outs[True]["wav"]) - 44) / 2 / outs[True]["sr"]
        ms = {False: [], True: []}
        for _ in range(args.reps):
            for on in (False, True):
                ms[on].append(call(on, n)["time_used_backend"])
        s = {on: stats(ms[on]) for on in ms}
        wins = float(np.mean(np.asarray(ms[True]) < np.asarray(ms[False])))
        if crossover is None and n > 1 and s[True]["median"] < s[False]["median"]:
            crossover = n
        result["n"][str(n)] = {"audio_s": seconds, "sequential": s[False], "batched": s[True],
                               "batched_wins": wins}
        for on, label in ((False, "sequential (device_post) "), (True, "batch_segments=True      ")):
            print(f"N={n:2d} {label}: {s[on]['median']:8.3f} ms per request "
                  f"(p10 {s[on]['p10']:.3f}, p90 {s[on]['p90']:.3f}, min {s[on]['min']:.3f}), "
                  f"{s[on]['median'] / n:7.3f} ms per segment, {args.reps} calls, "
                  f"{seconds:.2f} s of audio")
        print(f"N={n:2d} batched / sequential (medians) "
              f"{s[True]['median'] / s[False]['median']:.3f}; batched faster in "
              f"{100 * wins:.0f}% of pairs; identical bytes")
    result["smallest_n_batching_wins"] = crossover
    print("smallest N at which batching wins (medians): "
          + (str(crossover) if crossover else "none"))
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""A/B of N single-segment requests, each with its own speed, pitch and output
rate: VITSWrap.speaking in a loop (device_post=True: N B=1 graph replays, N
copies, N host syncs, one graph capture per distinct speed / pitch) against
VITSWrap.speaking_many (batch_segments=True: one replay of a rate-free batched
graph, the per-row output stage, one copy, one sync), base config, fp16
EmoVITS, every request Tx = 100 tokens.

Both wrappers share one EmoVITS (same graph cache, same noise), alternate call
by call in one process after warm-up, and see the same seed before every call,
so each pair synthesises the same requests; the N results of a pair are
compared byte for byte.  The figure is a host clock around the whole call (for
the loop: around the N speaking calls), from the request dicts to the int16
PCM of every request on the host; the front end is a table lookup.
MANY_MIN_ROWS is set to 1 for the run, so that every N is measured batched
whatever the class attribute says.  Prints one line per N with the medians per
call and per request, the share of pairs speaking_many wins, the graph
captures either side made (counted at SynthesizerTrn.capture_infer_bucketed,
from an empty graph cache), the smallest N at which speaking_many wins in
every pair, then one JSON line.

    python tools/serve_mixed_bench.py [--reps 30] [--warmup 4] [--tokens 100]
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
from vits_amd.vits_wrap import VITSWrap

REQUESTS = (1, 2, 4, 8, 16)
# request i of a call: a mix of voices' speeds, pitches and telephony /
# wide-band output rates (the model's own rate is SR)
SPEEDS = (1.0, 0.8, 1.25, 0.9, 1.1, 1.5, 0.7, 1.2)
PITCHES = (1.0, 1.1, 1.0, 0.9, 1.0, 1.2, 1.0, 0.95)
RATES = (SR, 8000, 16000, SR, 24000, 8000, 48000, SR)


class FixedParser:
    """Front-end stand-in: the same text vectors for every request."""
    max_utt_length = 256

    def __init__(self, vec):
        self.vec = vec

    def __call__(self, utt_id, text):
        return utt_id, text, self.vec


def requests(n):
    return [dict(id=f"u{i}", text="x", spkid=1, emotion=(1, i % 4), speed=SPEEDS[i % 8],
                 pitch=PITCHES[(i // 2) % 8], sampling_rate=RATES[i % 8],
                 volume=1.0 - 0.05 * (i % 4), tail_silence=0.01 * (i % 3))
            for i in range(n)]


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
        sys.exit("serve_mixed_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": 1024, "hop_length": HOP,
                 "n_speakers": 2048, "sampling_rate": SR, "noise_scale": 0.707},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        np.random.RandomState(0).randn(4, 1024).astype(np.float32).tofile(os.path.join(root, "1.emo"))
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=64)
    vec = np.random.RandomState(2).randn(args.tokens, 256).astype(np.float32)
    VITSWrap.MANY_MIN_ROWS = 1
    wraps = {False: VITSWrap(textparser=FixedParser(vec), speecher=tts, device_post=True),
             True: VITSWrap(textparser=FixedParser(vec), speecher=tts, batch_segments=True)}
    captures = {False: 0, True: 0}
    side = [False]
    real = tts.model.capture_infer_bucketed

    def counting(*a, **kw):
        captures[side[0]] += 1
        return real(*a, **kw)

    tts.model.capture_infer_bucketed = counting

    def call(on, n):
        """(wavs, milliseconds) of one call of either side."""
        side[0] = on
        np.random.seed(3)
        reqs = requests(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = wraps[True].speaking_many(reqs) if on else [wraps[False].speaking(r) for r in reqs]
        ms = (time.perf_counter() - t0) * 1e3
        return [o["wav"] for o in outs], ms

    result = {"tool": "serve_mixed_bench", "tokens": args.tokens, "reps": args.reps, "n": {}}
    threshold = None
    for n in REQUESTS:
        before = dict(captures)
        for _ in range(args.warmup):
            outs = {on: call(on, n)[0] for on in (False, True)}
        assert outs[False] == outs[True] and len(outs[True]) == n, n
        made = {on: captures[on] - before[on] for on in captures}
        seconds = sum((len(w) - 44) / 2 / r["sampling_rate"] for w, r in zip(outs[True], requests(n)))
        ms = {False: [], True: []}
        for _ in range(args.reps):
            pair = {on: call(on, n) for on in (False, True)}
            assert pair[False][0] == pair[True][0], n  # identical bytes in every pair
            for on in pair:
                ms[on].append(pair[on][1])
        s = {on: stats(ms[on]) for on in ms}
        wins = float(np.mean(np.asarray(ms[True]) < np.asarray(ms[False])))
        if wins < 1.0:
            threshold = None  # (the threshold is the N from which on it wins every pair)
        elif threshold is None:
            threshold = n
        result["n"][str(n)] = {"audio_s": seconds, "loop": s[False], "many": s[True],
                               "many_wins": wins, "captures_loop": made[False],
                               "captures_many": made[True]}
        for on, label in ((False, "speaking in a loop (device_post)"),
                          (True, "speaking_many                   ")):
            print(f"N={n:2d} {label}: {s[on]['median']:8.3f} ms per call "
                  f"(p10 {s[on]['p10']:.3f}, p90 {s[on]['p90']:.3f}, min {s[on]['min']:.3f}), "
                  f"{s[on]['median'] / n:7.3f} ms per request, {args.reps} calls, "
                  f"{seconds:.2f} s of audio, {made[on]} new graph captures")
        print(f"N={n:2d} speaking_many / loop (medians) "
              f"{s[True]['median'] / s[False]['median']:.3f}; speaking_many faster in "
              f"{100 * wins:.0f}% of pairs; identical bytes in every pair")
    result["captures_total"] = {"loop": captures[False], "many": captures[True]}
    result["smallest_n_many_wins_every_pair"] = threshold
    print(f"graph captures in all: loop {captures[False]}, speaking_many {captures[True]}")
    print("smallest N from which speaking_many wins every pair: "
          + (str(threshold) if threshold else "none"))
    print(json.dumps(result))


if __name__ == "__main__":
    main()

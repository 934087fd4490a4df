"""A/B of VITSWrap.speaking's output stage: host chain (device_post=False,
scipy.signal.resample_poly + numpy) against the device stage (device_post=
True, csrc/post.hip), base config, one utterance of about 6 s, B = 1.

Both wrappers share one EmoVITS (same graphs, same noise), alternate call by
call in one process after warm-up, and see the same seed before every call,
so each pair synthesises the same utterance.  The figure is
``time_used_backend`` (ms) of the returned dict: a host clock from the end of
the text front-end to the int16 PCM on the host, i.e. it ends behind the
device-to-host copy that synchronises.  Prints one line per case with the
median, the 10th / 90th percentile and the minimum of each side, the share of
pairs the device stage wins, then one JSON line.

    python tools/post_bench.py [--reps 40] [--warmup 5] [--seconds 6.0]
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

# pitch 1.1 at the base config's own 16 kHz: one 11/10 pass; with a rate
# change on top: two passes (11/10 then 1/2); defaults: the int16 conversion
# alone
CASES = [("pitch=1.1 sr=16000", dict(pitch=1.1, sampling_rate=16000)),
         ("pitch=1.1 sr=8000", dict(pitch=1.1, sampling_rate=8000)),
         ("defaults", dict())]


class FixedParser:
    """Front-end stand-in: the same text vectors for every request."""
    max_utt_length = 1 << 20

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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=6.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("post_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": 1024, "hop_length": HOP,
                 "n_speakers": 2048, "sampling_rate": SR, "noise_scale": 0.707},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        np.random.RandomState(0).randn(4, 1024).astype(np.float32).tofile(os.path.join(root, "1.emo"))
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"))
    text = np.random.RandomState(2).randn(4096, 256).astype(np.float32)

    def frames(tokens):
        np.random.seed(3)
        return len(tts.infer(1, text[:tokens], None)[0]) // HOP

    # the duration predictor decides the length: adjust the token count until
    # the utterance is within 3% of the wanted length
    want = args.seconds * SR / HOP
    tokens = 100
    for _ in range(6):
        got = frames(tokens)
        if abs(got - want) <= 0.03 * want:
            break
        tokens = max(4, min(4096, round(tokens * want / got)))
    vec = text[:tokens]
    wraps = {False: VITSWrap(textparser=FixedParser(vec), speecher=tts),
             True: VITSWrap(textparser=FixedParser(vec), speecher=tts, device_post=True)}

    def call(on, kw):
        np.random.seed(3)
        return wraps[on].speaking(dict(text="x", spkid=1, id="u", **kw))

    result = {"tool": "post_bench", "tokens": tokens, "reps": args.reps, "cases": {}}
    for name, kw in CASES:
        for _ in range(args.warmup):
            outs = {on: call(on, kw) for on in (False, True)}
        pcm = {on: np.frombuffer(outs[on]["wav"][44:], np.int16).astype(np.int32) for on in outs}
        assert len(pcm[False]) == len(pcm[True]) and outs[False]["sr"] == outs[True]["sr"]
        lsb = int(np.abs(pcm[False] - pcm[True]).max())
        seconds = len(pcm[True]) / outs[True]["sr"]
        ms = {False: [], True: []}
        for _ in range(args.reps):
            for on in (False, True):
                ms[on].append(call(on, kw)["time_used_backend"])
        s = {on: stats(ms[on]) for on in ms}
        wins = float(np.mean(np.asarray(ms[True]) < np.asarray(ms[False])))
        result["cases"][name] = {"audio_s": seconds, "pcm_max_diff_lsb": lsb, "host": s[False],
                                 "device": s[True], "device_wins": wins}
        for on, label in ((False, "device_post=False (host) "), (True, "device_post=True (device)")):
            print(f"{name:20s} {label}: time_used_backend median {s[on]['median']:.3f} ms "
                  f"(p10 {s[on]['p10']:.3f}, p90 {s[on]['p90']:.3f}, min {s[on]['min']:.3f}), "
                  f"{args.reps} calls, {seconds:.2f} s of audio")
        print(f"{name:20s} device - host (medians) "
              f"{s[True]['median'] - s[False]['median']:+.3f} ms; device faster in "
              f"{100 * wins:.0f}% of pairs; PCM differs by at most {lsb} LSB")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

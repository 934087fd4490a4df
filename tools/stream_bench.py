"""Latency of streamed synthesis as served: base config, fp16 EmoVITS,
deterministic-fill weights, 100 tokens of text pinned to about 500 and about
4000 frames (``target_frames``), so both sides of a pair do the same work.

Per length and first-chunk size, alternating pairs: ``infer_pcm`` (the call
to its whole result on the host), then ``infer_pcm_stream`` of the same input
(the call to its first chunk on the host, and to its last).  A host clock
(time.perf_counter) around each, started behind a device synchronisation; the
stream's clock starts before the call that runs the front.  The first-chunk
size is swept over the cores of 64-, 128-, 256- and 512-frame windows with
the later chunks at their default, then the later chunks' size over the cores
of 512-, 1024-, 2048- and 4096-frame windows with the first at its default.
Reported: the median and p10 - p90 of the time
to the first chunk, the streamed total, infer_pcm's time, their ratio, and in
how many pairs the first chunk was on the host before infer_pcm's whole
result took.  The one condition: at about 4000 frames, in
every pair.  Before anything is timed the streamed bytes are compared with
infer_pcm's from the same seed: the fp16 decoder depends on a frame's place
in its row, the difference is reported as a maximum and a share of samples.

Prints the table and one JSON line; ``--out`` also writes the table to a file.

    python tools/stream_bench.py [--reps 20] [--warmup 3] [--out FILE]
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

TOKENS = 100
LENGTHS = (500, 4000)
WINDOWS = (64, 128, 256, 512)
CHUNK_WINDOWS = (512, 1024, 2048, 4096)


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
            "p90": float(np.percentile(a, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "hop_length": HOP, "n_speakers": 2048,
                 "sampling_rate": SR, "noise_scale": 0.707},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=64)
    ctx = tts.model.dec.context_frames()
    text = np.random.RandomState(1).randn(TOKENS, 256).astype(np.float32)
    emo = torch.zeros(1, 1024)
    lines = [f"streamed synthesis latency: {TOKENS} tokens, base config, fp16 EmoVITS, "
             f"{torch.cuda.get_device_name(0)}; host clock (time.perf_counter) from the call, "
             f"behind a device sync, to the result on the host; {args.reps} alternating pairs "
             f"(infer_pcm, then infer_pcm_stream) after {args.warmup} warm-up pairs; decoder "
             f"context {ctx} frames, default chunks of "
             f"{' .. '.join(str(v) for v in tts._stream_sizes(None, None, ctx))} frames"]
    result = {}
    for frames in LENGTHS:
        kw = dict(target_frames=frames)
        np.random.seed(0)
        ref = tts.infer_pcm(7, text, emo, **kw)[0]
        np.random.seed(0)
        got = np.concatenate(list(tts.infer_pcm_stream(7, text, emo, **kw)))
        d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
        lines.append(f"{frames} frames ({frames * HOP / SR:.1f} s of audio): streamed bytes "
                     f"against infer_pcm's, same seed: max difference {int(d.max())} of 32767 "
                     f"({d.max() / 32767:.1e}), {int((d > 0).sum())} of {d.size} samples differ "
                     f"({(d > 0).mean() * 100:.2f} %)")
        result[str(frames)] = {"pcm_max_diff": int(d.max()), "pcm_share": float((d > 0).mean())}
        d_first, d_chunk = tts._stream_sizes(None, None, ctx)
        sweep = [(W - 2 * ctx, d_chunk) for W in WINDOWS]
        sweep += [(d_first, W - 2 * ctx) for W in CHUNK_WINDOWS if W - 2 * ctx != d_chunk]
        for first, chunk in sweep:
            whole, ttfc, total, n_chunks = [], [], [], 0
            for rep in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tts.infer_pcm(7, text, emo, **kw)
                t_whole = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stream = tts.infer_pcm_stream(7, text, emo, first_chunk_frames=first,
                                              chunk_frames=chunk, **kw)
                next(stream)
                t_first = (time.perf_counter() - t0) * 1e3
                n_chunks = 1 + sum(1 for _ in stream)
                t_last = (time.perf_counter() - t0) * 1e3
                if rep >= args.warmup:
                    whole.append(t_whole)
                    ttfc.append(t_first)
                    total.append(t_last)
            earlier = sum(f < w for f, w in zip(ttfc, whole))
            s_f, s_t, s_w = stats(ttfc), stats(total), stats(whole)
            lines.append(
                f"  {frames:4d} frames, chunks of {first:3d} .. {chunk:4d} frames, {n_chunks:2d} "
                f"chunks: first chunk {s_f['median']:7.3f} ms (p10 {s_f['p10']:.3f}, p90 "
                f"{s_f['p90']:.3f}), streamed total {s_t['median']:7.3f} ms, infer_pcm "
                f"{s_w['median']:7.3f} ms, total / infer_pcm {s_t['median'] / s_w['median']:.3f}, "
                f"first chunk earlier in {earlier} of {len(whole)} pairs")
            result[str(frames)][f"{first}/{chunk}"] = {"first": s_f, "total": s_t, "infer_pcm": s_w,
                                               "chunks": n_chunks, "earlier": earlier,
                                               "pairs": len(whole)}
    ok = all(v["earlier"] == v["pairs"] for k, v in result[str(LENGTHS[-1])].items()
             if isinstance(v, dict))
    lines.append(f"the one condition (first chunk before infer_pcm's whole result in every pair "
                 f"at {LENGTHS[-1]} frames): {'met' if ok else 'NOT met'}")
    print("\n".join(lines))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Latency of voice conversion of long recordings (EmoVITS.convert_pcm_long,
DESIGN.md 4t): base config, fp16 EmoVITS, seeded recordings of 1, 5 and 10
minutes at the model's rate.  Every figure is a host clock from the int16
samples on the host to the int16 PCM on the host (the call ends in the host
sync of its one device-to-host copy), the median of ``--rounds`` calls after
warm-up (the graphs are captured and the filters cached by then).

1. Window choice.  For every (window bucket, rows per replay) pair of
   ``--windows`` x ``--rows`` the ``--sweep-minutes`` recording runs
   ``--sweep-rounds`` times: time per call and per converted frame, the batch
   buckets its replays use, the frames the rows compute per converted frame
   (the plan's own overhead, next to the expected 1 + 2 * context / Cf and to
   the extra frames per window frame, 2 * context / window) and
   the device memory the graphs of that pair hold (allocated after the first
   call minus before, graph cache empty before).  Rows per replay is
   EmoVITS.MAX_BATCH, set for the run.
2. The default (EmoVITS.LONG_WINDOW_FRAMES, MAX_BATCH) on the three
   recordings, next to the recipe the error message of ``convert`` gives: the
   loop of convert_pcm over consecutive chunks of 4096 frames, concatenated.
   The two outputs are compared: SNR of the chunked PCM against the long
   path's within ``context`` frames of a cut, and the number of differing
   samples elsewhere.

Prints a report and one JSON line; ``--out`` also writes the report there.

    python tools/vc_long_bench.py [--rounds 30] [--out profiles/vc_long_latency.txt]
"""
import argparse
import gc
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

SRC, TGT = 7, 1500
CHUNK = 4096  # frames: the largest conversion bucket


def recording(minutes, seed=0):
    g = torch.Generator().manual_seed(seed + int(minutes * 60))
    n = int(minutes * 60 * SR)
    return (torch.randn(n, generator=g) * 0.25).clamp(-1, 1).mul(32767).to(torch.int16).numpy()


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    a = np.asarray(ms)
    return out, {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
                 "p90": float(np.percentile(a, 90)), "min": float(a.min())}


def chunked(tts, rec):
    """The recipe of convert's error message: consecutive chunks of 4096
    frames through convert_pcm, concatenated (the last one takes the rest)."""
    step = CHUNK * HOP
    cuts = list(range(0, max(1, len(rec) - len(rec) % HOP), step))
    parts = [tts.convert_pcm(rec[lo:(len(rec) if lo == cuts[-1] else lo + step)], SRC, TGT)[0]
             for lo in cuts]
    return np.concatenate(parts)


def snr_db(a, ref):
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    noise = ((a - ref) ** 2).sum()
    return float("inf") if noise == 0 else float(10 * np.log10((ref ** 2).sum() / noise))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--minutes", type=float, nargs="+", default=[1, 5, 10])
    ap.add_argument("--windows", type=int, nargs="+", default=[512, 1024, 2048, 4096])
    ap.add_argument("--rows", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--sweep-minutes", type=float, default=5)
    ap.add_argument("--sweep-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vc_long_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": 1024, "hop_length": HOP, "win_length": 768,
                 "n_speakers": 2048, "sampling_rate": SR, "noise_scale": 0.667},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=64)
    ctx = tts.model.vc_context_frames(tts._vc_stft())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"vc_long_bench: base config, fp16, {torch.cuda.get_device_name(0)}; context "
        f"{ctx} frames per side; host clock, samples on the host -> int16 PCM on the host")
    result = {"tool": "vc_long_bench", "context": ctx, "sweep": [], "default": {}}

    # 1. the window choice
    rec = recording(args.sweep_minutes)
    F = len(rec) // HOP
    default_rows = EmoVITS.MAX_BATCH
    say(f"\nwindow choice: {args.sweep_minutes:g} min ({F} frames), median of "
        f"{args.sweep_rounds} calls after 1")
    best = None
    try:
        for wf in args.windows:
            for rows in args.rows:
                EmoVITS.MAX_BATCH = rows
                plan = tts._long_plan(len(rec), wf, ctx)
                groups = [hi - lo for lo, hi in tts._groups(len(plan))]
                buckets = sorted({1 if m == 1 else tts._batch_bucket(m) for m in groups})
                computed = sum(w.b - w.a for w in plan) / F
                tts._graphs.clear()
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                m0 = torch.cuda.memory_allocated()
                tts.convert_pcm_long(rec, SRC, TGT, window_frames=wf)
                torch.cuda.synchronize()
                mem = (torch.cuda.memory_allocated() - m0) / 2 ** 20
                _, t = timed(lambda: tts.convert_pcm_long(rec, SRC, TGT, window_frames=wf),
                             args.sweep_rounds, 0)
                per_frame = t["median"] * 1e3 / F
                row = {"window": wf, "rows": rows, "windows": len(plan), "replays": len(groups),
                       "batch_buckets": buckets, "ms": t, "us_per_frame": per_frame,
                       "frames_computed_per_frame": computed,
                       "expected_overhead": 1 + 2 * ctx / (wf - 2 * ctx), "graph_mib": mem}
                result["sweep"].append(row)
                say(f"  window {wf:4d} x {rows:2d} rows: {len(plan):3d} windows in {len(groups):2d} "
                    f"replays (batch buckets {buckets}), {t['median']:9.2f} ms "
                    f"(p10 {t['p10']:.2f}, p90 {t['p90']:.2f}), {per_frame:7.3f} us per frame, "
                    f"{computed:.3f} frames computed per frame (1 + 2c/Cf = "
                    f"{row['expected_overhead']:.3f}, 2c/window = {2 * ctx / wf:.3f}), graphs hold "
                    f"{mem:8.1f} MiB")
                if best is None or per_frame < best["us_per_frame"]:
                    best = row
    finally:
        EmoVITS.MAX_BATCH = default_rows
    if best is not None:
        say(f"  fastest per converted frame: window {best['window']} x {best['rows']} rows "
            f"({best['us_per_frame']:.3f} us per frame, graphs {best['graph_mib']:.1f} MiB); the "
            f"default is window {EmoVITS.LONG_WINDOW_FRAMES} x {default_rows} rows")
        result["fastest"] = {"window": best["window"], "rows": best["rows"]}
    tts._graphs.clear()
    torch.cuda.empty_cache()

    # 2. the default against the loop over chunks of 4096 frames
    wf = EmoVITS.LONG_WINDOW_FRAMES
    say(f"\ndefault (window {wf} x {default_rows} rows) against the loop of convert_pcm over "
        f"chunks of {CHUNK} frames; median of {args.rounds} calls after {args.warmup}")
    for minutes in args.minutes:
        rec = recording(minutes)
        F = len(rec) // HOP
        plan = tts._long_plan(len(rec), wf, ctx)
        computed = sum(w.b - w.a for w in plan) / F
        (pcm, n), t_long = timed(lambda: tts.convert_pcm_long(rec, SRC, TGT), args.rounds,
                                 args.warmup)
        loop, t_loop = timed(lambda: chunked(tts, rec), args.rounds, args.warmup)
        assert n == F * HOP == len(pcm) == len(loop)
        near = np.zeros(len(pcm), dtype=bool)
        for cut in range(CHUNK, F, CHUNK):
            near[max(0, cut - ctx) * HOP:min(F, cut + ctx) * HOP] = True
        differ_far = int((pcm[~near] != loop[~near]).sum())
        row = {"frames": F, "long_ms": t_long, "chunked_ms": t_loop,
               "long_over_chunked": t_long["median"] / t_loop["median"],
               "frames_computed_per_frame": computed,
               "expected_overhead": 1 + 2 * ctx / (wf - 2 * ctx),
               "rtf": t_long["median"] / 1e3 / (minutes * 60),
               "snr_db_near_cuts": snr_db(loop[near], pcm[near]) if near.any() else None,
               "differ_near_cuts": int((pcm[near] != loop[near]).sum()),
               "samples_near_cuts": int(near.sum()), "differ_elsewhere": differ_far,
               "snr_db_elsewhere": snr_db(loop[~near], pcm[~near])}
        result["default"][f"{minutes:g}"] = row
        say(f"  {minutes:4g} min ({F:6d} frames, {len(plan)} windows): convert_pcm_long "
            f"{t_long['median']:9.2f} ms (p10 {t_long['p10']:.2f}, p90 {t_long['p90']:.2f}; RTF "
            f"{row['rtf']:.5f}), chunked loop {t_loop['median']:9.2f} ms (p10 {t_loop['p10']:.2f}, "
            f"p90 {t_loop['p90']:.2f}); long / chunked {row['long_over_chunked']:.3f} with "
            f"{computed:.3f} frames computed per frame (1 + 2c/Cf = {row['expected_overhead']:.3f}, "
            f"2c/window = {2 * ctx / wf:.3f})")
        say(f"            chunked against long, int16: within {ctx} frames of a cut SNR "
            f"{row['snr_db_near_cuts']} dB ({row['differ_near_cuts']} of "
            f"{row['samples_near_cuts']} samples differ); elsewhere {differ_far} samples differ "
            f"(SNR {row['snr_db_elsewhere']} dB)")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

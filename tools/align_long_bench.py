"""Latency of forced alignment of long recordings (EmoVITS.align_long,
DESIGN.md 4u): base config, fp16 EmoVITS, seeded recordings of 1, 5 and 10
minutes at the model's rate with text at about 1 token per 6 frames in
segments of about 100 tokens.

1. The call: a host clock from the int16 samples on the host to the durations
   on the host (the call ends in the host sync of its one device-to-host
   copy), median and p10-p90 of ``--rounds`` calls after warm-up (the graphs
   are captured by then).
2. Its parts, by HIP events around each on one stream, the same sequence
   restated on the call's own building blocks: the latent windows, the text
   side, the first sweep (scores + forward step per panel), the backtrack, the
   second sweep (scores + gather per panel, then the sums).  Median of
   ``--part-rounds``.
3. The scale: ``align`` on a 4096-frame recording with the 2048 tokens its
   kernel takes, as time per DP cell, next to the long path's first sweep per
   cell.

Prints a report and one JSON line; ``--out`` also writes the report there.

    python tools/align_long_bench.py [--rounds 30] [--out profiles/align_long_latency.txt]
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
from vits_amd.infer import EmoVITS, _Window

SPK = 7
FRAMES_PER_TOKEN = 6
SEGMENT_TOKENS = 100


def recording(minutes, seed=0):
    g = torch.Generator().manual_seed(seed + int(minutes * 60))
    n = int(minutes * 60 * SR)
    return (torch.randn(n, generator=g) * 0.25).clamp(-1, 1).mul(32767).to(torch.int16).numpy()


def segments(frames, channels, seed=1):
    """About frames / 6 tokens in segments of about 100 (the last one takes
    the rest), one emotion vector each."""
    total = max(1, frames // FRAMES_PER_TOKEN)
    sizes = [SEGMENT_TOKENS] * (total // SEGMENT_TOKENS)
    if total % SEGMENT_TOKENS:
        sizes.append(total % SEGMENT_TOKENS)
    g = torch.Generator().manual_seed(seed + total)
    texts = [torch.randn(t, channels, generator=g).numpy() for t in sizes]
    emos = [torch.randn(1, 1024, generator=g) for _ in sizes]
    return texts, emos, total


def stats(ms):
    a = np.asarray(ms)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)),
            "p90": float(np.percentile(a, 90))}


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, stats(ms)


PARTS = ("latent windows", "text side", "first sweep", "backtrack", "second sweep")


def parts_once(tts, rec, texts, emos):
    """align_long's sequence on its own building blocks with an event between
    the parts: ({part: ms}, durations on the device)."""
    stft = tts._vc_stft()
    tokens = [t.shape[0] for t in texts]
    F, wf, strip, panel = tts._align_long_check(len(rec), None, tokens, None, None, None)
    resolved = [tts._resolve(SPK, e) for e in emos]
    sids = [int(s) for s, _ in resolved]
    x, _, _ = tts._vc_input(rec, None, capped=False)
    plan = ([_Window(0, F, 0, F, 0, x.numel(), 0)] if F <= wf
            else tts._long_plan(x.numel(), wf, tts.model.align_context_frames(stft)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PARTS) + 1)]
    ev[0].record()
    z_p = tts._latent_windows(x, plan, wf, sids[0])
    ev[1].record()
    m_p, logs_p = tts._segment_priors(texts, tokens, sids, [e for _, e in resolved])
    ev[2].record()
    total = sum(tokens)
    lens = torch.tensor([F, total], dtype=torch.int32).to(tts.device)
    C = z_p.shape[1]
    job = ops._MasLongJob("align_long_bench", 1, F, total, lens[:1], lens[1:], strip, panel, True,
                          False, tts.device)
    zpan = torch.empty(C * job.panel, device=tts.device)
    nc = torch.empty(job.panel * total, device=tts.device)

    def score(y0, rows):
        ops.copy_windows(z_p, zpan, [(y0, 0, rows, rows)], channels=C, src_rstride=F,
                         dst_rstride=rows)
        ops.check(job.lib.vits_neg_cent(zpan.data_ptr(), m_p.data_ptr(), logs_p.data_ptr(),
                                        nc.data_ptr(), 1, C, rows, total, job.stream),
                  "vits_neg_cent")

    for y0, rows in job.panels():
        score(y0, rows)
        job.forward(nc.data_ptr(), rows * total, y0, rows)
    ev[3].record()
    job.backtrack()
    ev[4].record()
    for y0, rows in job.panels():
        score(y0, rows)
        job.gather(nc.data_ptr(), rows * total, y0, rows)
    job.sums()
    ev[5].record()
    torch.cuda.synchronize()
    return {p: ev[i].elapsed_time(ev[i + 1]) for i, p in enumerate(PARTS)}, job.dur


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--part-rounds", type=int, default=5)
    ap.add_argument("--minutes", type=float, nargs="+", default=[1, 5, 10])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("align_long_bench: needs a ROCm GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    hps = utils.get_hparams_from_dict({
        "data": {"text_channels": 256, "filter_length": 1024, "hop_length": HOP, "win_length": 768,
                 "n_speakers": 2048, "sampling_rate": SR, "noise_scale": 0.667},
        "model": BASE_MODEL})
    with tempfile.TemporaryDirectory() as root:
        tts = EmoVITS(os.path.join(root, "model.pth"), dev, hps=hps, model=build_model("cpu"),
                      max_graphs=64)
    ctx = tts.model.align_context_frames(tts._vc_stft())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"align_long_bench: base config, fp16, {torch.cuda.get_device_name(0)}; context {ctx} "
        f"frames per side, windows of {EmoVITS.LONG_WINDOW_FRAMES} frames, panels of "
        f"{EmoVITS.ALIGN_LONG_PANEL_FRAMES} frames, strips of {EmoVITS.ALIGN_LONG_STRIP_TOKENS} "
        f"tokens; text at 1 token per {FRAMES_PER_TOKEN} frames in segments of {SEGMENT_TOKENS}")
    say(f"the call: host clock, int16 samples on the host -> durations on the host; median of "
        f"{args.rounds} calls after {args.warmup}.  the parts: HIP events, median of "
        f"{args.part_rounds}")
    result = {"tool": "align_long_bench", "context": ctx, "calls": {}}
    for minutes in args.minutes:
        rec = recording(minutes)
        F = len(rec) // HOP
        texts, emos, total = segments(F, 256)
        need = tts._align_long_bytes(F, total, EmoVITS.ALIGN_LONG_STRIP_TOKENS,
                                     EmoVITS.ALIGN_LONG_PANEL_FRAMES)[0]
        out, t = timed(lambda: tts.align_long(rec, SPK, texts, emos), args.rounds, args.warmup)
        d = np.concatenate(out[0])
        assert out[3] == F and d.sum() == F and d.min() >= 1
        runs = [parts_once(tts, rec, texts, emos) for _ in range(args.part_rounds + 1)][1:]
        assert np.array_equal(runs[-1][1][0].cpu().numpy(), d)  # (the restated sequence is the call's)
        part = {p: float(np.median([r[0][p] for r in runs])) for p in PARTS}
        cells = F * total
        row = {"frames": F, "tokens": total, "segments": len(texts), "ms": t, "parts_ms": part,
               "workspace_and_panel_mb": need / 1e6, "rtf": t["median"] / 1e3 / (minutes * 60),
               "first_sweep_ns_per_cell": part["first sweep"] * 1e6 / cells}
        result["calls"][f"{minutes:g}"] = row
        say(f"  {minutes:4g} min ({F:6d} frames x {total:5d} tokens in {len(texts):3d} segments, "
            f"{need / 1e6:6.1f} MB of workspace and panel): align_long {t['median']:9.2f} ms "
            f"(p10 {t['p10']:.2f}, p90 {t['p90']:.2f}; RTF {row['rtf']:.5f})")
        say("            parts: " + ", ".join(f"{p} {part[p]:.2f} ms" for p in PARTS)
            + f"; first sweep {row['first_sweep_ns_per_cell']:.3f} ns per DP cell")
    # the scale: align at the largest shape its kernel takes
    # (align's graph holds the text encoder's position table: a text bucket
    # beyond the table's 384 positions cannot be captured, so that is what fits
    # the call; the kernel alone is timed at its own 2048 columns)
    F, total = 4096, 2048
    fit = min(total, tts.model.enc_p.sin_table.size(1))
    rec = recording(1)[:F * HOP]
    g = torch.Generator().manual_seed(5)
    text, emo = torch.randn(fit, 256, generator=g).numpy(), torch.randn(1, 1024, generator=g)
    out, t = timed(lambda: tts.align(rec, SPK, text, emo), args.rounds, args.warmup)
    assert out[2] == F and out[0].sum() == F
    nc = torch.randn(1, F, total, device=dev)
    lens = torch.tensor([F, total], dtype=torch.int32, device=dev)
    ker = []
    for _ in range(args.part_rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.maximum_path_durations(nc, lens[:1], lens[1:])
        b.record()
        torch.cuda.synchronize()
        ker.append(a.elapsed_time(b))
    k = float(np.median(ker[1:]))
    result["scale"] = {"frames": F, "align_tokens": fit, "align_ms": t,
                       "align_ns_per_cell": t["median"] * 1e6 / (F * fit), "kernel_tokens": total,
                       "mas_kernel_ms": k, "mas_kernel_ns_per_cell": k * 1e6 / (F * total)}
    say(f"\nthe scale: align, {F} frames x {fit} tokens (one segment, one graph replay; the "
        f"widest text its graph captures): {t['median']:.2f} ms per call (p10 {t['p10']:.2f}, "
        f"p90 {t['p90']:.2f}) = {t['median'] * 1e6 / (F * fit):.3f} ns per DP cell, everything "
        f"included; its MAS kernel alone on random scores of {F} x {total} (HIP events): "
        f"{k:.3f} ms = {k * 1e6 / (F * total):.3f} ns per DP cell")
    say("not measured: other window, panel and strip sizes, noise_scale > 0, inputs at another "
        "rate, anti-diagonal tiles across workgroups (one workgroup per recording here)")
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

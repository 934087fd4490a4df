"""Summarise tools/run_train_profiles.sh into profiles/<tag>_train_summary.json
(+ profiles/<tag>_train_kernel_stats.csv: the R=2 run's --stats table).

Per step = counters of the R=2 run - counters of the R=1 run, over
every kernel dispatch.  HBM bytes follow MI355X_MICROARCH.md §HBM: FETCH_SIZE
and WRITE_SIZE are KiB; FETCH_SIZE is doubled (gfx950 reports half of a wide
coalesced read stream); WRITE_SIZE is used as is.  The per-family table
gives each kernel family's share of the step's GPU time and its HBM bytes."""
import csv
import json
import os
import shutil
import sys
from collections import defaultdict

tag = sys.argv[1] if len(sys.argv) > 1 else "r03"
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 32
kind = sys.argv[3] if len(sys.argv) > 3 else "train"  # or "longform" (tools/run_longform_profiles.sh)
src = os.path.join(os.environ.get("LOGS", "bench_logs"), f"prof_{tag}_{kind}")  # as the run_*.sh


def family(name):
    n = name.replace("(anonymous namespace)::", "").replace("void ", "")
    for key in ("conv1d_mfma_kernel", "wgrad_kernel", "wgrad_reduce", "gate_fwd", "gate_bwd",
                "stft_", "mas_kernel", "neg_cent", "radam", "wnorm", "sn_", "wn_update",
                "pack16", "Cijk", "igemm", "naive_conv", "elementwise", "reduce_kernel",
                "multi_tensor_apply", "fused_adam", "copy", "cat", "index"):
        if key.lower() in n.lower():
            return key
    return n.split("(")[0].split("<")[0][:48]


def counters(name):
    fam = defaultdict(float)
    path = os.path.join(src, name, "run_counter_collection.csv")
    for r in csv.DictReader(open(path)):
        fam[family(r["Kernel_Name"])] += float(r["Counter_Value"])
    return fam


def trace(name):
    fam = defaultdict(lambda: [0, 0.0])
    for r in csv.DictReader(open(os.path.join(src, name, "run_kernel_stats.csv"))):
        f = fam[family(r["Name"])]
        f[0] += int(r["Calls"])
        f[1] += float(r["TotalDurationNs"])
    return fam


def diff(a, b, scale):
    return {k: (b.get(k, 0.0) - a.get(k, 0.0)) * scale for k in set(a) | set(b)}


f = diff(counters("fetch1"), counters("fetch2"), 2.0 * 1024)
w = diff(counters("write1"), counters("write2"), 1024.0)
t1, t5 = trace("trace1"), trace("trace2")
fams = {}
# MIOpen's exhaustive find (cudnn.benchmark, as bench.py) runs its reference
# naive_conv kernels in the warm-up of every process: their bytes cancel in
# R=2 - R=1 (same work), their durations do not - left out of the per-step
# time and dispatch counts (they are not part of the replayed step)
SEARCH_ONLY = ("naive_conv",)
for k in set(t1) | set(t5):
    if k in SEARCH_ONLY:
        continue
    calls = t5.get(k, [0, 0])[0] - t1.get(k, [0, 0])[0]
    ns = t5.get(k, [0, 0.0])[1] - t1.get(k, [0, 0.0])[1]
    if calls <= 0 and ns <= 0:
        continue
    fams[k] = {"dispatches_per_step": round(calls, 1), "ms_per_step": round(ns / 1e6, 3),
               "hbm_bytes_per_step": round(f.get(k, 0.0) + w.get(k, 0.0))}
tot_ms = sum(v["ms_per_step"] for v in fams.values())
for v in fams.values():
    v["share"] = round(v["ms_per_step"] / tot_ms, 4) if tot_ms else 0.0
    v["GBps"] = round(v["hbm_bytes_per_step"] / (v["ms_per_step"] * 1e6), 1) if v["ms_per_step"] else None
hbm = sum(f.values()) + sum(w.values())
summary = {"tag": tag, "batch": batch, "hbm_bytes_per_step": round(hbm),
           "hbm_fetch_bytes_per_step": round(sum(f.values())),
           "hbm_write_bytes_per_step": round(sum(w.values())),
           "dispatches_per_step": round(sum(v["dispatches_per_step"] for v in fams.values()), 1),
           "kernel_ms_per_step": round(tot_ms, 3),
           "note": f"(R=2 replays - R=1 replay) of the captured {'C5 long-form infer_p2' if kind == 'longform' else 'train_stft'} step; FETCH_SIZE x2 "
                   "(gfx950 wide-read correction), KiB->B",
           "families": dict(sorted(fams.items(), key=lambda kv: -kv[1]["ms_per_step"]))}
os.makedirs("profiles", exist_ok=True)
if kind == "longform":  # C5: B=4 x Ty=2500 frames per step
    frames = batch * 2500
    summary["frames_per_step"] = frames
    summary["hbm_bytes_per_frame"] = round(hbm / frames)
with open(os.path.join("profiles", f"{tag}_{kind}_summary.json"), "w") as fh:
    json.dump(summary, fh, indent=1)
shutil.copy(os.path.join(src, "trace2", "run_kernel_stats.csv"),
            os.path.join("profiles", f"{tag}_{kind}_kernel_stats.csv"))
print(json.dumps({k: v for k, v in summary.items() if k != "families"}, indent=1))

"""Report of tools/pmc_pairs.sh for the fused split-fp32 pair kernels: per
template instance (resblock_f32p_kernel<C, 0>) of the LAST profiled infer_p2
step, the summed kernel time (trace run), and from the two counter runs the
issue mix per MFMA, MFMA-pipe utilisation (SQ_VALU_MFMA_BUSY_CYCLES over
1024 SIMDs x GRBM_GUI_ACTIVE / 8), the wait shares of the wave cycles and
LDS bank-conflict cycles per LDS instruction.
usage: python tools/pmc_pairs_report.py OUTDIR"""
import csv
import glob
import os
import re
import sys
from collections import defaultdict

base = sys.argv[1] if len(sys.argv) > 1 else "bench_logs/pmc_pairs"
# KEY=wn_layer_f32p_kernel: the same report for the fused WN layer kernel
# (csrc/wn_f32p.hip; instances <H, NG>)
KEY = os.environ.get("KEY", "resblock_f32p_kernel")
# fused pair launches of one infer_p2 step (9 per stage pair index and
# accumulating launch; override when the plan changes)
LAST = int(os.environ.get("LAST", "0"))


def inst(name):
    if KEY != "resblock_f32p_kernel":
        m = re.search(KEY + r"<([^>]*)>", name)
        return f"{KEY}<{m.group(1).replace(' ', '')}>" if m else name
    m = re.search(KEY + r"<(\d+)", name)
    return f"{KEY}<{m.group(1)},0>" if m else name


def counters(p):
    rows = defaultdict(dict)
    meta = {}
    for f in glob.glob(os.path.join(base, p, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if KEY not in r["Kernel_Name"]:
                continue
            d = int(r["Dispatch_Id"])
            rows[d][r["Counter_Name"]] = float(r["Counter_Value"])
            meta[d] = (inst(r["Kernel_Name"]), int(r["VGPR_Count"]), int(r["Accum_VGPR_Count"]),
                       int(r["LDS_Block_Size"]))
    return rows, meta


def last_step(ids):
    """The dispatches of the last of the 3 warm-up + 1 timed steps."""
    ids = sorted(ids)
    n = LAST or len(ids) // 4
    return ids[-n:]


def trace():
    t = defaultdict(lambda: [0, 0])
    rows = []
    for f in glob.glob(os.path.join(base, "trace", "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if KEY in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), inst(r["Kernel_Name"]),
                             int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    n = LAST or len(rows) // 4
    for _, k, d in rows[-n:]:
        t[k][0] += 1
        t[k][1] += d
    return t, n


t, n = trace()
print(f"kernel trace, last step: {n} fused-pair launches")
for k in sorted(t):
    print(f"  {k:32s} {t[k][0]:3d} launches {t[k][1] / 1e6:7.3f} ms")
print(f"  {'total':32s} {sum(v[0] for v in t.values()):3d} launches "
      f"{sum(v[1] for v in t.values()) / 1e6:7.3f} ms")

p1, m1 = counters("p1")
p2, m2 = counters("p2")
agg = defaultdict(lambda: defaultdict(float))
info = {}
for rows, meta in ((p1, m1), (p2, m2)):
    for d in last_step(rows):
        k = meta[d][0]
        info[k] = meta[d][1:]
        for c, v in rows[d].items():
            agg[k][("2:" if rows is p2 and c in ("GRBM_GUI_ACTIVE", "SQ_WAVE_CYCLES") else "") + c] += v
print("\ncounters, last step (sums over the instance's launches)")
print(f"{'kernel':32s} {'valu/mf':>7} {'salu/mf':>7} {'lds/mf':>6} {'vmem/mf':>7} {'mfma%':>6} "
      f"{'wait':>5} {'winst':>5} {'ldsconf':>7} {'vgpr':>4} {'lds':>6}")
for k in sorted(agg):
    a = agg[k]
    mf = max(a["SQ_INSTS_MFMA"], 1.0)
    gui = a["GRBM_GUI_ACTIVE"] / 8
    vg, ag, lds = info[k]
    print(f"{k:32s} {a['SQ_INSTS_VALU'] / mf:7.2f} {a['SQ_INSTS_SALU'] / mf:7.2f} "
          f"{a['SQ_INSTS_LDS'] / mf:6.2f} {(a['SQ_INSTS_VMEM_RD'] + a['SQ_INSTS_VMEM_WR']) / mf:7.3f} "
          f"{a['SQ_VALU_MFMA_BUSY_CYCLES'] / (1024 * gui) * 100 if gui else 0:6.1f} "
          f"{a['SQ_WAIT_ANY'] / max(a['SQ_WAVE_CYCLES'], 1):5.2f} "
          f"{a['SQ_WAIT_INST_ANY'] / max(a['2:SQ_WAVE_CYCLES'], 1):5.2f} "
          f"{a['SQ_LDS_BANK_CONFLICT'] / max(a['SQ_INSTS_LDS'], 1):7.3f} {vg + ag:4d} {lds:6d}")
    print("    raw: " + " ".join(f"{c}={v:.4g}" for c, v in sorted(a.items())))
# effective clock (reads high on dispatches shorter than ~0.3 ms): the counter
# runs' GRBM_GUI_ACTIVE / 8 XCDs over the trace run's kernel time
print("\neffective clock, GRBM_GUI_ACTIVE / 8 / trace time")
for k in sorted(agg):
    if t[k][1]:
        print(f"  {k:32s} {agg[k]['GRBM_GUI_ACTIVE'] / 8 / t[k][1]:5.2f} GHz")

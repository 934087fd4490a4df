"""Fused WN layer (csrc/wn_f32p.hip) vs the two launches it replaces
(in_layer with the gate epilogue + res_skip with the res / skip epilogue), on
random data with HIP events: a middle layer and the last layer at the
headline flow shape (B=16, T=500, H=256, k=5), at B=1, T=512, and at B=16,
T=1024 (where 64-column tiles fill the chip: the library's tile rule).  Per
shape: the two-conv pair REPS times (median, min, max: its run-to-run
spread), the fused layer at 32- and 64-column tiles and at the library's own
choice.  REPS / ITERS from the environment."""
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402

from vits_amd import ops  # noqa: E402
from vits_amd.ops import make_desc, make_out  # noqa: E402

dev = torch.device("cuda:0")
H, K = 256, 5
reps = int(os.environ.get("REPS", "7"))
iters = int(os.environ.get("ITERS", "20"))


def timeit(fn):
    """Median / min / max over `reps` timings of `iters` back-to-back calls (us)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(1e3 * s.elapsed_time(e) / iters)
    return statistics.median(out), min(out), max(out)


def layer(last):
    w1 = torch.randn(2 * H, H, K, device=dev) / (H * K) ** 0.5
    m2 = H if last else 2 * H
    w2 = torch.randn(m2, H, 1, device=dev) / H ** 0.5
    c1 = ops.to_lowp(ops.pack_conv(w1, torch.randn(2 * H, device=dev) * 0.1, padding=K // 2,
                                   gate=True), ops.WDT_F32S)
    c2 = ops.to_lowp(ops.pack_conv(w2, torch.randn(m2, device=dev) * 0.1), ops.WDT_F32S)
    return c1, c2


for B, T in ((16, 500), (1, 512), (16, 1024)):
    for last in (False, True):
        c1, c2 = layer(last)
        h = torch.randn(B, H, T, device=dev) * 0.5
        cond = torch.randn(B, 2 * H, device=dev) * 0.3
        abuf, h2, skip = torch.empty_like(h), torch.empty_like(h), torch.zeros_like(h)
        d1 = make_desc(c1, h, make_out(abuf), cond=cond)
        if last:
            d2 = make_desc(c2, abuf, make_out(skip, accumulate=True))
        else:
            d2 = make_desc(c2, abuf, make_out(h2, res=h), out1=make_out(skip, accumulate=True),
                           split=H)
        assert ops.wn_layer_f32p_supported(c1, c2, h)
        name = f"B{B} T{T} {'last' if last else 'mid '}"
        t_in = timeit(lambda: ops.conv1d_launch(d1, B, dev))
        t_rs = timeit(lambda: ops.conv1d_launch(d2, B, dev))
        t2 = timeit(lambda: ops.conv1d_launch_seq([d1, d2], B, dev))
        print(f"{name} two-conv  {t2[0]:7.1f} us  (min {t2[1]:.1f} max {t2[2]:.1f}; "
              f"in_layer {t_in[0]:.1f} + res_skip {t_rs[0]:.1f})", flush=True)
        for ng in (32, 64, 0):
            ops.WN_NG = ng
            wd = ops.wn_layer_desc(c1, c2, h, None if last else h2, skip, accumulate=True,
                                   cond=cond)
            ops.WN_NG = 0
            tf = timeit(lambda: ops.conv1d_launch_seq([wd], B, dev))
            tiles = -(-T // (ng or 32)) * B
            print(f"{name} fused ng={ng or 'auto':>4} {tf[0]:7.1f} us  (min {tf[1]:.1f} max "
                  f"{tf[2]:.1f})  {100 * (tf[0] / t2[0] - 1):+.1f} %"
                  + (f"  {tiles} workgroups" if ng else ""), flush=True)

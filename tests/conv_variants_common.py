"""Shared case table, builders, float64 reference and derived error bound of
the conv1d kernel-variant tests (test_conv1d_plan.py on the CPU,
test_conv1d_variants_gpu.py on the GPU).  A plain module, not a conftest.

A case names one launch of vits_conv1d_forward: the weight / MFMA kind, a
forced tile (or None for the library's picker), the epilogue, the shape, the
layout and epilogue options, and the kernel variant the library must plan
for it (``plan``: "BMxBN/WMxWN/v4|el[/ga][/uplds]").

Reference (float64), the operation include/vits_amd.h documents, in order:
prologue leaky-relu; zero outside [0, tin); taps at n - pad_left + j*dil;
bias + cond; act; gmask; res + res_scale * v; accumulate; post_div; zero at
t >= lengths[b].  The gate pairs logical channels p and m/2 + p, the
polyphase upsample is computed as the transposed convolution it lowers
(t = q*u - up_pad + kk), STORE with ``split`` writes rows [0, split) and
[split, m) to two outputs with their own options.  The prologue is evaluated
in fp32 as the kernel's staging does (its result IS the fp32 operand); for
16-bit kinds both operands are then rounded to the type.

Per-element bound, derived (not measured).  With A = conv(|x'|, |w|) +
|bias| + |cond| in float64, K = cin * k taps x channels, u = 2^-24:
  exact fp32, and 16-bit operands with fp32 accumulation:  2 * K * u * A
      (the bound of a K-term fp32 sum in any order, times 2 for the MFMA's
      internal order);
  split fp32:  (6 * K * u + 2^-22) * A
      (six accumulating MFMAs per k-step; 2^-22 |x||w| for the dropped
      m*l + l*m + l*l terms, conv1d_impl.h split3_bf16).
It is carried through the epilogue by the slope of each step: <= 1 for RELU /
TANH, exp(v) for EXP, |gmask factor|, |res_scale|, 1 / post_div, plus 4 ulp
(fp32) of the result.  The gate's fast_tanh / fast_sigmoid add the figure of
the comment at fast_tanh, 1e-7 absolute per factor, doubled; 16-bit outputs
add half an ulp of the output type.
"""
from __future__ import annotations

import dataclasses
import zlib

import numpy as np
import torch

from vits_amd import _lib, ops
from vits_amd._lib import (ACT_EXP, ACT_NONE, ACT_RELU, ACT_TANH, TILE_32x256, TILE_64x128,
                           TILE_64x256, TILE_128x128, WDT_BF16, WDT_F16, WDT_F32, WDT_F32P,
                           WDT_F32S)

U = 2.0 ** -24
SENTINEL = 1536.0            # guard-band fill: exact in fp32, bf16 and fp16
KINDS = {"f32": WDT_F32, "bf16": WDT_BF16, "f16": WDT_F16, "f32s": WDT_F32S, "f32p": WDT_F32P}
TORCH16 = {WDT_BF16: torch.bfloat16, WDT_F16: torch.float16}
TILES = {"128x128": TILE_128x128, "64x256": TILE_64x256, "32x256": TILE_32x256,
         "64x128": TILE_64x128}
EPI_CODE = {"store": _lib.EPI_STORE, "store2": _lib.PLAN_EPI_STORE2, "gate": _lib.EPI_GATE,
            "up": _lib.EPI_UPSAMPLE}
GUARD_C = 2                  # sentinel channels before every output; after it GUARD_C plus
                             # the rest of the last 128-row block (guard_post): a kernel
                             # that lost its row guard still writes inside the allocation
X_PRE_C, X_POST_C = 1, 64    # NaN channels around x (cin_pad - cin < 64)


# ---------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------

_DEFAULTS = dict(
    tile=None, dil=1, pad_left=None, tin=None, n_out=None, in_slope=0.1, bias=True, cond=False,
    act=ACT_NONE, res=False, res_alias=False, res_scale=1.0, accumulate=False, post_div=1.0,
    split=None, act1=ACT_NONE, accumulate1=False, gate_pre=False, up=None, t_out=None,
    lengths=None, len_skip=0, gmask=False, io16=0, time_major=False, x_off=0, x_tpad=8,
    y_tpad=4)


def case(name, kind, epi, plan, B, cin, m, k, **kw):
    c = dict(_DEFAULTS, name=name, kind=kind, epi=epi, plan=plan, B=B, cin=cin, m=m, k=k)
    unknown = set(kw) - set(_DEFAULTS)
    assert not unknown, unknown
    c.update(kw)
    if c["up"] is not None:                      # (K, u, up_pad): m = cout * u rows, k = K / u taps
        K, u, _ = c["up"]
        assert c["m"] % u == 0 and c["k"] == K // u and c["pad_left"] is None
        c["pad_left"] = c["k"] - 1
    if c["pad_left"] is None:
        c["pad_left"] = (c["k"] - 1) * c["dil"] // 2
    assert c["tin"] is not None
    if c["n_out"] is None:
        c["n_out"] = c["tin"] + (-(-c["up"][2] // c["up"][1]) if c["up"] else 0)
    if c["up"] is not None and c["t_out"] is None:
        c["t_out"] = c["tin"] * c["up"][1]
    return c


def expected_plan(c) -> dict:
    parts = c["plan"].split("/")
    bm, bn = (int(v) for v in parts[0].split("x"))
    wm, wn = (int(v) for v in parts[1].split("x"))
    assert parts[2] in ("v4", "el")
    return dict(wdtype=KINDS[c["kind"]], ga=int("ga" in parts[3:]), bm=bm, bn=bn, waves_m=wm,
                waves_n=wn, v4=int(parts[2] == "v4"), io16=int(c["io16"] != 0),
                epi=EPI_CODE[c["epi"]], up_lds=int("uplds" in parts[3:]))


def variant_key(plan: dict):
    return (plan["wdtype"], plan["ga"], plan["bm"], plan["bn"], plan["waves_m"], plan["waves_n"],
            plan["v4"])


def _table():
    T = []
    # ---- real large tiles: >= 512 workgroups, everything else minimal -------
    # 128x128: m = 130 (two row blocks, the second two rows), B = 4, 64 column
    # tiles; T = 8192 stages 16-byte blocks, T = 8191 element-wise
    for kind, k, ga in (("f32", 3, ""), ("f32s", 3, ""), ("f32p", 3, ""), ("bf16", 3, ""),
                        ("f16", 3, ""), ("bf16", 5, "/ga"), ("f16", 5, "/ga")):
        for tin, st in ((8192, "v4"), (8191, "el")):
            epi = "gate" if (kind in ("f32p", "bf16") and st == "v4") else "store"
            T.append(case(f"big128-{kind}{ga[1:]}-{st}", kind, epi, f"128x128/2x2/{st}{ga}", 4, 16,
                          130, k, tile="128x128", tin=tin, cond=epi == "gate",
                          res=epi == "store"))
    # 64x256 where the window also fits the 128-column tile: m = 66, B = 4
    for kind, k, ga, wv in (("f32s", 9, "", "2x2"), ("f32p", 9, "", "2x2"), ("bf16", 3, "", "1x4"),
                            ("f16", 3, "", "1x4"), ("bf16", 9, "/ga", "1x4"),
                            ("f16", 9, "/ga", "1x4")):
        for tin, st in ((16384, "v4"), (16383, "el")):
            T.append(case(f"big256-{kind}{ga[1:]}-{st}", kind, "store", f"64x256/{wv}/{st}{ga}", 4,
                          16, 66, k, tile="64x256", tin=tin, res=st == "el"))
    # exact fp32 64x256: a chunk window too wide for the 128-column tile keeps
    # the small grid on 64x256 (no fallback)
    for tin, st in ((516, "v4"), (515, "el")):
        T.append(case(f"f32-64x256-{st}", "f32", "store", f"64x256/1x4/{st}", 3, 20, 66, 3,
                      tile="64x256", dil=40, tin=tin))
    # ... and the fallback of a 64x256 layer whose window fits
    T.append(case("f32-64x256-fallback", "f32", "store", "64x128/2x2/v4", 2, 16, 66, 3,
                  tile="64x256", tin=260))
    # ---- small-grid kernels: every (kind, tile, staging) the pickers reach --
    for kind in ("f32", "bf16", "f16", "f32s", "f32p"):
        for ga in (("",) if kind in ("f32", "f32s", "f32p") else ("", "/ga")):
            k = 5 if ga else 3
            for tin, st in ((132, "v4"), (131, "el")):
                T.append(case(f"s64x128-{kind}{ga[1:]}-{st}", kind, "store", f"64x128/2x2/{st}{ga}",
                              3, 17, 66, k, tile="64x128", tin=tin, res=True))
                T.append(case(f"s32x256-{kind}{ga[1:]}-{st}", kind, "store", f"32x256/1x4/{st}{ga}",
                              3, 17, 30, k, tile="32x256", tin=tin + 128, act=ACT_RELU))
    # ---- epilogues, once per kind (64x128 tiles of 128x128 / picker layers) --
    for kind in ("f32", "bf16", "f16", "f32s", "f32p"):
        for ga in (("",) if kind in ("f32", "f32s", "f32p") else ("", "/ga")):
            k = 5 if ga else 3
            tag = f"{kind}{ga[1:]}"
            T.append(case(f"gate-{tag}", kind, "gate", f"64x128/2x2/v4{ga}", 2, 16, 70, k,
                          tile="64x128", tin=140, cond=True, gate_pre=kind != "f32p"))
            T.append(case(f"store2-{tag}", kind, "store2", f"64x128/2x2/el{ga}", 2, 16, 70, k,
                          tile="64x128", tin=131, split=48, act=ACT_TANH, act1=ACT_RELU,
                          accumulate1=True, res=True))
            kk = 6 if ga else 2                    # taps of the polyphase conv
            T.append(case(f"uplds-{tag}", kind, "up", f"64x128/2x2/v4{ga}/uplds", 2, 16, 66, kk,
                          tile="64x128", up=(kk * 2, 2, kk - 1), tin=136, t_out=270,
                          lengths=[270, 131]))
            T.append(case(f"up-{tag}", kind, "up", f"64x128/2x2/el{ga}", 2, 16, 66, kk,
                          tile="64x128", up=(kk * 2, 2, kk - 1), tin=133, res=True,
                          lengths=[266, 7]))
    # ---- 16-bit activations: io16 = 1 (LDS weights), io16 = 2 (global A) ----
    for kind in ("bf16", "f16"):
        T.append(case(f"io16-1-{kind}", kind, "store", "64x128/2x2/v4", 2, 32, 66, 3, tile="64x128",
                      tin=136, io16=1, res=True))
        T.append(case(f"io16-2-{kind}", kind, "store", "64x128/2x2/v4/ga", 2, 32, 66, 3,
                      tile="64x128", tin=136, io16=2, res=True))
        T.append(case(f"io16-2-{kind}-el-gate", kind, "gate", "64x128/2x2/el/ga", 2, 17, 66, 3,
                      tile="64x128", tin=133, io16=2, cond=True))
    # ---- forced combinations no picker produces --------------------------------
    T.append(case("forced-f32-128x128", "f32", "store", "64x128/2x2/v4", 2, 16, 130, 3,
                  tile="128x128", tin=132))
    T.append(case("forced-f32p-64x256", "f32p", "store", "64x256/2x2/v4", 2, 16, 66, 3,
                  tile="64x256", dil=130, tin=516))
    T.append(case("forced-f32p-32x256", "f32p", "store", "32x256/1x4/el", 2, 16, 30, 3,
                  tile="32x256", tin=259))
    T.append(case("forced-f32s-32x256", "f32s", "store", "32x256/1x4/v4", 2, 16, 30, 3,
                  tile="32x256", tin=260))
    # ---- tile edges on the small-grid kernels (picker tiles, default F32P) --
    for n in (1, 3, 4, 127, 128, 129, 260):
        T.append(case(f"edge-n{n}", "f32p", "store", f"64x128/2x2/{'v4' if n % 4 == 0 else 'el'}",
                      3, 17, 66, 3, tin=n, res=True))
    for n in (255, 256, 257, 516):
        T.append(case(f"edge256-n{n}", "f32", "store", f"32x256/1x4/{'v4' if n % 4 == 0 else 'el'}",
                      3, 33, 30, 3, tin=n))
    for m_ in (2, 62, 66):
        T.append(case(f"edge-m{m_}", "f32p", "gate", "64x128/2x2/el", 3, 33, m_, 3, tin=37,
                      cond=True))
    T.append(case("edge-cin1", "f32p", "store", "64x128/2x2/v4", 3, 1, 34, 3, tin=36))
    T.append(case("edge-cin1-f32", "f32", "store", "64x128/2x2/v4", 3, 1, 34, 1, tin=36))
    T.append(case("edge-cin33-bf16", "bf16", "store", "64x128/2x2/el", 3, 33, 34, 3, tin=35))
    # ---- staging geometry -----------------------------------------------------
    for kind in ("f32", "f32p", "bf16"):
        k, dil = 5, 3
        for tag, pad, tin, st in (("pad0", 0, 136, "v4"), ("causal", 12, 136, "v4"),
                                  ("pad5", 5, 136, "v4"), ("pad5-odd", 5, 135, "el")):
            T.append(case(f"stage-{kind}-{tag}", kind, "store",
                          f"64x128/2x2/{st}{'/ga' if kind == 'bf16' else ''}", 2, 17, 34, k,
                          tile="64x128", dil=dil, pad_left=pad, tin=tin))
        T.append(case(f"stage-{kind}-tin-short", kind, "store",
                      f"64x128/2x2/v4{'/ga' if kind == 'bf16' else ''}", 2, 17, 34, k,
                      tile="64x128", dil=dil, tin=100, n_out=140))
        T.append(case(f"stage-{kind}-tin-long", kind, "store",
                      f"64x128/2x2/v4{'/ga' if kind == 'bf16' else ''}", 2, 17, 34, k,
                      tile="64x128", dil=dil, tin=140, n_out=100))
        T.append(case(f"stage-{kind}-cstride-odd", kind, "store",
                      f"64x128/2x2/el{'/ga' if kind == 'bf16' else ''}", 2, 17, 34, k,
                      tile="64x128", dil=dil, tin=136, x_tpad=7))
        T.append(case(f"stage-{kind}-ptr-off1", kind, "store",
                      f"64x128/2x2/el{'/ga' if kind == 'bf16' else ''}", 2, 17, 34, k,
                      tile="64x128", dil=dil, tin=136, x_off=1))
        T.append(case(f"stage-{kind}-time-major", kind, "store", "64x128/2x2/el", 2, 17, 34, 1,
                      tile="64x128", tin=70, time_major=True))
    T.append(case("stage-f32p-halo96", "f32p", "store", "64x128/2x2/v4", 2, 16, 34, 3,
                  tile="64x128", dil=48, tin=260))
    # (the widest window of a 16-channel F32S chunk on 128 columns: halo 64)
    T.append(case("stage-f32s-halo64", "f32s", "store", "64x128/2x2/el", 2, 16, 34, 3,
                  tile="64x128", dil=32, tin=259))
    # ---- epilogue options -------------------------------------------------------
    for act, an in ((ACT_RELU, "relu"), (ACT_TANH, "tanh"), (ACT_EXP, "exp")):
        for res in (False, True):
            T.append(case(f"act-{an}{'-res' if res else ''}", "f32p", "store", "64x128/2x2/v4", 2,
                          16, 34, 3, tin=132, act=act, res=res, cond=True))
    T.append(case("res-half-alias", "f32p", "store", "64x128/2x2/v4", 2, 16, 34, 3, tin=132,
                  res=True, res_alias=True, res_scale=0.5))
    T.append(case("res-neg-alias", "f32", "store", "64x128/2x2/el", 2, 16, 34, 3, tin=131,
                  res=True, res_alias=True, res_scale=-1.0))
    T.append(case("acc-div3", "f32p", "store", "64x128/2x2/v4", 2, 16, 34, 3, tin=132,
                  accumulate=True, post_div=3.0))
    T.append(case("gmask", "f32", "store", "64x128/2x2/v4", 2, 16, 34, 3, tin=132, gmask=True,
                  res=True))
    for sp in (32, 48, 68):
        T.append(case(f"split{sp}", "f32p", "store2", "64x128/2x2/v4", 2, 16, 70, 3, tin=132,
                      split=sp, act=ACT_EXP, accumulate1=True, res=True, cond=True))
    T.append(case("gate-nopre-bf16", "bf16", "gate", "64x128/2x2/v4", 2, 16, 34, 3, tile="64x128",
                  tin=132, cond=True))
    T.append(case("up16x8-lds", "f32p", "up", "64x128/2x2/v4/uplds", 2, 16, 64, 2, tile="64x128",
                  up=(16, 8, 4), tin=40, t_out=300, lengths=[300, 150]))
    T.append(case("up16x8-res", "f32", "up", "64x128/2x2/el", 2, 16, 64, 2, tile="64x128",
                  up=(16, 8, 4), tin=39, t_out=300, res=True, lengths=[300, 150]))
    # ---- lengths and len_skip: lengths {0, 1, a tile boundary, n_out} ---------
    T.append(case("lenskip-store", "f32p", "store", "64x128/2x2/v4", 4, 16, 34, 3, tin=516,
                  lengths=[0, 1, 128, 516], len_skip=64))
    T.append(case("lenskip-gate", "f32", "gate", "64x128/2x2/el", 4, 16, 34, 3, tile="64x128",
                  tin=515, cond=True, lengths=[0, 1, 256, 515], len_skip=64))
    T.append(case("lenskip-up", "bf16", "up", "64x128/2x2/v4/uplds", 4, 16, 64, 2, tile="64x128",
                  up=(4, 2, 1), tin=260, lengths=[0, 1, 254, 520], len_skip=64))
    T.append(case("lenskip-up-res", "f32p", "up", "64x128/2x2/v4", 4, 16, 64, 2, tile="64x128",
                  up=(4, 2, 1), tin=260, res=True, lengths=[0, 1, 254, 520], len_skip=64))
    names = [c["name"] for c in T]
    assert len(set(names)) == len(names)
    return T


CASES = _table()
CASE_IDS = [c["name"] for c in CASES]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------


def _vals(rng, shape, scale=1.0):
    """O(1) values away from zero: +-[0.25, 1) * scale, as fp32."""
    v = rng.uniform(0.25, 1.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return (v * scale).astype(np.float32)


def _round_to(a: np.ndarray, dtype) -> np.ndarray:
    """fp32 array rounded once to ``dtype`` (a torch 16-bit type), as fp32."""
    if dtype is None or dtype == torch.float32:
        return a.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def io_dtype(c):
    return TORCH16[KINDS[c["kind"]]] if c["io16"] else torch.float32


def out_shapes(c):
    """[(channels, time)] of out0 (and out1)."""
    if c["epi"] == "up":
        return [(c["m"] // c["up"][1], c["t_out"])]
    if c["epi"] == "gate":
        return [(c["m"] // 2, c["n_out"])] + ([(c["m"], c["n_out"])] if c["gate_pre"] else [])
    if c["epi"] == "store2":
        return [(c["split"], c["n_out"]), (c["m"] - c["split"], c["n_out"])]
    return [(c["m"], c["n_out"])]


def guard_post(c) -> int:
    return -c["m"] % 128 + GUARD_C


def make_inputs(c) -> dict:
    """Logical (unpadded) operands of a case as numpy fp32 arrays, values
    O(1): |w| sums to <= 2 per output so that |pre-activation| <= 3."""
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    B, cin, m, k = c["B"], c["cin"], c["m"], c["k"]
    dt = io_dtype(c)
    inp = {"x": _round_to(_vals(rng, (B, cin, c["tin"])), dt)}
    if c["up"] is not None:
        K, u, _ = c["up"]
        inp["w"] = _vals(rng, (cin, m // u, K), 2.0 / (cin * k))       # ConvTranspose1d layout
        nb = m // u
    else:
        inp["w"] = _vals(rng, (m, cin, k), 2.0 / (cin * k))            # Conv1d layout
        nb = m
    inp["bias"] = _vals(rng, (nb,), 0.5) if c["bias"] else None
    inp["cond"] = _vals(rng, (B, m), 0.5) if c["cond"] else None
    shapes = out_shapes(c)
    inp["res"] = [_round_to(_vals(rng, (B,) + s), dt) for s in shapes]
    inp["y_old"] = [_round_to(_vals(rng, (B,) + s), dt) for s in shapes]
    inp["gmask"] = _round_to(_vals(rng, (B, m, c["n_out"])), dt) if c["gmask"] else None
    return inp


# ---------------------------------------------------------------------------
# float64 reference and bound
# ---------------------------------------------------------------------------


def operands64(c, inp):
    """(x', w) as float64: the prologue in fp32, 16-bit kinds rounded to type."""
    x = inp["x"].astype(np.float32)
    xp = np.where(x > 0, x, x * np.float32(c["in_slope"])).astype(np.float32)
    w = inp["w"].astype(np.float32)
    wdt = KINDS[c["kind"]]
    if wdt in TORCH16:
        xp, w = _round_to(xp, TORCH16[wdt]), _round_to(w, TORCH16[wdt])
    return xp.astype(np.float64), w.astype(np.float64)


def _conv64(c, xp, w, drop_tap=None):
    """acc[b][row][n] = sum_{c,j} w[row][c][j] x'[b][c][n - pad_left + j*dil]
    over logical rows (Conv1d layout), x' zero outside [0, tin)."""
    B, k, dil, pad, n_out, tin = c["B"], c["k"], c["dil"], c["pad_left"], c["n_out"], c["tin"]
    lo = min(0, -pad)
    hi = max(tin, n_out - pad + (k - 1) * dil)
    xz = np.zeros((B, xp.shape[1], hi - lo), dtype=xp.dtype)
    xz[:, :, -lo:-lo + tin] = xp
    acc = np.zeros((B, w.shape[0], n_out), dtype=xp.dtype)
    for j in range(k):
        if j == drop_tap:
            continue
        s = -pad + j * dil - lo
        acc += np.matmul(w[None, :, :, j], xz[:, :, s:s + n_out])
    return acc


def _convT64(c, xp, w, drop_tap=None):
    """Transposed convolution by its definition: y[b][o][q*u - pad + kk] +=
    w[c][o][kk] x'[b][c][q], kept for the GEMM columns n = (t + pad) // u <
    n_out the launch computes (every t when n_out is make_desc's default)."""
    K, u, pad = c["up"]
    B, tin, t_out = c["B"], c["tin"], c["t_out"]
    y = np.zeros((B, w.shape[1], t_out), dtype=xp.dtype)
    q = np.arange(tin)
    for kk in range(K):
        if drop_tap is not None and kk // u == (K // u - 1 - drop_tap):
            continue                              # polyphase tap j' = K/u - 1 - kk // u
        t = q * u - pad + kk
        ok = (t >= 0) & (t < t_out) & ((t + pad) // u < c["n_out"])
        y[:, :, t[ok]] += np.matmul(w[:, :, kk].T[None], xp[:, :, ok])
    return y


def coef(c) -> float:
    K = c["cin"] * c["k"]
    if KINDS[c["kind"]] in (WDT_F32S, WDT_F32P):
        return 6 * K * U + 2.0 ** -22
    return 2 * K * U


def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _half_ulp16(v, e, dtype):
    a = np.maximum(np.abs(v) + e, 2.0 ** -126)
    ex = np.floor(np.log2(a))
    if dtype == torch.bfloat16:
        return 0.5 * 2.0 ** (ex - 7)
    return 0.5 * 2.0 ** (np.maximum(ex, -14) - 10)


def _epilogue(c, v, e, side, inp, lengths, *, act, accumulate, res, gmask=None):
    """act -> gmask -> res + res_scale*v -> accumulate -> post_div -> mask; the
    error is scaled by each step's slope."""
    if act == ACT_RELU:
        v = np.maximum(v, 0.0)
    elif act == ACT_TANH:
        v = np.tanh(v)
    elif act == ACT_EXP:
        e = e * np.exp(v)
        v = np.exp(v)
    if gmask is not None:
        f = np.where(gmask > 0, 1.0, 0.1)
        v, e = v * f, e * np.abs(f)
    if res:
        r = inp["y_old"][side] if c["res_alias"] else inp["res"][side]
        v, e = r.astype(np.float64) + c["res_scale"] * v, e * abs(c["res_scale"])
    if accumulate:
        v = inp["y_old"][side].astype(np.float64) + v
    if c["post_div"] != 1.0 and side == 0:
        v, e = v / c["post_div"], e / c["post_div"]
    e = e + 4 * _ulp32(v)
    if c["io16"]:
        e = e + _half_ulp16(v, e, io_dtype(c))
    if lengths is not None:
        t = np.arange(v.shape[2])[None, None, :]
        dead = t >= np.asarray(lengths)[:, None, None]
        v, e = np.where(dead, 0.0, v), np.where(dead, 0.0, e)
    return v, e


def abs_conv(c, operands):
    """A without the bias / cond terms: conv(|x'|, |w|)."""
    xp, w = operands
    return (_convT64 if c["up"] is not None else _conv64)(c, np.abs(xp), np.abs(w))


def reference(c, inp, *, drop_tap=None, operands=None, A=None):
    """[(ref, bound)] per output, float64 [B, channels, time].  ``drop_tap``
    leaves one tap out of the sum (the mutation the bound must catch);
    ``operands`` / ``A`` reuse operands64 / abs_conv of an earlier call."""
    xp, w = operands if operands is not None else operands64(c, inp)
    conv = _convT64 if c["up"] is not None else _conv64
    acc = conv(c, xp, w, drop_tap)
    if A is None:
        A = abs_conv(c, (xp, w))
    bias = inp["bias"].astype(np.float64)[None, :, None] if inp["bias"] is not None else 0.0
    cond = inp["cond"].astype(np.float64)[:, :, None] if inp["cond"] is not None else 0.0
    L = c["lengths"]
    cf = coef(c)
    if c["epi"] == "up":                          # (cond is not applied to UPSAMPLE)
        v, e = acc + bias, cf * (A + np.abs(bias))
        return [_epilogue(c, v, e, 0, inp, L, act=c["act"], accumulate=c["accumulate"],
                          res=c["res"])]
    v, e = acc + bias + cond, cf * (A + np.abs(bias) + np.abs(cond))
    if c["epi"] == "gate":
        h = c["m"] // 2
        ta, sb = np.tanh(v[:, :h]), 1.0 / (1.0 + np.exp(-v[:, h:]))
        eg = e[:, :h] * sb + e[:, h:] * 0.25 * np.abs(ta) + 2e-7 * (sb + np.abs(ta))
        outs = [_epilogue(c, ta * sb, eg, 0, inp, L, act=c["act"], accumulate=c["accumulate"],
                          res=c["res"])]
        if c["gate_pre"]:                         # acc + bias, no cond, logical rows [a | b]
            pv, pe = acc + bias, cf * (A + np.abs(bias))
            pe = pe + 4 * _ulp32(pv)
            if c["io16"]:
                pe = pe + _half_ulp16(pv, pe, io_dtype(c))
            t = np.arange(pv.shape[2])[None, None, :]
            dead = t >= (np.asarray(L)[:, None, None] if L is not None else pv.shape[2])
            outs.append((np.where(dead, 0.0, pv), np.where(dead, 0.0, pe)))
        return outs
    if c["epi"] == "store2":
        s = c["split"]
        return [_epilogue(c, v[:, :s], e[:, :s], 0, inp, L, act=c["act"],
                          accumulate=c["accumulate"], res=c["res"]),
                _epilogue(c, v[:, s:], e[:, s:], 1, inp, L, act=c["act1"],
                          accumulate=c["accumulate1"], res=False)]
    return [_epilogue(c, v, e, 0, inp, L, act=c["act"], accumulate=c["accumulate"], res=c["res"],
                      gmask=inp["gmask"])]


def untouched_columns(c, plan):
    """[B, time] bool: output columns a len_skip launch must leave as they
    were - those of tiles that start at or past lengths[b] + len_skip (tile
    width from the plan; UPSAMPLE tiles start at time n0 * u - up_pad)."""
    T = out_shapes(c)[0][1]
    keep = np.zeros((c["B"], T), dtype=bool)
    if not (c["lengths"] and c["len_skip"] > 0):
        return keep
    bn = plan["bn"]
    n = np.arange(c["n_out"])
    n0 = n // bn * bn
    for b, ln in enumerate(c["lengths"]):
        if c["up"] is not None:
            _, u, pad = c["up"]
            skipped = n0 * u - pad >= ln + c["len_skip"]
            for ph in range(u):
                t = n * u + ph - pad
                ok = skipped & (t >= 0) & (t < T)
                keep[b, t[ok]] = True
        else:
            keep[b, n[n0 >= ln + c["len_skip"]]] = True
    return keep


# ---------------------------------------------------------------------------
# layers and descriptors
# ---------------------------------------------------------------------------


def pack_layer(c, inp, device):
    """The case's layer through ops.pack_conv / pack_conv_transpose; a forced
    tile re-packs it with the library's own chunk pickers."""
    wdt = KINDS[c["kind"]]
    w = torch.from_numpy(inp["w"]).to(device)
    b = None if inp["bias"] is None else torch.from_numpy(inp["bias"]).to(device)
    if c["up"] is not None:
        base = ops.pack_conv_transpose(w, b, c["up"][1], c["up"][2])
    else:
        base = ops.pack_conv(w, b, dilation=c["dil"], padding=c["pad_left"],
                             gate=c["epi"] == "gate")
    assert base.wdtype == WDT_F32
    tile = TILES[c["tile"]] if c["tile"] else None
    if wdt == WDT_F32:
        if tile is None or tile == base.tile:
            return base
        kc = ops._pick_kc(c["cin"], c["k"], c["dil"], tile)
        cin_pad = -(-c["cin"] // kc) * kc
        wp = base.w.new_zeros(cin_pad, base.w.shape[1], base.w.shape[2])
        wp[:c["cin"]] = base.w[:c["cin"]]
        return dataclasses.replace(base, w=wp, tile=tile, kc=kc)
    old = ops.SPLIT_W
    ops.SPLIT_W = wdt != WDT_F32S
    try:
        layer = ops.to_lowp(base, WDT_F32S if wdt == WDT_F32P else wdt, min_rows=0)
    finally:
        ops.SPLIT_W = old
    assert layer.wdtype == wdt
    if tile is not None and tile != layer.tile:
        kc = ops._kc_f32p(layer.cin_pad, c["k"], c["dil"], tile) if wdt == WDT_F32P else 16
        layer = dataclasses.replace(layer, tile=tile, kc=kc)
    if c["io16"]:
        layer = dataclasses.replace(layer, kc=ops.io16_kc(layer))
    return layer


class Built:
    pass


def build(c, inp, device) -> Built:
    """Allocate the case's tensors on ``device`` (a CPU device serves the
    plan tests: the plan reads no memory) and build its descriptor.  Inputs
    are interior views of NaN-filled allocations, outputs of sentinel-filled
    ones."""
    bt = Built()
    dt = io_dtype(c)
    B, cin, tin = c["B"], c["cin"], c["tin"]
    layer = pack_layer(c, inp, device)
    bt.layer = layer
    # ---- x: NaN around the valid [cin][tin] block of every utterance ----------
    x_log = torch.from_numpy(inp["x"]).to(dt).to(device)
    tp = c["x_tpad"]
    if c["time_major"]:
        # [B][tp + tin + tp][X_PRE_C + cin + X_POST_C], element (b, ch, t) at
        # t * C + ch: x_cstride = 1, x_tstride = C
        xbig = torch.full((B, tin + 2 * tp, X_PRE_C + cin + X_POST_C), float("nan"), dtype=dt,
                          device=device)
        xbig[:, tp:tp + tin, X_PRE_C:X_PRE_C + cin] = x_log.permute(0, 2, 1)
        xv = xbig[:, tp:tp + tin].permute(0, 2, 1)          # [B][Call][tin], strides (., 1, C)
    else:
        # rows long enough that every masked column a tile could name still
        # lies inside the allocation; x_cstride % 4 == x_tpad % 4
        trow = (tin + 512 + (c["k"] - 1) * c["dil"] + 19) // 4 * 4 + tp % 4
        xbig = torch.full((B, X_PRE_C + cin + X_POST_C, trow), float("nan"), dtype=dt,
                          device=device)
        # (the valid block starts 256 columns in: at a multiple of 4, + x_off)
        t0 = 256 + c["x_off"]
        xbig[:, X_PRE_C:X_PRE_C + cin, t0:t0 + tin] = x_log
        xv = xbig[:, :, t0:t0 + tin]
    bt.xbig = xbig
    # ---- outputs -------------------------------------------------------------
    sent = SENTINEL
    bt.ybig, bt.yview, outs = [], [], []
    shapes = out_shapes(c)
    prefill = [c["accumulate"] or (c["res"] and c["res_alias"]),
               c["accumulate1"] if c["epi"] == "store2" else False]
    for i, (C_, T_) in enumerate(shapes):
        yp = c["y_tpad"]
        big = torch.full((B, GUARD_C + C_ + guard_post(c), T_ + 2 * yp), sent, dtype=dt,
                         device=device)
        view = big[:, :, yp:yp + T_]
        if prefill[i]:
            view[:, GUARD_C:GUARD_C + C_] = torch.from_numpy(inp["y_old"][i]).to(dt).to(device)
        bt.ybig.append(big)
        bt.yview.append(view)
    bt.res = None
    res_t = None
    if c["res"]:
        if c["res_alias"]:
            res_t = bt.yview[0]
        else:
            C_, T_ = shapes[0]
            rbig = torch.full((B, C_ + 2 * GUARD_C, T_ + 2), float("nan"), dtype=dt, device=device)
            rbig[:, GUARD_C:GUARD_C + C_, 1:1 + T_] = torch.from_numpy(inp["res"][0]).to(dt).to(device)
            bt.res = rbig
            res_t = rbig[:, :, 1:1 + T_]
    o0 = ops.make_out(bt.yview[0], act=c["act"], res=res_t, res_scale=c["res_scale"],
                      accumulate=c["accumulate"], post_div=c["post_div"], channel_offset=GUARD_C)
    o1 = None
    if len(shapes) > 1:
        o1 = ops.make_out(bt.yview[1], act=c["act1"], accumulate=c["accumulate1"],
                          channel_offset=GUARD_C)
    bt.cond = None
    if c["cond"]:
        # [B][m + 3]: a batch stride wider than the row
        bt.cond = torch.full((B, c["m"] + 3), float("nan"), device=device)
        bt.cond[:, :c["m"]] = torch.from_numpy(inp["cond"]).to(device)
    bt.lengths = None
    if c["lengths"] is not None:
        bt.lengths = torch.tensor(c["lengths"], dtype=torch.int32, device=device)
    d = ops.make_desc(layer, xv, o0, out1=o1, split=c["split"] if c["epi"] == "store2" else None,
                      tin=tin, n_out=c["n_out"], in_slope=c["in_slope"], cond=bt.cond,
                      lengths=bt.lengths, t_out=c["t_out"] or 0, x_channel_offset=X_PRE_C,
                      io16=c["io16"])
    d.len_skip = c["len_skip"]
    bt.gmask = None
    if c["gmask"]:
        bt.gmask = torch.from_numpy(inp["gmask"]).to(dt).to(device).contiguous()
        d.gmask = bt.gmask.data_ptr()
        d.gmask_bstride = bt.gmask.stride(0)
        d.gmask_cstride = bt.gmask.stride(1)
        d.gmask_slope = 0.1
    bt.desc = d
    return bt


# ---------------------------------------------------------------------------
# CPU stand-ins for the kernels' arithmetic (validation of the bound)
# ---------------------------------------------------------------------------


def split3(a32: np.ndarray):
    """conv1d_impl.h split3_bf16 on the host: (hi, mid, lo) fp32 arrays holding
    bf16 values, hi + mid + lo == a exactly."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    h = (a32.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r = a32 - h
    m = (r.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    return h, m, (r - m).astype(np.float32)


def conv_fp32_sequential(c, xp32, w32, split: bool):
    """The case's GEMM accumulated in fp32, term by term over (channel, tap):
    ``split`` = the six kept products (hh, hm, mh, mm, hl, lh) of the split-fp32
    kernels, each exact in fp32; else the plain fp32 product."""
    B, k, dil, pad, n_out, tin = c["B"], c["k"], c["dil"], c["pad_left"], c["n_out"], c["tin"]
    lo = min(0, -pad)
    hi = max(tin, n_out - pad + (k - 1) * dil)
    xz = np.zeros((B, xp32.shape[1], hi - lo), dtype=np.float32)
    xz[:, :, -lo:-lo + tin] = xp32
    xs = split3(xz) if split else (xz,)
    ws = split3(w32) if split else (w32.astype(np.float32),)
    pairs = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)) if split else ((0, 0),)
    acc = np.zeros((B, w32.shape[0], n_out), dtype=np.float32)
    for ch in range(xp32.shape[1]):
        for j in range(k):
            s = -pad + j * dil - lo
            for a, b in pairs:
                acc += ws[a][None, :, ch, j, None] * xs[b][:, None, ch, s:s + n_out]
    return acc

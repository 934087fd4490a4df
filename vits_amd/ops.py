"""Tensor-level wrappers over the C-ABI (libvits_amd.so).

Every function here requires CUDA(ROCm) tensors and launches HIP kernels on
the current torch stream; there is no CPU path (a CPU tensor raises).
Weight packing helpers turn reference-layout conv weights into the
``[cin_pad][k][m_pad]`` slabs the MFMA conv kernel streams.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import threading
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_NONE, WDT_BF16, WDT_F16, WDT_F32, WDT_F32P, WDT_F32S, ConvDesc, ConvOut, EPI_GATE, EPI_STORE,
                   ResblockPairDesc, WnLayerDesc,
                   EPI_UPSAMPLE, TILE_128x128, TILE_32x256, TILE_64x128, TILE_64x256, TILE_ROWS,
                   check)

# ---------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device(*tensors: torch.Tensor):
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise _lib.VitsAmdError(
                "vits_amd HIP ops need tensors on a ROCm GPU (device 'cuda'); "
                f"got {t.device}. There is no CPU path.")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_WEIGHT_CACHE: dict = {}


def set_weight_cache(cache: dict) -> dict:
    """Install ``{module: effective weight}`` (wnorm.WeightNormCache.active:
    every weight-normed layer of a network computed in one launch); returns
    the previous mapping."""
    global _WEIGHT_CACHE
    prev, _WEIGHT_CACHE = _WEIGHT_CACHE, cache
    return prev


def cached_weight(module: torch.nn.Module):
    return _WEIGHT_CACHE.get(module)


def weight_norm_effective(module: torch.nn.Module, name: str = "weight") -> torch.Tensor:
    """Effective weight of a (legacy) weight-normed or plain layer."""
    w = _WEIGHT_CACHE.get(module) if name == "weight" else None
    if w is not None:
        return w
    g = getattr(module, name + "_g", None)
    v = getattr(module, name + "_v", None)
    if g is not None and v is not None:
        return torch._weight_norm(v, g, 0)
    return getattr(module, name)


# ---------------------------------------------------------------------------
# conv layer packing
# ---------------------------------------------------------------------------


def _pick_tile(m: int, k: int) -> int:
    """fp32 workgroup tile by GEMM rows and taps, from the per-shape sweep of
    tools/conv_bench.py on MI355X (B=16, Ty=500 decoder/flow shapes, 16-byte
    X staging): 32 rows -> 32x256; the 2-tap polyphase ups and 1x1 convs ->
    64x128; everything else -> 64x256 (k=3: +3..5 %, k=7: +6 %, k=11: +5 %
    over 128x128 / 64x128).  Grids too small to fill the chip twice fall back
    to 64x128 at launch (conv1d.hip)."""
    if m <= 32:
        return TILE_32x256
    if k <= 2:
        return TILE_64x128
    return TILE_64x256


def _pick_tile_bf16(m: int, k: int) -> int:
    """bf16-MFMA tile (same sweep, BF=1): short kernels on >= 128 rows are
    fastest as 128x128 (k=3: 430 vs 340 TF/s), long ones as 64x256
    (k=11: 730 vs 555), 64-row k<=7 as 64x128, 32 rows as 32x256."""
    if m <= 32:
        return TILE_32x256
    if k <= 3:
        return TILE_128x128 if m >= 128 else TILE_64x128
    if m >= 128 or k >= 9:
        return TILE_64x256
    return TILE_64x128


TILE_COLS = {TILE_128x128: 128, TILE_64x256: 256, TILE_32x256: 256, TILE_64x128: 128}
W_TILE_FLOATS = 4096                                   # conv1d.hip VITS_W_TILE
X_TILE_FLOATS = {128: 2048, 256: 4096}                  # conv1d.hip XTile<BN>::floats


# workgroups per CU each tile reaches by its VGPR count (ISA dump of
# conv1d.hip: 128x128 154 VGPRs -> 3 waves/SIMD, 64x256 / 32x256 ~122 -> 4,
# 64x128 89 -> 5; 64x256 is budgeted at 3: its k=7 convs run faster with the
# bigger chunk); the K-chunk is sized so that LDS does not cut this further
TILE_OCCUPANCY = {TILE_128x128: 3, TILE_64x256: 3, TILE_32x256: 4, TILE_64x128: 5}
LDS_BYTES_PER_CU = 160 * 1024


def _pick_kc(cin: int, k: int, dil: int, tile: int) -> int:
    """Input channels per K-chunk: the largest even kc within the kernel's
    per-stage LDS/register budgets (W chunk kc*k*BM floats, X chunk
    kc*xw_pad floats) AND within the LDS share that keeps the tile's VGPR
    occupancy (the conv is latency-bound at small K: on MI355X a 64x128 k=3
    conv runs 86 TF/s at kc=10 / 5 WGs per CU but 77 TF/s at kc=14 / 4)."""
    bm, bn = TILE_ROWS[tile], TILE_COLS[tile]
    # + 4: the 16-byte staging path aligns the window start down to 4 columns
    xw_pad = (bn + (k - 1) * dil + 3) // 4 * 4 + 4
    lds_fixed = 4 * (2 * k * bm + 2 * xw_pad + 64)
    lds_floats = (LDS_BYTES_PER_CU // TILE_OCCUPANCY[tile] - lds_fixed) // 8  # per stage, W+X
    occ_kc = lds_floats // (k * bm + xw_pad)
    occ_kc = max(occ_kc, 2 * -(-12 // k))  # but keep >= ~24 taps x channels per chunk
    budget = min(32, W_TILE_FLOATS // (k * bm), X_TILE_FLOATS[bn] // xw_pad, occ_kc,
                 cin + (cin & 1))
    budget = max(2, budget - (budget & 1))
    # zero-padded channels cost MFMA work, each chunk costs a fixed overhead
    # (~2 channels' worth): minimise ceil(cin/kc) * (kc + 2)
    kc = min(range(2, budget + 1, 2), key=lambda c: (-(-cin // c) * (c + 2), -(-cin // c) * c, -c))
    assert kc * k * bm <= W_TILE_FLOATS and kc * xw_pad <= X_TILE_FLOATS[bn], (cin, k, dil, tile)
    return kc


@dataclass
class PackedConv:
    """A conv (or polyphase conv-transpose) lowered for vits_conv1d_forward."""

    w: torch.Tensor            # [cin_pad, k, m_pad] fp32 contiguous
    bias: Optional[torch.Tensor]
    cin: int
    m: int                     # GEMM rows
    k: int
    dil: int
    pad_left: int
    epi: int
    tile: int
    kc: int
    up_u: int = 1
    up_pad: int = 0
    out_channels: int = 0      # channels of the produced tensor
    extra: dict = field(default_factory=dict)
    wdtype: int = WDT_F32      # WDT_BF16 / WDT_F16: w is [cin_pad/16][k][2][m_pad][8] 16-bit
                               # (16-channel slabs; a K-chunk of kc channels = kc/16 slabs)

    @property
    def m_pad(self) -> int:
        if self.wdtype == WDT_F32P:
            return self.w.shape[4]
        return self.w.shape[3] if self.wdtype != WDT_F32 else self.w.shape[2]

    @property
    def cin_pad(self) -> int:
        return self.w.shape[0] * 16 if self.wdtype != WDT_F32 else self.w.shape[0]


def _finish_pack(rows_w: torch.Tensor, k: int, tile: int, dil: int = 1) -> tuple[torch.Tensor, int]:
    """rows_w: [m, cin, k] -> packed [cin_pad, k, m_pad]."""
    m, cin, _ = rows_w.shape
    kc = _pick_kc(cin, k, dil, tile)
    cin_pad = (cin + kc - 1) // kc * kc
    m_pad = (m + 127) // 128 * 128
    packed = rows_w.new_zeros(cin_pad, k, m_pad, dtype=torch.float32)
    packed[:cin, :, :m] = rows_w.permute(1, 2, 0).to(torch.float32)
    return packed.contiguous(), kc


class _PackPrecision(threading.local):
    wdtype = WDT_F32


PACK_PRECISION = _PackPrecision()
_WDT_TORCH = {WDT_BF16: torch.bfloat16, WDT_F16: torch.float16}


@contextlib.contextmanager
def pack_lowp(wdtype: int = WDT_BF16):
    """While active, pack_conv / pack_conv_transpose return 16-bit-MFMA layers
    (WDT_BF16 or WDT_F16; WDT_F32 = exact fp32).  Engine plans of a bf16 /
    fp16 model are built under it."""
    old = PACK_PRECISION.wdtype
    PACK_PRECISION.wdtype = int(wdtype)
    try:
        yield
    finally:
        PACK_PRECISION.wdtype = old


def pack_bf16(enabled: bool = True):
    return pack_lowp(WDT_BF16 if enabled else WDT_F32)


def _pick_tile_f32s(m: int, k: int) -> int:
    """Split-fp32 tile (VITS_WDT_F32S), from the per-shape sweep of
    tools/conv_bench.py (WDT=3 TILES=0,1,2,3) on MI355X at B=16, Ty=500
    (profiles/r02_split_conv_sweep.txt): k = 3 on >= 128 rows -> 128x128
    (W pre-split too, 131-140 TF/s), k <= 8 otherwise -> 64x128 (k=7
    147-159, the polyphase upsamplers 111-117, conv_pre 135, flow k=5 133),
    k >= 9 -> 64x256 (k=11 145-158)."""
    if k == 3 and m >= 128:
        return TILE_128x128
    if k <= 8:
        return TILE_64x128
    return TILE_64x256


def _pick_tile_f32p(m: int, k: int) -> int:
    """Tile of the pre-split-weight kernel (VITS_WDT_F32P): W is read from
    global memory, so the LDS holds only the double-buffered window and
    128x128 (2x2 waves of 64x64: two A and two B fragment triples feed 24
    MFMAs per k-step) fits every decoder shape; grids too small to fill the
    chip twice fall back to 64x128 in the dispatcher."""
    return TILE_128x128 if m >= 128 else TILE_64x128


# channels per K-chunk of the pre-split kernel: 32 (two slabs, half the
# chunk barriers) when the window of a 32-channel chunk fits the staging
# budget (conv1d_impl.h XTile<BN, true, true>: 6144 / 10240 elements for 128
# / 256 columns), else 16; F32P_MAX_KC = 16 forces single slabs
F32P_MAX_KC = 32


def _kc_f32p(cin_pad: int, k: int, dil: int, tile: int) -> int:
    if tile == TILE_64x128:
        # 64-row layers (the 64-channel decoder stage): 16-channel chunks halve
        # the double-buffered window (3 instead of 2 workgroups per CU);
        # measured on MI355X (tools/conv_bench.py WDT=3, r03): c1 k=3/7/11
        # +15/+8/+3 %, c2 +12..17 % over 32-channel chunks.  A 1x1 layer's
        # window is one tile wide, and its chunks are latency-bound: 32
        # channels (the flow's 96-row post conv: 29.5 -> 21.6 us, r06; the
        # k-steps and so the accumulation order are the same either way)
        return 32 if (k == 1 and cin_pad % 32 == 0) else 16
    bn = TILE_COLS[tile]
    xrs = (bn + (k - 1) * dil + 3 + 3) // 4 * 4  # window row incl. the 16-byte alignment shift
    budget = 6144 if bn <= 128 else 10240
    if F32P_MAX_KC >= 32 and cin_pad % 32 == 0 and 32 * xrs <= budget:
        return 32
    return 16


# pre-split weights for split fp32 (False: the F32S kernel, which
# splits the fp32 weight slabs per fragment in registers)
SPLIT_W = True


def split_planes(w: torch.Tensor) -> torch.Tensor:
    """Exact three-term bf16 split of an fp32 tensor, stacked on a new
    dimension -4 as (hi, mid, lo) planes: hi = x truncated to bf16, mid =
    (x - hi) truncated, lo = x - hi - mid (<= 8 significant bits), so
    hi + mid + lo == x bit for bit - conv1d_impl.h split3_bf16 on the host."""
    w = w.to(torch.float32).contiguous()
    mask = -65536  # (a Python scalar: no host-to-device copy, graph-capture safe)
    h = (w.view(torch.int32) & mask).view(torch.float32)
    # (a non-finite weight keeps mid = lo = 0: inf - inf would make them NaN;
    # a NaN stays NaN in hi even when its payload sits in the truncated bits)
    h = torch.where(torch.isnan(w), w, h)
    r = torch.where(torch.isfinite(w), w - h, torch.zeros_like(w))
    m = (r.view(torch.int32) & mask).view(torch.float32)
    lo = r - m
    return torch.stack([h, m, lo], dim=-3).to(torch.bfloat16)


# Split-fp32 layers need >= this many GEMM rows: the r02 sweep measured the
# per-fragment split (F32S) ahead of the exact-f32 kernel on every 128- /
# 256-channel decoder conv (+8..35 %), the upsamplers, conv_pre and the flow,
# but behind it on the 32- / 64-channel stages.  With pre-split weights
# (F32P, tools/conv_bench.py on MI355X, r03) the 64-channel stage gains too
# (k=11 c1 180 vs 122 TF/s exact, c2 138 vs 107, k=7 c1 154 vs 104; k=3 c2
# 56 vs 60), the 32-channel one still does not (k=11 92 vs 108): 64 rows.
F32S_MIN_ROWS = 0


def _f32s_min_rows() -> int:
    return F32S_MIN_ROWS or (64 if SPLIT_W else 128)


def to_lowp(layer: PackedConv, wdtype: int = WDT_BF16, min_rows: Optional[int] = None) -> PackedConv:
    """Re-pack an fp32 layer for the 16-bit-MFMA kernel variant (bf16 or
    fp16 operands, fp32 accumulation): K-chunks of 16 channels, W as
    [cin_pad/16][k][2][m_pad][8] (one 16-byte A fragment per row and 8
    channels), tile by _pick_tile_bf16.  WDT_F32S keeps that slab image in
    fp32 (split into three exact bf16 terms inside the kernel)."""
    if layer.wdtype != WDT_F32 or wdtype == WDT_F32:
        return layer
    if wdtype == WDT_F32S:
        # (min_rows: the fused split-fp32 pairs take the 32-row convs too)
        if layer.m < (_f32s_min_rows() if min_rows is None else min_rows):
            return layer
        kc = 16
        w32 = layer.w[:layer.cin]
        cin_pad = (layer.cin + kc - 1) // kc * kc
        k, m_pad = w32.shape[1], w32.shape[2]
        w = w32.new_zeros(cin_pad, k, m_pad)
        w[:layer.cin] = w32
        w = w.view(cin_pad // kc, kc // 8, 8, k, m_pad).permute(0, 3, 1, 4, 2).contiguous()
        if SPLIT_W:
            # [cin_pad/16][k][2][3][m_pad][8] bf16: planes next to the lane half
            tile = _pick_tile_f32p(layer.m, layer.k)
            return PackedConv(split_planes(w), layer.bias, layer.cin, layer.m, layer.k,
                              layer.dil, layer.pad_left, layer.epi, tile,
                              _kc_f32p(cin_pad, layer.k, layer.dil, tile), up_u=layer.up_u,
                              up_pad=layer.up_pad, out_channels=layer.out_channels,
                              extra=layer.extra, wdtype=WDT_F32P)
        return PackedConv(w, layer.bias, layer.cin, layer.m, layer.k, layer.dil,
                          layer.pad_left, layer.epi, _pick_tile_f32s(layer.m, layer.k), kc,
                          up_u=layer.up_u, up_pad=layer.up_pad,
                          out_channels=layer.out_channels, extra=layer.extra, wdtype=wdtype)
    kc = 16
    w32 = layer.w[:layer.cin]                          # [cin, k, m_pad]
    cin_pad = (layer.cin + kc - 1) // kc * kc
    k, m_pad = w32.shape[1], w32.shape[2]
    w = w32.new_zeros(cin_pad, k, m_pad)
    w[:layer.cin] = w32
    w = w.view(cin_pad // kc, kc // 8, 8, k, m_pad).permute(0, 3, 1, 4, 2).contiguous()
    tile = _pick_tile_bf16(layer.m, layer.k)
    return PackedConv(w.to(_WDT_TORCH[wdtype]), layer.bias, layer.cin, layer.m, layer.k,
                      layer.dil, layer.pad_left, layer.epi, tile, kc, up_u=layer.up_u,
                      up_pad=layer.up_pad, out_channels=layer.out_channels, extra=layer.extra,
                      wdtype=wdtype)


# K-chunk of 16-bit inference layers whose activations are 16-bit too
# (engine.ACT16): the X window of a chunk stages at 2 bytes per element, so a
# chunk can hold 32-64 channels instead of 16 (fewer barriers per tile).
# VITS_LOWP_KCK caps kc * k (16: keep kc = 16, for A/B).
LOWP_KCK = 512


def io16_kc(layer: PackedConv) -> int:
    """Largest kc in (64, 48, 32, 16) dividing cin_pad that fits the kernel's
    W stage (kc*k*BM/2 <= 6144 slots, for the LDS-weight groups) and the
    16-bit X budget (conv1d_impl.h XTile<BN, BF, true>: 6144 / 10240
    elements for BN 128 / 256)."""
    bm, bn = TILE_ROWS[layer.tile], TILE_COLS[layer.tile]
    xrs = bn + (layer.k - 1) * layer.dil + 8
    xbudget = 6144 if bn <= 128 else 10240
    for kc in (64, 48, 32):
        if (kc * layer.k <= LOWP_KCK and layer.cin_pad % kc == 0
                and kc * layer.k * bm // 2 <= 6144 and kc * xrs <= xbudget):
            return kc
    return 16


def to_bf16(layer: PackedConv) -> PackedConv:
    return to_lowp(layer, WDT_BF16)


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], *, dilation: int = 1,
              padding: Optional[int] = None, gate: bool = False) -> PackedConv:
    """nn.Conv1d weight [Cout, Cin, k].  ``gate``: rows (a_p, b_p) interleaved
    so the tanh/sigmoid pair of output p lands in one lane (EPI_GATE)."""
    w = weight.detach().to(torch.float32)
    cout, cin, k = w.shape
    if padding is None:
        padding = (k * dilation - dilation) // 2
    if gate:
        assert cout % 2 == 0
        h = cout // 2
        rows = torch.stack([w[:h], w[h:]], dim=1).reshape(cout, cin, k)
        epi, outc = EPI_GATE, h
    else:
        rows, epi, outc = w, EPI_STORE, cout
    tile = _pick_tile(cout, k)
    packed, kc = _finish_pack(rows, k, tile, dilation)
    b = None if bias is None else bias.detach().to(torch.float32).contiguous()
    layer = PackedConv(packed, b, cin, cout, k, dilation, padding, epi, tile, kc,
                       out_channels=outc)
    return to_lowp(layer, PACK_PRECISION.wdtype)


def pack_conv_transpose(weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int,
                        padding: int) -> PackedConv:
    """nn.ConvTranspose1d weight [Cin, Cout, K] (K % stride == 0) as one
    polyphase conv: GEMM row (o*u + r) holds phase r of output channel o,
    tap j' reads x[q - (K/u - 1) + j'] with W'[(o,r)][c][j'] = W[c][o][(K/u-1-j')u + r]."""
    w = weight.detach().to(torch.float32)
    cin, cout, K = w.shape
    u = stride
    assert K % u == 0, "polyphase lowering needs kernel_size % stride == 0"
    kp = K // u
    # W[c][o][i*u + r] -> [c][o][i][r]
    w4 = w.reshape(cin, cout, kp, u)
    # rows (o, r), taps j' = kp-1-i
    rows = w4.flip(2).permute(1, 3, 0, 2).reshape(cout * u, cin, kp)
    tile = _pick_tile(cout * u, kp)
    packed, kc = _finish_pack(rows, kp, tile)
    b = None if bias is None else bias.detach().to(torch.float32).contiguous()
    layer = PackedConv(packed, b, cin, cout * u, kp, 1, kp - 1, EPI_UPSAMPLE, tile, kc,
                       up_u=u, up_pad=padding, out_channels=cout)
    return to_lowp(layer, PACK_PRECISION.wdtype)


# ---------------------------------------------------------------------------
# conv descriptor construction / launch
# ---------------------------------------------------------------------------


def make_out(y: torch.Tensor, *, act: int = ACT_NONE, res: Optional[torch.Tensor] = None,
             res_scale: float = 1.0, accumulate: bool = False, post_div: float = 1.0,
             channel_offset: int = 0) -> ConvOut:
    o = ConvOut()
    o.y = y.data_ptr() + y.element_size() * channel_offset * y.stride(1)
    o.y_bstride = y.stride(0)
    o.y_cstride = y.stride(1)
    o.act = act
    if res is not None:
        o.res = res.data_ptr() + res.element_size() * channel_offset * res.stride(1)
        o.res_bstride = res.stride(0)
        o.res_cstride = res.stride(1)
    else:
        o.res = None
        o.res_bstride = 0
        o.res_cstride = 0
    o.res_scale = res_scale
    o.accumulate = 1 if accumulate else 0
    o.post_div = post_div
    return o


_LOWP_TORCH = {WDT_F16: torch.float16, WDT_BF16: torch.bfloat16}


class _LenSkip(threading.local):
    margin = 0


LEN_SKIP = _LenSkip()


@contextlib.contextmanager
def length_skip(margin: int = 64):
    """While active, descriptors built with ``lengths`` skip every tile that
    starts ``margin`` or more positions past lengths[b] (no compute, no
    write; vits_conv1d_desc.len_skip): the bucketed whole-utterance infer
    then costs what the utterance needs, not what the bucket holds.
    ``margin`` must exceed every consumer's input halo ((k - 1) * dil / 2 <=
    25 in the decoder)."""
    old = LEN_SKIP.margin
    LEN_SKIP.margin = int(margin)
    try:
        yield
    finally:
        LEN_SKIP.margin = old


def make_desc(layer: PackedConv, x: torch.Tensor, out0: ConvOut, *, out1: Optional[ConvOut] = None,
              split: Optional[int] = None, tin: Optional[int] = None, n_out: Optional[int] = None,
              in_slope: float = 1.0, cond: Optional[torch.Tensor] = None, cond_offset: int = 0,
              lengths: Optional[torch.Tensor] = None, t_out: int = 0,
              x_channel_offset: int = 0, io16: bool = False) -> ConvDesc:
    """io16: x / outputs / residuals / gmask are tensors of the layer's
    16-bit operand type - 1 (True) the fp16 training convs, 2 the 16-bit
    inference decoder (csrc/conv1d.hip ga16); fp32 otherwise."""
    if io16:
        assert layer.wdtype != WDT_F32 and x.dtype == _LOWP_TORCH[layer.wdtype]
    else:
        assert x.dtype == torch.float32
    d = ConvDesc()
    d.x = x.data_ptr() + x.element_size() * x_channel_offset * x.stride(1)
    d.io16 = int(io16)
    d.x_bstride = x.stride(0)
    d.x_cstride = x.stride(1)
    d.x_tstride = x.stride(2)
    d.cin = layer.cin
    d.tin = x.shape[2] if tin is None else tin
    d.in_slope = in_slope
    d.w = layer.w.data_ptr()
    d.m = layer.m
    d.m_pad = layer.m_pad
    d.cin_pad = layer.cin_pad
    d.kc = layer.kc
    d.k = layer.k
    d.dil = layer.dil
    d.pad_left = layer.pad_left
    if n_out is None:
        if layer.epi == EPI_UPSAMPLE:
            # phases q = 0 .. Tin + ceil(pad/u) - 1 cover every t in [0, Tin*u)
            n_out = d.tin + (layer.up_pad + layer.up_u - 1) // layer.up_u
        else:
            n_out = d.tin
    d.n_out = n_out
    d.tile = layer.tile
    d.epi = layer.epi
    d.bias = _ptr(layer.bias)
    if cond is not None:
        d.cond = cond.data_ptr() + 4 * cond_offset
        d.cond_bstride = cond.stride(0)
    else:
        d.cond = None
        d.cond_bstride = 0
    d.split = layer.m if split is None else split
    d.up_u = layer.up_u
    d.up_pad = layer.up_pad
    d.t_out = t_out
    d.lengths = _ptr(lengths)
    d.len_skip = LEN_SKIP.margin if lengths is not None else 0
    d.out0 = out0
    if out1 is not None:
        d.out1 = out1
    d.wdtype = layer.wdtype
    return d


def conv_flops(desc: ConvDesc, batch: int) -> int:
    """Algorithmic FLOPs of one conv launch (2 * MACs of the convolution it
    implements; for the polyphase conv-transpose: Cout * Tout * Cin * K/u)."""
    cols = desc.tin if desc.epi == EPI_UPSAMPLE else desc.n_out
    return 2 * batch * desc.m * cols * desc.cin * desc.k


# Dense MFMA peaks (MI355X_MICROARCH.md) of the arithmetic each weight type
# runs: exact fp32 on v_mfma_f32_32x32x2_f32 (157.3 TF/s); bf16 / fp16 ~2.5
# PF/s; split fp32 = six bf16 MFMAs per fp32 product, 2.5 PF / 6.
BF16_DENSE_PEAK_TFLOPS = 2500.0
MFMA_PEAK_TFLOPS = {WDT_F32: 157.3, WDT_BF16: BF16_DENSE_PEAK_TFLOPS,
                    WDT_F16: BF16_DENSE_PEAK_TFLOPS, WDT_F32S: BF16_DENSE_PEAK_TFLOPS / 6,
                    WDT_F32P: BF16_DENSE_PEAK_TFLOPS / 6}


class ConvTimer:
    """Optional per-launch timing of the conv kernel with HIP events on the
    launch stream (used by bench.py for the roofline of the dominant kernel).
    While active, batched launches are issued one descriptor at a time."""

    active = None

    def __init__(self):
        self.records = []  # (start_event, end_event, flops)
        self.shapes = []   # one label per record (tools/infer_breakdown.py)
        self.peaks = []    # MFMA-bound TFLOP/s of each record's arithmetic (MFMA_PEAK)

    def __enter__(self):
        ConvTimer.active = self
        return self

    def __exit__(self, *exc):
        ConvTimer.active = None
        return False

    def launch(self, lib, desc, batch, device):
        """One launch: a ConvDesc, or a tuple of ConvDescs run as one grid."""
        group = tuple(desc) if isinstance(desc, (tuple, list)) else (desc,)
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream(device)
        s.record(stream)
        arr = (ConvDesc * len(group))(*group)
        sizes = (C.c_int32 * 1)(len(group))
        check(lib.vits_conv1d_forward_groups(arr, sizes, 1, batch, stream.cuda_stream),
              "vits_conv1d_forward_groups")
        e.record(stream)
        self.records.append((s, e, sum(conv_flops(d, batch) for d in group)))
        self.peaks.append(MFMA_PEAK_TFLOPS[group[0].wdtype])
        self.shapes.append("conv " + "+".join(
            f"m{d.m}c{d.cin}k{d.k}d{d.dil}T{d.n_out}e{d.epi}t{d.tile}" for d in group))

    def launch_pairs(self, lib, group, batch, device, wdtype=None, mean=False):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream(device)
        s.record(stream)
        arr = (ResblockPairDesc * len(group))(*group)
        if wdtype is None:
            check(lib.vits_resblock_pair_forward(arr, len(group), batch, stream.cuda_stream),
                  "vits_resblock_pair_forward")
        elif wdtype == WDT_F32P:
            fn = (lib.vits_resblock_pair_f32p_mean_forward if mean
                  else lib.vits_resblock_pair_f32p_forward)
            check(fn(arr, len(group), batch, stream.cuda_stream),
                  "vits_resblock_pair_f32p_forward")
        else:
            fn = lib.vits_resblock_pair16_mean_forward if mean else lib.vits_resblock_pair16_forward
            check(fn(arr, len(group), batch, int(wdtype), stream.cuda_stream),
                  "vits_resblock_pair16_forward")
        e.record(stream)
        self.records.append((s, e, sum(resblock_pair_flops(d, batch) for d in group)))
        self.peaks.append(MFMA_PEAK_TFLOPS[WDT_F32 if wdtype is None else
                                           WDT_F32S if wdtype == WDT_F32P else wdtype])
        self.shapes.append("pair " + "+".join(
            f"C{d.channels}k{d.k}d{d.dil}T{d.t_len}" for d in group))

    def launch_wn(self, lib, desc, batch, device):
        """One fused WN layer: the FLOPs of the two convs it replaces, at the
        split-fp32 peak."""
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream(device)
        s.record(stream)
        check(lib.vits_wn_layers_f32p_forward(C.byref(desc), 1, batch, stream.cuda_stream),
              "vits_wn_layers_f32p_forward")
        e.record(stream)
        self.records.append((s, e, wn_layer_flops(desc, batch)))
        self.peaks.append(MFMA_PEAK_TFLOPS[WDT_F32S])
        self.shapes.append(f"wn H{desc.hidden}k{desc.k}d{desc.dil}T{desc.t_len}"
                           + ("last" if desc.last else ""))

    def summary(self):
        torch.cuda.synchronize()
        ms = [s.elapsed_time(e) for s, e, _ in self.records]
        fl = [f for _, _, f in self.records]
        # the MFMA-bound minimum time of the same launches (each at the peak
        # of the MFMA form its arithmetic runs on)
        min_ms = sum(f / (pk * 1e9) for f, pk in zip(fl, self.peaks))
        return dict(launches=len(ms), total_ms=float(sum(ms)), total_flops=int(sum(fl)),
                    avg_ms=float(sum(ms) / max(1, len(ms))), mfma_bound_ms=float(min_ms),
                    f32s_flops=int(sum(f for f, pk in zip(fl, self.peaks)
                                       if pk == MFMA_PEAK_TFLOPS[WDT_F32S])))

    def per_launch(self):
        """[(label, ms, flops)] in launch order."""
        torch.cuda.synchronize()
        return [(lab, s.elapsed_time(e), f)
                for lab, (s, e, f) in zip(self.shapes, self.records)]


# ---------------------------------------------------------------------------
# fused ResBlock2 pair (csrc/resblock.hip)
# ---------------------------------------------------------------------------
_RB_KC = {}


RESBLOCK_PAIR_MAX_K = 7


def resblock_pair_supported(c1: PackedConv, c2: PackedConv, T: int) -> bool:
    """Pairs that run fused (csrc/resblock.hip): the fp32 32- and 64-channel
    stages (C' = C, 16-byte aligned time rows) with k <= 7.  tools/rb_bench.py
    on MI355X (B=16, Ty=500): fused vs the two-conv path k=3 +6..11 %, k=7
    +0..10 %, k=11 -4..-8 % (the c1 phase recomputes the c2 halo and the
    workgroup holds the gated tile in LDS: two workgroups per CU instead of
    three) - so k=11 pairs keep the two-conv path."""
    C = c2.out_channels
    return (c1.wdtype == WDT_F32 and c2.wdtype == WDT_F32 and C in (32, 64)
            and c1.m == C and c1.cin == C and c2.cin == C // 2 and c1.k == c2.k
            and c1.k <= RESBLOCK_PAIR_MAX_K and c2.dil == 1 and T % 4 == 0
            and _resblock_kc(C, c1.k, c1.dil) is not None)


# split-fp32 fused pairs (csrc/resblock_f32p.hip): channels -> largest k that
# runs fused.  tools/rbp_bench.py on MI355X (B=16, Ty=500, each branch alone,
# profiles/r05_rbp_bench*.txt): C=64 fused vs two-conv k=3 -23 %, k=7 -12 %,
# k=11 -2 %; C=128 k=3 -25 %, k=7 -4..-8 %, k=11 +-0 (the c1 phase
# recomputes c2's halo: 10 of 128 columns at k=11); C=256 (one 512-thread
# workgroup per CU, 543 tiles per utterance batch: 2.1 rounds of the chip)
# k=3 -17 %, k=7 / k=11 +30..40 %.  The 32-channel stage's convs stay exact
# fp32 as single convs (32 rows), but its pairs run split fused too
# (engine.GeneratorPlan keeps split images beside them): vs the shipped exact
# pair / two-conv path k=3 -2..-5 %, k=7 -25..-33 %, k=11 -34..-35 %.
# With the 32 x 64 wave tile (four waves per SIMD) C=128 k=11
# went from +-0 to -15..-20 % and is fused too; C=256 k=7 / k=11 came to
# +1..+10 % each alone and still lose on the whole step
# (profiles/pairs_w8_ab.txt), so 256 stays at 3.
F32P_PAIR_MAX_K = {32: 11, 64: 11, 128: 11, 256: 3}


def resblock_pair_f32p_supported(c1: PackedConv, c2: PackedConv, x: torch.Tensor) -> bool:
    """Pairs of an fp32 Generator's split-fp32 stages (pre-split images,
    VITS_WDT_F32P) that run fused (csrc/resblock_f32p.hip): odd k, 'same'
    padding, (k - 1) * dil <= 96, 16-byte aligned fp32 time rows."""
    C_ = c2.out_channels
    return (c1.wdtype == WDT_F32P and c2.wdtype == WDT_F32P and c1.k <= F32P_PAIR_MAX_K.get(C_, 0)
            and x.dtype == torch.float32 and c1.m == C_ and c1.cin == C_ and c2.cin == C_ // 2
            and c2.m == C_ and c1.k == c2.k and c1.k % 2 == 1 and (c1.k - 1) * c1.dil <= 96
            and c2.dil == 1 and c1.epi == EPI_GATE and c2.epi == EPI_STORE
            and (C_ != 256 or (c1.k - 1) * c1.dil <= 56)  # (its 64-channel X chunks' LDS)
            and c1.pad_left == (c1.k - 1) * c1.dil // 2 and c2.pad_left == (c2.k - 1) // 2
            and x.shape[2] % 4 == 0 and x.stride(2) == 1 and x.stride(1) % 4 == 0
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)


def _resblock_kc(ch: int, k: int, dil: int):
    key = (ch, k, dil)
    if key not in _RB_KC:
        kc1, kc2 = C.c_int(), C.c_int()
        rc = _lib.load().vits_resblock_pair_kc(ch, k, dil, kc1, kc2)
        _RB_KC[key] = (kc1.value, kc2.value) if rc == 0 else None
    return _RB_KC[key]


def resblock_pair_desc(c1: PackedConv, c2: PackedConv, x: torch.Tensor, y: torch.Tensor, *,
                       cond: Optional[torch.Tensor] = None, cond_offset: int = 0,
                       in_slope: float = 0.1, accumulate: bool = False,
                       post_div: float = 1.0,
                       lengths: Optional[torch.Tensor] = None) -> ResblockPairDesc:
    """y = x + c2(gate(c1(lrelu(x)) + cond)) in one launch (modules.py:250-260);
    ``lengths`` (int32 [B], device): the utterance ends there (zero past)."""
    assert x.dtype == torch.float32 and y.dtype == torch.float32 and x.stride(2) == 1
    C_, T = x.shape[1], x.shape[2]
    # (the split-fp32 kernel stages 16-channel slabs: no kc choice)
    kc1, kc2 = (16, 16) if c1.wdtype == WDT_F32P else _resblock_kc(C_, c1.k, c1.dil)
    d = ResblockPairDesc()
    d.x, d.x_bstride, d.x_cstride, d.t_len = x.data_ptr(), x.stride(0), x.stride(1), T
    d.channels, d.in_slope = C_, in_slope
    d.w1, d.m_pad1, d.cin_pad1, d.kc1 = c1.w.data_ptr(), c1.m_pad, c1.cin_pad, kc1
    d.k, d.dil, d.kc2 = c1.k, c1.dil, kc2
    d.b1 = _ptr(c1.bias)
    if cond is not None:
        d.cond, d.cond_bstride = cond.data_ptr() + 4 * cond_offset, cond.stride(0)
    d.w2, d.m_pad2, d.cin_pad2 = c2.w.data_ptr(), c2.m_pad, c2.cin_pad
    d.b2 = _ptr(c2.bias)
    d.y, d.y_bstride, d.y_cstride = y.data_ptr(), y.stride(0), y.stride(1)
    d.accumulate, d.post_div = int(accumulate), float(post_div)
    d.lengths = _ptr(lengths)
    d.len_skip = LEN_SKIP.margin if lengths is not None else 0
    return d


# fused pairs of 16-bit models (csrc/resblock16.hip): False keeps their
# two-conv path
FUSED_PAIRS16 = True
# largest k fused on the 256-channel stage (resblock_f32p.hip's 16-bit mode;
# 0 = none, the two-conv path)
PAIR16_256_MAX_K = 15


def resblock_pair16_supported(c1: PackedConv, c2: PackedConv, x: torch.Tensor) -> bool:
    """Pairs of a 16-bit model with 16-bit activations that run fused
    (csrc/resblock16.hip; the 256-channel stage csrc/resblock_f32p.hip),
    any odd k with (k - 1) * dil <= 96, 8-byte aligned time rows
    (T % 4 == 0)."""
    C_ = c2.out_channels
    if C_ == 256 and c1.k > PAIR16_256_MAX_K:
        return False
    return (FUSED_PAIRS16 and c1.wdtype in (WDT_BF16, WDT_F16) and c2.wdtype == c1.wdtype
            and x.dtype == _WDT_TORCH[c1.wdtype] and C_ in (32, 64, 128, 256) and c1.m == C_
            and c1.cin == C_ and c2.cin == C_ // 2 and c2.m == C_ and c1.k == c2.k
            and c1.k % 2 == 1 and (c1.k - 1) * c1.dil <= 96 and c2.dil == 1
            and c1.epi == EPI_GATE and x.shape[2] % 4 == 0 and x.stride(2) == 1
            and x.stride(1) % 4 == 0 and x.stride(0) % 4 == 0)


def resblock_pair16_desc(c1: PackedConv, c2: PackedConv, x: torch.Tensor, y: torch.Tensor, *,
                         cond: Optional[torch.Tensor] = None, cond_offset: int = 0,
                         in_slope: float = 0.1, accumulate: bool = False, post_div: float = 1.0,
                         lengths: Optional[torch.Tensor] = None) -> ResblockPairDesc:
    """resblock_pair_desc for resblock16 (16-bit x / y, 16-bit images)."""
    assert x.dtype == y.dtype == _WDT_TORCH[c1.wdtype] and x.stride(2) == 1 and y.stride(2) == 1
    C_, T = x.shape[1], x.shape[2]
    d = ResblockPairDesc()
    d.x, d.x_bstride, d.x_cstride, d.t_len = x.data_ptr(), x.stride(0), x.stride(1), T
    d.channels, d.in_slope = C_, in_slope
    d.w1, d.m_pad1, d.cin_pad1, d.kc1 = c1.w.data_ptr(), c1.m_pad, c1.cin_pad, 16
    d.k, d.dil, d.kc2 = c1.k, c1.dil, 16
    d.b1 = _ptr(c1.bias)
    if cond is not None:
        d.cond, d.cond_bstride = cond.data_ptr() + 4 * cond_offset, cond.stride(0)
    d.w2, d.m_pad2, d.cin_pad2 = c2.w.data_ptr(), c2.m_pad, c2.cin_pad
    d.b2 = _ptr(c2.bias)
    d.y, d.y_bstride, d.y_cstride = y.data_ptr(), y.stride(0), y.stride(1)
    d.accumulate, d.post_div = int(accumulate), float(post_div)
    d.lengths = _ptr(lengths)
    d.len_skip = LEN_SKIP.margin if lengths is not None else 0
    return d


def resblock_pair16_launch(descs, batch: int, device: torch.device, wdtype: int,
                           mean: bool = False):
    """One launch of up to 3 independent 16-bit pairs (tuple) or one pair;
    mean=True: the members' mean into descs[0]'s output
    (vits_resblock_pair16_mean_forward)."""
    group = tuple(descs) if isinstance(descs, (tuple, list)) else (descs,)
    lib = _lib.load()
    if ConvTimer.active is not None:
        return ConvTimer.active.launch_pairs(lib, group, batch, device, wdtype, mean=mean)
    arr = (ResblockPairDesc * len(group))(*group)
    fn = lib.vits_resblock_pair16_mean_forward if mean else lib.vits_resblock_pair16_forward
    check(fn(arr, len(group), batch, int(wdtype), _stream_ptr(device)),
          "vits_resblock_pair16_forward")


def resblock_pair_flops(d: ResblockPairDesc, batch: int) -> int:
    """Algorithmic FLOPs of the pair (c1 + c2 as the reference computes
    them; the kernel's recomputed halo columns are not counted)."""
    C_, k, T = d.channels, d.k, d.t_len
    return 2 * batch * T * (C_ * C_ * k + (C_ // 2) * C_ * k)


def resblock_pair_launch(descs, batch: int, device: torch.device, wdtype: int = WDT_F32,
                         mean: bool = False):
    """One launch of up to 3 independent pairs (tuple) or one pair; wdtype
    WDT_F32 (exact fp32, csrc/resblock.hip) or WDT_F32P (split fp32,
    csrc/resblock_f32p.hip).  mean=True (WDT_F32P, 32 channels): the members'
    mean into their common output (vits_resblock_pair_f32p_mean_forward)."""
    group = tuple(descs) if isinstance(descs, (tuple, list)) else (descs,)
    lib = _lib.load()
    if mean and wdtype != WDT_F32P:
        raise NotImplementedError("branch-mean launch: split-fp32 pairs only")
    if ConvTimer.active is not None:
        return ConvTimer.active.launch_pairs(lib, group, batch, device,
                                             wdtype=WDT_F32P if wdtype == WDT_F32P else None,
                                             mean=mean)
    arr = (ResblockPairDesc * len(group))(*group)
    if wdtype == WDT_F32P:
        fn = (lib.vits_resblock_pair_f32p_mean_forward if mean
              else lib.vits_resblock_pair_f32p_forward)
        check(fn(arr, len(group), batch, _stream_ptr(device)), "vits_resblock_pair_f32p_forward")
        return
    check(lib.vits_resblock_pair_forward(arr, len(group), batch, _stream_ptr(device)),
          "vits_resblock_pair_forward")


# ---------------------------------------------------------------------------
# fused WN layer (csrc/wn_f32p.hip)
# ---------------------------------------------------------------------------
# columns per workgroup of the fused WN layer: 0 = chosen by grid size in the
# library, 32 / 64 force a tile (tools/wn_bench.py, the tests: no bit depends
# on it)
WN_NG = 0


def wn_layer_f32p_supported(in_layer: PackedConv, res_skip: PackedConv, h: torch.Tensor) -> bool:
    """WN layers of an fp32 model that run fused (csrc/wn_f32p.hip): both
    convs pre-split (VITS_WDT_F32P), H = 256, in_layer Conv1d(H, 2H, odd k,
    'same' padding) with the gate epilogue, res_skip 1x1 with 2H rows (last
    layer: H), 16-byte aligned fp32 time rows with T % 4 == 0.  Anything else
    keeps the two-conv path."""
    H = in_layer.cin
    return (in_layer.wdtype == WDT_F32P and res_skip.wdtype == WDT_F32P and H == 256
            and h.dtype == torch.float32 and h.dim() == 3 and h.shape[1] == H
            and in_layer.m == 2 * H and in_layer.epi == EPI_GATE and in_layer.cin_pad == H
            and in_layer.k % 2 == 1 and (in_layer.k - 1) * in_layer.dil <= 56
            and in_layer.pad_left == (in_layer.k - 1) * in_layer.dil // 2
            and res_skip.epi == EPI_STORE and res_skip.k == 1 and res_skip.cin == H
            and res_skip.cin_pad == H and res_skip.m in (H, 2 * H) and res_skip.pad_left == 0
            and h.shape[2] % 4 == 0 and h.stride(2) == 1 and h.stride(1) % 4 == 0
            and h.stride(0) % 4 == 0 and h.data_ptr() % 16 == 0
            and H * h.stride(1) < 2 ** 31)


def wn_layer_desc(in_layer: PackedConv, res_skip: PackedConv, h: torch.Tensor,
                  h_out: Optional[torch.Tensor], skip: torch.Tensor, *, accumulate: bool,
                  cond: Optional[torch.Tensor] = None, cond_offset: int = 0,
                  lengths: Optional[torch.Tensor] = None) -> WnLayerDesc:
    """One fused WN layer: h_out = h + res, skip (+)= skip part; h_out None:
    the last layer (res_skip has H rows, all to skip).  h_out and skip must
    not be h."""
    H, T = h.shape[1], h.shape[2]
    last = h_out is None
    assert res_skip.m == (H if last else 2 * H)
    assert skip.dtype == torch.float32 and skip.stride(2) == 1
    d = WnLayerDesc()
    d.h, d.h_bstride, d.h_cstride, d.t_len = h.data_ptr(), h.stride(0), h.stride(1), T
    d.hidden, d.k, d.dil, d.last = H, in_layer.k, in_layer.dil, int(last)
    d.w1, d.m_pad1, d.cin_pad1 = in_layer.w.data_ptr(), in_layer.m_pad, in_layer.cin_pad
    d.b1 = _ptr(in_layer.bias)
    if cond is not None:
        d.cond, d.cond_bstride = cond.data_ptr() + 4 * cond_offset, cond.stride(0)
    d.w2, d.m_pad2, d.cin_pad2 = res_skip.w.data_ptr(), res_skip.m_pad, res_skip.cin_pad
    d.b2 = _ptr(res_skip.bias)
    if not last:
        assert h_out.dtype == torch.float32 and h_out.stride(2) == 1
        d.h_out, d.ho_bstride, d.ho_cstride = h_out.data_ptr(), h_out.stride(0), h_out.stride(1)
    d.skip, d.skip_bstride, d.skip_cstride = skip.data_ptr(), skip.stride(0), skip.stride(1)
    d.accumulate = int(accumulate)
    d.lengths = _ptr(lengths)
    d.len_skip = LEN_SKIP.margin if lengths is not None else 0
    d.ng = WN_NG
    return d


def wn_layer_flops(d: WnLayerDesc, batch: int) -> int:
    """Algorithmic FLOPs of the layer: those of the two convs it replaces."""
    H = d.hidden
    return 2 * batch * d.t_len * (2 * H * H * d.k + (H if d.last else 2 * H) * H)


def conv1d_launch(desc: ConvDesc, batch: int, device: torch.device):
    lib = _lib.load()
    if ConvTimer.active is not None:
        return ConvTimer.active.launch(lib, desc, batch, device)
    check(lib.vits_conv1d_forward(C.byref(desc), batch, _stream_ptr(device)), "vits_conv1d_forward")


PLAN_FIELDS = ("wdtype", "ga", "bm", "bn", "waves_m", "waves_n", "v4", "io16", "epi", "up_lds",
               "lds_bytes")


def conv1d_plan(descs, batch: int):
    """Which kernel conv1d_launch / one shared-grid tuple of conv1d_launch_seq
    would run for ``descs`` (a ConvDesc or up to three) at ``batch``: the
    library's own launch path stopped before the launch
    (vits_conv1d_plan; host only - no device, nothing read through the
    pointers).  Returns ``(rc, plan)``: rc is the status the launch would
    return, plan a dict of PLAN_FIELDS plus ``grid`` (None when refused)."""
    group = tuple(descs) if isinstance(descs, (tuple, list)) else (descs,)
    arr = (ConvDesc * len(group))(*group)
    out = _lib.ConvPlan()
    rc = _lib.load().vits_conv1d_plan(arr, len(group), batch, C.byref(out))
    if rc != _lib.VITS_OK:
        return rc, None
    plan = {f: int(getattr(out, f)) for f in PLAN_FIELDS}
    plan["grid"] = tuple(out.grid)
    return rc, plan


def conv1d_launch_seq(descs, batch: int, device: torch.device):
    """Run descriptors in order, one host call.  An item may be a tuple of
    independent ConvDescs (the ResBlock2 branches of one Generator stage):
    they share one launch (vits_conv1d_forward_groups).  A sequence that holds
    fused WN layers (WnLayerDesc, between single ConvDescs) is one call of
    vits_conv1d_wn_seq_forward."""
    lib = _lib.load()
    if ConvTimer.active is not None:
        for d in descs:
            if isinstance(d, WnLayerDesc):
                ConvTimer.active.launch_wn(lib, d, batch, device)
            else:
                ConvTimer.active.launch(lib, d, batch, device)
        return
    if any(isinstance(d, WnLayerDesc) for d in descs):
        convs = [d for d in descs if not isinstance(d, WnLayerDesc)]
        wns = [d for d in descs if isinstance(d, WnLayerDesc)]
        assert all(isinstance(d, ConvDesc) for d in convs), "no grouped launches beside WN layers"
        kinds = (C.c_int32 * len(descs))(*[int(isinstance(d, WnLayerDesc)) for d in descs])
        check(lib.vits_conv1d_wn_seq_forward((ConvDesc * len(convs))(*convs), len(convs),
                                             (WnLayerDesc * len(wns))(*wns), len(wns), kinds,
                                             len(descs), batch, _stream_ptr(device)),
              "vits_conv1d_wn_seq_forward")
        return
    flat, sizes = [], []
    for d in descs:
        group = tuple(d) if isinstance(d, (tuple, list)) else (d,)
        flat.extend(group)
        sizes.append(len(group))
    arr = (ConvDesc * len(flat))(*flat)
    sz = (C.c_int32 * len(sizes))(*sizes)
    check(lib.vits_conv1d_forward_groups(arr, sz, len(sizes), batch, _stream_ptr(device)),
          "vits_conv1d_forward_groups")


def conv1d(x: torch.Tensor, layer: PackedConv, *, in_slope: float = 1.0, act: int = ACT_NONE,
           cond: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           res_scale: float = 1.0, lengths: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, accumulate: bool = False,
           post_div: float = 1.0, t_out: Optional[int] = None) -> torch.Tensor:
    """Run one packed conv on [B, cin, T] (device) and return [B, out_channels,
    T_out].  x fp32, or of the layer's 16-bit type (io16: output, residual
    and accumulator of that type too)."""
    require_device(x, cond, residual, lengths)
    B, _, T = x.shape
    io16 = x.dtype != torch.float32
    if layer.epi == EPI_UPSAMPLE:
        T_out = T * layer.up_u if t_out is None else t_out
    else:
        T_out = T
    if out is None:
        out = torch.empty(B, layer.out_channels, T_out, device=x.device, dtype=x.dtype)
    o0 = make_out(out, act=act, res=residual, res_scale=res_scale, accumulate=accumulate,
                  post_div=post_div)
    if lengths is not None:
        lengths = lengths.to(device=x.device, dtype=torch.int32).contiguous()
    d = make_desc(layer, x, o0, in_slope=in_slope, cond=cond, lengths=lengths, t_out=T_out,
                  io16=2 if io16 else 0)
    conv1d_launch(d, B, x.device)
    return out


# ---------------------------------------------------------------------------
# small kernels
# ---------------------------------------------------------------------------


def linear_rows(g: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[b] = weight @ g[b] + bias (per-utterance conditioning)."""
    require_device(g, weight, bias)
    g = g.contiguous().float()
    B, n_in = g.shape
    n_out = weight.shape[0]
    if out is None:
        out = torch.empty(B, n_out, device=g.device, dtype=torch.float32)
    lib = _lib.load()
    check(lib.vits_linear_forward(g.data_ptr(), g.stride(0), weight.data_ptr(), _ptr(bias),
                                  out.data_ptr(), out.stride(0), B, n_out, n_in,
                                  _stream_ptr(g.device)), "vits_linear_forward")
    return out


def expand_prior(attn: torch.Tensor, m_p: torch.Tensor, s_p: torch.Tensor, noise: torch.Tensor,
                 out: Optional[torch.Tensor] = None, exp_s: bool = False,
                 noise_scale: float = 1.0) -> torch.Tensor:
    require_device(attn, m_p, s_p, noise)
    attn = attn.contiguous().float()
    m_p = m_p.contiguous().float()
    s_p = s_p.contiguous().float()
    noise = noise.contiguous().float()
    B, Ty, Tx = attn.shape
    Cc = m_p.shape[1]
    if out is None:
        out = torch.empty(B, Cc, Ty, device=attn.device, dtype=torch.float32)
    lib = _lib.load()
    check(lib.vits_expand_prior(attn.data_ptr(), m_p.data_ptr(), s_p.data_ptr(), noise.data_ptr(),
                                out.data_ptr(), B, Cc, Ty, Tx, 1 if exp_s else 0, noise_scale,
                                _stream_ptr(attn.device)),
          "vits_expand_prior")
    return out


ED_DRAWS = 32  # VITS_ED_DRAWS (include/vits_amd.h)


def numpy_draw_pool(n: int = ED_DRAWS):
    """The next ``n`` raw 32-bit MT19937 words of numpy's global legacy
    generator (RandomState.randint over the full uint32 range returns them
    unmasked, one word each) and the generator state before them.  The
    device consumes k of them the way ``np.random.randint(high)`` would;
    ``numpy_draw_commit`` then leaves the generator exactly where that
    randint call would have left it."""
    state = np.random.get_state()
    words = np.random.randint(0, 2 ** 32, size=n, dtype=np.uint32)
    return words.view(np.int32).copy(), state


def numpy_draw_commit(state, used: int) -> None:
    """Rewind numpy's global generator to ``state`` and advance it by the
    ``used`` words the device consumed (see numpy_draw_pool)."""
    np.random.set_state(state)
    if used > 0:
        np.random.randint(0, 2 ** 32, size=used, dtype=np.uint32)


def _rate_arg(rate, B: int, what: str):
    """``rate`` of expand_durations / draw_starts: a number (one speed for
    every row, passed by value) or a contiguous fp32 [B] device tensor (row
    b's speed, read on the device: the ``*_rows`` entry points).  Returns
    (scalar, tensor): exactly one is not None."""
    if isinstance(rate, torch.Tensor):
        if rate.dtype != torch.float32 or tuple(rate.shape) != (B,) or not rate.is_contiguous():
            raise _lib.VitsAmdError(
                f"{what}: a per-row rate must be a contiguous fp32 [{B}] tensor, got "
                f"{rate.dtype} {tuple(rate.shape)}")
        require_device(rate)
        return None, rate
    numbers = (int, float, np.integer, np.floating)
    if isinstance(rate, bool) or not isinstance(rate, numbers):
        raise _lib.VitsAmdError(f"{what}: rate must be a number or an fp32 [{B}] device tensor, "
                                f"got {type(rate).__name__}")
    return float(rate), None


def _durations_arg(durations, B: int, t_x: int, rate, half_round, what: str):
    """``durations`` of expand_durations / draw_starts: an int32 [B, t_x]
    device tensor whose rows are contiguous; it replaces logw, rate and
    half_round, so a non-default one of those next to it is an error."""
    if isinstance(rate, torch.Tensor) or rate != 1.0 or half_round:
        raise _lib.VitsAmdError(f"{what}: durations already hold the speed and the rounding; "
                                "give durations or rate / half_round, not both")
    if (not isinstance(durations, torch.Tensor) or durations.dtype != torch.int32
            or tuple(durations.shape) != (B, t_x) or durations.stride(1) != 1
            or durations.stride(0) < t_x):
        raise _lib.VitsAmdError(f"{what}: durations must be an int32 [{B}, {t_x}] tensor with "
                                "contiguous rows")
    require_device(durations)
    return durations


def duration_plan(logw: torch.Tensor, *, rate=1.0, x_len: Optional[torch.Tensor] = None,
                  half_round: bool = False, given: Optional[torch.Tensor] = None,
                  tok_scale: Optional[torch.Tensor] = None,
                  target: Optional[torch.Tensor] = None, w_out=False,
                  dur: Optional[torch.Tensor] = None, meta: Optional[torch.Tensor] = None):
    """The integer durations of every token under a caller's controls, on the
    device with no host sync (vits_duration_plan, include/vits_amd.h has the
    arithmetic).  ``logw`` [B, t_x] or [B, 1, t_x] (rows may be strided);
    ``rate`` as in expand_durations; ``given`` int32 [B, t_x]: >= 0 pins a
    token to that many frames (0 allowed), < 0 leaves it free; ``tok_scale``
    fp32 [B, t_x]: a per-token factor (>= 0) on the free tokens; ``target``
    int32 [B]: > 0 = the row lasts exactly that many frames (the free tokens
    are fitted, ``rate`` is not applied), <= 0 = none.  Returns (dur int32 [B,
    t_x] (0 at and past x_len), total int32 [B], status int32 [B]) and, with
    ``w_out`` (True, or an fp32 [B, t_x] tensor to fill), the w behind every
    free token's duration.  status 1: the target cannot be met and the row
    holds the no-target durations.  total and status are views of ``meta``
    (int32 [2, B]).  ``dur`` feeds ``expand_durations(durations=)`` and
    ``draw_starts(durations=)``."""
    require_device(logw)
    B = logw.shape[0]
    if logw.dim() == 3:
        logw = logw.reshape(B, -1)
    if logw.dim() != 2 or logw.dtype != torch.float32 or logw.stride(1) != 1:
        logw = logw.reshape(B, -1).float().contiguous()
    t_x = logw.shape[1]
    rate, rates = _rate_arg(rate, B, "duration_plan")
    dev = logw.device

    def opt(t, dtype, shape, name):
        if t is None:
            return None
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape
                or not t.is_contiguous()):
            raise _lib.VitsAmdError(f"duration_plan: {name} must be a contiguous {dtype} "
                                    f"{list(shape)} tensor")
        require_device(t)
        return t

    given = opt(given, torch.int32, (B, t_x), "given")
    tok_scale = opt(tok_scale, torch.float32, (B, t_x), "tok_scale")
    target = opt(target, torch.int32, (B,), "target")
    x_len = opt(x_len, torch.int32, (B,), "x_len")
    if dur is None:
        dur = torch.empty(B, t_x, device=dev, dtype=torch.int32)
    if meta is None:
        meta = torch.empty(2, B, device=dev, dtype=torch.int32)
    opt(dur, torch.int32, (B, t_x), "dur")
    opt(meta, torch.int32, (2, B), "meta")
    w = None
    if w_out is True:
        w = torch.empty(B, t_x, device=dev, dtype=torch.float32)
    elif w_out is not False and w_out is not None:
        w = opt(w_out, torch.float32, (B, t_x), "w_out")
    check(_lib.load().vits_duration_plan(
        logw.data_ptr(), logw.stride(0), _ptr(x_len), t_x,
        1.0 if rates is not None else rate, _ptr(rates), int(half_round), _ptr(given),
        _ptr(tok_scale), _ptr(target), dur.data_ptr(), meta.data_ptr(), _ptr(w), B,
        _stream_ptr(dev)), "vits_duration_plan")
    if w is not None:
        return dur, meta[0], meta[1], w
    return dur, meta[0], meta[1]


def expand_durations(logw: torch.Tensor, m_p: torch.Tensor, s_p: torch.Tensor,
                     noise: torch.Tensor, t_y: int, *, rate=1.0,
                     noise_scale: float = 1.0, x_len: Optional[torch.Tensor] = None,
                     noise_start: Optional[torch.Tensor] = None, half_round: bool = False,
                     stage_mult=(1,), out: Optional[torch.Tensor] = None,
                     lens: Optional[torch.Tensor] = None,
                     starts: Optional[torch.Tensor] = None,
                     durations: Optional[torch.Tensor] = None):
    """Durations -> (z [B, C, t_y], lens int32 [n_stage, B]) on the device,
    without the host sync of models.py:547 / infer.py:171: w_ceil =
    ceil(exp(logw) * rate), y_len = max(sum, 1), z = the one-hot expansion of
    m_p + noise * s_p * noise_scale over the static bucket t_y (0 past
    y_len), lens[i] = y_len * stage_mult[i].  ``noise`` is [B, C, t_y], or
    with ``noise_start`` (int32 [B]) a flat buffer read as EmoVITS slices it
    (element (c, t) at s + c * y_len + t): ``noise_start`` is then an int32
    [B, ED_DRAWS] pool of raw MT19937 words (``numpy_draw_pool``) from which the
    device draws s = np.random.randint(numel - C * y_len) exactly as numpy's
    legacy RandomState would, and ``lens`` gets one more row: the words
    consumed per utterance (-1: the slice does not fit; -2: every word of the
    pool was rejected, the caller advances by the pool and calls again; z is
    zero for both).  ``starts`` (int64 [B], from ``draw_starts``) instead of
    ``noise_start``: the flat buffer read at those explicit starts (a
    negative one: z = 0, nothing read); ``lens`` stays [n_stage, B].
    ``rate``: a number, or a contiguous fp32 [B] device tensor of per-row
    speeds (row b is then bit for bit the call with ``rate=float(rate[b])``).
    ``durations`` (int32 [B, t_x] device tensor, e.g. ``duration_plan``'s):
    the integer durations themselves in place of ceil(exp(logw) * rate)
    (vits_expand_durations_int: a token of 0 frames gets none, y_len = max(sum,
    1) as a plain integer sum); ``logw`` may then be None, and ``rate`` and
    ``half_round`` must be left at their defaults."""
    if durations is not None:
        durations = _durations_arg(durations, m_p.shape[0], m_p.shape[2], rate, half_round,
                                   "expand_durations")
        rate, rates = None, None
        require_device(m_p, s_p, noise)
    else:
        rate, rates = _rate_arg(rate, m_p.shape[0], "expand_durations")
        require_device(logw, m_p, s_p, noise)
    if starts is not None:
        if noise_start is not None:
            raise _lib.VitsAmdError("expand_durations: give noise_start or starts, not both")
        require_device(starts)
        if (tuple(starts.shape) != (m_p.shape[0],) or starts.dtype != torch.int64
                or not starts.is_contiguous()):
            raise _lib.VitsAmdError(f"expand_durations: starts must be int64 [{m_p.shape[0]}]")
    B, C_, t_x = m_p.shape
    if durations is None:
        logw = logw.reshape(B, t_x).float().contiguous()
    m_p = m_p.float().contiguous()
    s_p = s_p.float().contiguous()
    noise = noise.float().contiguous()
    if out is None:
        out = torch.empty(B, C_, t_y, device=m_p.device, dtype=torch.float32)
    n_stage = len(stage_mult)
    rows = n_stage + (0 if noise_start is None else 1)
    if lens is None:
        lens = torch.empty(rows, B, device=m_p.device, dtype=torch.int32)
    if tuple(lens.shape) != (rows, B) or lens.dtype != torch.int32 or not lens.is_contiguous():
        raise _lib.VitsAmdError(f"expand_durations: lens must be int32 [{rows}, {B}]")
    mult = (C.c_int32 * n_stage)(*[int(v) for v in stage_mult])
    if starts is not None:
        mode, start_ptr = 2, starts.data_ptr()
    elif noise_start is None:
        assert tuple(noise.shape) == (B, C_, t_y), noise.shape
        mode, start_ptr = 0, None
    elif (tuple(noise_start.shape) != (B, ED_DRAWS) or noise_start.dtype != torch.int32
          or not noise_start.is_contiguous()):
        raise _lib.VitsAmdError(f"expand_durations: noise_start must be int32 [{B}, {ED_DRAWS}]")
    else:
        mode, start_ptr = 1, noise_start.data_ptr()
    lib = _lib.load()
    if durations is not None:
        check(lib.vits_expand_durations_int(
            durations.data_ptr(), durations.stride(0), _ptr(x_len), t_x,
            m_p.data_ptr(), s_p.data_ptr(), m_p.stride(0), m_p.stride(1), noise.data_ptr(),
            mode, start_ptr, noise.numel(), float(noise_scale), out.data_ptr(),
            B, C_, t_y, lens.data_ptr(), mult, n_stage, _stream_ptr(m_p.device)),
            "vits_expand_durations_int")
        return out, lens
    fn, what = ((lib.vits_expand_durations, "vits_expand_durations") if rates is None else
                (lib.vits_expand_durations_rows, "vits_expand_durations_rows"))
    check(fn(
        logw.data_ptr(), logw.stride(0), _ptr(x_len), t_x,
        rate if rates is None else rates.data_ptr(), int(half_round),
        m_p.data_ptr(), s_p.data_ptr(), m_p.stride(0), m_p.stride(1), noise.data_ptr(),
        mode, start_ptr, noise.numel(), float(noise_scale),
        out.data_ptr(),
        B, C_, t_y, lens.data_ptr(), mult, n_stage, _stream_ptr(m_p.device)), what)
    return out, lens


def _n_rows_ptr(n_rows, B: int, device, what: str):
    """n_rows of the batched serving kernels: None (all B rows), a host int
    or an int32 [1] device tensor (a graph's static buffer).  Returns the
    tensor to keep alive and its pointer."""
    if n_rows is None:
        return None, None
    if not isinstance(n_rows, torch.Tensor):
        if not 0 <= int(n_rows) <= B:
            raise _lib.VitsAmdError(f"{what}: n_rows must be in [0, {B}], got {n_rows}")
        n_rows = torch.tensor([int(n_rows)], dtype=torch.int32, device=device)
    require_device(n_rows)
    if n_rows.dtype != torch.int32 or n_rows.numel() != 1:
        raise _lib.VitsAmdError(f"{what}: n_rows must be an int or an int32 [1] device tensor")
    return n_rows, n_rows.data_ptr()


def draw_starts(logw: torch.Tensor, channels: int, noise_len: int, pool: torch.Tensor, *,
                rate=1.0, x_len: Optional[torch.Tensor] = None,
                half_round: bool = False, n_rows=None, starts: Optional[torch.Tensor] = None,
                meta: Optional[torch.Tensor] = None,
                durations: Optional[torch.Tensor] = None):
    """The noise-slice starts of B utterances as B consecutive EmoVITS.infer
    calls would draw them (infer.py:173): y_len[b] from ``logw`` with
    expand_durations' arithmetic, then np.random.randint(noise_len - channels
    * y_len[b]) in row order from ONE ``pool`` of raw MT19937 words (int32
    [P] device tensor of ``numpy_draw_pool(P)``), row b reading on from where
    row b - 1 stopped.  Returns (starts int64 [B], y_len int32 [B], status
    int32 [B], used_total int32 [1]); the last three are views of ``meta``
    (int32 [2 B + 1]).  status: words consumed, -1 = the slice does not fit
    (nothing consumed), -2 = the pool ran out at this row; starts is -1 for
    both.  Rows at or past ``n_rows`` (None, int or int32 [1] device tensor)
    draw nothing.  When everything is >= 0, ``numpy_draw_commit(state,
    used_total)`` leaves numpy's generator where the B calls would.
    ``rate``: a number or an fp32 [B] device tensor, as in expand_durations.
    ``durations`` (int32 [B, t_x] device tensor): y_len[b] = max(sum of row b,
    1) from the integer durations themselves (vits_draw_starts_int); ``logw``
    may then be None, ``rate`` and ``half_round`` stay at their defaults."""
    if durations is not None:
        if durations.dim() != 2:
            raise _lib.VitsAmdError("draw_starts: durations must be an int32 [B, t_x] tensor")
        B, t_x = durations.shape
        durations = _durations_arg(durations, B, t_x, rate, half_round, "draw_starts")
        rate, rates = None, None
        require_device(pool)
    else:
        B = logw.shape[0]
        rate, rates = _rate_arg(rate, B, "draw_starts")
        require_device(logw, pool)
        logw = logw.reshape(B, -1).float().contiguous()
        t_x = logw.shape[1]
    if pool.dtype != torch.int32 or pool.dim() != 1 or not pool.is_contiguous() or not pool.numel():
        raise _lib.VitsAmdError("draw_starts: pool must be a contiguous int32 [P] tensor, P >= 1")
    dev = pool.device
    if starts is None:
        starts = torch.empty(B, device=dev, dtype=torch.int64)
    if meta is None:
        meta = torch.empty(2 * B + 1, device=dev, dtype=torch.int32)
    if (tuple(starts.shape) != (B,) or starts.dtype != torch.int64 or not starts.is_contiguous()
            or tuple(meta.shape) != (2 * B + 1,) or meta.dtype != torch.int32
            or not meta.is_contiguous()):
        raise _lib.VitsAmdError(f"draw_starts: starts must be int64 [{B}], meta int32 [{2 * B + 1}]")
    if x_len is not None and (x_len.dtype != torch.int32 or tuple(x_len.shape) != (B,)
                              or not x_len.is_contiguous()):
        raise _lib.VitsAmdError(f"draw_starts: x_len must be a contiguous int32 [{B}] tensor")
    keep, nr_ptr = _n_rows_ptr(n_rows, B, dev, "draw_starts")
    lib = _lib.load()
    if durations is not None:
        check(lib.vits_draw_starts_int(
            durations.data_ptr(), durations.stride(0), _ptr(x_len), t_x,
            int(channels), int(noise_len), pool.data_ptr(), pool.numel(), nr_ptr, B,
            starts.data_ptr(), meta.data_ptr(), _stream_ptr(dev)), "vits_draw_starts_int")
        return starts, meta[:B], meta[B:2 * B], meta[2 * B:]
    fn, what = ((lib.vits_draw_starts, "vits_draw_starts") if rates is None else
                (lib.vits_draw_starts_rows, "vits_draw_starts_rows"))
    check(fn(
        logw.data_ptr(), logw.stride(0), _ptr(x_len), t_x,
        rate if rates is None else rates.data_ptr(), int(half_round),
        int(channels), int(noise_len), pool.data_ptr(), pool.numel(), nr_ptr, B,
        starts.data_ptr(), meta.data_ptr(), _stream_ptr(logw.device)), what)
    return starts, meta[:B], meta[B:2 * B], meta[2 * B:]


def conv_post_tanh(x: torch.Tensor, weight: torch.Tensor, out: Optional[torch.Tensor] = None):
    require_device(x, weight)
    B, Cc, T = x.shape
    k = weight.shape[-1]
    w = weight.reshape(Cc, k).contiguous().float()
    if out is None:
        out = torch.empty(B, 1, T, device=x.device, dtype=torch.float32)
    xdt = {torch.float32: WDT_F32, torch.bfloat16: WDT_BF16, torch.float16: WDT_F16}[x.dtype]
    lib = _lib.load()
    check(lib.vits_conv_post_tanh_lowp(x.data_ptr(), x.stride(0), x.stride(1), w.data_ptr(),
                                       out.data_ptr(), B, Cc, T, k, xdt, _stream_ptr(x.device)),
          "vits_conv_post_tanh_lowp")
    return out


def layer_norm_channels(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                        eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None,
                        lengths: Optional[torch.Tensor] = None,
                        post_add: Optional[torch.Tensor] = None, scale: float = 1.0,
                        pos: Optional[torch.Tensor] = None,
                        pos_alpha: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = ((LN(x + residual) * gamma + beta) + post_add[b]) * scale + pos[t] * alpha,
    zeroed at t >= lengths[b]; x, residual, out are [B, C, T] contiguous."""
    require_device(x, residual, lengths, post_add, pos, pos_alpha)
    assert x.is_contiguous() and (residual is None or residual.is_contiguous())
    B, Cc, T = x.shape
    if out is None:
        out = torch.empty_like(x)
    if pos is not None:
        assert pos.is_contiguous() and pos.shape[-1] == Cc and pos.numel() >= T * Cc
    lib = _lib.load()
    check(lib.vits_layer_norm_channels(x.data_ptr(), _ptr(residual), _ptr(gamma), _ptr(beta),
                                       out.data_ptr(), B, Cc, T, eps, _ptr(lengths),
                                       _ptr(post_add), 0 if post_add is None else post_add.stride(0),
                                       scale, _ptr(pos), _ptr(pos_alpha),
                                       _stream_ptr(x.device)), "vits_layer_norm_channels")
    return out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_heads: int,
              lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """softmax((q/sqrt(d)) k^T, masked -1e4) v on [B, H*D, T] channel-major tensors."""
    require_device(q, k, v, lengths)
    B, Cc, T = q.shape
    D = Cc // n_heads
    assert q.stride() == k.stride() == v.stride() and q.stride(2) == 1 and q.stride(1) == T
    if out is None:
        out = torch.empty(B, Cc, T, device=q.device, dtype=torch.float32)
    assert out.stride(2) == 1 and out.stride(1) == T
    lib = _lib.load()
    check(lib.vits_attention_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B,
                                     n_heads, D, T, q.stride(0), out.stride(0), _ptr(lengths),
                                     _stream_ptr(q.device)), "vits_attention_forward")
    return out


_DT = {torch.float32: _lib.DT_F32, torch.float16: _lib.DT_F16, torch.bfloat16: _lib.DT_BF16,
       torch.int32: _lib.DT_I32}

ATTN_HEAD_DIMS = (16, 32, 48, 64, 96, 128)


def _attn_layout(q, k, v):
    B, Cc, T = q.shape
    assert q.dtype == k.dtype == v.dtype and q.dtype in (torch.float32, torch.float16,
                                                         torch.bfloat16), q.dtype
    assert q.shape == k.shape == v.shape, "self-attention: equal query and key lengths"
    assert q.stride() == k.stride() == v.stride() and q.stride(2) == 1 and q.stride(1) == T
    return B, Cc, T


def _attn_seed(p_drop: float, seed):
    if p_drop > 0.0:
        assert seed is not None and seed.dtype == torch.int64 and seed.device.type == "cuda"
        return seed.data_ptr()
    return None


def attention_train_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_heads: int,
                            lengths: Optional[torch.Tensor] = None, p_drop: float = 0.0,
                            seed: Optional[torch.Tensor] = None):
    """``attention`` for training: (out, lse) with out = dropout(softmax(...), p_drop) v in
    q's dtype (fp32 / fp16 / bf16) and lse fp32 [B, H, T], the log-sum-exp of every
    query's masked scores.  ``seed``: int64 device tensor (1 element), read by the kernel;
    the keep mask is ``attention_dropout_mask(seed, ...)``."""
    require_device(q, k, v, lengths, seed)
    B, Cc, T = _attn_layout(q, k, v)
    out = torch.empty(B, Cc, T, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, n_heads, T, device=q.device, dtype=torch.float32)
    check(_lib.load().vits_attention_train_forward(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, n_heads,
        Cc // n_heads, T, q.stride(0), out.stride(0), _ptr(lengths), _DT[q.dtype], p_drop,
        _attn_seed(p_drop, seed), _stream_ptr(q.device)), "vits_attention_train_forward")
    return out, lse


def attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor,
                       dout: torch.Tensor, lse: torch.Tensor, n_heads: int,
                       lengths: Optional[torch.Tensor] = None, p_drop: float = 0.0,
                       seed: Optional[torch.Tensor] = None, grads=None):
    """(dq, dk, dv) of ``attention_train_forward`` in q's dtype.  ``grads``: optional
    (dq, dk, dv) tensors to write (equal strides; e.g. the channel slices of one
    [B, 3C, T] buffer); by default the slices of one new such buffer.  Two launches,
    no atomics: the same call twice is bit-identical."""
    require_device(q, k, v, out, dout, lse, lengths, seed)
    B, Cc, T = _attn_layout(q, k, v)
    assert out.dtype == q.dtype and dout.dtype == q.dtype
    for t in (out, dout):
        assert t.shape == q.shape and t.stride(2) == 1 and t.stride(1) == T
    assert lse.dtype == torch.float32 and lse.shape == (B, n_heads, T) and lse.is_contiguous()
    if grads is None:
        grads = torch.empty(B, 3 * Cc, T, device=q.device, dtype=q.dtype).split(Cc, 1)
    dq, dk, dv = grads
    for t in (dq, dk, dv):
        assert t.shape == q.shape and t.dtype == q.dtype
    assert dq.stride() == dk.stride() == dv.stride() and dq.stride(2) == 1 and dq.stride(1) == T
    delta = torch.empty(B, n_heads, T, device=q.device, dtype=torch.float32)
    check(_lib.load().vits_attention_backward(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, n_heads, Cc // n_heads,
        T, q.stride(0), out.stride(0), dout.stride(0), dq.stride(0), _ptr(lengths), _DT[q.dtype],
        p_drop, _attn_seed(p_drop, seed), _stream_ptr(q.device)), "vits_attention_backward")
    return dq, dk, dv


def attention_dropout_mask(seed: torch.Tensor, B: int, H: int, T: int, p: float) -> torch.Tensor:
    """The keep mask (uint8 [B, H, T, T], [query][key], 1 = kept) the training attention
    draws for ``seed`` at dropout probability ``p`` (tests)."""
    require_device(seed)
    mask = torch.empty(B, H, T, T, device=seed.device, dtype=torch.uint8)
    check(_lib.load().vits_attention_dropout_mask(_attn_seed(p, seed), mask.data_ptr(), B, H, T, p,
                                                  _stream_ptr(seed.device)),
          "vits_attention_dropout_mask")
    return mask


def neg_cent(z_p: torch.Tensor, m_p: torch.Tensor, logs_p: torch.Tensor) -> torch.Tensor:
    """MAS scores [B, t_t, t_s] of models.py:483-490 in one fp32 MFMA kernel
    (no autograd: the reference computes them under torch.no_grad)."""
    require_device(z_p, m_p, logs_p)
    z = z_p.detach().to(torch.float32).contiguous()
    m = m_p.detach().to(torch.float32).contiguous()
    lg = logs_p.detach().to(torch.float32).contiguous()
    B, C, Tt = z.shape
    if m.shape != lg.shape or m.shape[0] != B or m.shape[1] != C:
        raise _lib.VitsAmdError(f"neg_cent: z_p {tuple(z.shape)} m_p {tuple(m.shape)} "
                                f"logs_p {tuple(lg.shape)}")
    Ts = m.shape[2]
    out = torch.empty(B, Tt, Ts, device=z.device, dtype=torch.float32)
    check(_lib.load().vits_neg_cent(z.data_ptr(), m.data_ptr(), lg.data_ptr(), out.data_ptr(),
                                    B, C, Tt, Ts, _stream_ptr(z.device)), "vits_neg_cent")
    return out


def maximum_path(neg_cent: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """monotonic_align.maximum_path on the GPU (models.py:498 call contract)."""
    require_device(neg_cent, mask)
    dtype = neg_cent.dtype
    if dtype not in _DT:
        raise _lib.VitsAmdError(f"maximum_path: unsupported dtype {dtype}")
    nc = neg_cent.detach().to(torch.float32).contiguous()
    mk = mask.detach()
    if mk.dtype not in _DT:
        mk = mk.to(torch.float32)
    mk = mk.contiguous()
    B, Tt, Ts = nc.shape
    if mk.shape != nc.shape:
        raise _lib.VitsAmdError(f"maximum_path: mask {tuple(mk.shape)} vs neg_cent {tuple(nc.shape)}")
    path = torch.empty(B, Tt, Ts, device=nc.device, dtype=dtype)
    lib = _lib.load()
    wsb = int(lib.vits_maximum_path_workspace(B, Tt, Ts))
    ws = torch.empty(max(wsb, 16), device=nc.device, dtype=torch.uint8)
    check(lib.vits_maximum_path(nc.data_ptr(), mk.data_ptr(), _DT[mk.dtype], path.data_ptr(),
                                _DT[dtype], B, Tt, Ts, ws.data_ptr(), ws.numel(),
                                _stream_ptr(nc.device)), "vits_maximum_path")
    return path


def maximum_path_lengths(neg_cent: torch.Tensor, t_t: torch.Tensor, t_s: torch.Tensor,
                         dtype: torch.dtype = torch.float32) -> torch.Tensor:
    require_device(neg_cent, t_t, t_s)
    nc = neg_cent.detach().to(torch.float32).contiguous()
    B, Tt, Ts = nc.shape
    tt = t_t.to(torch.int32).contiguous()
    ts = t_s.to(torch.int32).contiguous()
    path = torch.empty(B, Tt, Ts, device=nc.device, dtype=dtype)
    lib = _lib.load()
    wsb = int(lib.vits_maximum_path_workspace(B, Tt, Ts))
    ws = torch.empty(max(wsb, 16), device=nc.device, dtype=torch.uint8)
    check(lib.vits_maximum_path_lengths(nc.data_ptr(), tt.data_ptr(), ts.data_ptr(),
                                        path.data_ptr(), _DT[dtype], B, Tt, Ts, ws.data_ptr(),
                                        ws.numel(), _stream_ptr(nc.device)),
          "vits_maximum_path_lengths")
    return path


def maximum_path_durations(neg_cent: torch.Tensor, t_t: torch.Tensor, t_s: torch.Tensor, *,
                           scores: bool = True, frame_token: bool = False):
    """Forced alignment of neg_cent [B, Tt, Ts] fp32 at per-row lengths t_t /
    t_s (int32 [B], device): the DP and backtrack of maximum_path_lengths
    with the path reduced in the kernel (vits_maximum_path_durations; no [B,
    Tt, Ts] path is written).  Returns (durations int32 [B, Ts], scores fp32
    [B, Ts] or None, frame_token int32 [B, Tt] or None): frames per token, the
    sequential fp32 sum of the token's neg_cent entries, the token of every
    frame (-1 past the row's frames).  A row with an empty side or fewer
    frames than tokens has no alignment: durations 0, scores 0, tokens -1.
    No host sync: capture-safe."""
    require_device(neg_cent, t_t, t_s)
    if neg_cent.dim() != 3:
        raise _lib.VitsAmdError(f"maximum_path_durations: neg_cent {tuple(neg_cent.shape)}")
    nc = neg_cent.detach().to(torch.float32).contiguous()
    B, Tt, Ts = nc.shape
    tt = t_t.to(torch.int32).contiguous()
    ts = t_s.to(torch.int32).contiguous()
    if tt.numel() != B or ts.numel() != B:
        raise _lib.VitsAmdError(f"maximum_path_durations: {B} rows need {B} lengths, got "
                                f"{tt.numel()} and {ts.numel()}")
    dur = torch.empty(B, Ts, device=nc.device, dtype=torch.int32)
    sc = torch.empty(B, Ts, device=nc.device, dtype=torch.float32) if scores else None
    ft = torch.empty(B, Tt, device=nc.device, dtype=torch.int32) if frame_token else None
    lib = _lib.load()
    wsb = int(lib.vits_maximum_path_workspace(B, Tt, Ts))
    ws = torch.empty(max(wsb, 16), device=nc.device, dtype=torch.uint8)
    check(lib.vits_maximum_path_durations(nc.data_ptr(), tt.data_ptr(), ts.data_ptr(),
                                          dur.data_ptr(), _ptr(sc), _ptr(ft), B, Tt, Ts,
                                          ws.data_ptr(), ws.numel(), _stream_ptr(nc.device)),
          "vits_maximum_path_durations")
    return dur, sc, ft


MAS_LONG_STRIPS = (64, 128, 256, 512, 1024, 2048)


def mas_long_plan(Tt: int, Ts: int, strip: int, panel: int) -> tuple[int, int]:
    """(strip, panel) the long MAS runs a [Tt, Ts] job at: the asked-for ones,
    shrunk to the narrowest strip that still holds Ts and to Tt rounded up to
    whole decision words where the job is smaller than one strip / panel."""
    strip, panel = int(strip), int(panel)
    if strip not in MAS_LONG_STRIPS:
        raise _lib.VitsAmdError(f"maximum_path_durations_long: strip {strip} not in "
                                f"{MAS_LONG_STRIPS}")
    if panel <= 0 or panel % 32:
        raise _lib.VitsAmdError(f"maximum_path_durations_long: panel {panel} is no positive "
                                "multiple of 32")
    strip = min(strip, next(s for s in MAS_LONG_STRIPS if s >= min(Ts, MAS_LONG_STRIPS[-1])))
    panel = min(panel, (Tt + 31) // 32 * 32)
    return strip, panel


class _MasLongJob:
    """Allocation and launches of one long MAS job (vits_mas_long_*)."""

    def __init__(self, what, B, Tt, Ts, t_t, t_s, strip, panel, scores, frame_token, device):
        self.what = what
        self.lib = _lib.load()
        self.B, self.Tt, self.Ts = B, Tt, Ts
        self.strip, self.panel = mas_long_plan(Tt, Ts, strip, panel)
        self.tt = t_t.to(torch.int32).contiguous()
        self.ts = t_s.to(torch.int32).contiguous()
        if self.tt.numel() != B or self.ts.numel() != B:
            raise _lib.VitsAmdError(f"{what}: {B} rows need {B} lengths, got {self.tt.numel()} "
                                    f"and {self.ts.numel()}")
        wsb = int(self.lib.vits_mas_long_workspace(B, Tt, Ts, self.strip, self.panel))
        if wsb <= 0:
            raise _lib.VitsAmdError(f"{what}: no plan for [{B}, {Tt}, {Ts}] at strip "
                                    f"{self.strip}, panel {self.panel}")
        self.ws = torch.empty(wsb, device=device, dtype=torch.uint8)
        self.dur = torch.empty(B, Ts, device=device, dtype=torch.int32)
        self.sc = torch.empty(B, Ts, device=device, dtype=torch.float32) if scores else None
        self.ft = torch.empty(B, Tt, device=device, dtype=torch.int32) if frame_token else None
        self.stream = _stream_ptr(device)

    def panels(self):
        return [(y0, min(self.panel, self.Tt - y0)) for y0 in range(0, self.Tt, self.panel)]

    def _dims(self):
        return (self.B, self.Tt, self.Ts, self.strip, self.panel)

    def _tail(self):
        return (self.ws.data_ptr(), self.ws.numel(), self.stream)

    def forward(self, ptr, bstride, y0, rows):
        check(self.lib.vits_mas_long_panel(ptr, bstride, self.tt.data_ptr(), self.ts.data_ptr(),
                                           *self._dims(), y0, rows, *self._tail()),
              "vits_mas_long_panel")

    def backtrack(self):
        check(self.lib.vits_mas_long_backtrack(self.tt.data_ptr(), self.ts.data_ptr(),
                                               self.dur.data_ptr(), _ptr(self.ft), *self._dims(),
                                               *self._tail()), "vits_mas_long_backtrack")

    def gather(self, ptr, bstride, y0, rows):
        check(self.lib.vits_mas_long_gather(ptr, bstride, self.tt.data_ptr(), self.ts.data_ptr(),
                                            *self._dims(), y0, rows, *self._tail()),
              "vits_mas_long_gather")

    def sums(self):
        check(self.lib.vits_mas_long_scores(self.tt.data_ptr(), self.ts.data_ptr(),
                                            self.sc.data_ptr(), *self._dims(), *self._tail()),
              "vits_mas_long_scores")

    def result(self):
        return self.dur, self.sc, self.ft


def maximum_path_durations_panels(neg_cent: torch.Tensor, t_t: torch.Tensor, t_s: torch.Tensor, *,
                                  strip: int, panel: int, scores: bool = True,
                                  frame_token: bool = False):
    """maximum_path_durations through the kernels of the long search
    (vits_mas_long_*): the materialised neg_cent [B, Tt, Ts] fp32 is fed
    ``panel`` frames at a time and searched in strips of ``strip`` tokens, Ts
    of any size.  Same outputs, bit for bit.  No host sync: capture-safe."""
    what = "maximum_path_durations_panels"
    require_device(neg_cent, t_t, t_s)
    if neg_cent.dim() != 3:
        raise _lib.VitsAmdError(f"{what}: neg_cent {tuple(neg_cent.shape)}")
    nc = neg_cent.detach().to(torch.float32).contiguous()
    B, Tt, Ts = nc.shape
    job = _MasLongJob(what, B, Tt, Ts, t_t, t_s, strip, panel, scores, frame_token, nc.device)
    at = lambda y0: nc.data_ptr() + 4 * y0 * Ts
    for y0, rows in job.panels():
        job.forward(at(y0), Tt * Ts, y0, rows)
    job.backtrack()
    if scores:
        for y0, rows in job.panels():
            job.gather(at(y0), Tt * Ts, y0, rows)
        job.sums()
    return job.result()


def maximum_path_durations_long(z_p: torch.Tensor, m_p: torch.Tensor, logs_p: torch.Tensor,
                                t_t: torch.Tensor, t_s: torch.Tensor, *, strip: int = 2048,
                                panel: int = 4096, scores: bool = True,
                                frame_token: bool = False):
    """Forced alignment from the latents, for recordings and texts of any
    length: maximum_path_durations(neg_cent(z_p, m_p, logs_p), t_t, t_s) in
    every bit, without the [B, Tt, Ts] matrix.  z_p [B, C, Tt], m_p / logs_p
    [B, C, Ts] fp32.  A panel of ``panel`` frames of z_p is copied out
    (copy_windows), scored by the neg_cent kernel and searched; with
    ``scores`` a second sweep scores every panel again (the same kernel, the
    same bits) and gathers the path's entries.  Memory: one panel of scores
    and the decision words (Tt * Ts / 8 bytes).  No host sync: capture-safe."""
    what = "maximum_path_durations_long"
    require_device(z_p, m_p, logs_p, t_t, t_s)
    z = z_p.detach().to(torch.float32).contiguous()
    m = m_p.detach().to(torch.float32).contiguous()
    lg = logs_p.detach().to(torch.float32).contiguous()
    if z.dim() != 3 or m.shape != lg.shape or m.dim() != 3 or m.shape[:2] != z.shape[:2]:
        raise _lib.VitsAmdError(f"{what}: z_p {tuple(z.shape)} m_p {tuple(m.shape)} "
                                f"logs_p {tuple(lg.shape)}")
    B, C, Tt = z.shape
    Ts = m.shape[2]
    if B > COPY_MAX_JOBS:
        raise _lib.VitsAmdError(f"{what}: at most {COPY_MAX_JOBS} recordings a call")
    job = _MasLongJob(what, B, Tt, Ts, t_t, t_s, strip, panel, scores, frame_token, z.device)
    zpan = torch.empty(B * C * job.panel, device=z.device, dtype=torch.float32)
    nc = torch.empty(B * job.panel * Ts, device=z.device, dtype=torch.float32)

    def score(y0, rows):
        # rows frames of every recording, contiguous [B][C][rows]
        copy_windows(z, zpan, [(b * C * Tt + y0, b * C * rows, rows, rows) for b in range(B)],
                     channels=C, src_rstride=Tt, dst_rstride=rows)
        check(job.lib.vits_neg_cent(zpan.data_ptr(), m.data_ptr(), lg.data_ptr(), nc.data_ptr(),
                                    B, C, rows, Ts, job.stream), "vits_neg_cent")

    for y0, rows in job.panels():
        score(y0, rows)
        job.forward(nc.data_ptr(), rows * Ts, y0, rows)
    job.backtrack()
    if scores:
        for y0, rows in job.panels():
            score(y0, rows)
            job.gather(nc.data_ptr(), rows * Ts, y0, rows)
        job.sums()
    return job.result()


# ---------------------------------------------------------------------------
# STFT magnitude with autograd
# ---------------------------------------------------------------------------


def _stft_frames(what: str, B: int, L: int, n_fft: int, hop: int, win: int, pad: int) -> int:
    """Frames of a reflect-padded [B, L] signal; a padded signal shorter than
    one frame has none (torch.stft raises): refused here, so no empty tensor
    reaches the library."""
    if hop <= 0 or L + 2 * pad < n_fft:
        raise _lib.VitsAmdError(
            f"{what}: no frame fits: x [{B}, {L}] with pad {pad} gives {L + 2 * pad} samples "
            f"for n_fft {n_fft} (hop {hop}, win {win})")
    return (L + 2 * pad - n_fft) // hop + 1


class _StftMag(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, window, n_fft, hop, win, pad, eps):
        require_device(x, window)
        x = x.contiguous().float()
        window = window.contiguous().float()
        B, L = x.shape
        frames = _stft_frames("stft_mag", B, L, n_fft, hop, win, pad)
        nb = n_fft // 2 + 1
        mag = torch.empty(B, nb, frames, device=x.device, dtype=torch.float32)
        need_grad = ctx.needs_input_grad[0]
        re = torch.empty_like(mag) if need_grad else None
        im = torch.empty_like(mag) if need_grad else None
        lib = _lib.load()
        check(lib.vits_stft_mag_forward(x.data_ptr(), B, L, window.data_ptr(), n_fft, hop, win, pad,
                                        eps, mag.data_ptr(), _ptr(re), _ptr(im),
                                        _stream_ptr(x.device)), "vits_stft_mag_forward")
        if need_grad:
            ctx.save_for_backward(mag, re, im, window)
        ctx.cfg = (B, L, n_fft, hop, win, pad)
        return mag

    @staticmethod
    def backward(ctx, gmag):
        mag, re, im, window = ctx.saved_tensors
        B, L, n_fft, hop, win, pad = ctx.cfg
        gmag = gmag.contiguous().float()
        gx = torch.empty(B, L, device=gmag.device, dtype=torch.float32)
        lib = _lib.load()
        nws = int(lib.vits_stft_workspace(B, L, n_fft, hop, pad))
        ws = torch.empty(max(nws, 1), device=gmag.device, dtype=torch.float32)
        check(lib.vits_stft_mag_backward(gmag.data_ptr(), mag.data_ptr(), re.data_ptr(),
                                         im.data_ptr(), window.data_ptr(), B, L, n_fft, hop, win,
                                         pad, gx.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream_ptr(gmag.device)), "vits_stft_mag_backward")
        return gx, None, None, None, None, None, None


class _StftMagMulti(torch.autograd.Function):
    """Magnitudes of several (signal, resolution) jobs in one launch each way
    (vits_stft_mag_{forward,backward}_multi); gradients flow to every input
    signal that requires them."""

    @staticmethod
    def forward(ctx, specs, *xs):
        # specs: tuple of (window, n_fft, hop, win, pad, eps) per job
        require_device(*xs)
        jobs = (_lib.StftJob * len(xs))()
        keep, mags, saved = [], [], []
        for i, (x, (window, n_fft, hop, win, pad, eps)) in enumerate(zip(xs, specs)):
            x = x.contiguous().float()
            window = window.contiguous().float()
            B, L = x.shape
            frames = _stft_frames(f"stft_mag_multi job {i}", B, L, n_fft, hop, win, pad)
            # frame-major storage (coalesced kernel stores, layout 1); the
            # caller gets the [B, n_fft/2+1, frames] view torch.stft returns
            mag = torch.empty(B, frames, n_fft // 2 + 1, device=x.device, dtype=torch.float32)
            need = ctx.needs_input_grad[i + 1]
            re = torch.empty_like(mag) if need else None
            im = torch.empty_like(mag) if need else None
            j = jobs[i]
            j.x, j.window, j.mag, j.re, j.im = x.data_ptr(), window.data_ptr(), mag.data_ptr(), \
                _ptr(re), _ptr(im)
            j.batch, j.length, j.n_fft, j.hop, j.win, j.pad, j.eps = B, L, n_fft, hop, win, pad, eps
            j.layout = 1
            keep += [x, window]
            mags.append(mag.transpose(1, 2))
            saved.append((mag, re, im, window, B, L, n_fft, hop, win, pad) if need else None)
        check(_lib.load().vits_stft_mag_forward_multi(jobs, len(xs), _stream_ptr(xs[0].device)),
              "vits_stft_mag_forward_multi")
        ctx.saved = saved
        ctx.dev = xs[0].device
        # magnitudes of signals that need no gradient (the MR-STFT target y)
        # stay plain tensors, as torch.stft of such a signal would be
        nd = [m for m, sv in zip(mags, saved) if sv is None]
        if nd:
            ctx.mark_non_differentiable(*nd)
        return tuple(mags)

    @staticmethod
    def backward(ctx, *gmags):
        idx = [i for i, sv in enumerate(ctx.saved) if sv is not None]
        grads = [None] * len(ctx.saved)
        if not idx:
            return (None,) + tuple(grads)
        jobs = (_lib.StftJob * len(idx))()
        keep = []
        for q, i in enumerate(idx):
            mag, re, im, window, B, L, n_fft, hop, win, pad = ctx.saved[i]
            g = gmags[i]
            # frame-major like the saved forward outputs (free when the
            # gradient is itself a transposed view of frame-major storage)
            g = torch.zeros_like(mag) if g is None else g.transpose(1, 2).contiguous().float()
            gx = torch.empty(B, L, device=ctx.dev, dtype=torch.float32)
            j = jobs[q]
            j.grad_mag, j.mag, j.re, j.im, j.window, j.grad_x = g.data_ptr(), mag.data_ptr(), \
                re.data_ptr(), im.data_ptr(), window.data_ptr(), gx.data_ptr()
            j.batch, j.length, j.n_fft, j.hop, j.win, j.pad = B, L, n_fft, hop, win, pad
            j.layout = 1
            keep.append(g)
            grads[i] = gx
        lib = _lib.load()
        nws = int(lib.vits_stft_workspace_multi(jobs, len(idx)))
        ws = torch.empty(max(nws, 1), device=ctx.dev, dtype=torch.float32)
        check(lib.vits_stft_mag_backward_multi(jobs, len(idx), ws.data_ptr(), ws.numel(),
                                               _stream_ptr(ctx.dev)), "vits_stft_mag_backward_multi")
        return (None,) + tuple(grads)


def stft_mag_multi(xs, specs):
    """[sqrt(|STFT(x_i)|^2 + eps_i)] for jobs (x_i, window_i, n_fft_i, hop_i,
    win_i, pad_i, eps_i) in one launch (at most 16 jobs); differentiable in
    every x_i.  specs: sequence of (window, n_fft, hop, win, pad, eps)."""
    if len(xs) > 16:
        raise _lib.VitsAmdError("stft_mag_multi: at most 16 jobs per launch")
    specs = tuple((w, int(n), int(h), int(wl), int(n) // 2 if p is None else int(p), float(e))
                  for (w, n, h, wl, p, e) in specs)
    # cast outside the Function so autograd returns gradients in each x's dtype
    return list(_StftMagMulti.apply(specs, *[x.float() for x in xs]))


def stft_mag(x: torch.Tensor, window: torch.Tensor, n_fft: int, hop: int, win: int,
             pad: Optional[int] = None, eps: float = 1e-7) -> torch.Tensor:
    """sqrt(|STFT(x)|^2 + eps), [B, n_fft//2+1, frames]; differentiable in x."""
    if pad is None:
        pad = n_fft // 2
    # cast outside the Function so autograd returns the gradient in x's dtype
    # (fp16 under autocast, as y_hat is in train_stft.py)
    return _StftMag.apply(x.float(), window, n_fft, hop, win, pad, eps)


def stft_rows_frames(length: int, n_fft: int, hop: int, pad: int,
                     frames_cap: Optional[int] = None, cap: Optional[int] = None) -> int:
    """Frames stft_mag_rows gives a row of ``length`` samples (the host
    restatement of csrc/stft.hip stft_row_job)."""
    L = max(0, int(length)) if cap is None else min(max(0, int(length)), int(cap))
    if L <= pad or L + 2 * pad < n_fft:
        return 0
    frames = (L + 2 * pad - n_fft) // hop + 1
    return frames if frames_cap is None else min(frames, int(frames_cap))


def stft_mag_rows(x: torch.Tensor, lens: torch.Tensor, window: torch.Tensor, n_fft: int, hop: int,
                  win: int, frames_cap: int, pad: Optional[int] = None, eps: float = 1e-7,
                  out: Optional[torch.Tensor] = None, frames_out: Optional[torch.Tensor] = None):
    """Magnitude STFT of a ragged batch without a host sync: x [B, cap] fp32
    (rows may be strided), ``lens`` int32 [B] on the device.  Row b is
    transformed at its own length clamp(lens[b], 0, cap) - the reflect padding
    folds at its own end and nothing past it is read - into the first
    frames_b columns of mag [B, n_fft//2+1, frames_cap], bit for bit
    ``stft_mag`` of that row alone; later columns are 0.  Returns (mag,
    frames int32 [B]).  Inference only (not differentiable)."""
    if pad is None:
        pad = n_fft // 2
    require_device(x, lens, window)
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise _lib.VitsAmdError(f"stft_mag_rows: x must be fp32 [B, cap] with unit sample stride, "
                                f"got {x.dtype} {tuple(x.shape)}")
    B, cap = x.shape
    if lens.dtype != torch.int32 or tuple(lens.shape) != (B,) or not lens.is_contiguous():
        raise _lib.VitsAmdError(f"stft_mag_rows: lens must be a contiguous int32 [{B}] tensor")
    window = window.contiguous().float()
    nb = n_fft // 2 + 1
    if out is None:
        out = torch.empty(B, nb, int(frames_cap), device=x.device, dtype=torch.float32)
    if frames_out is None:
        frames_out = torch.empty(B, device=x.device, dtype=torch.int32)
    assert out.is_contiguous() and tuple(out.shape) == (B, nb, int(frames_cap))
    assert frames_out.is_contiguous() and frames_out.dtype == torch.int32
    check(_lib.load().vits_stft_mag_forward_rows(
        x.data_ptr(), x.stride(0) if B > 1 else cap, B, cap, lens.data_ptr(), window.data_ptr(),
        n_fft, hop, win, pad, eps, out.data_ptr(), int(frames_cap), frames_out.data_ptr(),
        _stream_ptr(x.device)), "vits_stft_mag_forward_rows")
    return out, frames_out


def posterior_sample(m: torch.Tensor, s: torch.Tensor, noise: Optional[torch.Tensor],
                     lens: torch.Tensor, noise_scale: float = 1.0, stage_mult=None,
                     out: Optional[torch.Tensor] = None):
    """z = m + noise * s * noise_scale for t < lens[b], 0 past it (noise None:
    z = m); m, s [B, C, T] fp32 views with unit time stride and equal strides,
    noise [B, C, T] contiguous, lens int32 [B].  With ``stage_mult`` also
    returns the int32 [len(stage_mult), B] lengths lens[b] * stage_mult[i]
    that the flow and decoder plans take (expand_durations' layout)."""
    require_device(m, s, noise, lens)
    B, Cc, T = m.shape
    assert m.dtype == torch.float32 and s.dtype == torch.float32
    assert m.stride() == s.stride() and m.stride(2) == 1
    if lens.dtype != torch.int32 or tuple(lens.shape) != (B,) or not lens.is_contiguous():
        raise _lib.VitsAmdError(f"posterior_sample: lens must be a contiguous int32 [{B}] tensor")
    if noise is not None:
        noise = noise.float().contiguous()
        assert tuple(noise.shape) == (B, Cc, T), noise.shape
    if out is None:
        out = torch.empty(B, Cc, T, device=m.device, dtype=torch.float32)
    stage_lens, mult, n_stage = None, None, 0
    if stage_mult is not None:
        n_stage = len(stage_mult)
        mult = (C.c_int32 * n_stage)(*[int(v) for v in stage_mult])
        stage_lens = torch.empty(n_stage, B, device=m.device, dtype=torch.int32)
    check(_lib.load().vits_posterior_sample(
        m.data_ptr(), s.data_ptr(), m.stride(0), m.stride(1), _ptr(noise), float(noise_scale),
        lens.data_ptr(), out.data_ptr(), B, Cc, T, _ptr(stage_lens), mult, n_stage,
        _stream_ptr(m.device)), "vits_posterior_sample")
    return out if stage_mult is None else (out, stage_lens)


# ---------------------------------------------------------------------------
# PCM output stage: polyphase resampler + int16 epilogue (csrc/post.hip)
# ---------------------------------------------------------------------------


def resample_ratio(orig_sr: int, target_sr: int) -> tuple[int, int]:
    """(up, down) of one resampling step of the wrappers (pitch, sampling
    rate): target / orig as a fraction with a denominator of at most 1000."""
    fr = Fraction(int(target_sr), int(orig_sr)).limit_denominator(1000)
    return fr.numerator, fr.denominator


def _reduced(up: int, down: int) -> tuple[int, int]:
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise _lib.VitsAmdError(f"resample: up and down must be >= 1, got {up}/{down}")
    g = math.gcd(up, down)
    return up // g, down // g


def resample_out_len(n: int, up: int, down: int) -> int:
    """len(scipy.signal.resample_poly(x[:n], up, down)) = ceil(n * up / down)."""
    up, down = _reduced(up, down)
    return -(-int(n) * up // down)


_RESAMPLE_FILTERS: dict = {}


def resample_filter(up: int, down: int, device="cpu") -> tuple[torch.Tensor, int]:
    """(table, half_len) of resample_poly's default filter for up / down
    (reduced by their gcd): h = float32(firwin(2 * half_len + 1, 1 / max(up,
    down), window=('kaiser', 5.0))) * float32(up), half_len = 10 * max(up,
    down), laid out by phase for the kernel: table [up, K] fp32 with
    table[r, k] = h[r + k * up] (zero past the last tap), so that
    table.t().reshape(-1)[:2 * half_len + 1] is h.  Designed once per (up,
    down, device) and cached; up == down has no filter."""
    up, down = _reduced(up, down)
    if up == down:
        raise _lib.VitsAmdError("resample_filter: up == down is a copy, it has no filter")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (up, down, device)
    hit = _RESAMPLE_FILTERS.get(key)
    if hit is None:
        from scipy.signal import firwin

        half_len = 10 * max(up, down)
        h = firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
        h = h.astype(np.float32) * np.float32(up)
        k = -(-(2 * half_len + 1) // up)
        flat = np.zeros(k * up, dtype=np.float32)
        flat[:h.size] = h
        table = torch.from_numpy(np.ascontiguousarray(flat.reshape(k, up).T)).to(device)
        hit = _RESAMPLE_FILTERS[key] = (table, half_len)
    return hit


def _post_launch(what, x, up, down, lengths, length_scale, out, out_lengths, volume, pcm):
    require_device(x, out, out_lengths)
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.VitsAmdError(f"{what}: x must be fp32, fp16 or bf16, got {x.dtype}")
    if x.dim() not in (1, 2) or x.stride(-1) != 1 or x.shape[-1] < 1:
        raise _lib.VitsAmdError(f"{what}: x must be [n] or [B, n] with unit stride along n")
    rows = x if x.dim() == 2 else x.unsqueeze(0)
    B, cap = rows.shape
    up, down = _reduced(up, down)
    if isinstance(lengths, torch.Tensor):
        require_device(lengths)
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous():
            raise _lib.VitsAmdError(f"{what}: lengths must be a contiguous int32 [{B}] tensor")
        lens_ptr, n_host, n_max = lengths.data_ptr(), 0, cap
    else:
        lens_ptr, n_host = None, cap if lengths is None else int(lengths)
        n_max = n_host
    odt = torch.int16 if pcm else torch.float32
    if out is None:
        out = torch.empty(B, max(1, resample_out_len(n_max, up, down)), device=x.device, dtype=odt)
        out_rows = out
    else:
        out_rows = out if out.dim() == 2 else out.unsqueeze(0)
        if (out.dtype != odt or out.dim() != x.dim() or out_rows.shape[0] != B
                or out.stride(-1) != 1 or out.shape[-1] < 1):
            raise _lib.VitsAmdError(f"{what}: out must be {odt}, {x.dim()}-d like x, unit stride")
    if out_lengths is not None and (out_lengths.dtype != torch.int32
                                    or tuple(out_lengths.shape) != (B,)
                                    or not out_lengths.is_contiguous()):
        raise _lib.VitsAmdError(f"{what}: out_lengths must be a contiguous int32 [{B}] tensor")
    x_bstride = rows.stride(0) if B > 1 else cap
    out_cap = out_rows.shape[1]
    out_bstride = out_rows.stride(0) if B > 1 else out_cap
    lib = _lib.load()
    if up == down and pcm and out_lengths is None:
        check(lib.vits_pcm16(rows.data_ptr(), _DT[x.dtype], x_bstride, cap, lens_ptr,
                             int(length_scale), n_host, float(volume), out_rows.data_ptr(),
                             out_bstride, out_cap, B, _stream_ptr(x.device)), what)
    else:
        table, half_len = (None, 0) if up == down else resample_filter(up, down, x.device)
        check(lib.vits_resample_poly(
            rows.data_ptr(), _DT[x.dtype], x_bstride, cap, lens_ptr, int(length_scale), n_host,
            _ptr(table), up, 0 if table is None else table.shape[1], up, down, half_len,
            None if pcm else out_rows.data_ptr(), out_rows.data_ptr() if pcm else None,
            out_bstride, out_cap, float(volume), _ptr(out_lengths), B, _stream_ptr(x.device)),
            what)
    return out if x.dim() == 2 else out.reshape(-1)


def resample_poly(x: torch.Tensor, up: int, down: int, *, lengths=None, length_scale: int = 1,
                  out: Optional[torch.Tensor] = None,
                  out_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scipy.signal.resample_poly(x, up, down) (defaults: Kaiser 5.0, zero
    extension) along the last axis of x [n] or [B, n] (fp32 / fp16 / bf16),
    fp32 out.  Row length: ``lengths`` None = all of x, an int = the same
    host length for every row, or an int32 [B] device tensor times the host
    integer ``length_scale`` (frame counts times the hop), read on the device
    without a host sync.  Samples at or past the length count as zero and
    out is zero from n_out = resample_out_len(length, up, down) to its end;
    ``out_lengths`` (int32 [B]) receives n_out for a following pass.  With
    ``out`` and ``out_lengths`` given, and the ratio's filter already cached
    (resample_filter, one eager call), the call allocates nothing and can be
    captured in a graph.  up == down (after reduction) is a masked copy."""
    return _post_launch("resample_poly", x, up, down, lengths, length_scale, out, out_lengths,
                        1.0, False)


def resample_pcm16(x: torch.Tensor, up: int, down: int, volume: float = 1.0, *, lengths=None,
                   length_scale: int = 1, out: Optional[torch.Tensor] = None,
                   out_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resample_poly with the int16 epilogue of pcm16 fused into the pass:
    int16 out, zero (silence) past n_out."""
    return _post_launch("resample_pcm16", x, up, down, lengths, length_scale, out, out_lengths,
                        volume, True)


def pcm16(x: torch.Tensor, volume: float = 1.0, *, lengths=None, length_scale: int = 1,
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """np.clip(x * volume * 32767, -32768, 32767).astype(np.int16) on the
    device, bit for bit for fp32 x (two fp32 multiplies in that order,
    truncation toward zero); zero past the row length (see resample_poly)."""
    return _post_launch("pcm16", x, 1, 1, lengths, length_scale, out, None, volume, True)


# -- span form: a stretch of the whole signal's output from a window of its input --


def resample_span_input(out_lo: int, out_hi: int, n_in: int, up: int, down: int,
                        half_len: Optional[int] = None) -> tuple[int, int]:
    """The exact input range [i_lo, i_hi) that the output samples [out_lo,
    out_hi) of resample_poly over a signal of ``n_in`` samples depend on: the
    inputs in [0, n_in) under one of the 2 * half_len + 1 taps of an output
    below n_out = resample_out_len(n_in, up, down) (outputs at or past n_out
    are zero and need nothing).  Output n reads the inputs i with 0 <= n *
    down - i * up + half_len <= 2 * half_len; both ends grow with n.  up ==
    down (the copy) needs [out_lo, min(out_hi, n_in)).  An empty need is (i,
    i).  ``half_len`` defaults to the filter's 10 * max(up, down), which is
    what a given value must equal.  Host integers only; this is the check
    vits_resample_poly_span makes on its window."""
    up, down = _reduced(up, down)
    out_lo, out_hi, n_in = int(out_lo), int(out_hi), int(n_in)
    if out_lo < 0 or out_hi < out_lo or n_in < 0:
        raise _lib.VitsAmdError(f"resample_span_input: bad span [{out_lo}, {out_hi}) of {n_in}")
    hl = 0 if up == down else 10 * max(up, down)
    if half_len is not None and up != down and int(half_len) != hl:
        raise _lib.VitsAmdError(f"resample_span_input: half_len of {up}/{down} is {hl}, got "
                                f"{half_len}")
    end = min(out_hi, resample_out_len(n_in, up, down))
    if end <= out_lo:
        i = out_lo if up == down else 0
        return i, i
    if up == down:
        return out_lo, end
    lo = max(0, -(-(out_lo * down - hl) // up))
    hi = min(n_in, ((end - 1) * down + hl) // up + 1)
    return (lo, hi) if lo < hi else (lo, lo)


def _span_launch(what, x, x_lo, n_in, up, down, out_lo, out_len, out, volume, pcm):
    require_device(x, out)
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.VitsAmdError(f"{what}: x must be fp32, fp16 or bf16, got {x.dtype}")
    if x.dim() != 1 or x.stride(0) != 1:
        raise _lib.VitsAmdError(f"{what}: x must be a window [x_len] with unit stride")
    up, down = _reduced(up, down)
    out_len = int(out_len)
    odt = torch.int16 if pcm else torch.float32
    if out is None:
        out = torch.empty(max(0, out_len), device=x.device, dtype=odt)
    if out.dtype != odt or out.dim() != 1 or out.stride(0) != 1 or out.numel() < out_len:
        raise _lib.VitsAmdError(f"{what}: out must be {odt} [>= {out_len}] with unit stride")
    table, half_len = (None, 0) if up == down else resample_filter(up, down, x.device)
    check(_lib.load().vits_resample_poly_span(
        x.data_ptr() if x.numel() else None, _DT[x.dtype], int(x_lo), x.numel(), int(n_in),
        _ptr(table), up, 0 if table is None else table.shape[1], up, down, half_len,
        None if pcm else out.data_ptr(), out.data_ptr() if pcm else None, int(out_lo), out_len,
        float(volume), _stream_ptr(x.device)), what)
    return out[:out_len]


def resample_poly_span(x: torch.Tensor, x_lo: int, n_in: int, up: int, down: int, out_lo: int,
                       out_len: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The samples [out_lo, out_lo + out_len) of resample_poly(whole, up,
    down) over a signal of ``n_in`` samples, bit for bit, from the window
    ``x`` [x_len] (fp32 / fp16 / bf16) that holds its samples [x_lo, x_lo +
    x_len): fp32 [out_len], zero from n_out on.  The window must hold
    resample_span_input(out_lo, out_lo + out_len, n_in, up, down); a shorter
    one is refused and nothing outside it is read.  Every offset is a host
    integer; with ``out`` given and the filter cached the call allocates
    nothing.  up == down is the copy."""
    return _span_launch("resample_poly_span", x, x_lo, n_in, up, down, out_lo, out_len, out, 1.0,
                        False)


def resample_pcm16_span(x: torch.Tensor, x_lo: int, n_in: int, up: int, down: int, out_lo: int,
                        out_len: int, volume: float = 1.0, *,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """resample_poly_span with the int16 epilogue of pcm16: the same span of
    resample_pcm16 over the whole signal (int16, silence from n_out on); up
    == down is the span form of pcm16."""
    return _span_launch("resample_pcm16_span", x, x_lo, n_in, up, down, out_lo, out_len, out,
                        volume, True)


PACK_MAX_BATCH = 64  # post.hip PK_MAX_BATCH


def pack_header_len(B: int) -> int:
    """int16 elements in front of pack_pcm's stream: the int32 [B + 1]
    offsets, rounded up to 16 bytes."""
    return -(-2 * (B + 1) // 8) * 8


def pack_pcm(rows: torch.Tensor, y_len: torch.Tensor, hop: int, passes=(), tail: int = 0, *,
             n_rows=None, out: Optional[torch.Tensor] = None, header: Optional[int] = None):
    """A request's segments in one buffer: rows int16 [B, cap] (the last post
    pass's output), each cut at n_out[b] = y_len[b] * hop passed through
    resample_out_len for every (up, down) of ``passes`` (at most two) and
    followed by ``tail`` zeros, written back to back.  ``out`` is ONE int16
    tensor: int32 offsets [B + 1] in front (``header`` int16 elements, at
    least pack_header_len(B); the caller may keep more words behind the
    offsets), then the stream, so a single device-to-host copy returns both;
    offsets[b + 1] = offsets[b] + n_out[b] + tail, rows at or past ``n_rows``
    (None, int or int32 [1] device tensor) add nothing.  y_len (int32 [B])
    and n_rows are read on the device: no host sync, capturable.  Returns
    (out, offsets int32 [B + 1] view, stream int16 view)."""
    require_device(rows, y_len, out)
    if rows.dtype != torch.int16 or rows.dim() != 2 or rows.stride(1) != 1:
        raise _lib.VitsAmdError("pack_pcm: rows must be int16 [B, cap] with unit stride along cap")
    B, cap = rows.shape
    if B > PACK_MAX_BATCH:
        raise _lib.VitsAmdError(f"pack_pcm: at most {PACK_MAX_BATCH} rows, got {B}")
    if y_len.dtype != torch.int32 or tuple(y_len.shape) != (B,) or not y_len.is_contiguous():
        raise _lib.VitsAmdError(f"pack_pcm: y_len must be a contiguous int32 [{B}] tensor")
    passes = [_reduced(u, d) for u, d in passes]
    passes = [(u, d) for u, d in passes if u != d]
    if len(passes) > 2:
        raise _lib.VitsAmdError("pack_pcm: at most two resampling passes")
    tail = int(tail)
    header = pack_header_len(B) if header is None else int(header)
    if header < pack_header_len(B) or header % 8:
        raise _lib.VitsAmdError(f"pack_pcm: header must be a multiple of 8, >= {pack_header_len(B)}")
    if out is None:
        out = torch.empty(header + B * (cap + tail), device=rows.device, dtype=torch.int16)
    if out.dtype != torch.int16 or out.dim() != 1 or not out.is_contiguous() or out.numel() <= header:
        raise _lib.VitsAmdError("pack_pcm: out must be a contiguous int16 [> header] tensor")
    offsets = out[:2 * (B + 1)].view(torch.int32)
    stream = out[header:]
    up = (C.c_int32 * 2)(*([u for u, _ in passes] + [1] * (2 - len(passes))))
    down = (C.c_int32 * 2)(*([d for _, d in passes] + [1] * (2 - len(passes))))
    keep, nr_ptr = _n_rows_ptr(n_rows, B, rows.device, "pack_pcm")
    check(_lib.load().vits_pack_pcm(
        rows.data_ptr(), rows.stride(0) if B > 1 else cap, cap, y_len.data_ptr(), int(hop), up,
        down, len(passes), tail, nr_ptr, B, offsets.data_ptr(), stream.data_ptr(),
        stream.numel(), _stream_ptr(rows.device)), "vits_pack_pcm")
    return out, offsets, stream


# -- per-row output stage: rows of different requests in one launch -------------


def _row_ratios(what: str, ratios, B: int):
    ratios = [_reduced(u, d) for u, d in ratios]
    if len(ratios) != B:
        raise _lib.VitsAmdError(f"{what}: one (up, down) per row: {B} rows, got {len(ratios)}")
    return ratios


def resample_rows(x: torch.Tensor, passes_per_row, *, lengths: torch.Tensor,
                  length_scale: int = 1, volumes=None, pcm: bool = False,
                  out: Optional[torch.Tensor] = None,
                  out_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE resampling pass over x [B, cap] (fp32 / fp16 / bf16) in which row b
    has its own ratio: ``passes_per_row`` holds one (up, down) per row, (1,
    1) being the masked copy.  Row b is bit for bit resample_poly(x[b], up,
    down) (``pcm=False``: fp32 out) or resample_pcm16 / pcm16 with
    ``volumes[b]`` (``pcm=True``: int16 out; volumes None = 1.0).  The row
    length is ``lengths[b] * length_scale`` (int32 [B] device tensor, read on
    the device).  ``out`` is [B, out_cap] for one shared out_cap (default:
    the largest resample_out_len(cap, up, down) of the rows); every row is
    zero from its own n_out to out_cap and ``out_lengths`` (int32 [B])
    receives n_out.  The filters are the cached tables of resample_filter
    (the cache keeps them alive); the descriptors travel in the kernel
    arguments, so the call makes no copy.  At most PACK_MAX_BATCH rows."""
    what = "resample_rows"
    require_device(x, lengths, out, out_lengths)
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.VitsAmdError(f"{what}: x must be fp32, fp16 or bf16, got {x.dtype}")
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < 1:
        raise _lib.VitsAmdError(f"{what}: x must be [B, n] with unit stride along n")
    B, cap = x.shape
    if B > PACK_MAX_BATCH:
        raise _lib.VitsAmdError(f"{what}: at most {PACK_MAX_BATCH} rows, got {B}")
    ratios = _row_ratios(what, passes_per_row, B)
    if (not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32
            or tuple(lengths.shape) != (B,) or not lengths.is_contiguous()):
        raise _lib.VitsAmdError(f"{what}: lengths must be a contiguous int32 [{B}] device tensor")
    volumes = [1.0] * B if volumes is None else [float(v) for v in volumes]
    if len(volumes) != B:
        raise _lib.VitsAmdError(f"{what}: one volume per row: {B} rows, got {len(volumes)}")
    odt = torch.int16 if pcm else torch.float32
    if out is None:
        out_cap = max(resample_out_len(cap, u, d) for u, d in ratios)
        out = torch.empty(B, max(1, out_cap), device=x.device, dtype=odt)
    if (out.dtype != odt or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1
            or out.shape[1] < 1):
        raise _lib.VitsAmdError(f"{what}: out must be {odt} [{B}, out_cap] with unit stride")
    if out_lengths is not None and (out_lengths.dtype != torch.int32
                                    or tuple(out_lengths.shape) != (B,)
                                    or not out_lengths.is_contiguous()):
        raise _lib.VitsAmdError(f"{what}: out_lengths must be a contiguous int32 [{B}] tensor")
    rows = (_lib.PostRow * B)()
    for b, (up, down) in enumerate(ratios):
        table, half_len = (None, 0) if up == down else resample_filter(up, down, x.device)
        rows[b] = _lib.PostRow(_ptr(table), up, down, half_len,
                               0 if table is None else table.shape[1], volumes[b], 0)
    out_cap = out.shape[1]
    check(_lib.load().vits_resample_poly_rows(
        x.data_ptr(), _DT[x.dtype], x.stride(0) if B > 1 else cap, cap, lengths.data_ptr(),
        int(length_scale), rows, None if pcm else out.data_ptr(), out.data_ptr() if pcm else None,
        out.stride(0) if B > 1 else out_cap, out_cap, _ptr(out_lengths), B,
        _stream_ptr(x.device)), "vits_resample_poly_rows")
    return out


def pack_pcm_rows(rows: torch.Tensor, y_len: torch.Tensor, hop: int, passes_per_row, tails, *,
                  n_rows=None, out: Optional[torch.Tensor] = None,
                  header: Optional[int] = None):
    """pack_pcm for rows of different requests: ``passes_per_row[b]`` is row
    b's list of at most two (up, down) passes and ``tails[b]`` its tail, so
    n_out[b] and offsets[b + 1] = offsets[b] + n_out[b] + tails[b] follow the
    row's own output stage.  Everything else (the layout of ``out``, n_rows,
    no host sync) as pack_pcm; ``out`` defaults to header + B * (cap +
    max(tails)) elements."""
    what = "pack_pcm_rows"
    require_device(rows, y_len, out)
    if rows.dtype != torch.int16 or rows.dim() != 2 or rows.stride(1) != 1:
        raise _lib.VitsAmdError(f"{what}: rows must be int16 [B, cap] with unit stride along cap")
    B, cap = rows.shape
    if B > PACK_MAX_BATCH:
        raise _lib.VitsAmdError(f"{what}: at most {PACK_MAX_BATCH} rows, got {B}")
    if y_len.dtype != torch.int32 or tuple(y_len.shape) != (B,) or not y_len.is_contiguous():
        raise _lib.VitsAmdError(f"{what}: y_len must be a contiguous int32 [{B}] tensor")
    passes_per_row, tails = list(passes_per_row), [int(t) for t in tails]
    if len(passes_per_row) != B or len(tails) != B or min(tails) < 0:
        raise _lib.VitsAmdError(f"{what}: one pass list and one tail >= 0 per row ({B} rows)")
    up, down = (C.c_int32 * (2 * B))(), (C.c_int32 * (2 * B))()
    for b, passes in enumerate(passes_per_row):
        passes = [(u, d) for u, d in (_reduced(u, d) for u, d in passes) if u != d]
        if len(passes) > 2:
            raise _lib.VitsAmdError(f"{what}: at most two resampling passes per row")
        for i in range(2):
            up[2 * b + i], down[2 * b + i] = passes[i] if i < len(passes) else (1, 1)
    header = pack_header_len(B) if header is None else int(header)
    if header < pack_header_len(B) or header % 8:
        raise _lib.VitsAmdError(f"{what}: header must be a multiple of 8, >= {pack_header_len(B)}")
    if out is None:
        out = torch.empty(header + B * (cap + max(tails)), device=rows.device, dtype=torch.int16)
    if out.dtype != torch.int16 or out.dim() != 1 or not out.is_contiguous() or out.numel() <= header:
        raise _lib.VitsAmdError(f"{what}: out must be a contiguous int16 [> header] tensor")
    offsets = out[:2 * (B + 1)].view(torch.int32)
    stream = out[header:]
    keep, nr_ptr = _n_rows_ptr(n_rows, B, rows.device, what)
    check(_lib.load().vits_pack_pcm_rows(
        rows.data_ptr(), rows.stride(0) if B > 1 else cap, cap, y_len.data_ptr(), int(hop), up,
        down, (C.c_int32 * B)(*tails), nr_ptr, B, offsets.data_ptr(), stream.data_ptr(),
        stream.numel(), _stream_ptr(rows.device)), "vits_pack_pcm_rows")
    return out, offsets, stream


# -- window copy: the gathers and the scatter of long-recording conversion ------

COPY_MAX_JOBS = 64  # window.hip CW_MAX_JOBS


def copy_windows(src: torch.Tensor, dst: torch.Tensor, jobs, *, channels: int = 1,
                 src_rstride: int = 0, dst_rstride: int = 0) -> torch.Tensor:
    """Ranges of fp32 elements from ``src`` into ``dst``, both contiguous and
    addressed flat (element offsets into their storage as laid out): for
    every job (src_off, dst_off, len, fill_len) and channel r < ``channels``,
    dst[dst_off + r * dst_rstride + i] = src[src_off + r * src_rstride + i]
    for i < len and 0 for len <= i < fill_len; nothing else is written.  64
    jobs are one launch (more: one launch per 64); the jobs travel in the
    kernel arguments, so the call makes no copy, allocates nothing and can be
    captured.  A job that leaves either tensor is refused.  Returns dst."""
    what = "copy_windows"
    require_device(src, dst)
    for name, t in (("src", src), ("dst", dst)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.VitsAmdError(f"{what}: {name} must be a contiguous fp32 tensor")
    jobs = [tuple(int(v) for v in j) for j in jobs]
    if any(len(j) != 4 for j in jobs):
        raise _lib.VitsAmdError(f"{what}: a job is (src_off, dst_off, len, fill_len)")
    lib = _lib.load()
    for lo in range(0, len(jobs), COPY_MAX_JOBS):
        part = jobs[lo:lo + COPY_MAX_JOBS]
        table = (_lib.WindowJob * len(part))(*[_lib.WindowJob(*j) for j in part])
        check(lib.vits_copy_windows(
            src.data_ptr(), src.numel(), int(src_rstride), dst.data_ptr(), dst.numel(),
            int(dst_rstride), table, len(part), int(channels), _stream_ptr(src.device)),
            "vits_copy_windows")
    return dst


# ---------------------------------------------------------------------------
# speech editing (edit.hip)
# ---------------------------------------------------------------------------


def _edit_arg(what: str, t, dtype, shape, name: str, optional: bool = False):
    """A contiguous device tensor of exactly this dtype and shape (or None
    where ``optional``)."""
    if t is None and optional:
        return None
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape)
            or not t.is_contiguous()):
        raise _lib.VitsAmdError(f"{what}: {name} must be a contiguous {dtype} {list(shape)} tensor")
    require_device(t)
    return t


def edit_pins(dur_old: torch.Tensor, x_len_old: torch.Tensor, x_len_new: torch.Tensor,
              t_x_new: int, spans: torch.Tensor, y_len_old: torch.Tensor, *,
              span_given: Optional[torch.Tensor] = None,
              span_target: Optional[torch.Tensor] = None):
    """The inputs of ``duration_plan`` over the new text of an edit, on the
    device (vits_edit_pins, include/vits_amd.h has the rule): ``dur_old``
    int32 [B, t_x_old] (rows may be strided), ``x_len_old`` / ``x_len_new`` /
    ``y_len_old`` int32 [B], ``spans`` int32 [B, 3] = a | b_old | b_new,
    ``span_given`` int32 [B, t_x_new] (the caller's pins, read inside the span
    only), ``span_target`` int32 [B] (> 0: the new span lasts exactly that
    many frames, 0: free, < 0: the row keeps its length).  Returns (given
    int32 [B, t_x_new], target int32 [B], meta int32 [3, B] = f0 | f1 |
    status); a status-1 row has all-zero pins and target 0."""
    what = "edit_pins"
    if (not isinstance(dur_old, torch.Tensor) or dur_old.dim() != 2
            or dur_old.dtype != torch.int32 or dur_old.stride(1) != 1
            or dur_old.stride(0) < dur_old.shape[1]):
        raise _lib.VitsAmdError(f"{what}: dur_old must be an int32 [B, t_x_old] tensor with "
                                "contiguous rows")
    require_device(dur_old)
    B, t_x_old = dur_old.shape
    t_x_new = int(t_x_new)
    i32 = torch.int32
    x_len_old = _edit_arg(what, x_len_old, i32, (B,), "x_len_old")
    x_len_new = _edit_arg(what, x_len_new, i32, (B,), "x_len_new")
    y_len_old = _edit_arg(what, y_len_old, i32, (B,), "y_len_old")
    spans = _edit_arg(what, spans, i32, (B, 3), "spans")
    span_given = _edit_arg(what, span_given, i32, (B, t_x_new), "span_given", True)
    span_target = _edit_arg(what, span_target, i32, (B,), "span_target", True)
    dev = dur_old.device
    given = torch.empty(B, t_x_new, device=dev, dtype=i32)
    target = torch.empty(B, device=dev, dtype=i32)
    meta = torch.empty(3, B, device=dev, dtype=i32)
    check(_lib.load().vits_edit_pins(
        dur_old.data_ptr(), dur_old.stride(0), x_len_old.data_ptr(), t_x_old,
        x_len_new.data_ptr(), t_x_new, spans.data_ptr(), _ptr(span_given), _ptr(span_target),
        y_len_old.data_ptr(), given.data_ptr(), target.data_ptr(), meta.data_ptr(), B,
        _stream_ptr(dev)), "vits_edit_pins")
    return given, target, meta


def edit_splice(dur_new: torch.Tensor, spans: torch.Tensor, y_len_old: torch.Tensor,
                m_p: torch.Tensor, s_p: torch.Tensor, noise: torch.Tensor, z_p_rec: torch.Tensor,
                *, x_len: Optional[torch.Tensor] = None, stage_mult=(1,),
                out: Optional[torch.Tensor] = None):
    """The spliced latents of an edit in one pass (vits_edit_splice): the
    recording's ``z_p_rec`` fp32 [B, C, t_rec] outside the edited frames, the
    prior expansion m_p + noise * s_p of the new span under ``dur_new`` (int32
    [B, t_x], ``duration_plan``'s) between them, zero past y_new.  ``m_p`` /
    ``s_p`` [B, C, t_x]; ``noise`` fp32 [B, C, t_y], pre-scaled and indexed by
    output frame, fixes the bucket t_y.  Returns (z fp32 [B, C, t_y], lens
    int32 [n_stage, B] = y_new * stage_mult, meta int32 [4, B] = f0 | n_new |
    f1 | status); status -1: y_new > t_y, 1: an inconsistent span; the row is
    then zero with length 0."""
    what = "edit_splice"
    require_device(dur_new, m_p, s_p, noise, z_p_rec)
    B, C_, t_x = m_p.shape
    dur_new = _durations_arg(dur_new, B, t_x, 1.0, False, what)
    i32 = torch.int32
    spans = _edit_arg(what, spans, i32, (B, 3), "spans")
    y_len_old = _edit_arg(what, y_len_old, i32, (B,), "y_len_old")
    x_len = _edit_arg(what, x_len, i32, (B,), "x_len", True)
    if noise.dim() != 3 or tuple(noise.shape[:2]) != (B, C_):
        raise _lib.VitsAmdError(f"{what}: noise must be fp32 [{B}, {C_}, t_y]")
    t_y = noise.shape[2]
    noise = _edit_arg(what, noise, torch.float32, (B, C_, t_y), "noise")
    if z_p_rec.dim() != 3:
        raise _lib.VitsAmdError(f"{what}: z_p_rec must be fp32 [{B}, {C_}, t_rec]")
    t_rec = z_p_rec.shape[2]
    z_p_rec = _edit_arg(what, z_p_rec, torch.float32, (B, C_, t_rec), "z_p_rec")
    m_p = m_p.float().contiguous()
    s_p = s_p.float().contiguous()
    dev = m_p.device
    if out is None:
        out = torch.empty(B, C_, t_y, device=dev, dtype=torch.float32)
    _edit_arg(what, out, torch.float32, (B, C_, t_y), "out")
    n_stage = len(stage_mult)
    lens = torch.empty(n_stage, B, device=dev, dtype=i32)
    meta = torch.empty(4, B, device=dev, dtype=i32)
    mult = (C.c_int32 * n_stage)(*[int(v) for v in stage_mult])
    check(_lib.load().vits_edit_splice(
        dur_new.data_ptr(), dur_new.stride(0), _ptr(x_len), t_x, spans.data_ptr(),
        y_len_old.data_ptr(), m_p.data_ptr(), s_p.data_ptr(), m_p.stride(0), m_p.stride(1),
        noise.data_ptr(), z_p_rec.data_ptr(), t_rec, out.data_ptr(), B, C_, t_y, lens.data_ptr(),
        mult, n_stage, meta.data_ptr(), _stream_ptr(dev)), "vits_edit_splice")
    return out, lens, meta


def edit_patch(orig: torch.Tensor, o: torch.Tensor, y_len_old: torch.Tensor,
               splice_meta: torch.Tensor, hop: int, *, margin: int, fade: int,
               out: Optional[torch.Tensor] = None):
    """The waveform side of an edit (vits_edit_patch states the arithmetic):
    the recording ``orig`` fp32 [B, n] (at the model rate) outside the edited
    frames widened by ``margin`` frames, the synthesis ``o`` fp32 [B, n_o]
    inside, a linear cross-fade of ``fade`` samples at each seam, the
    recording's tail shifted by the change of length.  ``splice_meta`` is
    edit_splice's.  Rows may be strided.  Returns (out fp32 [B, n_o], out_len
    int32 [B] = y_new * hop); a row that cannot be patched is zero with length
    0."""
    what = "edit_patch"
    require_device(orig, o, y_len_old, splice_meta)
    for name, t in (("orig", orig), ("o", o)):
        if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            raise _lib.VitsAmdError(f"{what}: {name} must be fp32 [B, n] with contiguous rows")
    B = o.shape[0]
    if orig.shape[0] != B:
        raise _lib.VitsAmdError(f"{what}: orig has {orig.shape[0]} rows, o {B}")
    y_len_old = _edit_arg(what, y_len_old, torch.int32, (B,), "y_len_old")
    splice_meta = _edit_arg(what, splice_meta, torch.int32, (4, B), "splice_meta")
    if out is None:
        out = torch.empty(B, o.shape[1], device=o.device, dtype=torch.float32)
    _edit_arg(what, out, torch.float32, (B, out.shape[1] if out.dim() == 2 else -1), "out")
    out_len = torch.empty(B, device=o.device, dtype=torch.int32)
    check(_lib.load().vits_edit_patch(
        orig.data_ptr(), orig.stride(0), orig.shape[1], o.data_ptr(), o.stride(0), o.shape[1],
        y_len_old.data_ptr(), splice_meta.data_ptr(), int(hop), int(margin), int(fade),
        out.data_ptr(), out.stride(0), out.shape[1], out_len.data_ptr(), B,
        _stream_ptr(o.device)), "vits_edit_patch")
    return out, out_len


# ---------------------------------------------------------------------------
# retiming a recording (retime.hip)
# ---------------------------------------------------------------------------


def _dur_rows(what: str, t, B, t_x, name: str):
    """An int32 [B, t_x] device tensor whose rows are contiguous (B / t_x None:
    taken from the tensor)."""
    if (not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.int32
            or t.stride(1) != 1 or t.stride(0) < t.shape[1]
            or (B is not None and tuple(t.shape) != (B, t_x))):
        shape = "[B, t_x]" if B is None else f"[{B}, {t_x}]"
        raise _lib.VitsAmdError(f"{what}: {name} must be an int32 {shape} tensor with contiguous "
                                "rows")
    require_device(t)
    return t


def retime_plan(dur_old: torch.Tensor, y_len_old: torch.Tensor, *,
                x_len: Optional[torch.Tensor] = None, given: Optional[torch.Tensor] = None,
                tok_scale: Optional[torch.Tensor] = None, rate: Optional[torch.Tensor] = None,
                target: Optional[torch.Tensor] = None, dur: Optional[torch.Tensor] = None,
                meta: Optional[torch.Tensor] = None):
    """A recording's new per-token durations from its old ones, on the device
    with no host sync (vits_retime_plan, include/vits_amd.h has the rule).
    ``dur_old`` int32 [B, t_x] (rows may be strided), ``y_len_old`` / ``x_len``
    int32 [B]; ``given`` int32 [B, t_x]: >= 0 pins a token to that many frames,
    < 0 leaves it free; ``tok_scale`` fp32 [B, t_x] and ``rate`` fp32 [B]
    multiply the free tokens' durations; ``target`` int32 [B]: > 0 = the row
    lasts exactly that many frames (``rate`` is then not applied).  Returns
    (dur_new int32 [B, t_x], total int32 [B], status int32 [B]); status 1: the
    row is inconsistent or its target cannot be met, and it keeps dur_old.
    With no control dur_new == dur_old."""
    what = "retime_plan"
    dur_old = _dur_rows(what, dur_old, None, None, "dur_old")
    B, t_x = dur_old.shape
    i32 = torch.int32
    y_len_old = _edit_arg(what, y_len_old, i32, (B,), "y_len_old")
    x_len = _edit_arg(what, x_len, i32, (B,), "x_len", True)
    given = _edit_arg(what, given, i32, (B, t_x), "given", True)
    tok_scale = _edit_arg(what, tok_scale, torch.float32, (B, t_x), "tok_scale", True)
    rate = _edit_arg(what, rate, torch.float32, (B,), "rate", True)
    target = _edit_arg(what, target, i32, (B,), "target", True)
    dev = dur_old.device
    if dur is None:
        dur = torch.empty(B, t_x, device=dev, dtype=i32)
    if meta is None:
        meta = torch.empty(2, B, device=dev, dtype=i32)
    _edit_arg(what, dur, i32, (B, t_x), "dur")
    _edit_arg(what, meta, i32, (2, B), "meta")
    check(_lib.load().vits_retime_plan(
        dur_old.data_ptr(), dur_old.stride(0), _ptr(x_len), t_x, y_len_old.data_ptr(),
        _ptr(given), _ptr(tok_scale), _ptr(rate), _ptr(target), dur.data_ptr(), meta.data_ptr(),
        B, _stream_ptr(dev)), "vits_retime_plan")
    return dur, meta[0], meta[1]


def retime_warp(z_p_rec: torch.Tensor, dur_old: torch.Tensor, dur_new: torch.Tensor,
                y_len_old: torch.Tensor, t_y: int, *, x_len: Optional[torch.Tensor] = None,
                stage_mult=(1,), out: Optional[torch.Tensor] = None):
    """The recording's latents ``z_p_rec`` fp32 [B, C, t_rec] resampled along
    time so that token x lasts dur_new[x] frames instead of dur_old[x]
    (vits_retime_warp: the centre-aligned piecewise-linear map of each token's
    new frames onto its old ones; the exact copy where the two agree).
    ``dur_old`` / ``dur_new`` int32 [B, t_x] (rows may be strided), ``t_y`` the
    output bucket.  Returns (z fp32 [B, C, t_y], zero past y_new, lens int32
    [n_stage, B] = y_new * stage_mult, meta int32 [2, B] = y_new | status);
    status -1: y_new > t_y or no recording; the row is then zero with length
    0 and y_new is still reported."""
    what = "retime_warp"
    if (not isinstance(z_p_rec, torch.Tensor) or z_p_rec.dim() != 3
            or z_p_rec.dtype != torch.float32 or not z_p_rec.is_contiguous()):
        raise _lib.VitsAmdError(f"{what}: z_p_rec must be a contiguous fp32 [B, C, t_rec] tensor")
    require_device(z_p_rec)
    B, C_, t_rec = z_p_rec.shape
    dur_old = _dur_rows(what, dur_old, None, None, "dur_old")
    if dur_old.shape[0] != B:
        raise _lib.VitsAmdError(f"{what}: dur_old has {dur_old.shape[0]} rows, z_p_rec {B}")
    t_x = dur_old.shape[1]
    dur_new = _dur_rows(what, dur_new, B, t_x, "dur_new")
    i32 = torch.int32
    y_len_old = _edit_arg(what, y_len_old, i32, (B,), "y_len_old")
    x_len = _edit_arg(what, x_len, i32, (B,), "x_len", True)
    t_y = int(t_y)
    dev = z_p_rec.device
    if out is None:
        out = torch.empty(B, C_, t_y, device=dev, dtype=torch.float32)
    _edit_arg(what, out, torch.float32, (B, C_, t_y), "out")
    n_stage = len(stage_mult)
    lens = torch.empty(n_stage, B, device=dev, dtype=i32)
    meta = torch.empty(2, B, device=dev, dtype=i32)
    mult = (C.c_int32 * n_stage)(*[int(v) for v in stage_mult])
    check(_lib.load().vits_retime_warp(
        z_p_rec.data_ptr(), t_rec, dur_old.data_ptr(), dur_old.stride(0), dur_new.data_ptr(),
        dur_new.stride(0), _ptr(x_len), t_x, y_len_old.data_ptr(), out.data_ptr(), B, C_, t_y,
        lens.data_ptr(), mult, n_stage, meta.data_ptr(), _stream_ptr(dev)), "vits_retime_warp")
    return out, lens, meta

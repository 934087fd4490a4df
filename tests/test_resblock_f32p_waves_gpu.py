"""csrc/resblock_f32p.hip's wave mapping at 64, 128 and 256 channels: the
32 x 64 wave tile (two, four and eight row-waves over the workgroup tile) and
the 64 x 64 one compute the two-conv path's bits.  Every case runs on BOTH
sides of the per-C build switches (VITS_RP_TM64 / 128 / 256): the shipped
library, and libvits_rp_other.so - the same source with every switch flipped.

Shapes: the smallest with a first, a middle, an end and a past-length tile at
each C (B = 2, the second utterance ends at 0.6 T):
  C = 64,  T = 512: three 256-column tiles, two row-waves
  C = 128, T = 384: four 128-column tiles, four row-waves
  C = 256, T = 256: three 128-column tiles, eight row-waves
(test_interior_tile adds the select-free tile paths at 64 and 256 channels).
A failure lists the mismatching (32-row block, 64-column block of the tile)
cells, which name the wave: a wrong row base or bias offset fails whole rows
of cells, a wrong column base whole columns."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from vits_amd import _lib, ops

pytestmark = pytest.mark.gpu

B = 2
SHAPES = {64: 512, 128: 384, 256: 256}
SIDES = ["shipped", "other"]
OTHER_LIB = os.path.join(os.path.dirname(_lib.lib_path()), "libvits_rp_other.so")


@functools.lru_cache(maxsize=None)
def _other():
    assert os.path.exists(OTHER_LIB), f"{OTHER_LIB} missing: make -C vits_amd/csrc builds it"
    lib = ctypes.CDLL(OTHER_LIB)
    fn = lib.vits_resblock_pair_f32p_forward
    fn.restype, fn.argtypes = _lib._SIGS["vits_resblock_pair_f32p_forward"]
    return fn


@functools.lru_cache(maxsize=None)
def _setup(dev_str, C, ks, dil, T):
    """Packed split-fp32 pairs (one per k in ks), inputs zero past the
    utterance lengths (as the decoder's are), conds; CPU copies for the fp64
    reference.  Built once per shape; nothing writes to it."""
    device = torch.device(dev_str)
    g = torch.Generator().manual_seed(1000 * C + 100 * sum(ks) + dil)
    ends = (T, (int(T * 0.6) // 4) * 4 + 1)  # (an odd end: inside a 4-step block)
    mask = torch.zeros(B, 1, T)
    for b, e in enumerate(ends):
        mask[b, :, :e] = 1
    packs, xs, cpu = [], [], []
    for k in ks:
        x = torch.randn(B, C, T, generator=g) * 0.5 * mask
        w1 = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
        b1 = torch.randn(C, generator=g) * 0.1
        w2 = torch.randn(C, C // 2, k, generator=g) / (C * k / 2) ** 0.5
        b2 = torch.randn(C, generator=g) * 0.1
        cond = torch.randn(B, C, generator=g) * 0.3
        c1 = ops.to_lowp(ops.pack_conv(w1.to(device), b1.to(device), dilation=dil, gate=True),
                         ops.WDT_F32S, min_rows=0)
        c2 = ops.to_lowp(ops.pack_conv(w2.to(device), b2.to(device)), ops.WDT_F32S, min_rows=0)
        assert c1.wdtype == c2.wdtype == ops.WDT_F32P
        packs.append((c1, c2, cond.to(device)))
        xs.append(x.to(device))
        cpu.append((x, w1, b1, cond, w2, b2, k))
    lengths = torch.tensor(ends, dtype=torch.int32, device=device)
    return packs, xs, cpu, lengths, ends


@functools.lru_cache(maxsize=None)
def _ref64(dev_str, C, ks, dil, T, j):
    """modules.py:251-259 for pair j in fp64, each utterance on its own
    length, zero past it."""
    _, _, cpu, _, ends = _setup(dev_str, C, ks, dil, T)
    x, w1, b1, cond, w2, b2, k = (t.double() if torch.is_tensor(t) else t for t in cpu[j])
    ref = torch.zeros(B, C, T, dtype=torch.float64)
    for b, e in enumerate(ends):
        xe = x[b:b + 1, :, :e]
        xt = F.conv1d(F.leaky_relu(xe, 0.1), w1, b1, dilation=dil, padding=(k - 1) * dil // 2)
        xa, xb = torch.chunk(xt, 2, dim=1)
        sa, sb = torch.chunk(cond[b:b + 1], 2, dim=1)
        xt = torch.tanh(xa + sa.unsqueeze(-1)) * torch.sigmoid(xb + sb.unsqueeze(-1))
        ref[b, :, :e] = (F.conv1d(xt, w2, b2, padding=(k - 1) // 2) + xe)[0]
    return ref


def _nan(C, T, device):
    # an element the kernel skips stays NaN and fails the comparison
    return torch.full((B, C, T), float("nan"), device=device)


def _fused(side, packs, xs, js, ys, device, lengths, **kw):
    descs = tuple(ops.resblock_pair_desc(packs[j][0], packs[j][1], xs[j], y, cond=packs[j][2],
                                         lengths=lengths, **kw) for j, y in zip(js, ys))
    if side == "shipped":
        ops.resblock_pair_launch(descs, B, device, ops.WDT_F32P)
    else:
        arr = (_lib.ResblockPairDesc * len(descs))(*descs)
        _lib.check(_other()(arr, len(descs), B, ops._stream_ptr(device)), "other side")


def _two_conv(packs, xs, j, y, device, lengths, **kw):
    c1, c2, cd = packs[j]
    C, T = xs[j].shape[1], xs[j].shape[2]
    gbuf = torch.full((B, C // 2, T), float("nan"), device=device)
    ops.conv1d_launch_seq([
        ops.make_desc(c1, xs[j], ops.make_out(gbuf), in_slope=0.1, cond=cd, lengths=lengths),
        ops.make_desc(c2, gbuf, ops.make_out(y, res=xs[j], **kw), lengths=lengths)], B, device)


def _cells(a, b, C, k):
    """Mismatching elements per (32-row block, 64-column block of the tile):
    'rows 32-63 x tile cols 64-127: 2048' names the wave that owns them."""
    ng = 256 if C <= 64 else 128
    bn = ng - (k - 1)
    bad = (a.view(torch.int32) != b.view(torch.int32)).cpu()
    out = []
    for r0 in range(0, C, 32):
        cols = bad[:, r0:r0 + 32, :].any(dim=1).nonzero()[:, 1]
        n = bad[:, r0:r0 + 32, :].sum().item()
        if n:
            blocks = sorted({int(t % bn) // 64 for t in cols})
            where = ", ".join(f"{64 * c}-{64 * c + 63}" for c in blocks)
            out.append(f"rows {r0}-{r0 + 31} x tile cols {where}: {n}")
    return "; ".join(out)


def _assert_bits(y, y2, C, k, what):
    torch.cuda.synchronize()
    assert not torch.isnan(y).any(), f"{what}: elements not written"
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), \
        f"{what}: fused != two-conv at {_cells(y, y2, C, k)}"


def _assert_ref(y, ref, what):
    # fp32 arithmetic against fp64: 2e-6 of the output magnitude, the bound
    # of test_resblock_pair_f32p_fused
    err = (y.double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 2e-6 * scale, f"{what} vs fp64: max err {err:.3e} vs scale {scale:.3e}"


def _check_pair(device, C, T, k, dil, side):
    packs, xs, _, lengths, ends = _setup(str(device), C, (k,), dil, T)
    y, y2 = _nan(C, T, device), _nan(C, T, device)
    _fused(side, packs, xs, [0], [y], device, lengths)
    _two_conv(packs, xs, 0, y2, device, lengths)
    what = f"C{C} T{T} k{k} d{dil} {side}"
    _assert_bits(y, y2, C, k, what)
    assert (y[1, :, ends[1]:] == 0).all()
    _assert_ref(y, _ref64(str(device), C, (k,), dil, T, 0), what)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 5), (11, 1), (11, 5)])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_pair_matches_two_conv_path(device, C, k, dil, side):
    _check_pair(device, C, SHAPES[C], k, dil, side)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("k,dil", [(3, 1), (11, 5)])
@pytest.mark.parametrize("C,T", [(64, 772), (256, 388)])
def test_interior_tile(device, C, T, k, dil, side):
    """SHAPES' 64- and 256-channel cases are too short for a tile whose whole
    window lies inside the utterance (the kernel's select-free paths); here
    the first utterance's second tile is one."""
    _check_pair(device, C, T, k, dil, side)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("C", [64, 128, 256])
def test_grouped_launch_of_three(device, C, side):
    """One launch of three members (k = 3 / 7 / 11: three tile widths in one
    grid), each against its own two-conv path."""
    T, ks, dil = SHAPES[C], (3, 7, 11), 3
    packs, xs, _, lengths, _ = _setup(str(device), C, ks, dil, T)
    ys = [_nan(C, T, device) for _ in ks]
    _fused(side, packs, xs, range(3), ys, device, lengths)
    for j, k in enumerate(ks):
        y2 = _nan(C, T, device)
        _two_conv(packs, xs, j, y2, device, lengths)
        _assert_bits(ys[j], y2, C, k, f"C{C} member {j} {side}")
        _assert_ref(ys[j], _ref64(str(device), C, ks, dil, T, j), f"C{C} member {j} {side}")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("C", [64, 128, 256])
def test_accumulating_launch_with_division(device, C, side):
    """accumulate onto a stored output, then / 3 (a true division): the
    branch mean's last launch."""
    T, ks, dil = SHAPES[C], (3, 7, 11), 3
    packs, xs, _, lengths, _ = _setup(str(device), C, ks, dil, T)
    acc, acc2 = _nan(C, T, device), _nan(C, T, device)
    _two_conv(packs, xs, 0, acc, device, lengths)
    _two_conv(packs, xs, 0, acc2, device, lengths)
    kw = dict(accumulate=True, post_div=3.0)
    _fused(side, packs, xs, [2], [acc], device, lengths, **kw)
    _two_conv(packs, xs, 2, acc2, device, lengths, **kw)
    _assert_bits(acc, acc2, C, 11, f"C{C} accumulate / 3 {side}")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("C", [64, 128])
def test_widest_window(device, C, side):
    """(k - 1) dil = 96, the most the staging covers (256 channels stop at 56)."""
    T, k, dil = SHAPES[C], 7, 16
    packs, xs, _, lengths, _ = _setup(str(device), C, (k,), dil, T)
    y, y2 = _nan(C, T, device), _nan(C, T, device)
    _fused(side, packs, xs, [0], [y], device, lengths)
    _two_conv(packs, xs, 0, y2, device, lengths)
    _assert_bits(y, y2, C, k, f"C{C} k7 d16 {side}")
    _assert_ref(y, _ref64(str(device), C, (k,), dil, T, 0), f"C{C} k7 d16 {side}")

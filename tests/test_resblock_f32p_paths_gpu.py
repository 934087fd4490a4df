"""csrc/resblock_f32p.hip's tile paths: interior tiles (no validity / length
selects), end tiles and tiles an utterance ends in, the epilogue variants and
the one-launch branch mean - each BIT FOR BIT the path it replaces (the
two-conv path; for the mean launch the three accumulating launches)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from vits_amd import ops
from vits_amd._lib import VitsAmdError

pytestmark = pytest.mark.gpu

B = 2


@functools.lru_cache(maxsize=None)
def _setup(dev_str, C, ks, dil, T):
    """Three branches (kernel sizes ks) of one stage: packed split-fp32
    layers, inputs and conds on the device, CPU copies for the reference.
    Built once per shape and shared by the tests; nothing writes to it."""
    device = torch.device(dev_str)
    g = torch.Generator().manual_seed(C + sum(ks) + dil + T)
    packs, xs, cpu = [], [], []
    for k in ks:
        x = torch.randn(B, C, T, generator=g) * 0.5
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
    return packs, xs, cpu


def _lengths(kind, T, device):
    """None; the second utterance ends 37 before the end (in the last tile);
    or at T // 2 (inside the interior tile of the three-tile shapes)."""
    if kind == "none":
        return None
    second = max(1, T - 37) if kind == "tail" else T // 2
    return torch.tensor([T, second], dtype=torch.int32, device=device)


def _nan(C, T, device):
    # an element the kernel skips stays NaN and fails the comparison
    return torch.full((B, C, T), float("nan"), device=device)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _two_conv(packs, xs, j, y, device, lengths=None, **kw):
    c1, c2, cd = packs[j]
    C, T = xs[j].shape[1], xs[j].shape[2]
    gbuf = torch.full((B, C // 2, T), float("nan"), device=device)
    ops.conv1d_launch_seq([
        ops.make_desc(c1, xs[j], ops.make_out(gbuf), in_slope=0.1, cond=cd, lengths=lengths),
        ops.make_desc(c2, gbuf, ops.make_out(y, res=xs[j], **kw), lengths=lengths)], B, device)


def _fused(packs, xs, js, ys, device, lengths=None, mean=False, **kw):
    ops.resblock_pair_launch(tuple(
        ops.resblock_pair_desc(packs[j][0], packs[j][1], xs[j], y, cond=packs[j][2],
                               lengths=lengths, **kw) for j, y in zip(js, ys)),
        B, device, ops.WDT_F32P, mean=mean)


def _all_k(monkeypatch):
    # (the kernel takes every stage and k; the engine's rule picks where)
    monkeypatch.setattr(ops, "F32P_PAIR_MAX_K", {32: 15, 64: 15, 128: 15, 256: 15})


# first, interior and last tile (BN = 256 - (k - 1) columns; 128 - (k - 1) at
# 128 channels), and one tile with both ends outside
TILE_CASES = [
    (32, 3, 1, 764),   # BN = 254
    (64, 3, 1, 764),
    (64, 11, 5, 740),  # BN = 246
    (128, 7, 3, 368),  # BN = 122
    (64, 3, 1, 12),
]


@pytest.mark.parametrize("lens", ["none", "tail", "mid"])
@pytest.mark.parametrize("C,k,dil,T", TILE_CASES)
def test_tiles_match_two_conv_path(device, monkeypatch, C, k, dil, T, lens):
    """The three-branch grouped launch, interior / end / mixed tiles, with
    and without utterance lengths: the two-conv path's bits."""
    _all_k(monkeypatch)
    packs, xs, _ = _setup(str(device), C, (k, k, k), dil, T)
    for j in range(3):
        assert ops.resblock_pair_f32p_supported(packs[j][0], packs[j][1], xs[j])
    lengths = _lengths(lens, T, device)
    ys = [_nan(C, T, device) for _ in range(3)]
    _fused(packs, xs, range(3), ys, device, lengths=lengths)
    for j in range(3):
        y2 = _nan(C, T, device)
        _two_conv(packs, xs, j, y2, device, lengths=lengths)
        torch.cuda.synchronize()
        assert not torch.isnan(ys[j]).any(), f"pair {j}: elements not written"
        d = (ys[j] - y2).abs().max().item()
        assert _same_bits(ys[j], y2), f"pair {j}: fused != two-conv, max diff {d:.3e}"
        if lengths is not None:
            assert (ys[j][1, :, int(lengths[1]):] == 0).all()


@pytest.mark.parametrize("lens", ["none", "tail"])
@pytest.mark.parametrize("C,k,dil,T", TILE_CASES[:1] + TILE_CASES[2:])
def test_epilogue_variants_match_two_conv_path(device, monkeypatch, C, k, dil, T, lens):
    """Plain store, accumulate, and accumulate with post_div = 3 (a true
    division), chained as the branch mean chains them; compared after every
    launch."""
    _all_k(monkeypatch)
    packs, xs, _ = _setup(str(device), C, (k, k, k), dil, T)
    lengths = _lengths(lens, T, device)
    acc, acc2 = _nan(C, T, device), _nan(C, T, device)
    for j, kw in enumerate((dict(), dict(accumulate=True),
                            dict(accumulate=True, post_div=3.0))):
        _fused(packs, xs, [j], [acc], device, lengths=lengths, **kw)
        _two_conv(packs, xs, j, acc2, device, lengths=lengths, **kw)
        torch.cuda.synchronize()
        assert not torch.isnan(acc).any(), f"{kw}: elements not written"
        assert _same_bits(acc, acc2), f"epilogue {kw}"


def _pair_ref64(x, w1, b1, cond, w2, b2, k, dil):
    """modules.py:251-259 for one (c1, c2, cs) pair, fp64 on CPU."""
    x, w1, b1, w2, b2 = (t.double() for t in (x, w1, b1, w2, b2))
    xt = F.conv1d(F.leaky_relu(x, 0.1), w1, b1, dilation=dil, padding=(k - 1) * dil // 2)
    xa, xb = torch.chunk(xt, 2, dim=1)
    sa, sb = torch.chunk(cond.double(), 2, dim=1)
    xt = torch.tanh(xa + sa.unsqueeze(-1)) * torch.sigmoid(xb + sb.unsqueeze(-1))
    return F.conv1d(xt, w2, b2, padding=(k - 1) // 2) + x


@pytest.mark.parametrize("lens", ["none", "tail"])
def test_mean_launch_matches_accumulating_launches(device, monkeypatch, lens):
    """vits_resblock_pair_f32p_mean_forward (C = 32, k = 3 / 7 / 11, dil 5,
    T = 764: four tiles of 246 columns, interior and end) equals the three accumulating
    launches bit for bit, and the fp64 mean to 2e-6 of its magnitude (fp32
    arithmetic, as test_resblock_pair_f32p_fused).  With lengths the inputs
    are zero past them, as the decoder's are, and the reference is each
    utterance on its own length."""
    _all_k(monkeypatch)
    C, ks, dil, T = 32, (3, 7, 11), 5, 764
    packs, xs, cpu = _setup(str(device), C, ks, dil, T)
    lengths = _lengths(lens, T, device)
    ends = [T, T] if lengths is None else [int(v) for v in lengths.cpu()]
    mask = torch.zeros(B, 1, T)
    for b, e in enumerate(ends):
        mask[b, :, :e] = 1
    xs = [x * mask.to(device) for x in xs]
    acc = _nan(C, T, device)
    for j in range(3):
        _fused(packs, xs, [j], [acc], device, lengths=lengths, accumulate=j > 0,
               post_div=3.0 if j == 2 else 1.0)
    mean = _nan(C, T, device)
    _fused(packs, xs, range(3), [mean] * 3, device, lengths=lengths, mean=True)
    torch.cuda.synchronize()
    assert not torch.isnan(mean).any(), "elements not written"
    d = (mean - acc).abs().max().item()
    assert _same_bits(mean, acc), f"mean launch != accumulating launches, max diff {d:.3e}"
    ref = torch.zeros(B, C, T, dtype=torch.float64)
    for b, e in enumerate(ends):
        for x, w1, b1, cond, w2, b2, k in cpu:
            ref[b, :, :e] += _pair_ref64((x * mask)[b:b + 1, :, :e], w1, b1, cond[b:b + 1], w2, b2,
                                         k, dil)[0]
    ref /= 3
    err = (mean.double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"mean launch vs fp64: max err {err:.3e}, scale {scale:.3e}")
    assert err <= 2e-6 * scale, f"mean vs fp64: max err {err:.3e} vs scale {scale:.3e}"


def test_mean_launch_refuses_other_stages(device, monkeypatch):
    """The one-launch mean is built for the 32-channel stage only: 64
    channels are an error, not another kernel."""
    _all_k(monkeypatch)
    C, T = 64, 12
    packs, xs, _ = _setup(str(device), C, (3, 3, 3), 1, T)
    y = _nan(C, T, device)
    with pytest.raises(VitsAmdError, match="shape"):
        _fused(packs, xs, range(3), [y] * 3, device, mean=True)

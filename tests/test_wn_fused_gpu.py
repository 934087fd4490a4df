"""The fused WN layer (csrc/wn_f32p.hip) against the two-conv path it
replaces: engine._FUSED_WN flipped, torch.equal on the skip output and the
final residual stream.  Random weights, H = 256, k = 5."""
import contextlib

import pytest
import torch

from vits_amd import engine, models, modules, ops

pytestmark = pytest.mark.gpu

H, K = 256, 5
GIN = 64


@contextlib.contextmanager
def fused(on: bool, ng: int = 0):
    old, old_ng = engine._FUSED_WN, ops.WN_NG
    engine._FUSED_WN, ops.WN_NG = on, ng
    try:
        yield
    finally:
        engine._FUSED_WN, ops.WN_NG = old, old_ng


def _randomize(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.5 if p.dim() < 2 else 0.05)).to(p))
    return mod


_PLANS = {}


def wn_plan(device, n_layers, cond):
    """(WNPlan of a random split-fp32 WN, cond weight, cond bias), built once."""
    key = (n_layers, cond)
    if key not in _PLANS:
        wn = _randomize(modules.WN(H, K, 1, n_layers, gin_channels=GIN if cond else 0), n_layers)
        wn = wn.to(device).eval()
        with torch.no_grad(), ops.pack_lowp(ops.WDT_F32S):
            conds = engine._CondStack()
            plan = engine.WNPlan(wn, conds)
            cw, cb = conds.finish()
        assert plan.in_layers[0].wdtype == ops.WDT_F32P
        _PLANS[key] = (plan, cw, cb)
    return _PLANS[key]


def run_wn(plan_t, h0, g, lengths, on, ng=0):
    """(skip, final h) of the stack on a copy of h0; buffers zero-filled, so a
    tile that length_skip leaves out reads as zero on both paths."""
    plan, cw, cb = plan_t
    h = h0.clone()
    skip = torch.zeros_like(h)
    abuf = torch.zeros_like(skip)
    cond = None if cw is None else ops.linear_rows(g, cw, cb)
    with fused(on, ng):
        took = plan.fused(h)
        ops.conv1d_launch_seq(plan.descs(h, skip, abuf, cond, lengths), h.shape[0], h.device)
        hf = plan.final_h(h, abuf)
    torch.cuda.synchronize()
    return skip, hf, took


def _inputs(device, B, T, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    h = (torch.randn(B, H, T, generator=g) * 0.5).to(device)
    gg = (torch.randn(B, GIN, generator=g) * 0.5).to(device)
    return h, gg


@pytest.mark.parametrize("cond", [True, False], ids=["cond", "nocond"])
@pytest.mark.parametrize("n_layers", [1, 2, 4])
@pytest.mark.parametrize("T", [4, 36, 100, 132])
def test_bitwise_vs_two_conv(device, T, n_layers, cond):
    plan = wn_plan(device, n_layers, cond)
    h, gg = _inputs(device, 3, T)
    s0, h0, took0 = run_wn(plan, h, gg, None, False)
    assert not took0
    for ng in (0, 32, 64):
        s1, h1, took1 = run_wn(plan, h, gg, None, True, ng)
        assert took1
        assert torch.equal(s1, s0), (ng, (s1 - s0).abs().max().item())
        assert torch.equal(h1, h0), (ng, (h1 - h0).abs().max().item())
    assert torch.isfinite(s0).all() and s0.abs().max() > 0


@pytest.mark.parametrize("skip_tiles", [False, True], ids=["noskip", "length_skip"])
@pytest.mark.parametrize("ng", [32, 64])
def test_masked(device, ng, skip_tiles):
    """Per-row lengths 0, 1, a tile edge +- 1 and T: equal to the two-conv
    path, exact zeros past each length."""
    T = 200
    lens = [0, 1, ng - 1, ng, ng + 1, 2 * ng - 1, 2 * ng + 1, T]
    B = len(lens)
    plan = wn_plan(device, 4, True)
    h, gg = _inputs(device, B, T, seed=1)
    lengths = torch.tensor(lens, dtype=torch.int32, device=device)
    # the residual stream enters masked, as the callers' pre convs leave it
    h = h * (torch.arange(T, device=device)[None, None, :] < lengths[:, None, None])
    ctx = ops.length_skip(64) if skip_tiles else contextlib.nullcontext()
    with ctx:
        s0, h0, _ = run_wn(plan, h, gg, lengths, False)
        s1, h1, took = run_wn(plan, h, gg, lengths, True, ng)
    assert took
    assert torch.equal(s1, s0) and torch.equal(h1, h0)
    for b, n in enumerate(lens):
        if n < T:
            assert s1[b, :, n:].abs().max().item() == 0
            assert h1[b, :, n:].abs().max().item() == 0
        if n > 0:
            assert s1[b, :, :n].abs().max() > 0


def test_batch_independence(device):
    """Row b of a B = 3 call equals the B = 1 call on that row; and B * T on
    both sides of the tile choice (T = 1024: 64-column tiles from B = 16)
    gives identical rows."""
    plan = wn_plan(device, 4, True)
    h, gg = _inputs(device, 3, 100, seed=2)
    s3, h3, _ = run_wn(plan, h, gg, None, True)
    for b in range(3):
        s1, h1, _ = run_wn(plan, h[b:b + 1].contiguous(), gg[b:b + 1].contiguous(), None, True)
        assert torch.equal(s1[0], s3[b]) and torch.equal(h1[0], h3[b])
    hb, gb = _inputs(device, 16, 1024, seed=3)
    s16, h16, _ = run_wn(plan, hb, gb, None, True)       # 16 * 16 tiles of 64: NG = 64
    s2, h2, _ = run_wn(plan, hb[:2].contiguous(), gb[:2].contiguous(), None, True)  # NG = 32
    assert torch.equal(s2, s16[:2]) and torch.equal(h2, h16[:2])


def test_unsupported_shapes_keep_the_two_conv_path(device):
    plan = wn_plan(device, 4, True)
    # T % 4 != 0
    h, gg = _inputs(device, 2, 77, seed=4)
    s0, h0, took0 = run_wn(plan, h, gg, None, False)
    s1, h1, took1 = run_wn(plan, h, gg, None, True)
    assert not took0 and not took1
    assert torch.equal(s1, s0) and torch.equal(h1, h0)
    # a non-contiguous h: rows of 100 steps in a buffer 102 wide (row stride % 4 != 0)
    hw, _ = _inputs(device, 2, 102, seed=5)

    def run_view(on):
        plan_, cw, cb = plan
        v = hw.clone()[:, :, :100]
        assert not v.is_contiguous()
        skip = torch.zeros(2, H, 100, device=device)
        abuf = torch.zeros_like(skip)
        cond = ops.linear_rows(gg, cw, cb)
        with fused(on):
            took = plan_.fused(v)
            ops.conv1d_launch_seq(plan_.descs(v, skip, abuf, cond, None), 2, device)
            hf = plan_.final_h(v, abuf).clone()
        torch.cuda.synchronize()
        return skip, hf, took

    a, b = run_view(False), run_view(True)
    assert not a[2] and not b[2]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[0]).all() and a[0].abs().max() > 0


@pytest.fixture(scope="module")
def flow(device):
    blk = models.ResidualCouplingBlock(192, H, K, dilation_rate=[1, 1], n_layers=4, n_flows=2,
                                       gin_channels=GIN)
    return _randomize(blk, 11).to(device).eval()


@pytest.mark.parametrize("forward", [False, True], ids=["reverse", "forward"])
def test_whole_flow(device, flow, forward):
    g = torch.Generator().manual_seed(12)
    z = (torch.randn(3, 192, 100, generator=g) * 0.5).to(device)
    gg = (torch.randn(3, GIN, generator=g) * 0.5).to(device)
    plan = engine.get_plan(flow, engine.CouplingFlowPlan)
    outs = []
    for on in (False, True):
        with fused(on):
            outs.append(plan.run_(z.clone(), gg, forward=forward))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], z)


def test_flow_conv_timer_flops(device, flow):
    """One flow run records equal total_flops with the switch on and off, and
    the fused launches carry their own label."""
    g = torch.Generator().manual_seed(13)
    z = (torch.randn(2, 192, 100, generator=g) * 0.5).to(device)
    gg = (torch.randn(2, GIN, generator=g) * 0.5).to(device)
    plan = engine.get_plan(flow, engine.CouplingFlowPlan)
    res = {}
    for on in (False, True):
        with fused(on), ops.ConvTimer() as tm:
            out = plan.run_(z.clone(), gg)
        res[on] = (tm.summary(), [lab for lab, _, _ in tm.per_launch()], out)
    assert res[True][0]["total_flops"] == res[False][0]["total_flops"]
    assert res[True][0]["f32s_flops"] == res[False][0]["f32s_flops"]
    assert sum(lab.startswith("wn H256k5d1T100") for lab in res[True][1]) == 8
    assert not any(lab.startswith("wn ") for lab in res[False][1])
    assert res[True][0]["launches"] == res[False][0]["launches"] - 8
    assert torch.equal(res[True][2], res[False][2])


def test_posterior_bucketed(device):
    enc = models.PosteriorEncoder(80, 192, H, K, 1, 4)
    enc = _randomize(enc, 21).to(device).eval()
    plan = engine.get_plan(enc, engine.PosteriorPlan)
    g = torch.Generator().manual_seed(22)
    spec = torch.rand(3, 80, 64, generator=g).to(device)
    noise = torch.randn(3, 192, 64, generator=g).to(device)
    lens = torch.tensor([64, 33, 7], dtype=torch.int32, device=device)
    outs = []
    for on in (False, True):
        with fused(on):
            outs.append(plan.run_bucketed(spec, noise, lens))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert outs[0][1, :, 33:].abs().max().item() == 0 and outs[0][0].abs().max() > 0

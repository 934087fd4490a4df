"""Forced alignment on the GPU: the eager definition SynthesizerTrn.align
against the reference's golden (tests/golden/base_align.npz), the
host-sync-free bucketed path and its graph against that definition (BITWISE,
the contract of tests/test_vc_gpu.py), the serving entry points of EmoVITS and
VITSWrap, and the fp16 model that EmoVITS holds against the fp32 one.

Tolerances: REL = 1e-4 is tests/test_vc_gpu.py's bar for the latents; it is
applied to neg_cent and to the scores relative to their largest magnitude.
Durations are compared exactly: the fixture's path is unchanged by relative
perturbations of neg_cent ten times larger (make_golden_align.py asserts it)."""
import numpy as np
import pytest
import torch

import align_common as A
import vc_common as VC
from common import BASE_DATA, base_model, build_model, golden, rel_err, tiny_cfg

pytestmark = pytest.mark.gpu

REL = 1e-4
STFT = (VC.STFT["n_fft"], VC.STFT["hop"], VC.STFT["win"])
HOP = VC.STFT["hop"]
T_X, T_Y = 32, 256
# (seed, frames, tokens, speaker) of the ragged batch: the fixture and two more
ROWS = ((A.GOLDEN_SEED, A.GOLDEN_FRAMES, A.GOLDEN_TX, A.GOLDEN_SID), (2025, 40, 12, 1500),
        (11, 97, 32, 3))

# The fp16 model (what EmoVITS holds) against the fp32 model of the same
# weights on the fixture (61 frames, 20 tokens), measured on MI355X: the share
# of frames whose token differs and the largest shift of a token boundary, in
# frames.  Bars: twice the measurement (one fixture is a thin sample), the
# share's never below one frame of the fixture.
FP16_TOKEN_SHARE_MEASURED = 0.0
FP16_BOUNDARY_SHIFT_MEASURED = 0
FP16_TOKEN_SHARE_BAR = max(2 * FP16_TOKEN_SHARE_MEASURED, 1.0 / A.GOLDEN_FRAMES)
FP16_BOUNDARY_SHIFT_BAR = 2 * FP16_BOUNDARY_SHIFT_MEASURED


@pytest.fixture(scope="module")
def base(device):
    return base_model(device)


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in golden("base_align.npz").items()}


def _spec(wav, device):
    from vits_amd import ops

    window = torch.hann_window(STFT[2], device=device)
    return ops.stft_mag(wav.view(1, -1).contiguous(), window, STFT[0], HOP, STFT[2], pad=VC.PAD,
                        eps=1e-6)


def _align_alone(model, wav, x, emo, sid, device):
    """align of one row at its exact lengths: wav [n], x [Tx, c], emo [1024]."""
    spec = _spec(wav, device)
    f, t = spec.shape[2], x.shape[0]
    dur, sc, lat = model.align(x[None], torch.tensor([t], device=device), spec,
                               torch.tensor([f], device=device), emo[None], sid.view(1))
    return dur[0], sc[0], lat, f


def test_align_matches_reference_golden(base, gold, device):
    dur, sc, (z_p, m_p, logs_p, nc), f = _align_alone(
        base, gold["wav"][0].to(device), gold["x"][0].to(device), gold["emo"][0].to(device),
        gold["sid"].to(device), device)
    torch.cuda.synchronize()
    assert f == A.GOLDEN_FRAMES
    assert dur.dtype == torch.int32 and tuple(dur.shape) == (A.GOLDEN_TX,)
    assert sc.dtype == torch.float32 and tuple(sc.shape) == (A.GOLDEN_TX,)
    assert tuple(nc.shape) == (1, A.GOLDEN_FRAMES, A.GOLDEN_TX)
    for name, t in (("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p), ("neg_cent", nc),
                    ("scores", sc[None])):
        err = rel_err(t, gold[name])
        print(f"align {name}: rel_err {err:.2e}")
        assert err < REL, name
    assert np.array_equal(dur.cpu().numpy(), gold["durations"].numpy())
    # the scores are the sequential float32 sums of this run's own neg_cent
    d, s, _ = A.mas_reduce(nc[0].cpu().numpy(), A.GOLDEN_FRAMES, A.GOLDEN_TX)
    assert np.array_equal(d, dur.cpu().numpy()) and np.array_equal(s, sc.cpu().numpy())


def _ragged_inputs(device, rows=ROWS, t_x=T_X, t_y=T_Y):
    """(wav [B, cap] with NaN past each row's samples, n_samples, x [B, t_x,
    c] zero past each row's tokens, x_lengths, emo, sid) on the device."""
    B = len(rows)
    wav = torch.full((B, t_y * HOP + HOP - 1), float("nan"))
    x = torch.zeros(B, t_x, BASE_DATA["text_channels"])
    emo = torch.zeros(B, 1024)
    ns, xl, sid = [], [], []
    for b, (seed, frames, tokens, spk) in enumerate(rows):
        n = frames * HOP + 57
        w, xx, e = A.golden_inputs(seed, n, tokens, BASE_DATA["text_channels"])
        wav[b, :n], x[b, :tokens], emo[b] = w[0], xx[0], e[0]
        ns.append(n)
        xl.append(tokens)
        sid.append(spk)
    return (wav.to(device), torch.tensor(ns, dtype=torch.int32, device=device), x.to(device),
            torch.tensor(xl, dtype=torch.int32, device=device), emo.to(device),
            torch.tensor(sid, device=device))


@pytest.fixture(scope="module")
def ragged(base, device):
    """The ragged batch, its eager align_bucketed result and every row's
    exact-length definition: computed once, shared, left unchanged."""
    inp = _ragged_inputs(device)
    wav, n_t, x, xl, emo, sid = inp
    out = base.align_bucketed(wav, n_t, x, xl, emo, sid, None, T_X, T_Y, stft=STFT)
    alone = []
    for b, (_, frames, tokens, _) in enumerate(ROWS):
        d, s, _, f = _align_alone(base, wav[b, :int(n_t[b])], x[b, :tokens], emo[b], sid[b],
                                  device)
        assert f == frames
        alone.append((d.clone(), s.clone()))
    torch.cuda.synchronize()
    return inp, tuple(t.clone() for t in out), alone


def test_fixture_row_of_the_batch_is_the_golden(ragged, gold):
    inp, (dur, _, _), _ = ragged
    assert torch.equal(inp[0][0, :A.GOLDEN_L].cpu(), gold["wav"][0])
    assert np.array_equal(dur[0, :A.GOLDEN_TX].cpu().numpy(), gold["durations"].numpy())


def test_align_bucketed_bitwise_equals_align(ragged):
    _, (dur, sc, y_len), alone = ragged
    assert tuple(dur.shape) == tuple(sc.shape) == (len(ROWS), T_X)
    assert dur.dtype == torch.int32 and sc.dtype == torch.float32
    assert y_len.tolist() == [r[1] for r in ROWS]
    for b, (_, frames, tokens, _) in enumerate(ROWS):
        d, s = alone[b]
        assert torch.equal(dur[b, :tokens], d), b
        assert torch.equal(sc[b, :tokens], s), b
        assert int(d.min()) >= 1 and int(d.sum()) == frames
        assert torch.isfinite(s).all() and s.abs().max().item() > 0
        assert torch.count_nonzero(dur[b, tokens:]).item() == 0, b
        assert torch.count_nonzero(sc[b, tokens:]).item() == 0, b


def test_align_graph_replay(base, ragged, device):
    (wav, n_t, x, xl, emo, sid), ref, _ = ragged
    B = len(ROWS)
    run = base.capture_align_bucketed(T_X, T_Y, batch=B, stft=STFT)
    out = run(wav, n_t, x, xl, emo, sid)
    torch.cuda.synchronize()
    for got, want in zip(out, ref):
        assert torch.equal(got, want)
    # fewer rows into the same graph: the unused rows come back as "no alignment"
    dur, sc, y_len = run(wav[1:2], n_t[1:2], x[1:2, :ROWS[1][2]], [ROWS[1][2]], emo[1:2],
                         sid[1:2])
    torch.cuda.synchronize()
    assert y_len.tolist() == [ROWS[1][1], 0, 0]
    assert torch.equal(dur[0], ref[0][1]) and torch.equal(sc[0], ref[1][1])
    assert torch.count_nonzero(dur[1:]).item() == 0 and torch.count_nonzero(sc[1:]).item() == 0
    with pytest.raises(ValueError):
        run(wav, n_t, x, xl[:2], emo, sid)  # three rows need three lengths


def _emovits(device, model, tmp_path, text_channels, sr=16000, **kw):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    hps = get_hparams_from_dict({
        "data": {"sampling_rate": sr, "filter_length": STFT[0], "hop_length": HOP,
                 "win_length": STFT[2], "text_channels": text_channels,
                 "n_speakers": model.emb_g.num_embeddings, "noise_scale": 0.667},
        "model": {"inter_channels": model.inter_channels}})
    return EmoVITS(str(tmp_path / "ckpt.pth"), device, hps=hps, model=model, graph=True, **kw)


def _recording(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.25).clamp(-1, 1).mul(32767).to(torch.int16).numpy()


def _text(tokens, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tokens, c, generator=g).numpy(), torch.randn(1, 1024, generator=g)


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2])


def test_emovits_align_batch_rate_cache_and_wrapper(device, tmp_path):
    from vits_amd import ops, vits_wrap

    c = tiny_cfg()
    tc = c["data"]["text_channels"]
    model = build_model(c["model"], dict(c["data"], spec_channels=STFT[0] // 2 + 1), device)
    ev = _emovits(device, model, tmp_path, tc)
    shapes = ((30 * HOP + 11, 9), (12 * HOP + 190, 12), (47 * HOP, 33))
    items = []
    for i, (n, tokens) in enumerate(shapes):
        text, emo = _text(tokens, tc, 50 + i)
        items.append((_recording(n, i), 1 + i, text, emo))
    # batch == loop
    batch = ev.align_batch(items)
    assert ("align", 4, 64, 256) in ev._graphs
    singles = [ev.align(*it) for it in items]
    assert ("align", 1, 32, 256) in ev._graphs and ("align", 1, 64, 256) in ev._graphs
    for (n, tokens), got, one in zip(shapes, batch, singles):
        dur, sc, frames = one
        assert dur.dtype == np.int32 and sc.dtype == np.float32
        assert dur.shape == sc.shape == (tokens,) and frames == n // HOP
        assert dur.min() >= 1 and dur.sum() == frames and np.isfinite(sc).all()
        assert _same(got, one)
    # input at twice the model's rate == resampling first, aligning at the model's rate
    rec2 = _recording(2 * (20 * HOP + 7), 9)
    text, emo = items[0][2], items[0][3]
    a = ev.align(rec2, 1, text, emo, sampling_rate_in=32000)
    xr = torch.from_numpy(rec2.astype(np.float32) / 32768.0).to(device)
    up, down = ops.resample_ratio(32000, 16000)
    b = ev.align(ops.resample_poly(xr, up, down).cpu().numpy(), 1, text, emo)
    assert a[2] == 20 and _same(a, b)
    # refusals reach the caller: fewer frames than tokens, known on the host
    with pytest.raises(ValueError):
        ev.align(_recording(8 * HOP, 1), 1, text, emo)
    # the graph cache: keyed with the other graphs, bounded by max_graphs,
    # most recently used last, the oldest evicted
    assert list(ev._graphs)[-1] == ("align", 1, 32, 256)
    ev.max_graphs = len(ev._graphs)
    oldest = next(iter(ev._graphs))
    ev.convert(items[0][0], 1, 2)
    assert oldest not in ev._graphs and len(ev._graphs) == ev.max_graphs
    assert list(ev._graphs)[-1] == ("vc", 1, 256)
    ev.align(*items[0])
    assert list(ev._graphs)[-1] == ("align", 1, 32, 256) and len(ev._graphs) == ev.max_graphs
    # graph off: the same kernels eagerly, the same result
    ev.graph = False
    assert _same(ev.align(*items[1]), singles[1])
    assert all(_same(g, s) for g, s in zip(ev.align_batch(items), singles))
    ev.graph = True
    # a posterior draw comes from the object's generator
    ev.align(*items[0], noise_scale=0.667)
    assert ev._vc_gen is not None

    # the wrapper, with a stub front end: one vector per character
    class Front:
        max_utt_length = 16

        def __call__(self, uid, txt):
            g = torch.Generator().manual_seed(len(txt))
            return uid, txt, torch.randn(len(txt), tc, generator=g).numpy()

    wrap = vits_wrap.VITSWrap(textparser=Front(), speecher=ev)  # (no device_post needed)
    res = wrap.aligning({"wav": items[0][0], "text": "abcdefghi", "spkid": 1,
                         "emotion": items[0][3], "id": "u1"})
    want = ev.align(items[0][0], 1, Front()("u1", "abcdefghi")[2], items[0][3])
    assert res["id"] == "u1" and res["frames"] == want[2] == 30 and res["segtext"] == "abcdefghi"
    assert np.array_equal(res["durations"], want[0]) and np.array_equal(res["scores"], want[1])
    bounds = res["boundaries_s"]
    assert bounds.shape == (10,) and bounds[0] == 0.0
    assert np.array_equal(bounds, np.concatenate([[0], np.cumsum(want[0])]) * (HOP / 16000))
    assert bounds[-1] == pytest.approx(30 * HOP / 16000, rel=1e-12)
    assert res["time_used_backend"] > 0 and res["rtf"] > 0 and res["time_used_frontend"] >= 0
    with pytest.raises(ValueError):
        wrap.aligning({"wav": items[0][0], "text": "abcdefghijklmnopq rstu", "spkid": 1,
                       "emotion": items[0][3]})


def _frame_tokens(dur):
    return np.repeat(np.arange(len(dur)), dur)


def test_fp16_align_graph_equals_eager_and_tracks_fp32(base, ragged, gold, device, tmp_path):
    """What EmoVITS holds is the fp16 model: its graph replay equals its eager
    run bitwise, every row is a complete alignment, and on the fixture its
    path stays close to the fp32 model's of the same weights.  Bars: see
    FP16_TOKEN_SHARE_BAR / FP16_BOUNDARY_SHIFT_BAR and DESIGN.md (forced
    alignment)."""
    ev = _emovits(device, base_model(device), tmp_path, BASE_DATA["text_channels"])
    (wav, n_t, x, xl, emo, sid), _, alone = ragged
    items = [(wav[b, :int(n_t[b])].cpu().numpy(), spk, x[b, :tokens].cpu().numpy(),
              emo[b:b + 1].cpu()) for b, (_, _, tokens, spk) in enumerate(ROWS)]
    on_batch, on_one = ev.align_batch(items), ev.align(*items[0])
    ev.graph = False
    off_batch, off_one = ev.align_batch(items), ev.align(*items[0])
    assert _same(on_one, off_one) and _same(on_one, on_batch[0])
    for (_, frames, tokens, _), a, b in zip(ROWS, on_batch, off_batch):
        assert _same(a, b)
        dur, sc, f = a
        assert f == frames and dur.shape == (tokens,)
        assert dur.min() >= 1 and dur.sum() == frames and np.isfinite(sc).all()
    # the fixture row against the fp32 model
    d16 = on_one[0]
    d32 = alone[0][0].cpu().numpy()
    assert np.array_equal(d32, gold["durations"].numpy())
    share = float((_frame_tokens(d16) != _frame_tokens(d32)).mean())
    shift = int(np.abs(np.cumsum(d16) - np.cumsum(d32)).max())
    print(f"fp16 align vs fp32 on the fixture: {share:.4f} of the frames on another token "
          f"(bar {FP16_TOKEN_SHARE_BAR:.4f}), largest boundary shift {shift} frames "
          f"(bar {FP16_BOUNDARY_SHIFT_BAR})")
    assert share <= FP16_TOKEN_SHARE_BAR
    assert shift <= FP16_BOUNDARY_SHIFT_BAR

"""Retiming a recording on the GPU: the eager definition
SynthesizerTrn.retime against the reference's golden, the identity at neutral
controls (BITWISE voice_conversion), its locality (far from a retimed token it
is the plain conversion, shifted by the change of length behind it), the
host-sync-free bucketed path and its graph against the definition (bitwise),
and the serving entry points.

Bars: REL = 1e-4 and 60 dB, those of tests/test_vc_gpu.py.  The configurations
are those of tests/test_edit_gpu.py, for its reason."""
import math

import numpy as np
import pytest
import torch

import retime_common as RC
import vc_common as VC
from common import base_model, build_model, golden, rel_err, snr_db, tiny_cfg

pytestmark = pytest.mark.gpu

REL = 1e-4
SNR_DB = 60.0
N_FFT, HOP, WIN = VC.STFT["n_fft"], VC.STFT["hop"], VC.STFT["win"]
STFT = (N_FFT, HOP, WIN)
I32 = torch.int32
T_X, T_B = 16, 256


def _emovits(device, model, tmp_path, **kw):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "filter_length": N_FFT, "hop_length": HOP,
                 "win_length": WIN, "text_channels": 256,
                 "n_speakers": model.emb_g.num_embeddings, "noise_scale": 0.667},
        "model": {"inter_channels": model.inter_channels}})
    return EmoVITS(str(tmp_path / "ckpt.pth"), device, hps=hps, model=model, **kw)


@pytest.fixture(scope="module")
def base(device):
    return base_model(device)


@pytest.fixture(scope="module")
def ev_tiny(device, tmp_path_factory):
    """The tiny config as EmoVITS holds it: fp16, weight norm folded."""
    c = tiny_cfg()
    model = build_model(c["model"], dict(c["data"], spec_channels=N_FFT // 2 + 1), device)
    return _emovits(device, model, tmp_path_factory.mktemp("retime_tiny"), graph=True)


def _model(which, base, ev_tiny):
    return base if which == "base-fp32" else ev_tiny.model


def _spec(wav_row, device):
    """The exact-length linear spectrogram of one recording [n] (fp32, device)."""
    from vits_amd import ops

    window = torch.hann_window(WIN, device=device)
    return ops.stft_mag(wav_row.view(1, -1).contiguous(), window, N_FFT, HOP, WIN, pad=VC.PAD,
                        eps=1e-6)


def _text(model, n, seed, device):
    dt = next(model.parameters()).dtype
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, n, model.text_channels, generator=g)
    emo = torch.randn(1, 1024, generator=g)
    return x.to(device, dt), emo.to(device, dt)


def _wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.25).clamp(-1, 1)


def _same(out, ref, what=""):
    out, ref = torch.as_tensor(out).cpu(), torch.as_tensor(ref).cpu()
    if out.shape != ref.shape:
        print(f"{what}: shapes {tuple(out.shape)} and {tuple(ref.shape)}")
        return False
    bad = torch.nonzero(out.flatten() != ref.flatten()).flatten()
    if bad.numel():
        print(f"{what}: {bad.numel()} of {ref.numel()} samples differ, frames "
              f"{int(bad[0]) // HOP} .. {int(bad[-1]) // HOP}")
    return bad.numel() == 0


def _dev_i(v, device):
    return torch.tensor(v, dtype=I32, device=device)


# -- the definition against the reference ----------------------------------------------

def test_retime_matches_reference_golden(base, device):
    gold = {k: torch.from_numpy(v) for k, v in golden("base_retime.npz").items()}
    spec = _spec(gold["wav"][0].to(device), device)
    assert spec.shape[2] == 60
    o, (z_p, z_warp, z_hat) = base.retime(
        spec, torch.tensor([60]), gold["sid_src"].to(device), gold["sid_tgt"].to(device),
        gold["dur_old"], gold["dur_new"], noise=gold["noise_q"].to(device))
    torch.cuda.synchronize()
    assert tuple(o.shape) == (1, 1, 71 * HOP) and tuple(z_warp.shape) == (1, 192, 71)
    for name, t in (("z_p", z_p), ("z_warp", z_warp), ("z_hat", z_hat), ("o", o)):
        err = rel_err(t, gold[name])
        print(f"retime {name}: rel_err {err:.2e}")
        assert err < REL, name
    snr = snr_db(o, gold["o"])
    print(f"retime o: snr {snr:.1f} dB")
    assert snr >= SNR_DB
    # the device's plan finds the golden's new durations
    from vits_amd import ops

    dn, total, st = ops.retime_plan(
        gold["dur_old"].view(1, -1).to(device), _dev_i([60], device),
        given=gold["given"].view(1, -1).to(device), tok_scale=gold["tok_scale"].view(1, -1).to(device),
        target=gold["target"].to(device))
    assert dn[0].tolist() == gold["dur_new"].tolist() and total.item() == 71 and st.item() == 0
    with pytest.raises(ValueError, match="sum"):  # they sum to 59
        base.retime(spec, torch.tensor([60]), gold["sid_src"].to(device),
                    gold["sid_tgt"].to(device), [3] + RC.GOLDEN_DUR_OLD[1:], gold["dur_new"])


# -- the identity -------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["base-fp32", "tiny-fp16"])
def test_neutral_retime_is_voice_conversion_bitwise(which, base, ev_tiny, device):
    model = _model(which, base, ev_tiny)
    n = 67 * HOP + 57
    wav = _wave(n, 51).to(device)
    spec = _spec(wav, device)
    assert spec.shape[2] == 67
    src, tgt = torch.tensor([2], device=device), torch.tensor([3], device=device)
    yl = torch.tensor([67])
    rec = model.voice_conversion(spec, yl.to(device), src, tgt)[0]
    assert tuple(rec.shape) == (1, 1, 67 * HOP) and rec.abs().max().item() > 1e-4
    for durs in ([67], [7] * 8 + [11], [0, 30, 0, 37, 0]):
        o, (z_p, z_warp, _) = model.retime(spec, yl, src, tgt, durs, durs)
        assert torch.equal(z_p, z_warp) and _same(o, rec, f"retime {len(durs)} tokens")
    x, emo = _text(model, 9, 52, device)
    xp = torch.zeros(1, T_X, x.shape[2], device=device, dtype=x.dtype)
    xp[:, :9] = x
    wav_b = torch.full((1, T_B * HOP + HOP - 1), float("nan"), device=device)
    wav_b[0, :n] = wav
    common = (wav_b, _dev_i([n], device), src, tgt, None, T_B, T_B)
    # without text: one token; with text: MAS' durations, whatever they are
    o, y_new, d_old, d_new, meta, scores = model.retime_bucketed(*common, stft=STFT)
    assert y_new.tolist() == [67] and d_old.tolist() == [[67]] == d_new.tolist() and scores is None
    assert meta[:, 0].tolist() == [67, 0, 0]
    assert _same(o[:, :, :67 * HOP], rec, "bucketed, no text")
    assert torch.count_nonzero(o[:, :, 67 * HOP:]).item() == 0
    o, y_new, d_old, d_new, meta, scores = model.retime_bucketed(
        *common, stft=STFT, x=xp, x_lengths=_dev_i([9], device), emo=emo)
    assert y_new.tolist() == [67] and torch.equal(d_old, d_new) and int(d_old.sum()) == 67
    assert scores is not None and torch.count_nonzero(d_old[0, 9:]).item() == 0
    assert _same(o[:, :, :67 * HOP], rec, "bucketed, text")
    # the graphs, with no control passed
    run = model.capture_retime_bucketed(0, T_B, T_B, stft=STFT)
    got = run(wav.view(1, -1), [n], [2], [3])
    assert got[1].tolist() == [67] and _same(got[0][:, :, :67 * HOP], rec, "graph, no text")
    run = model.capture_retime_bucketed(T_X, T_B, T_B, stft=STFT)
    got = run(wav.view(1, -1), [n], [2], [3], x=x, x_lengths=[9], emo=emo)
    assert torch.equal(got[2], d_old) and _same(got[0][:, :, :67 * HOP], rec, "graph, text")


# -- locality -----------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["base-fp32", "tiny-fp16"])
def test_retime_is_local(which, base, ev_tiny, device):
    """200 frames + 57 samples, 20 tokens of 10 frames, token 9 stretched by 2:
    f0 = 90, f1 = 100, f1' = 110, y_new = 210, context 46.  The shifted suffix
    rests on the position independence DESIGN.md 4t measured for fp32 and for
    tiny fp16 (not asserted at base fp16, where 4t measured the opposite)."""
    model = _model(which, base, ev_tiny)
    ctx = model.edit_context_frames()
    assert ctx == 46
    wav = _wave(200 * HOP + 57, 61).to(device)
    spec = _spec(wav, device)
    assert spec.shape[2] == 200
    sid = torch.tensor([3], device=device)
    yl = torch.tensor([200])
    d_old = [10] * 20
    d_new = [10] * 9 + [20] + [10] * 10
    o, _ = model.retime(spec, yl, sid, sid, d_old, d_new)
    rec = model.voice_conversion(spec, yl.to(device), sid, sid)[0]
    torch.cuda.synchronize()
    assert tuple(o.shape) == (1, 1, 210 * HOP) and rec.abs().max().item() > 1e-4
    o, rec = o[0, 0], rec[0, 0]
    lo, hi = 90 - ctx, 110 + ctx
    assert (lo, hi) == (44, 156)
    assert _same(o[:lo * HOP], rec[:lo * HOP], "prefix")
    assert _same(o[hi * HOP:], rec[(hi - 10) * HOP:], "suffix")
    # the retimed token is retimed: next to it the result is not the conversion
    assert not torch.equal(o[lo * HOP:90 * HOP], rec[lo * HOP:90 * HOP])
    # the comparison needs its context: with 8 frames in place of 46 it fails
    assert not torch.equal(o[:(90 - 8) * HOP], rec[:(90 - 8) * HOP])


# -- the bucketed path and its graph ------------------------------------------------------

N_S = [67 * HOP + 57, 131 * HOP + 100]  # two ragged rows: 67 and 131 frames
N_TOK = [9, 14]
SRC, TGT = [1, 2], [3, 0]  # (the tiny config has four speakers)


def _bucket_inputs(model, device, seed):
    g = torch.Generator().manual_seed(seed)
    wav = torch.full((2, T_B * HOP + HOP - 1), float("nan"))  # (never read past a row's end)
    for b, n in enumerate(N_S):
        wav[b, :n] = _wave(n, seed + b)
    noise = (torch.randn(2, model.inter_channels, T_B, generator=g) * 0.3).to(device)
    return wav.to(device), noise


def _check_rows(model, device, wav, noise, out, n_tok):
    """Each row of a bucketed result against ``retime`` of that row alone
    under the durations the result reports."""
    o, y_new, d_old, d_new, meta, _ = out
    assert tuple(o.shape) == (2, 1, T_B * HOP) and o.dtype == torch.float32
    assert meta[1:].tolist() == [[0, 0]] * 2 and meta[0].tolist() == y_new.tolist()
    for b, n in enumerate(N_S):
        f = n // HOP
        yn = int(y_new[b])
        assert int(d_old[b, :n_tok[b]].sum()) == f and int(d_new[b, :n_tok[b]].sum()) == yn <= T_B
        assert torch.count_nonzero(d_new[b, n_tok[b]:]).item() == 0
        ref, _ = model.retime(_spec(wav[b, :n], device), torch.tensor([f]),
                              torch.tensor([SRC[b]], device=device),
                              torch.tensor([TGT[b]], device=device), d_old[b, :n_tok[b]],
                              d_new[b, :n_tok[b]], noise=noise[b:b + 1, :, :f].contiguous())
        assert _same(o[b, 0, :yn * HOP], ref[0, 0], f"row {b}")
        assert ref.abs().max().item() > 1e-4
        assert torch.count_nonzero(o[b, :, yn * HOP:]).item() == 0, b


def _replay_twice(run, args, kw, want):
    for rep in range(2):
        got = run(*args, **kw)
        torch.cuda.synchronize()
        for name, a, b in zip(("o", "y_new", "dur_old", "dur_new", "meta", "scores"), got, want):
            assert (a is None and b is None) or torch.equal(a, b), (rep, name)
        for v in run.static.values():
            v.fill_(float("nan") if v.is_floating_point() else -3)


@pytest.mark.parametrize("which", ["base-fp32", "tiny-fp16"])
def test_retime_bucketed_and_graph_equal_retime_bitwise(which, base, ev_tiny, device):
    model = _model(which, base, ev_tiny)
    wav, noise = _bucket_inputs(model, device, 71)
    src, tgt = torch.tensor(SRC, device=device), torch.tensor(TGT, device=device)
    common = (wav, _dev_i(N_S, device), src, tgt, noise, T_B, T_B)
    # 1) without text: a speed on row 0, a fitted length on row 1
    ctl = dict(rate=torch.tensor([1.3, 1.0], device=device), target=_dev_i([0, 100], device))
    out = model.retime_bucketed(*common, stft=STFT, controls=ctl)
    torch.cuda.synchronize()
    assert out[1].tolist() == [87, 100] and out[2].tolist() == [[67], [131]] and out[5] is None
    _check_rows(model, device, wav, noise, out, [1, 1])
    run = model.capture_retime_bucketed(0, T_B, T_B, batch=2, stft=STFT)
    flat = (wav[:, :max(N_S)].nan_to_num(0.0), N_S, SRC, TGT)
    _replay_twice(run, flat, dict(controls=[dict(rate=1.3), dict(target=100)], noise=noise), out)
    # 2) with text: 9 and 14 tokens; a scaled token and a pin on row 0, a speed on row 1
    texts = [_text(model, N_TOK[b], 80 + b, device) for b in range(2)]
    x = torch.zeros(2, T_X, texts[0][0].shape[2], device=device, dtype=texts[0][0].dtype)
    for b in range(2):
        x[b, :N_TOK[b]] = texts[b][0][0]
    emo = torch.cat([t[1] for t in texts])
    given = torch.full((2, T_X), -1, dtype=I32)
    given[0, 2] = 13
    scale = torch.ones(2, T_X)
    scale[0, 5] = 2.0
    ctl = dict(given=given.to(device), tok_scale=scale.to(device),
               rate=torch.tensor([1.0, 0.8], device=device))
    out = model.retime_bucketed(*common, stft=STFT, x=x, x_lengths=_dev_i(N_TOK, device), emo=emo,
                                controls=ctl)
    torch.cuda.synchronize()
    assert out[3][0, 2].item() == 13 and out[5] is not None
    assert out[3][0, 5].item() == 2 * out[2][0, 5].item()
    _check_rows(model, device, wav, noise, out, N_TOK)
    run = model.capture_retime_bucketed(T_X, T_B, T_B, batch=2, stft=STFT)
    rows_ctl = [dict(given=[-1, -1, 13], tok_scale=[1, 1, 1, 1, 1, 2.0]), dict(rate=0.8)]
    _replay_twice(run, flat, dict(x=x, x_lengths=N_TOK, emo=emo, controls=rows_ctl, noise=noise),
                  out)
    # a replay that passes no control resets them on the device: the durations come back as MAS'
    got = run(*flat, x=x, x_lengths=N_TOK, emo=emo, noise=noise)
    assert torch.equal(got[3], got[2]) and torch.equal(got[2], out[2])
    # the graph that is handed its durations holds no alignment
    run_d = model.capture_retime_bucketed(T_X, T_B, T_B, batch=2, stft=STFT, given_durations=True)
    d_old = [[7] * 8 + [11], [9] * 13 + [14]]
    got = run_d(*flat, x_lengths=N_TOK, controls=rows_ctl, noise=noise,
                durations_old=[d + [0] * (14 - len(d)) for d in d_old])
    torch.cuda.synchronize()
    assert got[5] is None and got[2][0, :9].tolist() == d_old[0]
    _check_rows(model, device, wav, noise, got, N_TOK)


# -- serving --------------------------------------------------------------------------------

def _recording(n, seed):
    return _wave(n, seed).mul(32767).to(torch.int16).numpy()


def test_serving(ev_tiny, device):
    from vits_amd import vits_wrap

    ev = ev_tiny
    rng = np.random.RandomState(9)
    text = rng.randn(10, ev.model.text_channels).astype(np.float32)
    emo = torch.from_numpy(rng.randn(1, 1024).astype(np.float32))
    rec = _recording(120 * HOP + 57, 8)
    x = torch.from_numpy(rec.astype(np.float32) / 32768.0).to(device)
    spec = _spec(x, device)
    sid = lambda v: torch.tensor([v], device=device)  # noqa: E731
    state = np.random.get_state()
    # 1) without text: it is the model's retime of the durations it returns
    wav, d_old, d_new, scores = ev.retime(rec, 1, 2, speed=1.1, return_durations=True)
    assert d_old.tolist() == [120] and d_new.tolist() == [132] and scores is None
    assert wav.dtype == np.float32 and wav.shape == (132 * HOP,) and np.abs(wav).max() > 1e-4
    ref, _ = ev.model.retime(spec, torch.tensor([120]), sid(1), sid(2), d_old, d_new)
    assert np.array_equal(wav, ref[0, 0].cpu().numpy())
    assert [k for k in ev._graphs if k[0] == "retime"] == [("retime", 1, 0, 256, 256, False)]
    # a second call captures nothing; graph=False gives the same bytes
    n_graphs = len(ev._graphs)
    assert np.array_equal(ev.retime(rec, 1, 2, speed=1.1), wav) and len(ev._graphs) == n_graphs
    assert np.array_equal(ev.retime(rec, 1, 2, speed=1.1, graph=False), wav)
    assert len(ev._graphs) == n_graphs and ev.graph is True
    # 2) with text: the alignment inside the graph, one token stretched, one pinned
    kw = dict(text=text, emo=emo, token_scale=[1.0] * 4 + [2.0] + [1.0] * 5,
              durations=[-1] * 7 + [9, -1, -1])
    wav_t, d_old, d_new, scores = ev.retime(rec, 1, 1, return_durations=True, **kw)
    assert ("retime", 1, 32, 256, 512, False) in ev._graphs
    assert int(d_old.sum()) == 120 and d_new[7] == 9 and d_new[4] == 2 * d_old[4]
    assert scores.shape == (10,) and scores.dtype == np.float32
    ali = ev.align(rec, 1, text, emo)
    assert np.array_equal(ali[0], d_old) and np.array_equal(ali[1], scores)
    ref, _ = ev.model.retime(spec, torch.tensor([120]), sid(1), sid(1), d_old, d_new)
    assert np.array_equal(wav_t, ref[0, 0].cpu().numpy())
    assert np.array_equal(ev.retime(rec, 1, 1, graph=False, **kw), wav_t)
    # ... and durations_old in place of the alignment: no text encoder in that graph
    wav_d = ev.retime(rec, 1, 1, text=text, durations_old=d_old, token_scale=kw["token_scale"],
                      durations=kw["durations"])
    assert ("retime", 1, 32, 256, 512, True) in ev._graphs and np.array_equal(wav_d, wav_t)
    # 3) the output stage: a fitted length, and a pitch that keeps the length
    ctl = dict(volume=0.8, tail_silence=0.01)
    pcm, n_model = ev.retime_pcm(rec, 1, 2, target_frames=150)
    assert n_model == 150 * HOP and pcm.shape == (150 * HOP,) and pcm.dtype == np.int16
    fit = ev.retime(rec, 1, 2, target_frames=150)
    assert np.array_equal(pcm, vits_wrap.host_pcm(fit, 16000, 1.0, 16000, 1.0, 0.0))
    plain = ev.convert_pcm(rec, 1, 2, pitch=1.0)[0]
    high, n_high, _, d_high, _ = ev.retime_pcm(rec, 1, 2, pitch=1.25, return_durations=True)
    assert d_high.tolist() == [96] and n_high == 96 * HOP
    assert abs(len(high) - len(plain)) <= math.ceil(HOP * 1.25)
    assert np.array_equal(ev.retime_pcm(rec, 1, 2, pitch=1.25, graph=False, **ctl)[0],
                          ev.retime_pcm(rec, 1, 2, pitch=1.25, **ctl)[0])
    # numpy's generator was not touched
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    # 4) what the device finds out is refused after the one copy
    with pytest.raises(ValueError, match="target_frames"):
        ev.retime(rec, 1, 1, text=text, emo=emo, durations=[20] * 9 + [-1], target_frames=150)
    # 5) the wrapper, with a stub front end
    wrap = vits_wrap.VITSWrap(textparser=lambda uid, t: (uid, t, text), speecher=ev,
                              device_post=True)
    res = wrap.retiming({"wav": rec, "spkid_src": 1, "speed": 1.1, "id": "r1", **ctl})
    want = ev.retime_pcm(rec, 1, 1, speed=1.1, **ctl)
    assert res["wav"][:4] == b"RIFF" and res["sr"] == 16000 and res["id"] == "r1"
    assert res["wav"][44:] == want[0].tobytes() and "durations" not in res
    assert res["length_s"] == 132 * HOP / 16000 and res["rtf"] > 0
    assert len(res["segment_info"]) == 1
    res = wrap.retiming({"wav": rec, "spkid_src": 1, "spkid_tgt": 2, "text": "the text",
                         "emotion": emo, "duration_s": 1.8, "token_scale": kw["token_scale"],
                         **ctl})
    want = ev.retime_pcm(rec, 1, 2, text=text, emo=emo, target_frames=150,
                         token_scale=kw["token_scale"], return_durations=True, **ctl)
    assert res["wav"][44:] == want[0].tobytes() and res["length_s"] == 150 * HOP / 16000
    assert res["durations_old"].tolist() == want[2].tolist()
    assert res["durations"].tolist() == want[3].tolist() and int(res["durations"].sum()) == 150
    assert len(res["boundaries_s"]) == 11
    with pytest.raises(ValueError, match="device_post"):
        vits_wrap.VITSWrap(textparser=lambda uid, t: (uid, t, text),
                           speecher=ev).retiming({"wav": rec, "spkid_src": 1})

"""Duration control through the model (SynthesizerTrn.infer_durations,
infer_bucketed(control=...), capture_infer_bucketed(control=True)), base
config, bucket 256.

infer_durations (infer_p1 -> commons.infer_path(durations) -> infer_p2, exact
lengths, eager) is the definition; the controlled bucketed path computes its
durations on the device (ops.duration_plan) and must then be that definition
applied to the durations it returns: every comparison of waveforms is BITWISE
on the first y_len * hop samples, eager, replayed from a graph, alone and as a
row of a ragged batch.  The golden (tests/golden/make_golden_durations.py) is
the reference model driven with a hand-made path; it is met within rel_err <
1e-4, the bar of the infer golden in test_configs_gpu.py."""
import numpy as np
import pytest
import torch

from common import base_model, golden, rel_err, snr_db
from serve_batch_common import shared_pool_draw

pytestmark = pytest.mark.gpu

HOP, C, T_Y = 192, 192, 256


@pytest.fixture(scope="module")
def base(device):
    return base_model(device)


@pytest.fixture(scope="module")
def graph1(base):
    """One controlled utterance graph (64 tokens, 256 frames) for every
    batch-1 replay of this file."""
    return base.capture_infer_bucketed(64, T_Y, padded_text=True, control=True)


def _inputs(device, t_x, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, t_x, 256, generator=g).to(device)
    emo = torch.randn(1, 1024, generator=g).to(device)
    sid = torch.tensor([int(torch.randint(0, 2048, (1,), generator=g))], device=device)
    noise = (torch.randn(1, C, T_Y, generator=g) * 0.707).to(device)
    return x, emo, sid, noise


def _cases(t_x):
    """(name, rate, given, tok_scale, target) on t_x tokens.  The rates and
    scales of the cases without a target are low, so that their totals fit
    the 256-frame bucket (asserted where they are used)."""
    rng = np.random.default_rng(t_x)
    pins = np.full(t_x, -1, np.int32)
    pins[0], pins[t_x // 2], pins[-1] = 0, 30, 4
    scale = rng.uniform(0.3, 1.0, t_x).astype(np.float32)
    scale[1] = 0.0
    all_pinned = rng.integers(0, 6, t_x).astype(np.int32)
    return [("pins and scales", 0.5, pins, scale, None),
            ("pins, scales and a target", 1.0, pins, scale, 200),
            ("a target alone", 1.7, None, None, 131),
            ("every token pinned", 1.0, all_pinned, None, None),
            ("an infeasible target", 0.4, pins, None, 34 + t_x - 4)]


def _ctl(device, given, scale, target):
    c = {}
    if given is not None:
        c["given"] = torch.from_numpy(given).to(device).view(1, -1)
    if scale is not None:
        c["tok_scale"] = torch.from_numpy(scale).to(device).view(1, -1)
    if target is not None:
        c["target"] = torch.tensor([target], dtype=torch.int32, device=device)
    return c


@pytest.mark.parametrize("t_x", [12, 37])
def test_infer_bucketed_control_equals_infer_durations(base, graph1, device, t_x):
    x, emo, sid, noise = _inputs(device, t_x, 100 + t_x)
    seen = []
    for name, rate, given, scale, target in _cases(t_x):
        wav, y_len, dur, meta = base.infer_bucketed(x, emo, sid, noise, T_Y, length_scale=rate,
                                                    control=_ctl(device, given, scale, target))
        n, total, status = int(y_len[0]), int(meta[0, 0]), int(meta[1, 0])
        d = dur[0].cpu().numpy()
        assert dur.shape == (1, t_x) and n == max(total, 1) == max(int(d.sum()), 1) <= T_Y, name
        assert status == int(name == "an infeasible target"), name
        if given is not None:
            assert np.array_equal(d[given >= 0], given[given >= 0]), name
        if target is not None and not status:
            assert total == target, name
        ref = base.infer_durations(x, emo, sid, dur[0], noise[:, :, :n])
        assert ref.shape == (1, 1, n * HOP)
        assert torch.equal(wav[:, :, :n * HOP], ref), name
        # the same utterance replayed from the one cached graph
        ctl = dict(given=given, tok_scale=scale, target=target)
        wav_g, yl_g, dur_g, meta_g = graph1(x, emo, sid, noise, x_length=t_x, rate=rate,
                                            control=ctl)
        assert torch.equal(dur_g[0, :t_x], dur[0]) and int(dur_g[0, t_x:].sum()) == 0, name
        assert torch.equal(meta_g, meta) and int(yl_g[0]) == n, name
        assert torch.equal(wav_g[:, :, :n * HOP], ref), name
        seen.append(d.tolist())
    assert len({tuple(s) for s in seen}) == len(seen)  # the controls did change the timing


def test_neutral_control_equals_no_control(base, graph1, device):
    """Every token free, scale 1, no target: bit for bit the uncontrolled
    call, eager and from the graph (whose replay without controls is
    neutral)."""
    t_x = 37
    x, emo, sid, noise = _inputs(device, t_x, 7)
    plain, yl = base.infer_bucketed(x, emo, sid, noise, T_Y, length_scale=0.6)
    n = int(yl[0])
    assert n <= T_Y
    neutral = dict(given=torch.full((1, t_x), -1, dtype=torch.int32, device=device),
                   tok_scale=torch.ones(1, t_x, device=device),
                   target=torch.zeros(1, dtype=torch.int32, device=device))
    for control in (neutral, {}):
        wav, yl2, dur, meta = base.infer_bucketed(x, emo, sid, noise, T_Y, length_scale=0.6,
                                                  control=control)
        assert torch.equal(yl, yl2) and torch.equal(wav[:, :, :n * HOP], plain[:, :, :n * HOP])
        assert int(meta[0, 0]) == n and int(meta[1, 0]) == 0
    wav_g, yl_g, _, _ = graph1(x, emo, sid, noise, x_length=t_x, rate=0.6)
    assert int(yl_g[0]) == n and torch.equal(wav_g[:, :, :n * HOP], plain[:, :, :n * HOP])
    with pytest.raises(ValueError, match="unknown control"):
        base.infer_bucketed(x, emo, sid, noise, T_Y, control=dict(durations=None))


def test_three_ragged_rows_equal_each_row_alone(base, device):
    """A ragged batch through the shared-pool form, eager and replayed from a
    batch-4 graph with a padding row: each row is infer_durations of its own
    durations on its own noise slice."""
    from vits_amd import ops

    lengths = [37, 12, 25]
    t_x, B = 37, 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, t_x, 256, generator=g)
    for b, n in enumerate(lengths):
        x[b, n:] = 0
    x = x.to(device)
    emo = torch.randn(B, 1024, generator=g).to(device)
    sid = torch.tensor([5, 1999, 310], device=device)
    flat = (torch.randn(C * 300, generator=g) * 0.707).to(device)
    given = np.full((B, t_x), -1, np.int32)
    given[0, 3], given[1, 0], given[2, 24] = 25, 0, 9
    scale = np.ones((B, t_x), np.float32)
    scale[1, :12] = 1.5
    target = np.array([150, 0, 90], np.int32)
    rates = [1.0, 1.2, 0.7]
    np.random.seed(17)
    pool, _ = ops.numpy_draw_pool(ops.ED_DRAWS * 4)
    pool_d = torch.from_numpy(pool).to(device)
    d = lambda a: torch.from_numpy(a).to(device)
    wav, y_len, status, used, dur, meta = base.infer_bucketed(
        x, emo, sid, flat, T_Y, x_lengths=torch.tensor(lengths, dtype=torch.int32, device=device),
        length_scale=torch.tensor(rates, device=device), noise_start=pool_d, n_rows=B,
        control=dict(given=d(given), tok_scale=d(scale), target=d(target)))
    ys = y_len.tolist()
    assert meta[0].tolist() == ys and meta[1].tolist() == [0, 0, 0]
    assert ys[0] == 150 and ys[2] == 90 and min(status.tolist()) >= 0
    starts, _, _ = shared_pool_draw(pool, [flat.numel() - C * n for n in ys])
    refs = []
    for b, n in enumerate(lengths):
        assert int(dur[b, n:].sum()) == 0
        noise = flat[starts[b]:starts[b] + C * ys[b]].view(1, C, ys[b])
        ref = base.infer_durations(x[b:b + 1, :n], emo[b:b + 1], sid[b:b + 1], dur[b, :n], noise)
        assert torch.equal(wav[b:b + 1, :, :ys[b] * HOP], ref), b
        refs.append(ref)
    run = base.capture_infer_bucketed(64, T_Y, noise_len=flat.numel(), padded_text=True, batch=4,
                                      control=True)
    run.static["noise"].copy_(flat)
    out = run(x, emo, sid, lengths, pool, rates=rates,
              control=dict(given=[given[b, :n] for b, n in enumerate(lengths)],
                           tok_scale=[None, scale[1, :12], None], target=target.tolist()))
    wav_g, yl_g, st_g, used_g, dur_g, meta_g = out
    assert yl_g.tolist() == ys + [1] and int(used_g) == int(used)
    assert meta_g[0].tolist()[3] == 0 and meta_g[1].tolist() == [0, 0, 0, 0]
    for b in range(B):
        assert torch.equal(dur_g[b, :t_x], dur[b]) and int(dur_g[b, t_x:].sum()) == 0
        assert torch.equal(wav_g[b:b + 1, :, :ys[b] * HOP], refs[b]), b
    # the next replay without controls is neutral again: the plain batch
    out2 = run(x, emo, sid, lengths, pool, rates=rates)
    plain = base.infer_bucketed(
        x, emo, sid, flat, T_Y, x_lengths=torch.tensor(lengths, dtype=torch.int32, device=device),
        length_scale=torch.tensor(rates, device=device), noise_start=pool_d, n_rows=B)
    assert out2[1].tolist()[:B] == plain[1].tolist()
    for b in range(B):
        n = int(plain[1][b])
        if n <= T_Y:  # (a row longer than the bucket is cut: nothing to compare)
            assert torch.equal(out2[0][b, :, :n * HOP], plain[0][b, :, :n * HOP])


def test_golden_reference_with_hand_made_durations(base, graph1, device):
    gd = golden("base_durations.npz")
    d = gd["durations"]
    t_x, n = len(d), int(d.sum())
    assert t_x == 20 and n == 98 and 0 in d and 30 in d
    x, emo = (torch.from_numpy(gd[k]).to(device) for k in ("x", "emo"))
    sid = torch.from_numpy(gd["sid"]).to(device)
    noise = torch.from_numpy(gd["noise"]).to(device)
    o = base.infer_durations(x, emo, sid, d, noise)
    err = rel_err(o, gd["wav"])
    print(f"infer_durations vs the reference: rel_err {err:.3e}, snr {snr_db(o, gd['wav']):.1f} dB")
    assert o.shape == gd["wav"].shape
    assert err < 1e-4
    padded = torch.zeros(1, C, T_Y, device=device)
    padded[:, :, :n] = noise
    wav, yl, dur, meta = graph1(x, emo, sid, padded, x_length=t_x, control=dict(given=d))
    assert int(yl[0]) == n and dur[0, :t_x].tolist() == d.tolist() and int(meta[1, 0]) == 0
    err_g = rel_err(wav[:, :, :n * HOP], gd["wav"])
    print(f"controlled graph vs the reference: rel_err {err_g:.3e}")
    assert err_g < 1e-4


def test_infer_durations_refuses_bad_durations(base, device):
    x, emo, sid, noise = _inputs(device, 12, 1)
    with pytest.raises(ValueError, match="durations"):
        base.infer_durations(x, emo, sid, [1] * 11, noise[:, :, :11])
    with pytest.raises(ValueError, match="durations"):
        base.infer_durations(x, emo, sid, [1] * 11 + [-1], noise[:, :, :11])


# -- EmoVITS ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emovits(device, tmp_path_factory):
    from common import BASE_MODEL
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    hps = get_hparams_from_dict({"data": {"sampling_rate": 16000, "hop_length": HOP,
                                          "text_channels": 256, "n_speakers": 2048,
                                          "noise_scale": 0.707},
                                 "model": dict(BASE_MODEL)})
    return EmoVITS(str(tmp_path_factory.mktemp("ev") / "ckpt.pth"), device, hps=hps,
                   model=base_model(device), graph=True)


def _model_calls(ev, device, text, emo_h, sid, seed, rate, kw, dur):
    """What EmoVITS' two modes must hand to the model, made by hand from the
    same numpy seed: (the bucketed controlled call over the 32-token / 256-frame
    bucket, infer_durations of ``dur`` on the eager mode's noise slice)."""
    from vits_amd import ops

    t_x, n = text.shape[0], max(int(dur.sum()), 1)
    x = torch.from_numpy(text).half().to(device).unsqueeze(0)
    x_pad = torch.zeros(1, 32, 256, dtype=torch.float16, device=device)
    x_pad[:, :t_x] = x
    given = torch.full((1, 32), -1, dtype=torch.int32)
    scale = torch.ones(1, 32)
    if kw.get("durations") is not None:
        given[0, :t_x] = torch.tensor(kw["durations"], dtype=torch.int32)
    if kw.get("token_scale") is not None:
        scale[0, :t_x] = torch.from_numpy(kw["token_scale"])
    target = torch.tensor([kw.get("target_frames") or 0], dtype=torch.int32)
    np.random.seed(seed)
    pool, _ = ops.numpy_draw_pool()
    wav, _, _, _ = ev.model.infer_bucketed(
        x_pad, emo_h, sid, ev.noise.float(), T_Y,
        x_lengths=torch.tensor([t_x], dtype=torch.int32, device=device),
        length_scale=torch.tensor([rate], device=device),
        noise_start=torch.from_numpy(pool).to(device).view(1, -1),
        control=dict(given=given.to(device), tok_scale=scale.to(device),
                     target=target.to(device)))
    np.random.seed(seed)
    start = np.random.randint(ev.noise.numel() - C * n)
    exact = ev.model.infer_durations(x, emo_h, sid, dur, ev.noise[start:start + C * n].view(1, C, n))
    return (wav[0, 0, :n * HOP].float().cpu().numpy(), exact.float().view(-1).cpu().numpy())


def test_emovits_controls_graph_on_and_graph_off(emovits, device):
    """infer / infer_pcm with durations, scales and a target (fp16 model),
    six control sets through ONE cached controlled graph.  Graph mode and
    eager mode (the plan's rule on the host, then infer_p2) give the same
    durations, the same sample counts and leave numpy's generator in the same
    state; the graph's samples are bitwise the model's bucketed controlled
    call, the eager mode's bitwise infer_durations of those durations on the
    slice the generator selects.

    The two waveforms themselves are not compared bitwise here.  The 16-bit
    conv kernels round a few samples of an exact-length run's partial last
    tile differently from the same tile inside a bucket, with or without
    controls: plain infer, graph on against off, is bitwise at 17 of 24 speeds
    from 1.0 to 4.45 on this text and up to 1,699 samples apart (last 64
    frames, one fp16 ulp) at the others, measured before this feature existed.
    Bucketed against exact-length IS compared bitwise, at every length, on the
    fp32 model in the tests above."""
    ev = emovits
    t_x = 20
    x, emo, sid, _ = _inputs(device, t_x, 5)
    text, emo_h, spk = x[0].float().cpu().numpy(), emo.half(), int(sid)
    d1 = [3, 5, 0, 7, 2, 30, 1, 4, 6, 2, 0, 3, 8, 1, 5, 4, 2, 9, 3, 3]
    d2 = [-1] * t_x
    d2[4], d2[19] = 12, 0
    scale = np.linspace(0.4, 1.2, t_x).astype(np.float32)
    calls = [dict(durations=d1), dict(durations=d2, duration_rate=0.6),
             dict(durations=d2, token_scale=scale, target_frames=150),
             dict(token_scale=scale, duration_rate=0.5), dict(target_frames=77),
             dict(duration_rate=0.7)]
    outs = {}
    for graph in (True, False):
        ev.graph = graph
        ev._graphs.clear()
        res = []
        for i, kw in enumerate(calls):
            np.random.seed(i)
            wav, _, dur = ev.infer(spk, text, emo_h, return_durations=True, **kw)
            pcm, _, n, dur2 = ev.infer_pcm(spk, text, emo_h, return_durations=True, volume=0.8,
                                           **kw)
            res.append((wav, dur, pcm, n, dur2, np.random.randint(1 << 30)))
        outs[graph] = res
        if graph:  # every control went through one graph (all totals fit 256 frames)
            assert list(ev._graphs) == [("ctl", 1, 32, 256)]
    ev.graph = True
    for i, (kw, g, e) in enumerate(zip(calls, outs[True], outs[False])):
        assert np.array_equal(g[1], e[1]) and np.array_equal(g[4], e[4]), kw
        assert np.array_equal(g[1], g[4]) and g[1].dtype == np.int32 and g[1].shape == (t_x,)
        total = max(int(g[1].sum()), 1)
        assert g[0].shape == e[0].shape == (total * HOP,) and g[3] == e[3] == total * HOP, kw
        assert g[2].shape == e[2].shape and g[2].dtype == e[2].dtype == np.int16, kw
        assert g[5] == e[5], kw  # numpy's generator ended in the same state
        rate = kw.get("duration_rate", 1.0)
        rest = {k: v for k, v in kw.items() if k != "duration_rate"}
        bucketed, exact = _model_calls(ev, device, text, emo_h, sid, i, rate, rest, g[1])
        assert np.array_equal(g[0], bucketed), kw
        assert np.array_equal(e[0], exact), kw
        print(f"{sorted(kw)}: {total} frames, graph vs eager samples apart "
              f"{int((g[0] != e[0]).sum())}, max {np.abs(g[0] - e[0]).max():.2e}")
    assert outs[True][0][1].tolist() == d1
    assert outs[True][2][1].sum() == 150 and outs[True][4][1].sum() == 77
    assert outs[True][4][0].shape == (77 * HOP,)
    pinned = np.array(d2) >= 0
    for i in (1, 2):
        assert np.array_equal(outs[True][i][1][pinned], np.array(d2)[pinned])


def test_emovits_plain_calls_are_untouched_by_return_durations(emovits, device):
    """return_durations alone reports ceil(exp(logw) * rate) and the samples
    of the plain call."""
    ev = emovits
    x, emo, sid, _ = _inputs(device, 20, 5)
    text, emo_h, spk = x[0].float().cpu().numpy(), emo.half(), int(sid)
    np.random.seed(3)
    plain, _ = ev.infer(spk, text, emo_h, duration_rate=0.7)
    s1 = np.random.randint(1 << 30)
    np.random.seed(3)
    wav, _, dur = ev.infer(spk, text, emo_h, duration_rate=0.7, return_durations=True)
    assert np.random.randint(1 << 30) == s1
    assert np.array_equal(wav, plain) and int(dur.sum()) * HOP == len(plain)
    with pytest.raises(ValueError, match="target_frames"):
        ev.infer(spk, text, emo_h, target_frames=19)


def test_emovits_fp32_graph_on_equals_graph_off(device, tmp_path):
    """The issue's check, on the engine that can meet it: an fp32 EmoVITS
    (half=False), six control sets, graph mode against eager mode: samples,
    PCM, durations and numpy's generator state, all bitwise."""
    from common import BASE_MODEL
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    hps = get_hparams_from_dict({"data": {"sampling_rate": 16000, "hop_length": HOP,
                                          "text_channels": 256, "n_speakers": 2048,
                                          "noise_scale": 0.707},
                                 "model": dict(BASE_MODEL)})
    ev = EmoVITS(str(tmp_path / "ckpt.pth"), device, hps=hps, model=base_model(device),
                 graph=True, half=False)
    assert ev.model.emb_g.weight.dtype == torch.float32 and ev.noise.dtype == torch.float32
    t_x = 20
    x, emo, sid, _ = _inputs(device, t_x, 5)
    text, spk = x[0].cpu().numpy(), int(sid)
    d1 = [3, 5, 0, 7, 2, 30, 1, 4, 6, 2, 0, 3, 8, 1, 5, 4, 2, 9, 3, 3]
    d2 = [-1] * t_x
    d2[4], d2[19] = 12, 0
    scale = np.linspace(0.4, 1.2, t_x).astype(np.float32)
    calls = [dict(durations=d1), dict(durations=d2, duration_rate=0.6),
             dict(durations=d2, token_scale=scale, target_frames=150),
             dict(token_scale=scale, duration_rate=0.5), dict(target_frames=77),
             dict(duration_rate=0.7), dict(target_frames=200, duration_rate=1.3)]
    outs = {}
    for graph in (True, False):
        ev.graph = graph
        res = []
        for i, kw in enumerate(calls):
            np.random.seed(i)
            wav, _, dur = ev.infer(spk, text, emo, return_durations=True, **kw)
            pcm, _, n, dur2 = ev.infer_pcm(spk, text, emo, return_durations=True, volume=0.8,
                                           pitch=1.2, **kw)
            res.append((wav, dur, pcm, n, dur2, np.random.randint(1 << 30)))
        outs[graph] = res
    assert list(ev._graphs) == [("ctl", 1, 32, 256)]
    for kw, g, e in zip(calls, outs[True], outs[False]):
        total = max(int(g[1].sum()), 1)
        assert np.array_equal(g[1], e[1]) and np.array_equal(g[4], e[4]), kw
        assert np.array_equal(g[1], g[4]) and g[3] == e[3] == total * HOP, kw
        assert g[0].shape == (total * HOP,) and np.array_equal(g[0], e[0]), kw
        assert g[2].dtype == np.int16 and np.array_equal(g[2], e[2]), kw
        assert g[5] == e[5], kw
    assert [int(o[1].sum()) for o in outs[True]][2::2] == [150, 77, 200]

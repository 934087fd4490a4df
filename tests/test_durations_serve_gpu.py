"""Duration control through the serving entry points, on the tiny checkpoint
(fp16 EmoVITS, graph mode): the batch calls with controlled and plain rows in
one group against the one-by-one loop (bytes, durations, numpy's generator),
VITSWrap.speaking with duration_s, and speaking_like against aligning followed
by speaking(durations=...), byte for byte.  Everything compared here runs
through utterance graphs on both sides (bucket against bucket), so the
comparisons are bitwise."""
import numpy as np
import pytest
import torch

import vc_common as VC
from common import build_model, tiny_cfg
from serve_batch_common import same_state

pytestmark = pytest.mark.gpu

STFT = (VC.STFT["n_fft"], VC.STFT["hop"], VC.STFT["win"])
HOP = VC.STFT["hop"]


@pytest.fixture(scope="module")
def ev(device, tmp_path_factory):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    c = tiny_cfg()
    model = build_model(c["model"], dict(c["data"], spec_channels=STFT[0] // 2 + 1), device)
    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "filter_length": STFT[0], "hop_length": HOP,
                 "win_length": STFT[2], "text_channels": c["data"]["text_channels"],
                 "n_speakers": model.emb_g.num_embeddings, "noise_scale": 0.667},
        "model": {"inter_channels": model.inter_channels}})
    return EmoVITS(str(tmp_path_factory.mktemp("ev") / "ckpt.pth"), device, hps=hps, model=model,
                   graph=True)


def _items(ev, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(1 + i % 3, torch.randn(n, ev.text_channels, generator=g).numpy(),
             torch.randn(1, 1024, generator=g)) for i, n in enumerate(lengths)]


def _controls(lengths):
    """Per item: all pinned (with zeros), none, scales, a target, none, pins
    and a target."""
    rng = np.random.default_rng(4)
    n = lengths
    d0 = rng.integers(0, 5, n[0]).tolist()
    d5 = [-1] * n[5]
    d5[0], d5[-1] = 0, 11
    durations = [d0, None, None, None, None, d5]
    scales = [None, None, rng.uniform(0.3, 1.5, n[2]).astype(np.float32), None, None, None]
    targets = [None, None, None, 120, None, 90]
    return durations, scales, targets


def _loop_pcm(ev, items, ctl, **post):
    out = []
    for (spk, text, emo), d, s, t in zip(items, *ctl):
        if d is None and s is None and t is None:
            pcm, _, n = ev.infer_pcm(spk, text, emo, **post)  # the plain path
            out.append((pcm, n, None))
        else:
            pcm, _, n, dur = ev.infer_pcm(spk, text, emo, durations=d, token_scale=s,
                                          target_frames=t, return_durations=True, **post)
            out.append((pcm, n, dur))
    return out


def test_infer_pcm_batch_mixed_rows_equal_the_loop(ev):
    lengths = [9, 12, 33, 5, 20, 14]
    items = _items(ev, lengths, 1)
    ctl = _controls(lengths)
    post = dict(duration_rate=0.9, pitch=1.1, sampling_rate=22050, volume=0.7, tail_silence=0.01)
    np.random.seed(3)
    want = _loop_pcm(ev, items, ctl, **post)
    want_state = np.random.get_state()
    np.random.seed(3)
    pcm, offs, _, n_model, durs = ev.infer_pcm_batch(
        items, durations=ctl[0], token_scale=ctl[1], target_frames=ctl[2],
        return_durations=True, **post)
    assert same_state(np.random.get_state(), want_state)
    assert any(k[0] == "ctl" and k[1] == 8 for k in ev._graphs)
    assert len(durs) == len(items) and n_model == [w[1] for w in want]
    for i, (w_pcm, _, w_dur) in enumerate(want):
        assert np.array_equal(pcm[offs[i]:offs[i + 1]], w_pcm), i
        assert durs[i].dtype == np.int32 and durs[i].shape == (lengths[i],)
        assert int(durs[i].sum()) * HOP == n_model[i] or n_model[i] == HOP
        if w_dur is not None:
            assert np.array_equal(durs[i], w_dur), i
    assert durs[0].tolist() == ctl[0][0] and durs[3].sum() == 120 and durs[5].sum() == 90
    assert durs[5][0] == 0 and durs[5][-1] == 11
    # without return_durations: the four results of before, the same bytes
    np.random.seed(3)
    again = ev.infer_pcm_batch(items, durations=ctl[0], token_scale=ctl[1],
                               target_frames=ctl[2], **post)
    assert len(again) == 4 and np.array_equal(again[0], pcm) and np.array_equal(again[1], offs)
    # infer_batch: the waveforms of the loop over infer
    np.random.seed(3)
    loop = [ev.infer(spk, text, emo, duration_rate=0.9, durations=d, token_scale=s,
                     target_frames=t)[0]
            for (spk, text, emo), d, s, t in zip(items, *ctl)]
    state = np.random.get_state()
    np.random.seed(3)
    got = ev.infer_batch(items, duration_rate=0.9, durations=ctl[0], token_scale=ctl[1],
                         target_frames=ctl[2], return_durations=True)
    assert same_state(np.random.get_state(), state)
    for i, (a, b) in enumerate(zip(loop, got)):
        assert np.array_equal(a, b[0]) and np.array_equal(b[2], durs[i]), i
    with pytest.raises(ValueError, match="one entry per item"):
        ev.infer_pcm_batch(items, durations=ctl[0][:3])
    with pytest.raises(ValueError, match="target_frames"):
        ev.infer_batch(items, target_frames=[None, 3, None, None, None, None])


def test_infer_pcm_requests_mixed_rows_equal_the_loop(ev):
    from vits_amd.infer import PcmRequest

    lengths = [9, 12, 33, 5, 20, 14]
    items = _items(ev, lengths, 2)
    d, s, t = _controls(lengths)
    reqs = [PcmRequest(items[:2], duration_rate=1.2, durations=d[:2]),
            PcmRequest(items[2:5], pitch=0.9, sampling_rate=8000, volume=0.5, tail_silence=0.02,
                       token_scale=s[2:5], target_frames=t[2:5]),
            PcmRequest(items[5:], duration_rate=0.8, durations=d[5:], target_frames=t[5:])]
    np.random.seed(9)
    want = []
    for r, lo in zip(reqs, (0, 2, 5)):
        n = len(r.items)
        want.append(_loop_pcm(ev, r.items, (d[lo:lo + n], s[lo:lo + n], t[lo:lo + n]),
                              duration_rate=r.duration_rate, pitch=r.pitch,
                              sampling_rate=r.sampling_rate, volume=r.volume,
                              tail_silence=r.tail_silence))
    want_state = np.random.get_state()
    np.random.seed(9)
    got = ev.infer_pcm_requests(reqs, return_durations=True)
    assert same_state(np.random.get_state(), want_state)
    for rows, (pcm, offs, _, n_model, durs) in zip(want, got):
        assert len(rows) == len(durs) == len(offs) - 1
        for i, (w_pcm, w_n, w_dur) in enumerate(rows):
            assert np.array_equal(pcm[offs[i]:offs[i + 1]], w_pcm) and n_model[i] == w_n
            if w_dur is not None:
                assert np.array_equal(durs[i], w_dur)
    np.random.seed(9)
    plain = ev.infer_pcm_requests(reqs)
    assert all(len(p) == 4 for p in plain)
    assert all(np.array_equal(p[0], g[0]) for p, g in zip(plain, got))


class _Front:
    max_utt_length = 16

    def __init__(self, channels):
        self.channels = channels

    def __call__(self, uid, txt):
        g = torch.Generator().manual_seed(len(txt))
        return uid, txt, torch.randn(len(txt), self.channels, generator=g).numpy()


def test_vitswrap_duration_s_and_speaking_like(ev):
    from vits_amd import vits_wrap

    g = torch.Generator().manual_seed(8)
    emo = torch.randn(1, 1024, generator=g)
    front = _Front(ev.text_channels)
    dev = vits_wrap.VITSWrap(textparser=front, speecher=ev, device_post=True)
    host = vits_wrap.VITSWrap(textparser=front, speecher=ev)
    # duration_s: round(s * rate / hop) frames of the model, before the output stage
    frames = round(0.5 * 16000 / HOP)
    for wrap in (dev, host):
        out = wrap.speaking({"text": "abcdefghi", "spkid": 1, "emotion": emo, "duration_s": 0.5})
        assert len(out["wav"]) == 44 + 2 * frames * HOP
        assert out["durations"].shape == (9,) and int(out["durations"].sum()) == frames
        assert out["boundaries_s"][-1] == pytest.approx(frames * HOP / 16000, rel=1e-12)
    out = dev.speaking({"text": "abcdefghi", "spkid": 1, "emotion": emo, "duration_s": 0.5,
                        "sampling_rate": 8000})
    assert len(out["wav"]) == 44 + 2 * (frames * HOP // 2)  # the stage halves the rate afterwards
    many = dev.speaking_many([{"text": "abc", "spkid": 1, "emotion": emo},
                              {"text": "abcdefghi", "spkid": 1, "emotion": emo,
                               "token_scale": [2.0] * 9}])
    assert "durations" in many[1] and "durations" not in many[0]
    # speaking_like == aligning, then speaking with its durations
    gen = torch.Generator().manual_seed(0)
    rec = (torch.randn(30 * HOP + 11, generator=gen) * 0.25).clamp(-1, 1).mul(32767).to(
        torch.int16).numpy()
    fields = {"text": "abcdefghi", "emotion": emo, "pitch": 1.1, "sampling_rate": 24000,
              "volume": 0.8, "tail_silence": 0.01, "id": "u"}
    al = dev.aligning({"wav": rec, "text": "abcdefghi", "spkid": 1, "emotion": emo})
    assert al["frames"] == 30
    np.random.seed(5)
    want = dev.speaking(dict(fields, spkid=2, durations=al["durations"]))
    want_state = np.random.get_state()
    np.random.seed(5)
    got = dev.speaking_like(dict(fields, spkid=2, spkid_src=1, wav=rec))
    assert same_state(np.random.get_state(), want_state)
    assert got["wav"] == want["wav"] and len(got["wav"]) > 44 + 2 * 30 * HOP
    assert np.array_equal(got["durations"], al["durations"])
    assert np.array_equal(got["boundaries_s"], al["boundaries_s"])
    assert got["segment_info"] == want["segment_info"] and got["sr"] == 24000
    # the eager mode of the same object gives the same durations and length
    ev.graph = False
    try:
        np.random.seed(5)
        eager = dev.speaking_like(dict(fields, spkid=2, spkid_src=1, wav=rec))
    finally:
        ev.graph = True
    assert np.array_equal(eager["durations"], al["durations"])
    assert len(eager["wav"]) == len(got["wav"])

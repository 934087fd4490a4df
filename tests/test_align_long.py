"""Forced alignment of long recordings, CPU side: the window plan with the
alignment context, SynthesizerTrn.align_context_frames against a restatement
from the config's numbers, the refusals of EmoVITS.align_long (host arithmetic,
before anything is uploaded), and the segment oracle of
tests/align_long_common.py against the reference's golden and under
perturbation.  No GPU."""
import numpy as np
import pytest
import torch

import align_common as A
import align_long_common as L
import vc_common as VC
from common import BASE_DATA, BASE_MODEL, base_model, build_model, golden, oracle_sd, tiny_cfg
from test_vc_long import HOP, N_FFT, STFT, WIN, _check_plan, _context_ref


@pytest.fixture(scope="module")
def ev_cpu(tmp_path_factory):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    c = tiny_cfg()
    data = dict(c["data"], spec_channels=N_FFT // 2 + 1)
    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "filter_length": N_FFT, "hop_length": HOP,
                 "win_length": WIN, "text_channels": data["text_channels"],
                 "n_speakers": data["n_speakers"], "noise_scale": 0.667},
        "model": c["model"]})
    model = build_model(c["model"], data, "cpu")
    return EmoVITS(str(tmp_path_factory.mktemp("al") / "ckpt.pth"), "cpu", hps=hps, model=model)


# -- the context and the plan ---------------------------------------------------


@pytest.mark.parametrize("which", ["base", "tiny"])
def test_align_context_matches_restatement(which):
    """The STFT's edge frames, enc_q's WN stack and the couplings' WN stacks
    once (the forward flow only), no decoder: base 3 + 32 + 32 = 67."""
    if which == "base":
        cfg, data = BASE_MODEL, BASE_DATA
    else:
        c = tiny_cfg()
        cfg, data = c["model"], dict(c["data"], spec_channels=N_FFT // 2 + 1)
    model = build_model(cfg, data, "cpu", fill=False)
    stft, enc_q, flows2, dec = _context_ref(cfg)
    assert flows2 % 2 == 0
    want = stft + enc_q + flows2 // 2
    assert model.align_context_frames(STFT) == want
    assert model.vc_context_frames(STFT) == want + flows2 // 2 + dec
    if which == "base":
        assert (stft, enc_q, flows2 // 2) == (3, 32, 32) and want == 67
    model.remove_weight_norm()
    assert model.align_context_frames(STFT) == want
    with pytest.raises(ValueError):
        model.align_context_frames((N_FFT, HOP // 2, WIN))


def test_plan_with_the_alignment_context(ev_cpu):
    """The properties tests/test_vc_long.py checks for the conversion plan, at
    the alignment context of the base config (67): windows of 256 (Cf = 122)
    and of 4096 frames, every remainder class, rows with one and with two
    artificial edges, and a recording of ten minutes."""
    ctx = 67
    both = 0
    for wf in (256, 4096):
        cf = wf - 2 * ctx
        lengths = (list(range(1, 140)) + [cf - 1, cf, cf + 1, 2 * cf, 2 * cf + 1, 3 * cf + 2,
                                          wf, wf + 1, 600, 5 * cf + 7, 50000])
        for F in lengths:
            for rem in (0, 1, HOP - 1):
                n = F * HOP + rem
                plan = ev_cpu._long_plan(n, wf, ctx)
                _check_plan(plan, n, wf, ctx)
                both += sum(1 for w in plan if w.a > 0 and w.b < F)
    assert both > 0
    # 600 frames at windows of 256: the shape of the GPU comparison, 5 windows
    assert len(ev_cpu._long_plan(600 * HOP + 57, 256, ctx)) == 5
    with pytest.raises(ValueError):
        ev_cpu._long_plan(1000 * HOP, 128, ctx)  # no core left


# -- the refusals of align_long -----------------------------------------------------


def test_align_long_on_cpu_raises(ev_cpu):
    from vits_amd._lib import VitsAmdError

    wav = np.zeros(5000 * HOP, dtype=np.int16)
    text = np.zeros((5, ev_cpu.text_channels), dtype=np.float32)
    emo = torch.zeros(1, 1024)
    with pytest.raises(VitsAmdError):
        ev_cpu.align_long(wav, 1, [text, text], [emo, emo])
    with pytest.raises(VitsAmdError):
        ev_cpu.model.align_segments([torch.zeros(5, ev_cpu.text_channels)], [emo[0]],
                                    torch.zeros(1, 513, 20), 20, 1)


def test_align_long_host_refusals(ev_cpu, monkeypatch):
    """Every length is known on the host: the refusals come before anything is
    uploaded (the device check is lifted for this test only; nothing here gets
    as far as the device)."""
    ev = ev_cpu
    monkeypatch.setattr(ev, "device", torch.device("cuda"))
    emo = torch.zeros(1, 1024)
    c = ev.text_channels

    def text(n):
        return np.zeros((n, c), np.float32)

    wav = np.zeros(5000 * HOP + 5, dtype=np.int16)
    with pytest.raises(ValueError, match="segment 1 is empty"):
        ev.align_long(wav, 1, [text(5), text(0), text(7)], [emo] * 3)
    with pytest.raises(ValueError, match="no text segment"):
        ev.align_long(wav, 1, [], [])
    with pytest.raises(ValueError, match="3 segments need 3 emotions"):
        ev.align_long(wav, 1, [text(5)] * 3, [emo] * 2)
    # 5000 frames, 5001 tokens in 51 segments
    with pytest.raises(ValueError, match="5000 frames cannot be aligned with 5001 tokens"):
        ev.align_long(wav, 1, [text(100)] * 50 + [text(1)], [emo] * 51)
    # 10 000 frames at twice the rate are 5000 at the model's
    with pytest.raises(ValueError, match="5000 frames"):
        ev.align_long(np.zeros(10000 * HOP, dtype=np.int16), 1, [text(2501)] * 2, [emo] * 2,
                      sampling_rate_in=32000)
    with pytest.raises(ValueError):  # at most pad samples
        ev.align_long(np.zeros(416, dtype=np.int16), 1, [text(1)], [emo])
    # one token over the cap, with frames enough
    cap = ev.ALIGN_LONG_MAX_TOKENS
    long_wav = np.zeros((cap + 1) * HOP, dtype=np.int16)
    with pytest.raises(ValueError, match=f"{cap + 1} tokens exceeds"):
        ev.align_long(long_wav, 1, [text(cap // 2), text(cap // 2 + 1)], [emo] * 2)
    # the workspace cap (lowered here: the real one needs a recording of hours)
    monkeypatch.setattr(ev, "ALIGN_LONG_MAX_BYTES", 1 << 20)
    with pytest.raises(ValueError, match="bytes of workspace"):
        ev.align_long(wav, 1, [text(1000)] * 2, [emo] * 2)
    monkeypatch.undo()
    monkeypatch.setattr(ev, "device", torch.device("cuda"))
    for kw in (dict(window_frames=300), dict(window_frames=8192), dict(panel_frames=100),
               dict(panel_frames=0), dict(strip_tokens=96), dict(strip_tokens=4096)):
        with pytest.raises(ValueError):
            ev.align_long(wav, 1, [text(5)], [emo], **kw)


def test_align_long_caps_are_what_the_design_states(ev_cpu):
    """ALIGN_LONG_MAX_BYTES bounds the decision words (frames * tokens / 8)
    plus one panel of scores; DESIGN 4u: ten minutes against 8192 tokens take
    under 200 MB, and at the token cap the byte cap is a recording of more
    than an hour."""
    ev = ev_cpu
    need, strip, panel = ev._align_long_bytes(50000, 8192, 2048, 4096)
    assert (strip, panel) == (2048, 4096)
    assert 50000 * 8192 // 8 + 4 * 4096 * 8192 <= need <= 200 * 10 ** 6
    T = ev.ALIGN_LONG_MAX_TOKENS
    hour = 3600 * 16000 // HOP
    assert ev._align_long_bytes(hour, T, 2048, 4096)[0] <= ev.ALIGN_LONG_MAX_BYTES
    assert ev._align_long_bytes(2 * hour, T, 2048, 4096)[0] > ev.ALIGN_LONG_MAX_BYTES
    # small jobs run at the narrowest strip and one short panel
    assert ev._align_long_bytes(600, 115, 2048, 4096)[1:] == (128, 608)


def test_aligning_still_refuses_segments_and_aligning_long_exists(ev_cpu):
    from vits_amd.vits_wrap import VITSWrap

    class Front:
        max_utt_length = 8

        def __call__(self, uid, text):
            raise AssertionError("the front end must not run for a refused request")

    wrap = VITSWrap(textparser=Front(), speecher=ev_cpu)
    with pytest.raises(ValueError, match="2 segments"):
        wrap.aligning({"wav": np.zeros(4000, dtype=np.int16), "text": "abcdefgh ijkl",
                       "spkid": 1})
    assert callable(wrap.aligning_long)


# -- the segment oracle ---------------------------------------------------------------


def test_segment_oracle_with_one_segment_is_the_golden():
    """One segment: the composition base_align.npz pins, to align_common's
    bars (1e-5 on the latents, neg_cent and scores; the durations exactly)."""
    from common import rel_err

    torch.set_num_threads(8)
    gold = {k: torch.from_numpy(v) for k, v in golden("base_align.npz").items()}
    wav, xs, emos = L.long_inputs(A.GOLDEN_SEED, A.GOLDEN_L, [A.GOLDEN_TX],
                                  BASE_DATA["text_channels"])
    assert torch.equal(wav, gold["wav"]) and torch.equal(xs[0], gold["x"])
    assert torch.equal(emos[0], gold["emo"])
    sd = oracle_sd(base_model("cpu"))
    with torch.no_grad():
        z_p, m_p, logs_p, nc, dur, sc, offs = L.segment_oracle(sd, VC.spectrogram(wav), xs, emos,
                                                               gold["sid"])
        one = A.align_oracle(sd, VC.spectrogram(wav), xs[0], emos[0], gold["sid"])
    assert offs == [0, A.GOLDEN_TX]
    for name, t in (("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p), ("neg_cent", nc),
                    ("scores", sc)):
        assert rel_err(t, gold[name]) <= 1e-5, name
    assert np.array_equal(dur, gold["durations"].numpy())
    for a, b in zip((z_p, m_p, logs_p, nc), one[:4]):
        assert torch.equal(a, b)
    assert np.array_equal(dur, one[4]) and np.array_equal(sc, one[5])


def test_segment_oracle_path_of_the_gpu_comparison_is_stable():
    """600 frames against 40 + 25 + 50 tokens at LONG_SEED: 20 relative
    perturbations of the oracle's neg_cent at each of 1e-6 .. 1e-3 leave its
    path unchanged, so a test may ask for exactly its durations from any
    implementation whose latents are within 1e-4.  The segments' emotion
    vectors differ, and encoding them apart is not encoding them together."""
    torch.set_num_threads(8)
    wav, xs, emos = L.long_inputs(L.LONG_SEED, L.LONG_L, L.LONG_TOKENS,
                                  BASE_DATA["text_channels"])
    sd = oracle_sd(base_model("cpu"))
    with torch.no_grad():
        spec = VC.spectrogram(wav)
        z_p, m_p, logs_p, nc, dur, sc, offs = L.segment_oracle(sd, spec, xs, emos, L.LONG_SID)
        _, m_joint, _, _, _, _ = A.align_oracle(sd, spec, torch.cat(xs, 1), emos[0], L.LONG_SID_T)
    assert z_p.shape[2] == L.LONG_FRAMES and offs == [0, 40, 65, 115]
    assert dur.min() >= 1 and dur.sum() == L.LONG_FRAMES
    changed = L.path_is_stable(nc.numpy())
    print("paths changed of 20:", changed)
    assert not any(changed.values()), changed
    assert not torch.equal(m_joint, m_p)

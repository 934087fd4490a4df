"""Forced alignment of long recordings on the GPU: z_p through overlapping
windows against z_p of the whole recording (BITWISE, and not with too little
context), EmoVITS.align_long against the eager definition
SynthesizerTrn.align_segments (bitwise) and against the segment oracle of
tests/align_long_common.py (the 1e-4 bars of tests/test_align_gpu.py on the
latents, the durations exactly: tests/test_align_long.py shows the oracle's
path stable under perturbations ten times larger), one segment against
EmoVITS.align, the fp16 model behind graphs, and VITSWrap.aligning_long."""
import numpy as np
import pytest
import torch

import align_long_common as L
import vc_common as VC
from common import BASE_DATA, base_model, build_model, oracle_sd, rel_err, tiny_cfg
from test_align_gpu import HOP, REL, STFT, _emovits, _recording, _spec, _text

pytestmark = pytest.mark.gpu

TC = BASE_DATA["text_channels"]


@pytest.fixture(scope="module")
def long_case(device, tmp_path_factory):
    """The fp32 base model behind EmoVITS, the 600-frame recording with its
    three segments, and the eager definition on the exact-length spectrogram:
    computed once, shared, left unchanged."""
    ev = _emovits(device, base_model(device), tmp_path_factory.mktemp("al"), TC, half=False)
    wav, xs, emos = L.long_inputs(L.LONG_SEED, L.LONG_L, L.LONG_TOKENS, TC)
    spec = _spec(wav[0].to(device), device)
    assert spec.shape[2] == L.LONG_FRAMES
    dur, sc, offs, lat = ev.model.align_segments(
        [x[0].to(device) for x in xs], [e[0].to(device) for e in emos], spec, L.LONG_FRAMES,
        L.LONG_SID)
    torch.cuda.synchronize()
    return dict(ev=ev, wav=wav[0].numpy(), xs=xs, emos=emos, spec=spec,
                texts=[x[0].numpy() for x in xs], dur=dur.cpu().numpy(), sc=sc.cpu().numpy(),
                offs=offs, lat=tuple(t.clone() for t in lat))


def _long(case, **kw):
    keep = {}
    out = case["ev"].align_long(case["wav"], L.LONG_SID, case["texts"], case["emos"], _keep=keep,
                                **kw)
    return out, keep


def test_windows_reproduce_the_whole_recording(long_case):
    """600 frames and 57 samples through windows of 256 frames with
    align_context_frames (67) of context: z_p equals z_p of _audio_latents on
    the exact-length spectrogram in every bit.  With 8 frames it does not."""
    ev = long_case["ev"]
    assert ev.model.align_context_frames(STFT) == 67
    z_whole = long_case["lat"][0]
    assert tuple(z_whole.shape) == (1, 192, L.LONG_FRAMES)
    (_, _, _, frames), keep = _long(long_case, window_frames=256)
    assert frames == L.LONG_FRAMES and ("latents", 8, 256) in ev._graphs
    assert torch.equal(keep["z_p"], z_whole)
    _, keep8 = _long(long_case, window_frames=256, _context=8)
    assert keep8["z_p"].shape == z_whole.shape and not torch.equal(keep8["z_p"], z_whole)
    # the recording as ONE window (600 <= 1024): the same bits again
    _, keep1 = _long(long_case, window_frames=1024)
    assert ("latents", 1, 1024) in ev._graphs and torch.equal(keep1["z_p"], z_whole)


def test_align_long_equals_align_segments_and_the_oracle(long_case):
    (durs, scs, seg_frames, frames), keep = _long(long_case, window_frames=256, panel_frames=96,
                                                  strip_tokens=64)
    assert [d.shape[0] for d in durs] == list(L.LONG_TOKENS)
    assert all(d.dtype == np.int32 for d in durs) and all(s.dtype == np.float32 for s in scs)
    d, s = np.concatenate(durs), np.concatenate(scs)
    # the eager definition, bit for bit
    assert long_case["offs"] == [0, 40, 65, 115]
    for got, want in zip((keep["z_p"], keep["m_p"], keep["logs_p"]), long_case["lat"]):
        assert torch.equal(got, want)
    assert np.array_equal(d, long_case["dur"]) and np.array_equal(s, long_case["sc"])
    assert d.min() >= 1 and d.sum() == frames == L.LONG_FRAMES
    assert seg_frames.dtype == np.int64
    assert seg_frames.tolist() == [0] + np.cumsum(d)[[39, 64, 114]].tolist()
    # the defaults (one strip of 128, one panel) give the same
    (durs2, scs2, _, _), _ = _long(long_case, window_frames=256)
    assert np.array_equal(np.concatenate(durs2), d) and np.array_equal(np.concatenate(scs2), s)
    # the segment oracle on the CPU
    sd = oracle_sd(base_model("cpu"))  # (the same deterministic fill, with weight norm)
    with torch.no_grad():
        z_p, m_p, logs_p, nc, odur, osc, _ = L.segment_oracle(
            sd, VC.spectrogram(torch.from_numpy(long_case["wav"])[None]), long_case["xs"],
            long_case["emos"], L.LONG_SID)
    for name, got, want in (("z_p", keep["z_p"], z_p), ("m_p", keep["m_p"], m_p),
                            ("logs_p", keep["logs_p"], logs_p), ("scores", s, osc)):
        err = rel_err(got, want)
        print(f"align_long {name}: rel_err {err:.2e}")
        assert err < REL, name
    assert np.array_equal(d, odur)


def test_one_segment_equals_align(long_case):
    ev = long_case["ev"]
    text, emo = long_case["texts"][0], long_case["emos"][0]
    want = ev.align(long_case["wav"], L.LONG_SID, text, emo)
    durs, scs, seg_frames, frames = ev.align_long(long_case["wav"], L.LONG_SID, [text], [emo])
    assert frames == want[2] == L.LONG_FRAMES and seg_frames.tolist() == [0, L.LONG_FRAMES]
    assert np.array_equal(durs[0], want[0]) and np.array_equal(scs[0], want[1])
    durs, scs, _, _ = ev.align_long(long_case["wav"], L.LONG_SID, [text], [emo], window_frames=256,
                                    panel_frames=32, strip_tokens=64)
    assert np.array_equal(durs[0], want[0]) and np.array_equal(scs[0], want[1])


def _same(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
            and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
            and np.array_equal(a[2], b[2]) and a[3] == b[3])


def test_fp16_tiny_model_behind_graphs_and_the_wrapper(device, tmp_path):
    """The precision EmoVITS holds: windows of 256 against one window of 4096,
    graph on against off, an input at twice the rate against resampling
    first, all bitwise; then VITSWrap.aligning_long with a stub front end."""
    from vits_amd import ops, vits_wrap

    c = tiny_cfg()
    tc = c["data"]["text_channels"]
    model = build_model(c["model"], dict(c["data"], spec_channels=STFT[0] // 2 + 1), device)
    ev = _emovits(device, model, tmp_path, tc)
    assert ev.dtype == torch.float16
    n = 700 * HOP + 101
    rec = _recording(n, 3)
    segs = [_text(t, tc, 70 + i) for i, t in enumerate((33, 9, 40, 21))]
    texts, emos = [t for t, _ in segs], [e for _, e in segs]
    a = ev.align_long(rec, 2, texts, emos, window_frames=256)
    assert ("latents", 8, 256) in ev._graphs or ("latents", 4, 256) in ev._graphs
    b = ev.align_long(rec, 2, texts, emos)  # one window of 4096
    assert ("latents", 1, 4096) in ev._graphs
    assert a[3] == 700 and sum(d.sum() for d in a[0]) == 700 and min(d.min() for d in a[0]) >= 1
    assert _same(a, b)
    assert _same(a, ev.align_long(rec, 2, texts, emos, window_frames=256, panel_frames=64,
                                  strip_tokens=64))
    ev.graph = False
    assert _same(a, ev.align_long(rec, 2, texts, emos, window_frames=256))
    ev.graph = True
    # twice the rate in == resampling first
    rec2 = _recording(2 * n, 9)
    r = ev.align_long(rec2, 2, texts, emos, sampling_rate_in=32000, window_frames=256)
    xr = torch.from_numpy(rec2.astype(np.float32) / 32768.0).to(device)
    up, down = ops.resample_ratio(32000, 16000)
    r2 = ev.align_long(ops.resample_poly(xr, up, down).cpu().numpy(), 2, texts, emos,
                       window_frames=256)
    assert r[3] == 700 and _same(r, r2)
    # a posterior draw: one for the whole recording, from the object's generator
    ev.align_long(rec, 2, texts, emos, window_frames=256, noise_scale=0.5)
    assert ev._vc_gen is not None
    with pytest.raises(ValueError):
        ev.align_long(_recording(60 * HOP, 1), 2, texts, emos)  # 60 frames, 103 tokens

    # the wrapper, with a stub front end: one vector per character
    class Front:
        max_utt_length = 16

        def __call__(self, uid, txt):
            g = torch.Generator().manual_seed(len(txt))
            return uid, txt, torch.randn(len(txt), tc, generator=g).numpy()

    wrap = vits_wrap.VITSWrap(textparser=Front(), speecher=ev)
    text = "abcdefghij klmno, pqrstuvwxyz abcdefg hijk. lmnopqrs"
    emo = emos[0]
    res = wrap.aligning_long({"wav": rec, "text": text, "spkid": 2, "emotion": emo, "id": "u1"})
    ids, parts = wrap._split_utt_text("u1", text)
    assert len(parts) >= 3 and "".join(parts) == text
    want = ev.align_long(rec, 2, [Front()(i, p)[2] for i, p in zip(ids, parts)],
                         [emo] * len(parts))
    sec = HOP / 16000
    assert res["id"] == "u1" and res["frames"] == 700 and res["segtext"] == parts
    assert np.array_equal(res["durations"], np.concatenate(want[0]))
    assert np.array_equal(res["scores"], np.concatenate(want[1]))
    bounds = res["boundaries_s"]
    assert bounds.shape == (len(text) + 1,) and bounds[0] == 0.0
    assert np.array_equal(bounds, np.concatenate([[0], np.cumsum(res["durations"])]) * sec)
    segs_out = res["segments"]
    assert [s["text"] for s in segs_out] == parts
    tok = 0
    for i, s in enumerate(segs_out):
        # the cut points are token boundaries, monotone, and tile the recording
        assert s["start_s"] == bounds[tok] and s["start_s"] < s["end_s"]
        tok += len(parts[i])
        assert s["end_s"] == bounds[tok]
        assert np.array_equal(s["durations"], want[0][i]) and np.array_equal(s["scores"], want[1][i])
        if i:
            assert s["start_s"] == segs_out[i - 1]["end_s"]
    assert segs_out[0]["start_s"] == 0.0
    assert segs_out[-1]["end_s"] == pytest.approx(700 * HOP / 16000, rel=1e-12)
    assert res["time_used_backend"] > 0 and res["rtf"] > 0 and res["time_used_frontend"] >= 0
    with pytest.raises(ValueError):  # aligning itself still takes one segment
        wrap.aligning({"wav": rec, "text": text, "spkid": 2, "emotion": emo})

"""Voice conversion of long recordings on the GPU: vits_copy_windows against
torch slicing, the windows of EmoVITS._long_plan through convert_bucketed
rows and the scatter against the definition (SynthesizerTrn.voice_conversion
of the WHOLE recording on its exact-length spectrogram), BITWISE, and the
serving entry points convert_long / convert_pcm_long / VITSWrap.converting.

Shapes.  At the base config the context is 113 frames, so windows of 256
frames have cores of Cf = 30.  The recordings of F = 2 * Cf + 7 (plus 57
samples), Cf + 1, 2 * Cf and 200 frames are cut into 3, 2, 2 and 7 windows,
but the rows of the first three still reach both true ends (F <= 113) and
those of the fourth at least one: they check the gather, the remainder, the
scatter and rows cut on one side.  A row with an
artificial edge on BOTH sides needs a = w * Cf - 113 > 0 and b = (w + 1) * Cf
+ 113 < F, so F = 9 * Cf + 7 = 277 frames (plus 57 samples) runs too: ten
windows, rows 0 .. 3 cut on the right, row 4 on both sides, rows 5 .. 9 on
the left.  That recording is also the one of the sensitivity test (at 67
frames a context of 8 gives one whole window, which cannot differ)."""
import numpy as np
import pytest
import torch

from common import base_model, build_model, tiny_cfg

pytestmark = pytest.mark.gpu

N_FFT, HOP, WIN = 1024, 192, 768
PAD = (N_FFT - HOP) // 2
WF = 256


# -- the kernel -------------------------------------------------------------------


def _bits(t):
    return t.cpu().view(torch.int32)


def _copy_ref(src, dst, jobs, channels=1, src_rstride=0, dst_rstride=0):
    """torch slicing on the host: what copy_windows must leave in dst."""
    src, dst = src.cpu().reshape(-1), dst.cpu().reshape(-1).clone()
    for so, do, n, fill in jobs:
        for r in range(channels):
            s, d = so + r * src_rstride, do + r * dst_rstride
            dst[d:d + n] = src[s:s + n]
            dst[d + n:d + fill] = 0
    return dst


def _check_copy(device, jobs, n_src, n_dst, **kw):
    from vits_amd import ops

    g = torch.Generator().manual_seed(len(jobs) + n_src)
    src = torch.randn(n_src, generator=g).to(device)
    dst = torch.full((n_dst,), float("nan"), device=device)
    want = _copy_ref(src, dst, jobs, **kw)
    ops.copy_windows(src, dst, jobs, **kw)
    torch.cuda.synchronize()
    # bit patterns: NaN where nothing may be written, the source's bits or +0 elsewhere
    assert torch.equal(_bits(dst), _bits(want))
    written = sum(j[3] for j in jobs) * kw.get("channels", 1)
    assert int(torch.isnan(dst).sum()) == n_dst - written


def test_copy_windows_offsets_lengths_and_fill(device):
    """R = 1: offsets co-aligned on a 16-byte boundary, co-aligned off it
    (head and tail element by element), not co-aligned (single elements);
    lengths of 0, 1, 3, less than a vector, one tile (1024) exactly, several
    tiles and a bit; fill_len == len, fill_len > len within a vector and
    across tiles, len = 0 with a fill."""
    jobs, d = [], 3
    for so, align in ((0, 0), (4, 0), (5, 1), (7, 3), (2, 0), (9, 2), (1, 1)):
        for n, fill in ((0, 0), (1, 1), (3, 9), (0, 5), (1024, 1024), (1021, 1030), (3000, 3000),
                        (2055, 4101), (0, 2049)):
            d += (align - d) % 4  # dst offset = align modulo 4
            jobs.append((so + 12 * len(jobs), d, n, fill))  # (src offset = so modulo 4)
            d += fill + 1 + len(jobs) % 3  # a NaN gap between the ranges
    assert len(jobs) == 63
    _check_copy(device, jobs, 4096, d + 8)


def test_copy_windows_channels_and_strides(device):
    """R = 5: a channel stride that keeps the alignment (a multiple of 4) on
    one side and one that changes it per channel (1003) on the other, both
    ways round, so co-aligned and single-element channels share a job."""
    jobs = [(0, 0, 700, 700), (4, 704, 1500, 1800), (33, 2511, 0, 40), (1, 2556, 1027, 1027)]
    _check_copy(device, jobs, 5 * 1003 + 1600, 5 * 4096, channels=5, src_rstride=1003,
                dst_rstride=4096)
    _check_copy(device, jobs, 5 * 2048, 5 * 3601 + 8, channels=5, src_rstride=2048 - 1600,
                dst_rstride=3601)


def test_copy_windows_64_jobs_one_launch_and_more(device):
    from vits_amd import ops

    jobs = [(17 * j, 300 * j + j % 4, 100 + j, 200 + j) for j in range(64)]
    _check_copy(device, jobs, 17 * 64 + 200, 300 * 64 + 300)
    # 70 jobs: the wrapper launches twice, the C entry point alone refuses
    jobs += [(j, 300 * (64 + j), 50, 60) for j in range(6)]
    _check_copy(device, jobs, 17 * 64 + 200, 300 * 70 + 100)
    # a job that leaves a tensor is refused, nothing is written
    src, dst = torch.zeros(100, device=device), torch.zeros(100, device=device)
    with pytest.raises(ops._lib.VitsAmdError):
        ops.copy_windows(src, dst, [(0, 0, 10, 10), (95, 0, 10, 10)])
    with pytest.raises(ops._lib.VitsAmdError):
        ops.copy_windows(src, dst, [(0, 95, 4, 10)])
    with pytest.raises(ops._lib.VitsAmdError):
        ops.copy_windows(src.half(), dst, [(0, 0, 4, 4)])


# -- model level: the plan against the definition, bitwise -----------------------


def _emovits(device, model, tmp_path, **kw):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "filter_length": N_FFT, "hop_length": HOP,
                 "win_length": WIN, "text_channels": 256,
                 "n_speakers": model.emb_g.num_embeddings, "noise_scale": 0.667},
        "model": {"inter_channels": model.inter_channels}})
    return EmoVITS(str(tmp_path / "ckpt.pth"), device, hps=hps, model=model, **kw)


def _float_recording(n, seed, device):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.25).clamp(-1, 1).to(device)


def _recording(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.25).clamp(-1, 1).mul(32767).to(torch.int16).numpy()


def _definition(model, x, src, tgt, noise=None):
    """voice_conversion of the whole recording x [n] (fp32, device) on its
    exact-length spectrogram: fp32 [(n // hop) * hop]."""
    from vits_amd import ops

    dev = x.device
    window = torch.hann_window(WIN, device=dev)
    spec = ops.stft_mag(x.view(1, -1).contiguous(), window, N_FFT, HOP, WIN, pad=PAD, eps=1e-6)
    F = x.numel() // HOP
    assert spec.shape[2] == F
    o, _, _ = model.voice_conversion(
        spec, torch.tensor([F], device=dev), torch.tensor([src], device=dev),
        torch.tensor([tgt], device=dev), None if noise is None else noise[None, :, :F].contiguous())
    assert tuple(o.shape) == (1, 1, F * HOP) and o.dtype == torch.float32
    return o[0, 0]


def _same(out, ref, what=""):
    """Bitwise equality of two waveforms; prints where they differ first."""
    out, ref = torch.as_tensor(out).cpu(), torch.as_tensor(ref).cpu()
    if out.shape != ref.shape:
        return False
    bad = torch.nonzero(out != ref).flatten()
    if bad.numel():
        print(f"{what}: {bad.numel()} of {ref.numel()} samples differ, frames "
              f"{int(bad[0]) // HOP} .. {int(bad[-1]) // HOP}, max "
              f"{(out - ref).abs().max().item():.3e}")
    return bad.numel() == 0


@pytest.fixture(scope="module")
def ev_base(device, tmp_path_factory):
    """The base config in fp32, eager: rows through convert_bucketed."""
    return _emovits(device, base_model(device), tmp_path_factory.mktemp("vcl"), half=False,
                    graph=False)


SRC, TGT = 7, 1500
_REFS = {}


def _base_case(ev, device, F, rem, with_noise):
    """(recording, noise or None, definition), computed once per case."""
    key = (F, rem, with_noise)
    if key not in _REFS:
        x = _float_recording(F * HOP + rem, 100 + F, device)
        noise = None
        if with_noise:
            g = torch.Generator().manual_seed(F)
            noise = (torch.randn(ev.inter_channels, F, generator=g) * 0.667).to(device)
        _REFS[key] = (x, noise, _definition(ev.model, x, SRC, TGT, noise))
    return _REFS[key]


CF = WF - 2 * 113
CASES = [(2 * CF + 7, 57, 3), (CF + 1, 0, 2), (2 * CF, 0, 2), (200, 0, 7), (9 * CF + 7, 57, 10)]


@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "mean"])
@pytest.mark.parametrize("F,rem,n_windows", CASES, ids=[f"F{c[0]}" for c in CASES])
def test_windows_equal_whole_recording_bitwise(ev_base, device, F, rem, n_windows, with_noise):
    ctx = ev_base.model.vc_context_frames((N_FFT, HOP, WIN))
    assert ctx == 113 and WF - 2 * ctx == CF
    x, noise, ref = _base_case(ev_base, device, F, rem, with_noise)
    plan = ev_base._long_plan(x.numel(), WF, ctx)
    assert len(plan) == n_windows
    kinds = [(w.a > 0, w.b < F) for w in plan]  # (cut on the left, cut on the right)
    if n_windows == 10:
        assert kinds == [(False, True)] * 4 + [(True, True)] + [(True, False)] * 5
    elif F <= ctx:
        assert kinds == [(False, False)] * n_windows
    else:  # 200 frames: every row reaches one true end
        assert (True, True) not in kinds and (False, True) in kinds and (True, False) in kinds
    out = ev_base._run_windows(x, plan, WF, SRC, TGT, noise)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, F * HOP)
    assert ref.abs().max().item() > 1e-3  # not silent
    assert _same(out[0], ref, f"F {F}")


def test_convert_long_equals_definition_and_needs_its_context(ev_base, device):
    """convert_long itself at the ten-window recording (posterior mean), and
    the sensitivity of the comparison: the same recording with 8 frames of
    context instead of 113 (two windows, cut at frames 248 and 232) must NOT
    reproduce the definition."""
    F, rem = 9 * CF + 7, 57
    x, _, ref = _base_case(ev_base, device, F, rem, False)
    rec = x.cpu().numpy()
    out = ev_base.convert_long(rec, SRC, TGT, window_frames=WF)
    assert out.dtype == np.float32 and out.shape == (F * HOP,)
    assert _same(out, ref, "convert_long")
    short = ev_base.convert_long(rec, SRC, TGT, window_frames=WF, _context=8)
    assert len(ev_base._long_plan(x.numel(), WF, 8)) == 2
    assert short.shape == out.shape and np.isfinite(short).all()
    assert not np.array_equal(short, out)
    # ... and it differs around the cut only: the first rows' cores are the true start's
    assert np.array_equal(short[:100 * HOP], out[:100 * HOP])
    # one posterior draw for the whole recording, from the object's generator
    ev_base._vc_gen = torch.Generator(device=device).manual_seed(5)
    drawn = ev_base.convert_long(rec, SRC, TGT, window_frames=WF, noise_scale=0.667)
    g = torch.Generator(device=device).manual_seed(5)
    noise = torch.randn(ev_base.inter_channels, F, device=device, generator=g) * 0.667
    assert np.array_equal(drawn, _definition(ev_base.model, x, SRC, TGT, noise).cpu().numpy())
    assert not np.array_equal(drawn, out)
    with pytest.raises(ValueError):
        ev_base.convert_long(rec, SRC, TGT, window_frames=300)  # not a bucket


# -- serving: the fp16 model EmoVITS holds, graphs ------------------------------


@pytest.fixture(scope="module")
def ev_tiny(device, tmp_path_factory):
    c = tiny_cfg()
    model = build_model(c["model"], dict(c["data"], spec_channels=N_FFT // 2 + 1), device)
    return _emovits(device, model, tmp_path_factory.mktemp("vcl_tiny"), graph=True)


def test_serving_equals_convert_below_the_cap(ev_tiny, device):
    from vits_amd import ops

    ev = ev_tiny
    assert ev.model.vc_context_frames((N_FFT, HOP, WIN)) == 85  # cores of 86 frames
    rec = _recording(600 * HOP + 11, 3)
    whole = ev.convert(rec, 1, 2)
    assert whole.shape == (600 * HOP,) and np.abs(whole).max() > 1e-4
    out = ev.convert_long(rec, 1, 2, window_frames=WF)
    assert out.dtype == np.float32 and np.array_equal(out, whole)
    # seven windows: one replay of the batch-8 graph of ordinary conversions
    assert ("vc", 8, WF) in ev._graphs and ("vc", 1, 1024) in ev._graphs
    # ... and with the default window, one row: the graph convert uses for 4096 frames
    assert np.array_equal(ev.convert_long(rec, 1, 2), whole)
    assert ("vc", 1, 4096) in ev._graphs
    ctl = dict(pitch=1.1, sampling_rate=22050, volume=0.8, tail_silence=0.02)
    pcm, n = ev.convert_pcm(rec, 1, 2, **ctl)
    pcm_l, n_l = ev.convert_pcm_long(rec, 1, 2, window_frames=WF, **ctl)
    assert n_l == n == 600 * HOP and pcm_l.dtype == np.int16 and np.abs(pcm_l).max() > 0
    assert np.array_equal(pcm_l, pcm)
    # eager: the same bytes
    ev.graph = False
    try:
        assert np.array_equal(ev.convert_long(rec, 1, 2, window_frames=WF), whole)
        assert np.array_equal(ev.convert_pcm_long(rec, 1, 2, window_frames=WF, **ctl)[0], pcm)
    finally:
        ev.graph = True
    # input at twice the model's rate == resampling first
    rec2 = _recording(2 * (300 * HOP + 7), 9)
    a = ev.convert_long(rec2, 1, 2, sampling_rate_in=32000, window_frames=WF)
    x = torch.from_numpy(rec2.astype(np.float32) / 32768.0).to(device)
    up, down = ops.resample_ratio(32000, 16000)
    b = ev.convert_long(ops.resample_poly(x, up, down).cpu().numpy(), 1, 2, window_frames=WF)
    assert a.shape == (300 * HOP,) and np.array_equal(a, b)


def test_past_the_cap(ev_tiny, device):
    from vits_amd import vits_wrap

    ev = ev_tiny
    F = 4096 + 300
    rec = _recording(F * HOP + 11, 4)
    with pytest.raises(ValueError):
        ev.convert(rec, 1, 2)
    out = ev.convert_long(rec, 1, 2)  # two windows of 4096 frames
    assert ("vc", 2, 4096) in ev._graphs
    assert out.dtype == np.float32 and out.shape == (F * HOP,) and np.isfinite(out).all()
    assert np.abs(out).max() > 1e-4
    small = ev.convert_long(rec, 1, 2, window_frames=WF)  # 52 windows: 16 + 16 + 16 + 4
    assert ("vc", 16, WF) in ev._graphs and ("vc", 4, WF) in ev._graphs
    assert _same(small, out, "windows of 256 against windows of 4096")
    x = torch.from_numpy(rec.astype(np.float32) / 32768.0).to(device)
    ref = _definition(ev.model, x, 1, 2)
    assert _same(out, ref, "windows of 4096 against the definition")
    # the wrapper takes the long path above the cap, with the same response
    ctl = dict(volume=0.8, tail_silence=0.01)
    pcm, n = ev.convert_pcm_long(rec, 1, 2, **ctl)
    assert n == F * HOP and len(pcm) == n + 160
    assert np.array_equal(pcm, vits_wrap.host_pcm(out, 16000, 1.0, 16000, 0.8, 0.01))
    wrap = vits_wrap.VITSWrap(textparser=lambda uid, text: (uid, text, None), speecher=ev,
                              device_post=True)
    res = wrap.converting({"wav": rec, "spkid_src": 1, "spkid_tgt": 2, "id": "long", **ctl})
    assert res["wav"][:4] == b"RIFF" and res["sr"] == 16000 and res["id"] == "long"
    assert res["wav"][44:] == pcm.tobytes()
    assert res["rtf"] > 0 and len(res["segment_info"]) == 1

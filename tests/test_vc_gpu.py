"""Voice conversion on the GPU: the ragged magnitude STFT
(vits_stft_mag_forward_rows, both forwards), the forward flow, the eager
definition SynthesizerTrn.voice_conversion against the reference's golden, the
host-sync-free bucketed path and its graph against that definition (BITWISE,
the contract of tests/test_infer_bucketed_gpu.py), and the serving entry
points of EmoVITS.

Tolerances are the project's own: TOL = 2e-5 per STFT frame
(tests/test_stft_edges_gpu.py), REL = 1e-4 and SNR_DB = 60
(tests/test_models_gpu.py; the reference's own fp32-vs-fp64 noise is 8e-7 /
120 dB)."""
import numpy as np
import pytest
import torch

import vc_common as VC
from common import base_model, build_model, golden, oracle_sd, rel_err, snr_db, tiny_cfg

pytestmark = pytest.mark.gpu

TOL = 2e-5
REL = 1e-4
SNR_DB = 60.0
# fp16 model vs the fp32 model of the same weights, see
# test_fp16_convert_graph_equals_eager_and_snr
FP16_SNR_DB = 45.0
STFT = (VC.STFT["n_fft"], VC.STFT["hop"], VC.STFT["win"])
HOP = VC.STFT["hop"]


@pytest.fixture(scope="module")
def base(device):
    return base_model(device)


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in golden("base_vc.npz").items()}


def _frame_err(mag, ref):
    """max over frames of max_k |mag - ref| / max_k ref ([bins, frames])."""
    err = (mag.double() - ref).abs().amax(0)
    return (err / ref.amax(0)).max().item()


def _ragged_stft(device, n_fft, hop, win, pad, lens, cap, frames_cap, want, eps):
    from vits_amd import ops

    B = len(lens)
    g = torch.Generator().manual_seed(n_fft + cap)
    x = (torch.randn(B, cap, generator=g) * 0.5).clamp(-1, 1)
    for b, L in enumerate(lens):
        x[b, L:] = float("nan")  # never read into a frame
    xd = x.to(device)
    window = torch.hann_window(win, device=device)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=device)
    mag, frames = ops.stft_mag_rows(xd, lens_d, window, n_fft, hop, win, frames_cap, pad=pad,
                                    eps=eps)
    torch.cuda.synchronize()
    assert tuple(mag.shape) == (B, n_fft // 2 + 1, frames_cap)
    assert frames.tolist() == want
    assert want == [ops.stft_rows_frames(L, n_fft, hop, pad, frames_cap, cap) for L in lens]
    for b, (L, f) in enumerate(zip(lens, want)):
        # dead columns: exactly 0 (not NaN from the tail, not stale memory)
        assert torch.count_nonzero(mag[b, :, f:]).item() == 0, b
        assert torch.isfinite(mag[b]).all(), b
        if f == 0:
            continue
        alone = ops.stft_mag(xd[b:b + 1, :L].contiguous(), window, n_fft, hop, win, pad=pad,
                             eps=eps)
        assert alone.shape[2] >= f
        assert torch.equal(mag[b, :, :f], alone[0, :, :f]), b
        ref = VC.stft_mag_ref(x[b, :L], n_fft, hop, win, pad, eps)
        err = _frame_err(mag[b, :, :f].cpu(), ref[:, :f])
        print(f"ragged stft n_fft {n_fft} row {b} (L {L}, {f} frames): per-frame err {err:.3e}")
        assert err <= TOL, (b, err)


def test_ragged_stft_spectrogram_config(device):
    """The two-pass register FFT at 1024/192/768/416: a full row, a ragged
    one, pad + 1 samples (both reflections in a frame) and pad samples (no
    frame)."""
    cap = 12 * 192 + 191
    _ragged_stft(device, 1024, 192, 768, 416, [cap, 7 * 192 + 57, 417, 416], cap, 12,
                 [12, 7, 2, 0], 1e-6)


def test_ragged_stft_stockham(device):
    """The Stockham LDS FFT (n_fft 64): 16 frames per workgroup, so the
    20-frame bucket has a partial second block."""
    _ragged_stft(device, 64, 16, 64, 24, [20 * 16, 9 * 16 + 5, 25], 20 * 16, 20, [20, 9, 1], 1e-7)


def test_posterior_sample_masks_and_stage_lengths(device):
    from vits_amd import ops

    B, C, T = 3, 5, 300
    g = torch.Generator().manual_seed(3)
    ms = torch.randn(B, 2 * C, T, generator=g).to(device)
    noise = torch.randn(B, C, T, generator=g).to(device)
    lens = torch.tensor([300, 257, 0], dtype=torch.int32, device=device)
    m, s = ms[:, :C], ms[:, C:]
    z, sl = ops.posterior_sample(m, s, noise, lens, noise_scale=0.5, stage_mult=(1, 1, 8, 48))
    mask = (torch.arange(T, device=device)[None, None, :] < lens[:, None, None])
    want = torch.where(mask, m.double() + noise.double() * s.double() * 0.5, 0.0)
    assert rel_err(z, want) < 1e-6
    assert torch.count_nonzero(z[1, :, 257:]).item() == 0 and torch.count_nonzero(z[2]).item() == 0
    assert sl.tolist() == [[300, 257, 0], [300, 257, 0], [2400, 2056, 0], [14400, 12336, 0]]
    zm = ops.posterior_sample(m, s, None, lens)
    assert torch.equal(zm, torch.where(mask, m, torch.zeros_like(m)))


def test_flow_infer_forward_direction(base, device):
    """flow.infer(reverse=False) is the forward flow of training (mask of
    ones), and the reverse flow with the same g undoes it."""
    sd = oracle_sd(base)
    g = torch.Generator().manual_seed(11)
    z = torch.randn(2, 192, 40, generator=g)
    gg = torch.randn(2, 1024, generator=g) * 0.5
    with torch.no_grad():
        ref = VC.flow_forward(sd, z, gg)
        out = base.flow.infer(z.to(device), gg.to(device), reverse=False)
        back = base.flow.infer(out, gg.to(device), reverse=True)
    torch.cuda.synchronize()
    err, rt = rel_err(out, ref), rel_err(back, z)
    print(f"flow forward: rel_err {err:.2e}, round trip {rt:.2e}")
    assert err < REL
    assert rt < REL
    assert rel_err(out, z) > 1e-2  # (it does something)


def test_voice_conversion_matches_reference_golden(base, gold, device):
    from vits_amd import ops

    wav = gold["wav"].to(device)
    window = torch.hann_window(STFT[2], device=device)
    spec = ops.stft_mag(wav, window, STFT[0], HOP, STFT[2], pad=VC.PAD, eps=1e-6)
    assert _frame_err(spec[0].cpu(), gold["spec"][0].double()) <= TOL
    src, tgt = gold["sid_src"].to(device), gold["sid_tgt"].to(device)
    yl = torch.tensor([spec.shape[2]], device=device)
    noise = gold["noise"].to(device)
    o, y_mask, (z, z_p, z_hat) = base.voice_conversion(spec, yl, src, tgt, noise)
    torch.cuda.synchronize()
    assert tuple(o.shape) == (1, 1, 24 * HOP) and tuple(y_mask.shape) == (1, 1, 24)
    for name, t in (("z", z), ("z_p", z_p), ("z_hat", z_hat), ("o", o)):
        err = rel_err(t, gold[name])
        print(f"voice_conversion {name}: rel_err {err:.2e}")
        assert err < REL, name
    snr = snr_db(o, gold["o"])
    print(f"voice_conversion o: snr {snr:.1f} dB")
    assert snr >= SNR_DB
    # the same speaker on both sides: the two flows cancel
    _, _, (z2, _, z_hat2) = base.voice_conversion(spec, yl, src, src, noise)
    assert rel_err(z_hat2, z2) < REL
    assert rel_err(z_hat, z) > 1e-2
    # no noise: the posterior mean, and masking at a shorter length
    o_m, mask2, (z_m, _, _) = base.voice_conversion(spec, torch.tensor([20], device=device), src,
                                                    tgt)
    assert torch.count_nonzero(z_m[:, :, 20:]).item() == 0 and mask2.sum().item() == 20
    assert torch.count_nonzero(o_m[:, :, 20 * HOP:]).item() == 0


def _vc_inputs(device, t_y, ns, seed):
    B = len(ns)
    g = torch.Generator().manual_seed(seed)
    wav = (torch.randn(B, t_y * HOP + HOP - 1, generator=g) * 0.3).clamp(-1, 1)
    for b, n in enumerate(ns):
        wav[b, n:] = float("nan")  # (what a bucket holds past a row's end is never read)
    noise = torch.randn(B, 192, t_y, generator=g) * 0.667
    src = torch.randint(0, 2048, (B,), generator=g)
    tgt = torch.randint(0, 2048, (B,), generator=g)
    n_t = torch.tensor(ns, dtype=torch.int32)
    return tuple(t.to(device) for t in (wav, n_t, src, tgt, noise))


def _row_alone(model, wav, n, src, tgt, noise, device):
    """voice_conversion of one row on its own exact-length spectrogram."""
    from vits_amd import ops

    window = torch.hann_window(STFT[2], device=device)
    spec = ops.stft_mag(wav[:n].view(1, -1).contiguous(), window, STFT[0], HOP, STFT[2],
                        pad=VC.PAD, eps=1e-6)
    f = spec.shape[2]
    o, _, _ = model.voice_conversion(spec, torch.tensor([f], device=device), src.view(1),
                                     tgt.view(1), None if noise is None else noise[None, :, :f])
    return o, f


def test_convert_bucketed_bitwise_equals_voice_conversion(base, device):
    t_y, ns = 32, [24 * HOP + 57, 13 * HOP + 1]
    wav, n_t, src, tgt, noise = _vc_inputs(device, t_y, ns, 21)
    out, y_len = base.convert_bucketed(wav, n_t, src, tgt, noise, t_y, stft=STFT)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 1, t_y * HOP) and out.dtype == torch.float32
    assert y_len.tolist() == [24, 13] == [n // HOP for n in ns]
    for b, n in enumerate(ns):
        ref, f = _row_alone(base, wav[b], n, src[b], tgt[b], noise[b], device)
        assert f == y_len[b].item()
        assert torch.equal(out[b:b + 1, :, :f * HOP], ref), b
        assert ref.abs().max().item() > 1e-3
        # past the row's end (the TTS path leaves its bucket unspecified there;
        # this one cuts it): zero, in particular past y_len * hop + 64 * hop
        assert torch.count_nonzero(out[b, :, f * HOP:]).item() == 0, b
    # the posterior mean: noise None
    out_m, _ = base.convert_bucketed(wav, n_t, src, tgt, None, t_y, stft=STFT)
    ref_m, f = _row_alone(base, wav[1], ns[1], src[1], tgt[1], None, device)
    assert torch.equal(out_m[1:2, :, :f * HOP], ref_m)
    assert not torch.equal(out_m, out)


def test_convert_graph_replay(base, device):
    t_y = 32
    run = base.capture_convert_bucketed(t_y, batch=2, stft=STFT)
    for seed, ns in ((5, [24 * HOP + 57, 13 * HOP + 1]), (6, [9 * HOP + 100, 31 * HOP + 191])):
        wav, n_t, src, tgt, noise = _vc_inputs(device, t_y, ns, seed)
        ref, ref_len = base.convert_bucketed(wav, n_t, src, tgt, noise, t_y, stft=STFT)
        out, y_len = run(wav, ns, src, tgt, noise)
        torch.cuda.synchronize()
        assert y_len.tolist() == ref_len.tolist() == [n // HOP for n in ns]
        assert torch.equal(out, ref), seed
    # one row into the batch-2 graph, no noise: row 1 has length 0 and is silent
    wav, n_t, src, tgt, _ = _vc_inputs(device, t_y, [17 * HOP + 3], 7)
    out, y_len = run(wav, [17 * HOP + 3], src, tgt)
    torch.cuda.synchronize()
    assert y_len.tolist() == [17, 0]
    ref, _ = base.convert_bucketed(wav, n_t, src, tgt, None, t_y, stft=STFT)
    assert torch.equal(out[:1], ref)
    assert torch.count_nonzero(out[1]).item() == 0


def _emovits(device, model, tmp_path, sr=16000):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    hps = get_hparams_from_dict({
        "data": {"sampling_rate": sr, "filter_length": STFT[0], "hop_length": HOP,
                 "win_length": STFT[2], "text_channels": 256, "n_speakers": 2048,
                 "noise_scale": 0.667},
        "model": {"inter_channels": model.inter_channels}})
    hps.data["n_speakers"] = model.emb_g.num_embeddings
    return EmoVITS(str(tmp_path / "ckpt.pth"), device, hps=hps, model=model, graph=True)


def _recording(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.25).clamp(-1, 1).mul(32767).to(torch.int16).numpy()


def test_emovits_convert_pcm_and_batch(device, tmp_path):
    from vits_amd import ops, vits_wrap

    c = tiny_cfg()
    model = build_model(c["model"], dict(c["data"], spec_channels=STFT[0] // 2 + 1), device)
    ev = _emovits(device, model, tmp_path)
    recs = [_recording(n, i) for i, n in enumerate((30 * HOP + 11, 12 * HOP + 190, 3 * HOP))]
    items = [(recs[0], 1, 2), (recs[1], 3, 0), (recs[2], 2, 1)]
    ctl = dict(pitch=1.1, sampling_rate=22050, volume=0.8, tail_silence=0.02)
    # batch == loop, byte for byte
    pcm, offsets, n_model = ev.convert_pcm_batch(items, **ctl)
    assert ("vc", 4, 256) in ev._graphs
    singles = [ev.convert_pcm(*it, **ctl) for it in items]
    assert ("vc", 1, 256) in ev._graphs
    assert n_model == [p[1] for p in singles] == [(len(r) // HOP) * HOP for r in recs]
    assert offsets.tolist() == np.cumsum([0] + [len(p[0]) for p in singles]).tolist()
    for i, (p, _) in enumerate(singles):
        assert p.dtype == np.int16 and np.abs(p).max() > 0
        assert np.array_equal(pcm[offsets[i]:offsets[i + 1]], p), i
    # the int16 stage: host_pcm of convert's float output
    wav = ev.convert(*items[0])
    assert wav.dtype == np.float32 and wav.shape == (30 * HOP,) and np.isfinite(wav).all()
    p0, n0 = ev.convert_pcm(*items[0], volume=0.8, tail_silence=0.01)
    assert n0 == 30 * HOP
    assert np.array_equal(p0, vits_wrap.host_pcm(wav, 16000, 1.0, 16000, 0.8, 0.01))
    # input at twice the model's rate == resampling first, converting at the model's rate
    rec2 = _recording(2 * (20 * HOP + 7), 9)
    a, _ = ev.convert_pcm(rec2, 1, 2, sampling_rate_in=32000)
    x = torch.from_numpy(rec2.astype(np.float32) / 32768.0).to(device)
    up, down = ops.resample_ratio(32000, 16000)
    b, _ = ev.convert_pcm(ops.resample_poly(x, up, down).cpu().numpy(), 1, 2)
    assert len(a) == 20 * HOP and np.array_equal(a, b)
    # the wrapper
    wrap = vits_wrap.VITSWrap(textparser=lambda uid, text: (uid, text, None), speecher=ev,
                              device_post=True)
    res = wrap.converting({"wav": recs[0], "spkid_src": 1, "spkid_tgt": 2, "volume": 0.8,
                           "tail_silence": 0.01, "id": "u1"})
    assert res["wav"][:4] == b"RIFF" and res["sr"] == 16000 and res["id"] == "u1"
    assert res["wav"][44:] == p0.tobytes()
    assert res["rtf"] > 0 and len(res["segment_info"]) == 1
    # refusals reach the caller
    with pytest.raises(ValueError):
        ev.convert(_recording(416, 1), 1, 2)
    # a posterior draw changes the result and comes from the object's generator
    w1 = ev.convert(*items[0], noise_scale=0.667)
    assert not np.array_equal(w1, wav) and ev._vc_gen is not None


def test_fp16_convert_graph_equals_eager_and_snr(base, gold, device, tmp_path):
    """What EmoVITS holds is the fp16 model: its graph replay equals its eager
    run bitwise, and its waveform stays close to the fp32 model's of the same
    weights.  Bar: see FP16_SNR_DB and DESIGN.md (voice conversion)."""
    ev = _emovits(device, base_model(device), tmp_path)
    rec = gold["wav"][0].numpy()
    src, tgt = VC.GOLDEN_SIDS
    a = ev.convert(rec, src, tgt)
    ev.graph = False
    b = ev.convert(rec, src, tgt)
    assert a.shape == (24 * HOP,) and np.array_equal(a, b)
    ref, _ = _row_alone(base, gold["wav"][0].to(device), VC.GOLDEN_L,
                        torch.tensor(src, device=device), torch.tensor(tgt, device=device), None,
                        device)
    snr = snr_db(a, ref)
    print(f"fp16 convert vs fp32 voice_conversion: snr {snr:.1f} dB (bar {FP16_SNR_DB})")
    assert snr >= FP16_SNR_DB

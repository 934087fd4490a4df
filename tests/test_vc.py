"""Voice conversion, CPU side: the test-side oracle (tests/vc_common.py: the
forward flow restated on oracle/vits_oracle.py's helpers) against the golden
fixture written from the reference's own modules (tests/golden/base_vc.npz,
make_golden_vc.py), the frame arithmetic of the ragged STFT, and the host
logic of EmoVITS.convert (refusals, bucket choice).  No GPU."""
import numpy as np
import pytest
import torch

import vc_common as VC
from common import base_model, golden, oracle_sd, rel_err, tiny_cfg, build_model


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in golden("base_vc.npz").items()}


def test_fixture_shape(gold):
    assert gold["wav"].shape == (1, VC.GOLDEN_L)
    assert (int(gold["sid_src"]), int(gold["sid_tgt"])) == VC.GOLDEN_SIDS
    assert gold["spec"].shape == (1, 513, 24) and gold["noise"].shape == (1, 192, 24)
    assert gold["o"].shape == (1, 1, 24 * 192)


def test_oracle_reproduces_reference_conversion(gold):
    """posterior_infer -> flow_forward -> flow_reverse -> generator on the
    project model's state dict (deterministic fill: the reference's weights)
    and the golden's inputs gives the reference's z, z_p, z_hat, o.  The
    same torch ops in the same order: 0.0 measured; 1e-6 allows for the
    reassociation of another thread count."""
    torch.set_num_threads(8)
    sd = oracle_sd(base_model("cpu"))
    spec = VC.spectrogram(gold["wav"])
    assert rel_err(spec, gold["spec"]) <= 1e-6
    with torch.no_grad():
        z, z_p, z_hat, o = VC.vc_oracle(sd, gold["spec"], gold["noise"], gold["sid_src"],
                                        gold["sid_tgt"])
    for name, t in (("z", z), ("z_p", z_p), ("z_hat", z_hat), ("o", o)):
        err = rel_err(t, gold[name])
        print(f"vc oracle {name}: rel_err {err:.2e}")
        assert err <= 1e-6, name
    # the fixture really converts: another speaker moves the latent
    assert rel_err(gold["z_hat"], gold["z"]) > 1e-2
    # and the forward flow really is the inverse of the reverse one
    with torch.no_grad():
        g_src = sd["emb_g.weight"][gold["sid_src"].long()]
        back = VC.V.flow_reverse(sd, z_p, g_src)
    assert rel_err(back, z) <= 1e-5


@pytest.mark.parametrize("n_fft,hop,win,pad", [(1024, 192, 768, 416), (64, 16, 64, 24)])
def test_frames_are_samples_over_hop(n_fft, hop, win, pad):
    """y_len = n // hop is the STFT's frame count for every length the
    conversion accepts (pad = (n_fft - hop) / 2, more than pad samples)."""
    from vits_amd import ops

    assert pad == (n_fft - hop) // 2
    for n in range(pad + 1, 3 * hop + 1):
        frames = ops.stft_rows_frames(n, n_fft, hop, pad)
        assert frames == n // hop, n
        if n + 2 * pad >= n_fft:  # what torch.stft gives the padded signal
            assert frames == (n + 2 * pad - n_fft) // hop + 1
    assert ops.stft_rows_frames(pad, n_fft, hop, pad) == 0
    assert ops.stft_rows_frames(10 * hop + 5, n_fft, hop, pad, frames_cap=7) == 7
    assert ops.stft_rows_frames(10 * hop + 5, n_fft, hop, pad, cap=4 * hop) == 4


@pytest.fixture(scope="module")
def ev_cpu(tmp_path_factory):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    c = tiny_cfg()
    data = dict(c["data"], spec_channels=513)
    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "filter_length": 1024, "hop_length": 192,
                 "win_length": 768, "text_channels": data["text_channels"],
                 "n_speakers": data["n_speakers"], "noise_scale": 0.667},
        "model": c["model"]})
    model = build_model(c["model"], data, "cpu")
    root = tmp_path_factory.mktemp("vc")
    return EmoVITS(str(root / "ckpt.pth"), "cpu", hps=hps, model=model)


def test_convert_on_cpu_raises(ev_cpu):
    from vits_amd._lib import VitsAmdError

    wav = np.zeros(4000, dtype=np.int16)
    with pytest.raises(VitsAmdError):
        ev_cpu.convert(wav, 1, 2)
    with pytest.raises(VitsAmdError):
        ev_cpu.convert_pcm(wav, 1, 2)
    with pytest.raises(VitsAmdError):
        ev_cpu.convert_pcm_batch([(wav, 1, 2), (wav, 2, 1)])


def test_convert_length_refusals(ev_cpu):
    assert ev_cpu._vc_stft() == (1024, 192, 768)
    for n in (0, 1, 416):  # at most pad samples
        with pytest.raises(ValueError):
            ev_cpu._vc_plan(n)
    assert ev_cpu._vc_plan(417) == (None, 417, 2, 256)
    with pytest.raises(ValueError):  # 4097 frames
        ev_cpu._vc_plan(4097 * 192)
    assert ev_cpu._vc_plan(4096 * 192 + 191)[2:] == (4096, 4096)
    # 832 samples at twice the rate are 416 at the model's: too short
    with pytest.raises(ValueError):
        ev_cpu._vc_plan(832, 32000)
    ratio, n, frames, bucket = ev_cpu._vc_plan(96000, 32000)
    assert ratio == (1, 2) and n == 48000 and frames == 250 and bucket == 256
    # a config without the STFT parameters cannot convert
    from vits_amd.utils import get_hparams_from_dict

    hps = ev_cpu.hps
    try:
        ev_cpu.hps = get_hparams_from_dict({"data": {"hop_length": 192}, "model": {}})
        with pytest.raises(ValueError):
            ev_cpu._vc_stft()
    finally:
        ev_cpu.hps = hps


def test_convert_bucket_choice(ev_cpu):
    b = ev_cpu._vc_bucket
    assert [b(f) for f in (0, 1, 255, 256, 257, 512, 513, 2049, 4096)] == \
        [256, 256, 256, 256, 512, 512, 1024, 4096, 4096]
    with pytest.raises(ValueError):
        b(4097)
    assert ev_cpu._batch_bucket(3) == 4


def test_converting_needs_device_post(ev_cpu):
    from vits_amd.vits_wrap import VITSWrap

    wrap = VITSWrap(textparser=lambda uid, text: (uid, text, None), speecher=ev_cpu,
                    device_post=True)  # (a CPU device turns device_post off)
    with pytest.raises(ValueError):
        wrap.converting({"wav": np.zeros(4000, dtype=np.int16), "spkid_src": 1, "spkid_tgt": 2})

"""Forced alignment, CPU side: the test-side oracle (tests/align_common.py)
against the golden fixture written from the reference's own modules
(tests/golden/base_align.npz, make_golden_align.py), the numpy reductions of a
path, and the host logic of EmoVITS.align / VITSWrap.aligning (refusals).  No
GPU."""
import numpy as np
import pytest
import torch

import align_common as A
import vc_common as VC
from common import BASE_DATA, base_model, golden, oracle_sd, rel_err, tiny_cfg, build_model


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in golden("base_align.npz").items()}


def test_fixture_shape(gold):
    assert gold["wav"].shape == (1, A.GOLDEN_L)
    assert gold["x"].shape == (1, A.GOLDEN_TX, BASE_DATA["text_channels"])
    assert gold["emo"].shape == (1, 1024) and int(gold["sid"]) == A.GOLDEN_SID
    assert gold["z_p"].shape == (1, 192, A.GOLDEN_FRAMES)
    assert gold["m_p"].shape == gold["logs_p"].shape == (1, 192, A.GOLDEN_TX)
    assert gold["neg_cent"].shape == (1, A.GOLDEN_FRAMES, A.GOLDEN_TX)
    d = gold["durations"].numpy()
    assert d.dtype == np.int32 and d.shape == (A.GOLDEN_TX,)
    assert d.min() >= 1 and d.sum() == A.GOLDEN_FRAMES
    # the inputs are the seeded ones the generator documents
    wav, x, emo = A.golden_inputs(A.GOLDEN_SEED, A.GOLDEN_L, A.GOLDEN_TX,
                                  BASE_DATA["text_channels"])
    assert torch.equal(wav, gold["wav"]) and torch.equal(x, gold["x"])
    assert torch.equal(emo, gold["emo"])


def test_oracle_reproduces_reference_alignment(gold):
    """text_encoder / posterior_infer / flow_forward / neg_cent / MAS on the
    project model's state dict (deterministic fill: the reference's weights)
    and the golden's inputs give the reference's latents, its neg_cent within
    1e-5 of its largest magnitude (the like bar of test_vc.py is 1e-6 and
    1.45e-6 has been seen on some CPUs: one decade wider) and exactly its
    durations; the scores are float32 sums of at most 35 such entries: the
    same 1e-5 of the largest score."""
    torch.set_num_threads(8)
    sd = oracle_sd(base_model("cpu"))
    with torch.no_grad():
        spec = VC.spectrogram(gold["wav"])
        z_p, m_p, logs_p, nc, dur, sc = A.align_oracle(sd, spec, gold["x"], gold["emo"],
                                                       gold["sid"])
    for name, t in (("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p), ("neg_cent", nc)):
        err = rel_err(t, gold[name])
        print(f"align oracle {name}: rel_err {err:.2e}")
        assert err <= 1e-5, name
    assert np.array_equal(dur, gold["durations"].numpy())
    err = rel_err(sc, gold["scores"])
    print(f"align oracle scores: rel_err {err:.2e}")
    assert err <= 1e-5


def test_fixture_scores_are_the_sequential_sums(gold):
    """The stored scores are float32 sums of the stored neg_cent along the
    stored durations' path, frame by frame."""
    nc = gold["neg_cent"][0].numpy()
    tokens = np.repeat(np.arange(A.GOLDEN_TX), gold["durations"].numpy())
    assert np.array_equal(A.token_scores(nc, tokens, A.GOLDEN_TX), gold["scores"].numpy())
    dur, sc, ft = A.mas_reduce(nc, A.GOLDEN_FRAMES, A.GOLDEN_TX)
    assert np.array_equal(dur, gold["durations"].numpy())
    assert np.array_equal(sc, gold["scores"].numpy()) and np.array_equal(ft, tokens)


def test_mas_reduce_no_alignment_rows():
    nc = np.random.default_rng(0).standard_normal((6, 4)).astype(np.float32)
    for t_t, t_s in ((0, 3), (5, 0), (3, 4)):
        dur, sc, ft = A.mas_reduce(nc, t_t, t_s)
        assert not dur.any() and not sc.any() and (ft == -1).all()
    dur, sc, ft = A.mas_reduce(nc, 4, 4)  # t_t == t_s: the diagonal
    assert dur.tolist() == [1, 1, 1, 1] and ft.tolist() == [0, 1, 2, 3, -1, -1]
    assert np.array_equal(sc, np.diag(nc[:4, :4]))


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
    root = tmp_path_factory.mktemp("align")
    return EmoVITS(str(root / "ckpt.pth"), "cpu", hps=hps, model=model)


def test_align_on_cpu_raises(ev_cpu):
    from vits_amd._lib import VitsAmdError

    wav = np.zeros(4000, dtype=np.int16)
    text = np.zeros((5, ev_cpu.text_channels), dtype=np.float32)
    emo = torch.zeros(1, 1024)
    with pytest.raises(VitsAmdError):
        ev_cpu.align(wav, 1, text, emo)
    with pytest.raises(VitsAmdError):
        ev_cpu.align_batch([(wav, 1, text, emo), (wav, 2, text, emo)])
    with pytest.raises(VitsAmdError):
        ev_cpu.model.align(torch.zeros(1, 5, ev_cpu.text_channels), torch.tensor([5]),
                           torch.zeros(1, 513, 20), torch.tensor([20]), emo, torch.tensor([1]))


def test_align_host_refusals(ev_cpu, monkeypatch):
    """The length checks need no GPU: they run on the host before anything is
    uploaded (the device check is lifted for this test only)."""
    ev = ev_cpu
    monkeypatch.setattr(ev, "device", torch.device("cuda"))
    emo = torch.zeros(1, 1024)
    c = ev.text_channels
    # 20 frames, 21 tokens: every token takes at least one frame
    with pytest.raises(ValueError, match="20 frames cannot be aligned with 21 tokens"):
        ev.align(np.zeros(20 * 192 + 5, dtype=np.int16), 1, np.zeros((21, c), np.float32), emo)
    # 40 frames at twice the rate are 20 at the model's
    with pytest.raises(ValueError, match="20 frames"):
        ev.align(np.zeros(40 * 192, dtype=np.int16), 1, np.zeros((21, c), np.float32), emo,
                 sampling_rate_in=32000)
    with pytest.raises(ValueError):  # no tokens
        ev.align(np.zeros(4000, dtype=np.int16), 1, np.zeros((0, c), np.float32), emo)
    with pytest.raises(ValueError):  # at most pad samples
        ev.align(np.zeros(416, dtype=np.int16), 1, np.zeros((1, c), np.float32), emo)
    with pytest.raises(ValueError):  # 4097 frames
        ev.align(np.zeros(4097 * 192, dtype=np.int16), 1, np.zeros((5, c), np.float32), emo)
    with pytest.raises(ValueError, match="2049 tokens"):  # beyond the kernel's width
        ev.align(np.zeros(4096 * 192, dtype=np.int16), 1, np.zeros((2049, c), np.float32), emo)
    # the second item of a batch is checked too
    good = (np.zeros(30 * 192, dtype=np.int16), 1, np.zeros((5, c), np.float32), emo)
    bad = (np.zeros(30 * 192, dtype=np.int16), 1, np.zeros((31, c), np.float32), emo)
    with pytest.raises(ValueError, match="30 frames cannot be aligned with 31 tokens"):
        ev.align_batch([good, bad])


def test_aligning_refuses_multi_segment_text(ev_cpu):
    from vits_amd.vits_wrap import VITSWrap

    class Front:
        max_utt_length = 8

        def __call__(self, uid, text):
            raise AssertionError("the front end must not run for a refused request")

    wrap = VITSWrap(textparser=Front(), speecher=ev_cpu)
    with pytest.raises(ValueError, match="2 segments"):
        wrap.aligning({"wav": np.zeros(4000, dtype=np.int16), "text": "abcdefgh ijkl",
                       "spkid": 1})

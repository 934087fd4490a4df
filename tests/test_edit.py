"""Speech editing, CPU side: the numpy oracle of pins, splice and patch
(tests/edit_common.py) against per-frame brute-force loops, EmoVITS.edit_span,
SynthesizerTrn.edit_context_frames against the sum restated from the config's
numbers, the refusals of EmoVITS.edit (host arithmetic, before anything is
uploaded), and the composition of the definition restated on
oracle/vits_oracle.py against the reference's golden.  No GPU."""
import numpy as np
import pytest
import torch

import edit_common as EC
import vc_common as VC
from common import BASE_DATA, BASE_MODEL, base_model, build_model, golden, oracle_sd, rel_err, \
    tiny_cfg

REL = 1e-4  # the project's fp32 parity bar (tests/test_models_gpu.py)
N_FFT, HOP, WIN = VC.STFT["n_fft"], VC.STFT["hop"], VC.STFT["win"]


# -- the oracle against brute force ---------------------------------------------

def _rows(seed, C=3):
    """Random consistent edits: (dur_old, span, dur_new, ty, m, s, noise, z_rec)."""
    rng = np.random.RandomState(seed)
    for _ in range(40):
        n_old = rng.randint(1, 9)
        a = rng.randint(0, n_old + 1)
        b_old = rng.randint(a, n_old + 1)
        b_new = a + rng.randint(0, 4)
        n_new = n_old - b_old + b_new
        if n_new == 0:
            continue
        dur_old = rng.randint(0, 5, n_old)
        dur_old[rng.randint(n_old)] += 1  # (never all zero)
        ty = int(dur_old.sum())
        dur_new = np.concatenate([dur_old[:a], rng.randint(0, 6, b_new - a), dur_old[b_old:]])
        t_y = int(dur_new.sum()) + rng.randint(0, 5)
        yield (dur_old, (a, b_old, b_new), dur_new, ty, rng.randn(C, n_new).astype(np.float32),
               rng.rand(C, n_new).astype(np.float32), rng.randn(C, max(t_y, 1)).astype(np.float32),
               rng.randn(C, ty + 2).astype(np.float32))


def test_pins_oracle_against_the_definition():
    for dur_old, span, dur_new, ty, *_ in _rows(1):
        a, b_old, b_new = span
        n_old, n_new = len(dur_old), len(dur_new)
        sg = np.full((1, n_new), 77)
        for st, want_t in ((0, 0), (9, ty - int(dur_old[a:b_old].sum()) + 9), (-1, ty)):
            given, target, meta = EC.pins(dur_old[None], [n_old], [n_new], n_new + 2, [span], [ty],
                                          span_given=np.pad(sg, ((0, 0), (0, 2))),
                                          span_target=[st])
            assert meta[:, 0].tolist() == [int(dur_old[:a].sum()), int(dur_old[:b_old].sum()), 0]
            for t in range(n_new):  # the issue's pins, token by token
                want = dur_old[t] if t < a else (dur_old[t - b_new + b_old] if t >= b_new else 77)
                assert given[0, t] == want
            assert given[0, n_new:].tolist() == [-1, -1] and target[0] == want_t
        # no caller pins: the span is free
        given, _, _ = EC.pins(dur_old[None], [n_old], [n_new], n_new, [span], [ty])
        assert (given[0, a:b_new] == -1).all()
    # refusals: a span that does not fit, no alignment, a sum that is not the recording's
    d = np.array([[2, 3, 4, 1]])
    for kw in (dict(spans=[(1, 3, 2)], xn=[4]), dict(spans=[(3, 2, 2)], xn=[4]),
               dict(spans=[(1, 2, 2)], xn=[4], ty=[11]), dict(spans=[(1, 2, 5)], xn=[4]),
               dict(spans=[(1, 2, 2)], xn=[4], d=np.zeros((1, 4), int), ty=[0]),
               dict(spans=[(1, 2, 2)], xn=[4], xo=[5])):
        given, target, meta = EC.pins(kw.get("d", d), kw.get("xo", [4]), kw["xn"], 4, kw["spans"],
                                      kw.get("ty", [10]))
        assert meta[2, 0] == 1 and not given.any() and target[0] == 0, kw
    assert EC.pins(d, [4], [4], 4, [(1, 2, 2)], [10])[2][2, 0] == 0


def test_splice_oracle_against_frame_loops():
    seen = set()
    for dur_old, span, dur_new, ty, m, s, noise, z_rec in _rows(2):
        nx = len(dur_new)
        z, lens, meta = EC.splice(dur_new[None], [nx], [span], [ty], m[None], s[None], noise[None],
                                  z_rec[None], stage_mult=(1, 8))
        want = EC.splice_brute(dur_new, nx, span, ty, m, s, noise, z_rec)
        assert want is not None and meta[3, 0] == 0
        assert np.array_equal(z[0].view(np.int32), want[0].view(np.int32))
        assert tuple(meta[:3, 0]) == want[1]
        f0, n_new, f1 = want[1]
        assert f0 == dur_old[:span[0]].sum() and f1 == dur_old[:span[1]].sum()
        y_new = f0 + n_new + ty - f1
        assert lens[:, 0].tolist() == [y_new, 8 * y_new] and not z[0, :, y_new:].any()
        seen.add((span[1] == span[0], span[2] == span[0], n_new == 0, span[0] == 0,
                  span[1] == len(dur_old)))
    # insertions, deletions, empty new spans and both ends were among them
    assert all(any(flags[i] for flags in seen) for i in range(5))
    # overflow and an inconsistent suffix
    dur_new = np.array([[3, 4, 5]])
    m = np.zeros((1, 2, 3), np.float32)
    args = ([3], [(1, 1, 2)], [8], m, m, np.zeros((1, 2, 11), np.float32),
            np.zeros((1, 2, 8), np.float32))
    assert EC.splice(dur_new, *args)[2][:, 0].tolist() == [3, 4, 3, -1]
    args = ([3], [(1, 1, 2)], [7], m, m, np.zeros((1, 2, 12), np.float32),
            np.zeros((1, 2, 8), np.float32))
    assert EC.splice(dur_new, *args)[2][:, 0].tolist() == [0, 0, 0, 1]


def test_patch_oracle_against_sample_loops():
    rng = np.random.RandomState(3)
    hop = 6
    cases = [(10, 3, 5, 5, 2, 4), (10, 3, 1, 5, 2, 4), (10, 3, 2, 5, 2, 4),  # shift > 0, < 0, = 0
             (10, 0, 4, 2, 1, 5), (10, 8, 3, 10, 1, 5), (10, 0, 0, 10, 0, 3),  # dropped fades
             (10, 3, 5, 5, 2, 0), (10, 4, 0, 6, 0, 7), (7, 2, 3, 4, 50, 9)]
    for ty, f0, n_new, f1, margin, fade in cases:
        y_new = f0 + n_new + ty - f1
        orig = rng.randn(1, ty * hop + 3).astype(np.float32)
        o = rng.randn(1, y_new * hop + 5).astype(np.float32)
        smeta = np.array([[f0], [n_new], [f1], [0]])
        out, out_len = EC.patch(orig, o, [ty], smeta, hop, margin, fade)
        want = EC.patch_brute(orig[0], o[0], ty, f0, n_new, f1, hop, margin, fade)
        L = y_new * hop
        assert out_len[0] == L == len(want)
        assert np.array_equal(out[0, :L].view(np.int32), want.view(np.int32)), (ty, f0, n_new, f1)
        assert not out[0, L:].any()
        # far from the edit: the recording itself, shifted behind it
        _, lo, hi, shift, fin, fout = EC.patch_bounds(f0, n_new, f1, ty, hop, margin, fade)
        if fin:
            assert np.array_equal(out[0, :lo - fade], orig[0, :lo - fade])
        if fout:
            assert np.array_equal(out[0, hi + fade:L], orig[0, hi + fade - shift:L - shift])
        assert np.array_equal(out[0, lo:hi], o[0, lo:hi])
    # a refused splice: silence
    out, out_len = EC.patch(orig, o, [ty], np.array([[0], [0], [0], [-1]]), hop, 1, 2)
    assert out_len[0] == 0 and not out.any()


# -- the span ---------------------------------------------------------------------

def test_edit_span():
    from vits_amd.infer import EmoVITS

    rng = np.random.RandomState(4)
    v = rng.randn(12, 5).astype(np.float32)
    new = rng.randn(4, 5).astype(np.float32)
    span = EmoVITS.edit_span
    assert span(v, np.concatenate([v[:4], new[:3], v[6:]])) == (4, 6, 7)      # replacement
    assert span(v, np.concatenate([v[:4], new[:2], v[4:]])) == (4, 4, 6)      # insertion
    assert span(v, np.concatenate([v[:4], v[7:]])) == (4, 7, 4)               # deletion
    assert span(v, v.copy()) == (12, 12, 12)                                  # identical
    assert span(v, np.concatenate([new[:2], v[3:]])) == (0, 3, 2)             # at token 0
    assert span(v, np.concatenate([v[:9], new])) == (9, 12, 13)               # through the end
    assert span(v, new) == (0, 12, 4)
    # a repeated token next to the edit: prefix first, then the suffix of what remains
    r = np.concatenate([v[:3], v[2:3], v[3:]])
    assert span(v, r) == (3, 3, 4)
    for old, nw in ((v, r), (r, v), (v, new)):
        a, b_old, b_new = span(old, nw)
        assert np.array_equal(old[:a], nw[:a]) and np.array_equal(old[b_old:], nw[b_new:])
        assert len(old) - b_old == len(nw) - b_new


# -- the context --------------------------------------------------------------------

@pytest.mark.parametrize("which", ["base", "tiny"])
def test_edit_context_matches_restatement(which):
    """The reverse flow's reach (every coupling's WN stack, once) plus the
    decoder's (Generator.context_frames): 32 + 14 = 46 at base and tiny."""
    if which == "base":
        cfg, data = BASE_MODEL, BASE_DATA
    else:
        c = tiny_cfg()
        cfg, data = c["model"], c["data"]
    model = build_model(cfg, data, "cpu", fill=False)
    # WN of a coupling: 4 layers of kernel_size 5, dilation_rate ** i
    flow = sum(sum((cfg["kernel_size"] - 1) // 2 * r ** i for i in range(4))
               for r in cfg["dilation_rate"][:cfg["n_flows"]])
    dec = model.dec.context_frames()
    assert (flow, dec) == (32, 14)
    assert model.edit_context_frames() == flow + dec == 46
    stft = (N_FFT, HOP, WIN) if which == "base" else None
    if stft is not None:  # the edit's reach is voice conversion's without the audio side
        assert model.edit_context_frames() < model.vc_context_frames(stft)
    model.remove_weight_norm()
    assert model.edit_context_frames() == 46


# -- refusals before upload -----------------------------------------------------------

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
    return EmoVITS(str(tmp_path_factory.mktemp("ed") / "ckpt.pth"), "cpu", hps=hps, model=model)


def test_edit_host_refusals(ev_cpu, monkeypatch):
    """Every refusal the host can make comes before anything is uploaded (the
    device check is lifted for this test only and the upload is made to fail:
    nothing here gets as far as the device)."""
    from vits_amd import _lib

    ev = ev_cpu
    emo = torch.zeros(1, 1024)
    rng = np.random.RandomState(5)
    c = ev.text_channels
    old = rng.randn(12, c).astype(np.float32)
    new = np.concatenate([old[:4], rng.randn(3, c).astype(np.float32), old[6:]])
    wav = np.zeros(60 * HOP + 57, np.float32)
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ev.edit(wav, 1, old, new, emo)
    monkeypatch.setattr(ev, "device", torch.device("cuda"))

    def no_upload(*a, **k):
        raise AssertionError("the upload was reached")

    monkeypatch.setattr(ev, "_vc_upload", no_upload)
    for call in (ev.edit, ev.edit_pcm):
        with pytest.raises(ValueError, match="span"):          # does not match the texts
            call(wav, 1, old, new, emo, span=(4, 6, 8))
        with pytest.raises(ValueError, match="span"):
            call(wav, 1, old, new, emo, span=(5, 6, 7))
        with pytest.raises(ValueError, match="span"):
            call(wav, 1, old, new, emo, span=(4, 6))
        with pytest.raises(ValueError, match="4096"):           # over VC_MAX_FRAMES
            call(np.zeros(4097 * HOP, np.float32), 1, old, new, emo)
        with pytest.raises(ValueError, match="at least one frame"):   # fewer frames than tokens
            call(np.zeros(11 * HOP, np.float32), 1, old, new, emo)
        with pytest.raises(ValueError, match="only deletes"):   # span_frames, empty new span
            call(wav, 1, old, np.concatenate([old[:4], old[6:]]), emo, span_frames=20)
        with pytest.raises(ValueError, match="span_frames"):
            call(wav, 1, old, new, emo, span_frames=0)
        with pytest.raises(ValueError, match="durations"):
            call(wav, 1, old, new, emo, durations=[3, 4])
        with pytest.raises(ValueError, match="token_scale"):
            call(wav, 1, old, new, emo, token_scale=[1.0] * 12)
        with pytest.raises(ValueError, match="durations_old"):  # 12 values that sum to 59
            call(wav, 1, old, new, emo, durations_old=[5] * 11 + [4])
        with pytest.raises(AssertionError, match="upload"):     # a good call gets that far
            call(wav, 1, old, new, emo, span_frames="keep", durations_old=[5] * 12)


# -- the composition against the reference's golden -----------------------------------------

def test_oracle_composition_matches_reference_golden():
    """The definition of SynthesizerTrn.edit restated on oracle/vits_oracle.py,
    vc_common.flow_forward and the numpy splice, against base_edit.npz (the
    reference's own modules): REL = 1e-4."""
    from oracle import vits_oracle as V

    gold = golden("base_edit.npz")
    t = {k: torch.from_numpy(v) for k, v in gold.items()}
    sd = oracle_sd(base_model("cpu"))
    cfg = BASE_MODEL
    H = cfg["hidden_channels"]
    span = tuple(int(v) for v in gold["span"])
    assert span == EC.GOLDEN_SPAN and gold["dur_old"].tolist() == EC.GOLDEN_DUR_OLD
    assert gold["wav"].shape == (1, EC.GOLDEN_L) and gold["x_old"].shape[1] == 12
    assert gold["x_new"].shape[1] == 13
    with torch.no_grad():
        spec = VC.spectrogram(t["wav"])
        ty = spec.shape[2]
        g = sd["emb_g.weight"][t["sid"].long()]
        z = V.posterior_infer(sd, spec, t["noise_q"], cfg["n_layers_q"], H)
        z_p_rec = VC.flow_forward(sd, z, g, cfg["n_flows"], 4, H)
        m_p, s_p, _, _ = V.infer_p1(sd, t["x_new"], t["emo"], t["sid"].long(), cfg)
        # the pins from the old durations, the span's own by hand: every token pinned
        given, target, meta = EC.pins(gold["dur_old"][None], [12], [13], 13, [span], [ty],
                                      span_given=gold["dur_new"][None])
        assert meta[2, 0] == 0 and target[0] == 0
        assert given[0].tolist() == gold["dur_new"].tolist()
        zs, lens, smeta = EC.splice(given, [13], [span], [ty], m_p.numpy(), s_p.numpy(),
                                    gold["noise"], z_p_rec.numpy())
        assert smeta[:, 0].tolist() == [20, 17, 36, 0] and lens[0, 0] == 61
        z_p = torch.from_numpy(zs)
        z_hat = V.flow_reverse(sd, z_p, g, cfg["n_flows"], 4, H)
        o = V.generator(sd, z_hat, g, cfg)
    for name, got in (("z_p_rec", z_p_rec), ("z_p", z_p), ("z_hat", z_hat), ("o", o)):
        err = rel_err(got, t[name])
        print(f"edit oracle {name}: rel_err {err:.2e}")
        assert err < REL, name
    assert tuple(o.shape) == (1, 1, 61 * HOP)

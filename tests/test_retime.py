"""Retiming a recording, CPU side: the numpy oracle of the plan and the warp
(tests/retime_common.py) against brute-force restatements (Python big integers
and fractions.Fraction; a per-frame loop), the properties the rule promises,
the refusals of EmoVITS.retime / retime_pcm and VITSWrap.retiming (host
arithmetic, before anything is uploaded), and the composition of the
definition restated on oracle/vits_oracle.py against the reference's golden.
No GPU."""
import itertools

import numpy as np
import pytest
import torch

import retime_common as RC
import vc_common as VC
from common import BASE_MODEL, base_model, build_model, golden, oracle_sd, rel_err, tiny_cfg

REL = 1e-4  # the project's fp32 parity bar (tests/test_edit.py, tests/test_vc.py)
N_FFT, HOP, WIN = VC.STFT["n_fft"], VC.STFT["hop"], VC.STFT["win"]
SCALES = [1.0, 0.5, 2.0, 1.1, 0.3, 3.7, 1 / 16, 16.0, np.nan, np.inf, 0.0, -1.0, 1e-9, 1e9]


# -- the plan ---------------------------------------------------------------------------

def _same(row, brute):
    out, total, st = row
    want, wst = brute
    assert st == wst and out.tolist() == want and total == sum(want)


def test_plan_oracle_exhaustive_small():
    """1-3 tokens, every duration in 0..4, every pin pattern over {free, 0,
    3}, a scale on the first token, no target / a target: the array form
    against the big-integer restatement."""
    n = 0
    for t_x in (1, 2, 3):
        for d in itertools.product(range(5), repeat=t_x):
            for g in itertools.product((-1, 0, 3), repeat=t_x):
                for s0, rate, target in ((1.0, None, 0), (2.5, 1.3, 0), (0.4, None, 7),
                                         (1.0, 0.5, 1)):
                    ts = [s0] + [1.0] * (t_x - 1)
                    ty = sum(d)
                    _same(RC.plan_row(d, t_x, ty, g, ts, rate, target),
                          RC.plan_brute(d, t_x, ty, g, ts, rate, target))
                    n += 1
    assert n == 4 * (5 * 3 + 25 * 9 + 125 * 27)


def _random_case(rng, big=False):
    t_x = int(rng.randint(1, 40))
    nx = t_x if rng.rand() < 0.7 else int(rng.randint(0, t_x + 1))
    d = rng.randint(0, 3000 if big else 12, t_x)
    if rng.rand() < 0.1:
        d[rng.randint(t_x)] = rng.choice([-5, (1 << 18) + 9])
    ty = int(np.clip(d[:nx], 0, RC.MAX_DUR).sum())
    given = None
    if rng.rand() < 0.5:
        given = np.where(rng.rand(t_x) < 0.3, rng.randint(0, 20, t_x), -1)
        if rng.rand() < 0.1:
            given[rng.randint(t_x)] = (1 << 18) + 77
    ts = None
    if rng.rand() < 0.5:
        ts = rng.choice(SCALES, t_x).astype(np.float32)
    rate = None if rng.rand() < 0.5 else float(rng.choice(SCALES))
    target = 0 if rng.rand() < 0.5 else int(rng.randint(1, max(3 * ty, 2)))
    return d, nx, ty, given, ts, rate, target


def test_plan_oracle_sampled_and_properties():
    rng = np.random.RandomState(11)
    served = refused = 0
    for i in range(4000):
        d, nx, ty, given, ts, rate, target = _random_case(rng, big=i % 4 == 0)
        out, total, st = RC.plan_row(d, nx, ty, given, ts, rate, target)
        _same((out, total, st), RC.plan_brute(d, nx, ty, given, ts, rate, target))
        assert (out[nx:] == 0).all() and (out >= 0).all()
        dc = np.clip(d, 0, RC.MAX_DUR)
        if st:
            refused += 1
            assert out[:nx].tolist() == dc[:nx].tolist()  # the row keeps its durations
            continue
        served += 1
        if target:
            assert total == target  # exact, whatever the scales
        if given is not None:
            pin = given[:nx] >= 0
            assert out[:nx][pin].tolist() == np.minimum(given[:nx][pin], RC.MAX_DUR).tolist()
    assert served > 1500 and refused > 300


def test_plan_identity_at_neutral_controls():
    """No control, or controls that say nothing: dur_new == dur_old exactly."""
    rng = np.random.RandomState(12)
    for _ in range(500):
        t_x = int(rng.randint(1, 60))
        d = rng.randint(0, 500, t_x)
        ty = int(d.sum())
        for kw in ({}, dict(given=np.full(t_x, -1)), dict(tok_scale=np.ones(t_x, np.float32)),
                   dict(rate=1.0), dict(target=ty) if ty else {}):
            out, total, st = RC.plan_row(d, t_x, ty, **kw)
            assert st == 0 and out.tolist() == d.tolist() and total == ty


def test_plan_every_refusal():
    d = [4, 0, 6, 5]
    ok = RC.plan_row(d, 4, 15)
    assert ok[2] == 0
    assert RC.plan_row(d, 4, 14)[2] == 1                              # sum != y_len_old
    assert RC.plan_row(d, 3, 15)[2] == 1                              # (x_len cuts the sum)
    assert RC.plan_row(d, 4, 15, given=[-1, 9, -1, -1], target=8)[2] == 1    # E < 0
    assert RC.plan_row(d, 4, 15, target=(1 << 24) + 1)[2] == 1         # target > 2^24
    assert RC.plan_row(d, 4, 15, given=[3, -1, 3, 3], target=10)[2] == 1     # Qtot == 0, E != 0
    out, total, st = RC.plan_row(d, 4, 15, given=[3, -1, 3, 3], target=9)    # Qtot == 0, E == 0
    assert st == 0 and out.tolist() == [3, 0, 3, 3] and total == 9
    big = [1 << 18, 1]
    assert RC.plan_row(big, 2, (1 << 18) + 1)[2] == 1                 # y_len_old > 2^18
    for row in (RC.plan_row(d, 4, 14), RC.plan_row(d, 4, 15, target=(1 << 24) + 1)):
        assert row[0].tolist() == d and row[1] == 15
    # a NaN or infinite scale never reaches the integers
    out, total, st = RC.plan_row(d, 4, 15, tok_scale=[np.nan, np.inf, -np.inf, 1.0])
    assert st == 0 and out.tolist() == RC.plan_brute(d, 4, 15, tok_scale=[np.nan, np.inf, -np.inf,
                                                                           1.0])[0]
    assert out[0] == 0 and out[2] == 0 and out[3] == 5  # 4 * 2^-8 and 6 * 2^-8 round to 0


# -- the warp ---------------------------------------------------------------------------

def _warp_cases(seed):
    rng = np.random.RandomState(seed)
    for _ in range(60):
        t_x = int(rng.randint(1, 9))
        nx = t_x if rng.rand() < 0.7 else int(rng.randint(1, t_x + 1))
        do = rng.randint(0, 7, t_x)
        do[rng.randint(nx)] += 1
        dn = rng.randint(0, 9, t_x)
        ty = int(do[:nx].sum())
        yield do, dn, nx, ty, rng.randn(3, ty + 2).astype(np.float32)


def test_warp_oracle_against_frame_loop():
    for do, dn, nx, ty, z in _warp_cases(21):
        z[:, ty:] = np.nan  # nothing past y_len_old is read
        y_new = int(dn[:nx].sum())
        t_y = y_new + 3
        got, lens, meta = RC.warp(z[None], do[None], dn[None], [nx], [ty], t_y, stage_mult=(1, 4))
        want, pos = RC.warp_brute(z, do, dn, nx, ty)
        assert meta[:, 0].tolist() == [y_new, 0] and lens[:, 0].tolist() == [y_new, 4 * y_new]
        assert got[0, :, :y_new].tobytes() == want.tobytes()
        assert not got[0, :, y_new:].any() and np.isfinite(got).all()
        # the source position never goes back, within a token or across tokens
        assert all(a <= b for a, b in zip(pos, pos[1:]))
        j0, j1, r, den = RC.warp_sources(do, dn, nx, ty)
        assert (np.diff(j0) >= 0).all() and (np.diff(j1) >= 0).all()
        assert (j0 >= 0).all() and (j1 <= ty - 1).all() and ((j1 - j0) >= 0).all()


def test_warp_copies_where_the_durations_agree():
    for do, _, nx, ty, z in _warp_cases(22):
        got, _, meta = RC.warp(z[None], do[None], do[None], [nx], [ty], ty + 5)
        assert meta[:, 0].tolist() == [ty, 0]
        assert got[0, :, :ty].tobytes() == z[:, :ty].tobytes()
    # one token of 67 frames: 67 -> 134 sits between neighbours at 1/4 and 3/4
    z = np.arange(67, dtype=np.float32)[None, None] * 4
    got, _, _ = RC.warp(z, [[67]], [[134]], None, [67], 134)
    assert got[0, 0, :5].tolist() == [0.0, 1.0, 3.0, 5.0, 7.0] and got[0, 0, -1] == 66 * 4


def test_warp_token_born_from_nothing_reads_clamped_neighbours():
    """dur_old == 0 with dur_new > 0: every new frame sits at c_old - 1/2, the
    midpoint of the two frames around the empty token, clamped at the
    recording's ends."""
    z = np.asarray([[10.0, 20.0, 40.0]], np.float32)
    for do, dn, want in (([2, 0, 1], [2, 3, 1], [10, 20, 30, 30, 30, 40]),
                         ([0, 3], [2, 3], [10, 10, 10, 20, 40]),
                         ([3, 0], [3, 2], [10, 20, 40, 40, 40])):
        got, _, meta = RC.warp(z[None], [do], [dn], None, [3], 8)
        assert meta[:, 0].tolist() == [sum(dn), 0]
        assert got[0, 0, :sum(dn)].tolist() == want
    # refusals: the bucket is too small, or there is no recording
    _, lens, meta = RC.warp(z[None], [[3]], [[9]], None, [3], 8)
    assert meta[:, 0].tolist() == [9, -1] and lens[0, 0] == 0
    _, _, meta = RC.warp(z[None], [[0]], [[2]], None, [0], 8)
    assert meta[:, 0].tolist() == [2, -1]


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
    return EmoVITS(str(tmp_path_factory.mktemp("rt") / "ckpt.pth"), "cpu", hps=hps, model=model)


def _no_upload(*a, **k):
    raise AssertionError("the upload was reached")


def test_retime_host_refusals(ev_cpu, monkeypatch):
    """Every refusal the host can make comes before anything is uploaded (the
    device check is lifted for this test only and the upload is made to fail:
    nothing here gets as far as the device)."""
    from vits_amd import _lib

    ev = ev_cpu
    text = np.random.RandomState(5).randn(12, ev.text_channels).astype(np.float32)
    wav = np.zeros(60 * HOP + 57, np.float32)
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ev.retime(wav, 1, 1)
    monkeypatch.setattr(ev, "device", torch.device("cuda"))
    monkeypatch.setattr(ev, "_vc_upload", _no_upload)
    for call in (ev.retime, ev.retime_pcm):
        with pytest.raises(ValueError, match="4096"):               # over VC_MAX_FRAMES
            call(np.zeros(4097 * HOP, np.float32), 1, 1)
        with pytest.raises(ValueError, match="at least one frame"):  # fewer frames than tokens
            call(np.zeros(11 * HOP, np.float32), 1, 1, text=text)
        for bad in (0.05, 16.5, float("nan"), float("inf"), -1.0, "fast"):
            with pytest.raises(ValueError, match="speed"):
                call(wav, 1, 1, speed=bad)
        for bad in ([1.0] * 11 + [17.0], [1.0] * 11 + [0.01], [1.0] * 11 + [np.nan],
                    [1.0] * 11 + [np.inf], [1.0] * 11):
            with pytest.raises(ValueError, match="token_scale"):
                call(wav, 1, 1, text=text, token_scale=bad)
        with pytest.raises(ValueError, match="need text"):          # per-token controls, no text
            call(wav, 1, 1, durations=[5] * 12)
        with pytest.raises(ValueError, match="need text"):
            call(wav, 1, 1, token_scale=[1.0] * 12)
        with pytest.raises(ValueError, match="durations need 12"):  # a length against the text
            call(wav, 1, 1, text=text, durations=[5] * 11)
        with pytest.raises(ValueError, match="durations_old"):      # 12 values that sum to 59
            call(wav, 1, 1, text=text, durations_old=[5] * 11 + [4])
        with pytest.raises(ValueError, match="durations_old"):      # 11 values against 12 tokens
            call(wav, 1, 1, text=text, durations_old=[5] * 10 + [10])
        with pytest.raises(ValueError, match="target_frames"):
            call(wav, 1, 1, target_frames=0)
        with pytest.raises(ValueError, match="target_frames"):
            call(wav, 1, 1, target_frames=4097)
        with pytest.raises(ValueError, match="largest bucket"):     # the host bound on y_new
            call(np.zeros(600 * HOP, np.float32), 1, 1, speed=8.0)
        for good in (dict(), dict(speed=1.1), dict(target_frames=70),
                     dict(text=text, durations_old=[5] * 12, token_scale=[1.0] * 11 + [2.0]),
                     dict(durations_old=[60])):
            with pytest.raises(AssertionError, match="upload"):     # a good call gets that far
                call(wav, 1, 1, **good)
    with pytest.raises(ValueError, match="speed / pitch"):          # in range each, not together
        ev.retime_pcm(wav, 1, 1, speed=0.1, pitch=2.0)


def test_retiming_request_refusals(ev_cpu, monkeypatch):
    from vits_amd.vits_wrap import VITSWrap

    vecs = np.random.RandomState(6).randn(12, ev_cpu.text_channels).astype(np.float32)
    front = lambda uid, text: (uid, text, vecs)  # noqa: E731
    wav = np.zeros(60 * HOP + 57, np.float32)
    with pytest.raises(ValueError, match="device_post"):
        VITSWrap(textparser=front, speecher=ev_cpu).retiming({"wav": wav, "spkid_src": 1})
    monkeypatch.setattr(ev_cpu, "device", torch.device("cuda"))
    monkeypatch.setattr(ev_cpu, "_vc_upload", _no_upload)
    wrap = VITSWrap(textparser=front, speecher=ev_cpu, device_post=True)
    with pytest.raises(ValueError, match="spkid_src"):
        wrap.retiming({"wav": wav})
    with pytest.raises(ValueError, match="need text"):
        wrap.retiming({"wav": wav, "spkid_src": 1, "token_scale": [1.0] * 12})
    with pytest.raises(ValueError, match="need text"):
        wrap.retiming({"wav": wav, "spkid_src": 1, "durations": [5] * 12})
    for sec in (0.0, -1.0, float("nan"), 1e-9):
        with pytest.raises(ValueError, match="duration_s"):
            wrap.retiming({"wav": wav, "spkid_src": 1, "duration_s": sec})
    with pytest.raises(ValueError, match="token_scale"):
        wrap.retiming({"wav": wav, "spkid_src": 1, "text": "abc", "token_scale": [1.0] * 5})
    with pytest.raises(AssertionError, match="upload"):
        wrap.retiming({"wav": wav, "spkid_src": 1, "text": "abc", "speed": 1.2,
                       "token_scale": [1.0] * 12})
    with pytest.raises(AssertionError, match="upload"):
        wrap.retiming({"wav": wav, "spkid_src": 1, "duration_s": 0.9})


# -- the composition against the reference's golden -----------------------------------------

def test_oracle_composition_matches_reference_golden():
    """The definition of SynthesizerTrn.retime restated on
    oracle/vits_oracle.py, vc_common.flow_forward, the numpy plan and the
    numpy warp, against base_retime.npz (the reference's own modules): REL =
    1e-4."""
    from oracle import vits_oracle as V

    gold = golden("base_retime.npz")
    t = {k: torch.from_numpy(v) for k, v in gold.items()}
    sd = oracle_sd(base_model("cpu"))
    cfg = BASE_MODEL
    H = cfg["hidden_channels"]
    assert gold["dur_old"].tolist() == RC.GOLDEN_DUR_OLD and gold["wav"].shape == (1, RC.GOLDEN_L)
    assert gold["given"].tolist() == RC.GOLDEN_GIVEN and int(gold["target"][0]) == RC.GOLDEN_TARGET
    assert 0 in gold["dur_old"] and gold["tok_scale"].tolist() == RC.GOLDEN_TOK_SCALE
    with torch.no_grad():
        spec = VC.spectrogram(t["wav"])
        ty = spec.shape[2]
        g_src = sd["emb_g.weight"][t["sid_src"].long()]
        g_tgt = sd["emb_g.weight"][t["sid_tgt"].long()]
        z = V.posterior_infer(sd, spec, t["noise_q"], cfg["n_layers_q"], H)
        z_p = VC.flow_forward(sd, z, g_src, cfg["n_flows"], 4, H)
        dur_new, total, st = RC.plan(gold["dur_old"][None], [12], [ty], gold["given"][None],
                                     gold["tok_scale"][None], None, gold["target"])
        assert st[0] == 0 and total[0] == 71 and dur_new[0].tolist() == gold["dur_new"].tolist()
        assert dur_new[0, 3] == 11  # the pin
        zw, lens, meta = RC.warp(z_p.numpy(), gold["dur_old"][None], dur_new, [12], [ty], 71)
        assert meta[:, 0].tolist() == [71, 0] and lens[0, 0] == 71
        z_warp = torch.from_numpy(zw)
        z_hat = V.flow_reverse(sd, z_warp, g_tgt, cfg["n_flows"], 4, H)
        o = V.generator(sd, z_hat, g_tgt, cfg)
    for name, got in (("z_p", z_p), ("z_warp", z_warp), ("z_hat", z_hat), ("o", o)):
        err = rel_err(got, t[name])
        print(f"retime oracle {name}: rel_err {err:.2e}")
        assert err < REL, name
    assert tuple(o.shape) == (1, 1, 71 * HOP)

"""The duration plan's rule on the host: properties of the numpy oracle
(tests/duration_common.py) on random cases, a comparison with a big-integer
restatement on small cases (exhaustive up to 3 tokens, sampled at 4 and 5), the package's host helper
(vits_amd/durations.py) against the oracle, and the host-side refusals.  No
GPU."""
import itertools

import numpy as np
import pytest

import duration_common as DC
from vits_amd import durations as D


def _random_case(rng, t_x):
    w = np.exp(rng.normal(0.5, 1.2, t_x)).astype(np.float32)
    kind = rng.integers(0, 4)
    given = np.full(t_x, -1, np.int64)
    if kind:
        pin = rng.random(t_x) < (0.3 if kind < 3 else 1.0)
        given[pin] = rng.integers(0, 12, t_x)[pin]
    return w, given


def test_fit_properties_on_random_cases():
    rng = np.random.default_rng(1234)
    n_fit = n_bad = 0
    for _ in range(3000):
        t_x = int(rng.integers(1, 60))
        w, given = _random_case(rng, t_x)
        free = given < 0
        P, nF = int(given[~free].sum()), int(free.sum())
        natural = P + int(np.ceil(w[free]).sum())
        T = int(rng.integers(1, 2 * natural + 4))
        d, total, status = DC.plan_row(w, given, T, t_x)
        ok = (T - P - nF >= 0) if nF else T == P
        assert status == int(not ok)
        assert np.array_equal(d[~free], given[~free])        # pins kept
        if ok:
            n_fit += 1
            assert total == T and d.sum() == T               # exact sum
            assert np.all(d[free] >= 1)                      # every free token sounds
        else:
            n_bad += 1
            assert np.array_equal(d[free], np.ceil(w[free]).astype(np.int64))
            assert total == natural
    assert n_fit > 500 and n_bad > 100


def test_fit_at_the_natural_total_stays_near_ceil():
    rng = np.random.default_rng(7)
    worst, mean = 0, []
    for _ in range(500):
        t_x = int(rng.integers(2, 80))
        w = np.exp(rng.normal(0.8, 0.8, t_x)).astype(np.float32)
        c = np.ceil(w).astype(np.int64)
        d, total, status = DC.plan_row(w, None, int(c.sum()), t_x)
        assert status == 0 and total == c.sum()
        worst = max(worst, int(np.abs(d - c).max()))
        mean.append(np.abs(d - c).mean())
    print(f"fit at the natural total: worst |d - ceil(w)| = {worst}, mean {np.mean(mean):.2f}")
    assert worst <= 2


def test_no_target_is_ceil_and_padding_is_zero():
    w = np.array([[0.2, 1.0, 2.5, 7.01, 3.0]], np.float32)
    d, total, status = DC.plan(w, given=np.array([[-1, 0, -1, 4, 9]]), x_len=[4])
    assert d.tolist() == [[1, 0, 3, 4, 0]] and total.tolist() == [8] and status.tolist() == [0]
    d, total, status = DC.plan(w, target=[0])
    assert d.tolist() == [[1, 1, 3, 8, 3]] and status.tolist() == [0]


def test_infeasible_cases_are_reported():
    w = np.full(4, 1.5, np.float32)
    # E < 0: two pins of 3 and two free tokens need at least 8 frames
    d, total, status = DC.plan_row(w, [3, -1, 3, -1], 7, 4)
    assert status == 1 and d.tolist() == [3, 2, 3, 2] and total == 10
    assert DC.plan_row(w, [3, -1, 3, -1], 8, 4)[1:] == (8, 0)   # E == 0: one frame each
    # nothing free and T != P
    assert DC.plan_row(w, [3, 1, 3, 0], 8, 4)[2] == 1
    d, total, status = DC.plan_row(w, [3, 1, 3, 0], 7, 4)
    assert status == 0 and total == 7 and d.tolist() == [3, 1, 3, 0]
    # past the range of the fit
    assert DC.plan_row(w, None, DC.MAX_TARGET + 1, 4)[2] == 1
    assert DC.plan_row(w, None, DC.MAX_TARGET, 4)[1:] == (DC.MAX_TARGET, 0)


def test_small_cases_match_the_big_integer_restatement():
    """Seven w values (both clamps, a half-way q) x three pins per token x
    seven targets.  EXHAUSTIVE at 1, 2 and 3 tokens (9,723 + 441 + 21
    combinations of w and pins); SAMPLED at 4 and 5 tokens, every 97th and
    every 2999th combination (the full sets are 194,481 and 4,084,101 x 7
    targets: minutes of run time)."""
    ws = [2.0 ** -10, 0.49, 1.0, 385 / 512, 2.75, 40000.0, 3.3e4]
    pins = [-1, 0, 2]
    n = 0
    for t_x in range(1, 6):
        cases = itertools.product(itertools.product(ws, repeat=t_x),
                                  itertools.product(pins, repeat=t_x))
        for k, (w, g) in enumerate(cases):
            if t_x >= 4 and k % (97 if t_x == 4 else 2999):
                continue
            P = sum(v for v in g if v >= 0)
            nF = sum(v < 0 for v in g)
            for T in {0, P, P + nF - 1, P + nF, P + nF + 1, P + nF + 7, 4096}:
                d, total, status = DC.plan_row(np.array(w, np.float32), g, T, t_x)
                d2, status2 = DC.plan_bigint(w, g, T)
                assert d.tolist() == d2 and status == status2, (w, g, T)
                n += 1
    assert n > 8000


def test_a_nan_weight_counts_as_the_smallest_in_a_fit():
    w = np.array([float("nan"), 1.0, 1.0], np.float32)
    d, total, status = DC.plan_row(w, None, 30, 3)
    assert DC.fit_weights(w).tolist() == [1, 128, 128]
    assert status == 0 and total == 30 and d.tolist() == [1, 15, 14]
    assert DC.plan_bigint(w, None, 30) == (d.tolist(), 0)


def test_host_helper_equals_the_oracle():
    rng = np.random.default_rng(99)
    for _ in range(1500):
        t_x = int(rng.integers(1, 50))
        w, given = _random_case(rng, t_x)
        T = int(rng.integers(0, 300))
        d, total, status = DC.plan_row(w, given, T, t_x)
        d2, status2 = D.plan_durations(w, given, T)
        assert np.array_equal(d, d2) and status == status2
    d, status = D.plan_durations(np.array([0.3, 2.2], np.float32))
    assert d.tolist() == [1, 3] and status == 0
    assert D.MAX_TARGET == DC.MAX_TARGET


REFUSED = [
    ("durations of another length", dict(durations=[1, 2, 3])),
    ("two-dimensional durations", dict(durations=[[1, 2, 3, 4]])),
    ("fractional durations", dict(durations=[1, 2.5, 3, 4])),
    ("non-finite durations", dict(durations=[1, float("nan"), 3, 4])),
    ("token_scale of another length", dict(token_scale=[1.0] * 5)),
    ("negative token_scale", dict(token_scale=[1, 1, -0.5, 1])),
    ("non-finite token_scale", dict(token_scale=[1, float("inf"), 1, 1])),
    ("NaN token_scale", dict(token_scale=[1, float("nan"), 1, 1])),
    ("target of 0", dict(target_frames=0)),
    ("target below one frame per token", dict(target_frames=3)),
    ("target below P + |F|", dict(durations=[5, -1, 5, -1], target_frames=11)),
    ("nothing free and T != P", dict(durations=[5, 0, 5, 1], target_frames=12)),
    ("target over 4096 frames", dict(target_frames=4097)),
    ("pinned total over 4096 frames", dict(durations=[2000, 2000, 97, 0])),
    ("one pin over 4096 frames", dict(durations=[5000, -1, -1, -1])),
]


@pytest.mark.parametrize("what,kw", REFUSED, ids=[c[0] for c in REFUSED])
def test_check_controls_refuses(what, kw):
    with pytest.raises(ValueError):
        D.check_controls(4, **kw)


def test_check_controls_accepts_and_knows_the_total():
    assert D.check_controls(4) == (None, None, 0, None)
    g, s, T, known = D.check_controls(4, durations=[5, -3, 0, -1], token_scale=[1, 0, 2, 1],
                                      target_frames=7)
    assert g.dtype == np.int32 and g.tolist() == [5, -1, 0, -1]
    assert s.dtype == np.float32 and (T, known) == (7, 7)
    assert D.check_controls(4, durations=[5, 1, 0, 2])[3] == 8          # all pinned
    assert D.check_controls(4, durations=[5, 1, 0, 2], target_frames=8)[3] == 8
    assert D.check_controls(4, durations=[5, -1, 0, 2])[3] is None      # the device decides
    assert D.check_controls(4, target_frames=4096)[3] == 4096
    assert D.check_controls(4, durations=np.array([1.0, 2.0, -1.0, 0.0]))[0].tolist() == [1, 2, -1, 0]


def test_emovits_refuses_bad_controls_before_touching_its_inputs(tmp_path):
    """EmoVITS.infer / infer_pcm on a CPU stub: a bad control is a ValueError
    raised before the speaker, the emotion or the text are looked at (the
    emotion given here has no bank: reaching the lookup would be an
    AssertionError)."""
    import torch

    from common import tiny_cfg, tiny_model
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    c = tiny_cfg()
    hps = get_hparams_from_dict({"data": dict(c["data"], sampling_rate=16000, hop_length=192,
                                              noise_scale=0.667), "model": c["model"]})
    ev = EmoVITS(str(tmp_path / "ckpt.pth"), torch.device("cpu"), hps=hps, model=tiny_model())
    text = np.zeros((4, c["data"]["text_channels"]), np.float32)
    for what, kw in REFUSED:
        for call in (ev.infer, ev.infer_pcm):
            with pytest.raises(ValueError):
                call(0, text, None, **kw)
    with pytest.raises(AssertionError, match="emotion bank"):
        ev.infer(0, text, None, durations=[1, 2, 3, 4])  # good controls: the lookup is reached


def test_vitswrap_refuses_bad_duration_requests_on_a_stub():
    """VITSWrap on a stub speecher (no model, no GPU): duration controls on a
    text that splits into segments, a duration_s that is no positive time and
    speaking_like without the device output stage are ValueErrors raised before
    the speecher is called."""
    import torch

    from vits_amd.vits_wrap import VITSWrap

    class Speecher:
        device = torch.device("cpu")
        sampling_rate, hop_size = 16000, 192

        def infer(self, *a, **k):
            raise AssertionError("the speecher must not be reached")

        infer_pcm = infer_pcm_like = infer

        def update(self):
            pass

    class Parser:
        max_utt_length = 10

        def __call__(self, utt_id, text):
            return utt_id, text, np.zeros((len(text), 8), np.float32)

    wrap = VITSWrap(textparser=Parser(), speecher=Speecher())
    long_text = "abcdefghi。jklmnopq。rstu"
    for ctl in (dict(durations=[1] * 5), dict(token_scale=[1.0] * 5), dict(duration_s=1.0)):
        with pytest.raises(ValueError, match="segments"):
            wrap.speaking(dict(text=long_text, **ctl))
        with pytest.raises(ValueError, match="segments"):
            wrap.speaking_many([dict(text="abc"), dict(text=long_text, **ctl)][::-1])
    for bad in (0, -1.5, float("nan"), float("inf"), 1e-6):
        with pytest.raises(ValueError, match="duration_s"):
            wrap.speaking(dict(text="hello", duration_s=bad))
    with pytest.raises(ValueError, match="device_post"):
        wrap.speaking_like(dict(text="hello", wav=np.zeros(4000, np.int16), spkid_src=1))
    # a good request reaches the speecher with the frame count of duration_s
    seen = {}

    def infer(spkid, vec, emo, **kw):
        seen.update(kw)
        return np.zeros(84 * 192, np.float32), emo, np.full(5, 17, np.int32)

    wrap.speecher.infer = infer
    out = wrap.speaking(dict(text="hello", duration_s=1.0, token_scale=[1, 1, 2, 1, 1]))
    assert seen["target_frames"] == round(16000 / 192) == 83 and seen["return_durations"] is True
    assert out["durations"].tolist() == [17] * 5
    assert np.allclose(out["boundaries_s"], np.arange(6) * 17 * 192 / 16000)

"""Streaming synthesis, CPU side: the chunk plan (EmoVITS._stream_plan), the
input range of a span of the output stage (ops.resample_span_input) against a
float64 restatement of the tap sum and against scipy, and infer_pcm_stream on
a CPU device.  No GPU."""
import numpy as np
import pytest
import torch
from scipy.signal import firwin, resample_poly

from common import build_model, tiny_cfg
from vits_amd import ops
from vits_amd.infer import PcmStream, _Output

HOP, CTX = 192, 14
RATIOS = [(3200, 2909), (1, 2), (2, 1)]


@pytest.fixture(scope="module")
def ev_cpu(tmp_path_factory):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    c = tiny_cfg()
    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "hop_length": HOP,
                 "text_channels": c["data"]["text_channels"],
                 "n_speakers": c["data"]["n_speakers"], "noise_scale": 0.667},
        "model": c["model"]})
    model = build_model(c["model"], c["data"], "cpu")
    return EmoVITS(str(tmp_path_factory.mktemp("st") / "ckpt.pth"), "cpu", hps=hps, model=model)


# -- the plan ---------------------------------------------------------------------

OUTPUTS = {
    "no pass": _Output(1.0, 16000, 1.0, 0.0, 0, []),
    "pitch 1.1": _Output(1.1, 16000, 1.0, 0.0, 0, [(3200, 2909)]),
    "half rate": _Output(1.0, 8000, 1.0, 0.0, 0, [(1, 2)]),
    "both + tail": _Output(1.1, 8000, 0.8, 0.05, 400, [(3200, 2909), (1, 2)]),
}
SIZES = [(1, 1), (8, 16), (36, 484)]


def _check_plan(plan, y_len, out, first, chunk):
    passes = out.passes or [(1, 1)]
    lens = [y_len * HOP]
    for up, down in passes:
        lens.append(ops.resample_out_len(lens[-1], up, down))
    core, span, size = 0, 0, first
    for k, c in enumerate(plan):
        # the cores partition [0, y_len): first, then doubling up to chunk
        assert c.core_lo == core and c.core_lo < c.core_hi <= y_len
        assert c.core_hi - c.core_lo == min(size, y_len - core)
        core, size = c.core_hi, min(2 * size, chunk)
        # the output spans partition [0, n_out + tail)
        assert c.out_lo == span and c.out_hi >= c.out_lo
        span = c.out_hi
        # the window lies in the utterance, holds the core, and an artificial
        # edge lies at least CTX frames from it
        assert 0 <= c.a <= c.core_lo and c.core_hi <= c.b <= y_len
        assert c.a == 0 or c.core_lo - c.a >= CTX
        assert c.b == y_len or c.b - c.core_hi >= CTX
        # pass i computes [o_lo, o_hi) of its output from [i_lo, i_hi) of its
        # input, which is what resample_span_input asks and lies inside what
        # the stage before provides: the pass before computes exactly it, and
        # the decoder window holds the first pass's with CTX frames to spare
        assert len(c.passes) == len(passes)
        assert c.passes[-1][2:] == (c.out_lo, c.out_hi)
        for i, (i_lo, i_hi, o_lo, o_hi) in enumerate(c.passes):
            assert (i_lo, i_hi) == ops.resample_span_input(o_lo, o_hi, lens[i], *passes[i])
            assert 0 <= i_lo <= i_hi <= lens[i]
            if i > 0:
                assert c.passes[i - 1][2:] == (i_lo, i_hi)
        i_lo, i_hi = c.passes[0][:2]
        if i_lo < i_hi:
            assert c.a * HOP <= i_lo and i_hi <= c.b * HOP
            assert c.a == 0 or i_lo // HOP - c.a >= CTX
            assert c.b == y_len or c.b - -(-i_hi // HOP) >= CTX
        # exactly: the window is no wider than the core, the frames under the
        # first pass's input and CTX frames on each side
        f_lo = min([c.core_lo] + ([i_lo // HOP] if i_lo < i_hi else []))
        f_hi = max([c.core_hi] + ([-(-i_hi // HOP)] if i_lo < i_hi else []))
        assert (c.a, c.b) == (max(0, f_lo - CTX), min(y_len, f_hi + CTX))
    assert core == y_len and span == lens[-1] + out.tail


@pytest.mark.parametrize("name", list(OUTPUTS))
@pytest.mark.parametrize("first,chunk", SIZES)
def test_plan_properties(ev_cpu, name, first, chunk):
    out = OUTPUTS[name]
    for y_len in list(range(1, 201)) + [4096]:
        plan = ev_cpu._stream_plan(y_len, out, first, chunk, CTX)
        _check_plan(plan, y_len, out, first, chunk)
        if y_len <= first:
            assert len(plan) == 1 and (plan[0].a, plan[0].b) == (0, y_len)


def test_plan_cores_of_the_gpu_test(ev_cpu):
    """61 frames at first = 8, chunk = 16: the window of [24, 40) is cut on
    both sides (what tests/test_stream_gpu.py relies on)."""
    plan = ev_cpu._stream_plan(61, OUTPUTS["no pass"], 8, 16, CTX)
    assert [(c.core_lo, c.core_hi) for c in plan] == [(0, 8), (8, 24), (24, 40), (40, 56), (56, 61)]
    assert (plan[2].a, plan[2].b) == (10, 54)
    assert (plan[0].a, plan[-1].b) == (0, 61)


def test_plan_refusals_and_defaults(ev_cpu):
    out = OUTPUTS["no pass"]
    for bad in ((0, 8, 16, CTX), (10, 0, 16, CTX), (10, 8, 0, CTX), (10, 8, 16, -1)):
        with pytest.raises(ValueError):
            ev_cpu._stream_plan(bad[0], out, *bad[1:])
    # the default cores fill windows of 256 and 2048 frames, from the model's own context
    assert ev_cpu.model.dec.context_frames() == CTX
    assert ev_cpu._stream_sizes(None, None, CTX) == (256 - 2 * CTX, 2048 - 2 * CTX)
    assert ev_cpu._stream_sizes(5, None, CTX) == (5, 2048 - 2 * CTX)
    for bad in ((0, None), (None, 0), (-3, 4)):
        with pytest.raises(ValueError):
            ev_cpu._stream_sizes(*bad, CTX)
    text = np.zeros((4, 16), np.float32)
    with pytest.raises(ValueError):  # (before the emotion lookup, which would assert)
        ev_cpu.infer_pcm_stream(0, text, None, chunk_frames=0)


# -- resample_span_input against the tap sum ----------------------------------------


def _filter(up, down):
    hl = 10 * max(up, down)
    return firwin(2 * hl + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up, hl


def _tap_sum(x, h, hl, up, down, n_lo, n_hi, i_lo, i_hi):
    """out[n] = sum_i x[i] * h[n * down - i * up + hl] over the inputs i in
    [i_lo, i_hi) whose tap exists, ascending i, float64: outputs [n_lo, n_hi),
    zero from n_out on."""
    n_out = -(-len(x) * up // down)
    out = np.zeros(n_hi - n_lo)
    for n in range(n_lo, min(n_hi, n_out)):
        acc = 0.0
        for i in range(max(i_lo, -(-(n * down - hl) // up)), min(i_hi, (n * down + hl) // up + 1)):
            acc += x[i] * h[n * down - i * up + hl]
        out[n - n_lo] = acc
    return out


def _spans(n_out):
    """The start, an interior stretch, the end with 7 samples past it."""
    return [(0, 1), (0, 37), (n_out // 2 - 20, n_out // 2 + 21), (n_out - 30, n_out + 7)]


@pytest.mark.parametrize("up,down", RATIOS)
def test_span_input_is_exact(up, down):
    rng = np.random.RandomState(3)
    n_in = 301
    x = rng.randn(n_in)
    h, hl = _filter(up, down)
    n_out = ops.resample_out_len(n_in, up, down)
    for n_lo, n_hi in _spans(n_out):
        i_lo, i_hi = ops.resample_span_input(n_lo, n_hi, n_in, up, down, hl)
        assert 0 <= i_lo < i_hi <= n_in
        whole = _tap_sum(x, h, hl, up, down, n_lo, n_hi, 0, n_in)
        assert np.array_equal(_tap_sum(x, h, hl, up, down, n_lo, n_hi, i_lo, i_hi), whole)
        # one sample more on either side changes nothing
        wide = _tap_sum(x, h, hl, up, down, n_lo, n_hi, max(0, i_lo - 1), min(n_in, i_hi + 1))
        assert np.array_equal(wide, whole)
        # one sample less on either side loses a tap of some output.  (The
        # filter's two end taps are 1e-18: in a sum of terms of order one
        # they drown, so each lost sample is shown alone, as an impulse.)
        for lost, rng_ in ((i_lo, (i_lo + 1, i_hi)), (i_hi - 1, (i_lo, i_hi - 1))):
            e = np.zeros(n_in)
            e[lost] = 1.0
            full = _tap_sum(e, h, hl, up, down, n_lo, n_hi, i_lo, i_hi)
            assert np.any(full != 0.0)
            assert not np.array_equal(_tap_sum(e, h, hl, up, down, n_lo, n_hi, *rng_), full)
    assert ops.resample_span_input(n_out, n_out + 9, n_in, up, down) == (0, 0)  # silence needs nothing


@pytest.mark.parametrize("up,down", RATIOS)
def test_spans_stitch_to_scipy(up, down):
    rng = np.random.RandomState(5)
    n_in = 301
    x = rng.randn(n_in)
    h, hl = _filter(up, down)
    n_out = ops.resample_out_len(n_in, up, down)
    parts, step = [], 53
    for n_lo in range(0, n_out, step):
        n_hi = min(n_out, n_lo + step)
        i_lo, i_hi = ops.resample_span_input(n_lo, n_hi, n_in, up, down)
        # only the window is handed over: a span sees nothing else
        win = np.full(n_in, np.nan)
        win[i_lo:i_hi] = x[i_lo:i_hi]
        parts.append(_tap_sum(win, h, hl, up, down, n_lo, n_hi, i_lo, i_hi))
    got = np.concatenate(parts)
    ref = resample_poly(x, up, down)
    assert got.shape == ref.shape and not np.isnan(got).any()
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_span_input_of_the_copy_and_refusals():
    assert ops.resample_span_input(5, 9, 100, 1, 1) == (5, 9)
    assert ops.resample_span_input(95, 120, 100, 7, 7) == (95, 100)
    assert ops.resample_span_input(100, 120, 100, 1, 1) == (100, 100)
    assert ops.resample_span_input(0, 5, 100, 2, 4) == ops.resample_span_input(0, 5, 100, 1, 2, 20)
    from vits_amd._lib import VitsAmdError

    for bad in ((-1, 5, 100, 1, 2), (6, 5, 100, 1, 2), (0, 5, -1, 1, 2), (0, 5, 100, 0, 2)):
        with pytest.raises(VitsAmdError):
            ops.resample_span_input(*bad)
    with pytest.raises(VitsAmdError):
        ops.resample_span_input(0, 5, 100, 1, 2, 10)  # (not this ratio's half_len)


# -- a CPU device -----------------------------------------------------------------


@pytest.fixture
def stub(ev_cpu, monkeypatch):
    """The model has no CPU path (its layers are HIP kernels), so the
    synthesis under infer_pcm is replaced by a stand-in that does what the
    engine's does to the outside: one draw from numpy's generator, a waveform
    of 61 frames that depends on the draw, the durations on request.  The
    output stage and everything infer_pcm_stream adds are the real code."""
    def infer_one(x_length, text_t, emo, sid, duration_rate, ctl=None, got=None):
        start = np.random.randint(1 << 20)
        if got is not None:
            got.append(np.full(x_length, 61 // x_length, np.int32))
        return (np.random.RandomState(start).rand(61 * HOP).astype(np.float32) * 2 - 1) * 0.9

    monkeypatch.setattr(ev_cpu, "_infer_one", infer_one)
    return ev_cpu


CALLS = [dict(), dict(pitch=1.1, sampling_rate=8000, volume=0.8, tail_silence=0.05)]


@pytest.mark.parametrize("kw", CALLS, ids=["defaults", "pitch rate volume tail"])
def test_cpu_stream_is_infer_pcm_in_slices(stub, kw):
    ev = stub
    text, emo = np.zeros((5, 16), np.float32), torch.zeros(1, 1024)
    np.random.seed(0)
    ref, _, n_model = ev.infer_pcm(1, text, emo, **kw)
    state = np.random.get_state()
    np.random.seed(0)
    stream = ev.infer_pcm_stream(1, text, emo, first_chunk_frames=8, chunk_frames=16, **kw)
    assert isinstance(stream, PcmStream)
    assert (stream.n_samples, stream.n_model, stream.durations) == (len(ref), n_model, None)
    chunks = list(stream)
    assert len(chunks) == 5 and all(c.dtype == np.int16 for c in chunks)
    assert np.array_equal(np.concatenate(chunks), ref)
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    # closed at the first chunk: the generator is where the complete call left
    # it, and the next infer_pcm is what it would have been
    np.random.seed(0)
    stream = ev.infer_pcm_stream(1, text, emo, first_chunk_frames=8, chunk_frames=16, **kw)
    first = next(stream)
    stream.close()
    assert np.array_equal(first, chunks[0])
    with pytest.raises(StopIteration):
        next(stream)
    assert np.array_equal(np.random.get_state()[1], state[1])
    nxt, _, _ = ev.infer_pcm(1, text, emo, **kw)
    np.random.set_state(state)
    assert np.array_equal(ev.infer_pcm(1, text, emo, **kw)[0], nxt)


def test_cpu_stream_reports_durations_under_controls(stub):
    text, emo = np.zeros((5, 16), np.float32), torch.zeros(1, 1024)
    stream = stub.infer_pcm_stream(1, text, emo, target_frames=61)
    assert stream.durations.tolist() == [12] * 5
    assert sum(len(c) for c in stream) == stream.n_samples == 61 * HOP
    assert stub.infer_pcm_stream(1, text, emo, return_durations=True).durations is not None

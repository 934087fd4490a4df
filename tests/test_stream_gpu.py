"""Streaming synthesis on the GPU: the chunks of EmoVITS.infer_pcm_stream,
joined, against infer_pcm of the same call from the same numpy seed, BYTE FOR
BYTE, and VITSWrap.speaking_stream against speaking.

Shapes.  The decoder's context is 14 frames at both configs.  12 tokens
pinned to 61 frames with cores of 8, then 16 frames give the chunks [0, 8)
[8, 24) [24, 40) [40, 56) [56, 61): the window of [24, 40) is the frames
[10, 54), cut on BOTH sides (the case that matters); the first two windows
start at the utterance's start, the last two end at its end.  With pitch 1.1
and 8 kHz the output stage has two passes, each span's input reaches into its
neighbours' samples, and the last chunk carries the tail.  Every window fits
the 64-frame decode graph."""
import numpy as np
import pytest
import torch

from common import base_model, build_model, tiny_cfg
from serve_batch_common import same_state

pytestmark = pytest.mark.gpu

HOP = 192
SIZES = dict(first_chunk_frames=8, chunk_frames=16)
CALLS = [dict(), dict(pitch=1.1, sampling_rate=8000, volume=0.8, tail_silence=0.05)]
CALL_IDS = ["defaults", "pitch rate volume tail"]


def _emovits(device, model, tmp_path, channels, **kw):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "hop_length": HOP, "text_channels": channels,
                 "n_speakers": model.emb_g.num_embeddings, "noise_scale": 0.667},
        "model": {"inter_channels": model.inter_channels}})
    return EmoVITS(str(tmp_path / "ckpt.pth"), device, hps=hps, model=model, **kw)


def _quiesce(ev):
    import gc

    ev._graphs.clear()
    ev._pinned.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _call(device, channels, t_x, seed):
    rs = np.random.RandomState(seed)
    text = rs.randn(t_x, channels).astype(np.float32)
    emo = torch.from_numpy(rs.randn(1, 1024).astype(np.float32)).to(device)
    return 3, text, emo


def _same(chunks, ref, what):
    """Byte equality of the joined chunks with infer_pcm's array; prints
    where they differ first."""
    got = np.concatenate(chunks)
    if got.shape != ref.shape:
        print(f"{what}: {got.shape} samples for {ref.shape}")
        return False
    bad = np.nonzero(got != ref)[0]
    if bad.size:
        d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
        print(f"{what}: {bad.size} of {ref.size} samples differ, {bad[0]} .. {bad[-1]}, max "
              f"{d.max()}")
    return bad.size == 0


def _out(ev, kw):
    return ev._output(kw.get("pitch", 1.0), kw.get("sampling_rate"), kw.get("volume", 1.0),
                      kw.get("tail_silence", 0.0))


def _pair(ev, call, seed, **kw):
    """(infer_pcm's array, the generator's state behind it, the stream of the
    same call from the same seed)."""
    np.random.seed(seed)
    ref, _, n_model = ev.infer_pcm(*call, **{k: v for k, v in kw.items() if k not in SIZES})
    state = np.random.get_state()
    np.random.seed(seed)
    stream = ev.infer_pcm_stream(*call, **kw)
    assert same_state(np.random.get_state(), state)  # (the draw is committed behind the front)
    assert stream.n_samples == len(ref) and stream.n_model == n_model
    return ref, state, stream


# -- the base config in fp32: bitwise --------------------------------------------


@pytest.fixture(scope="module")
def ev_base(device, tmp_path_factory):
    ev = _emovits(device, base_model(device), tmp_path_factory.mktemp("st"), 256, half=False)
    yield ev
    _quiesce(ev)


@pytest.mark.parametrize("kw", CALLS, ids=CALL_IDS)
def test_pinned_61_frames_chunks_equal_infer_pcm(ev_base, device, kw):
    ev = ev_base
    assert ev.model.dec.context_frames() == 14
    call = _call(device, 256, 12, 1)
    ref, state, stream = _pair(ev, call, 7, target_frames=61, **SIZES, **kw)
    assert stream.n_model == 61 * HOP and stream.durations.sum() == 61
    assert len(stream.durations) == 12 and stream.durations.dtype == np.int32
    plan = ev._stream_plan(61, _out(ev, kw), 8, 16, 14)
    assert [(c.core_lo, c.core_hi) for c in plan] == [(0, 8), (8, 24), (24, 40), (40, 56), (56, 61)]
    assert plan[2].a > 0 and plan[2].b < 61
    chunks = list(stream)
    assert [len(c) for c in chunks] == [c.out_hi - c.out_lo for c in plan]
    assert all(c.dtype == np.int16 for c in chunks) and np.abs(ref).max() > 100  # not silent
    assert _same(chunks, ref, "pinned")
    assert same_state(np.random.get_state(), state)
    assert ("dec", 64) in ev._graphs and any(k[:2] == ("front", "ctl") for k in ev._graphs)


def test_the_comparison_needs_the_context(ev_base, device, monkeypatch):
    """The same call with 2 frames of context instead of 14 does NOT
    reproduce infer_pcm: the test above can fail."""
    ev = ev_base
    call = _call(device, 256, 12, 1)
    monkeypatch.setattr(ev.model.dec, "context_frames", lambda: 2)
    ref, _, stream = _pair(ev, call, 7, target_frames=61, **SIZES)
    got = np.concatenate(list(stream))
    assert got.shape == ref.shape and not np.array_equal(got, ref)


@pytest.mark.parametrize("kw", CALLS, ids=CALL_IDS)
def test_predicted_length_chunks_equal_infer_pcm(ev_base, device, kw):
    """No duration control: the uncontrolled front graph, at whatever length
    the predictor gives."""
    ev = ev_base
    call = _call(device, 256, 48, 2)
    ref, state, stream = _pair(ev, call, 9, **SIZES, **kw)
    frames = stream.n_model // HOP
    print(f"predicted length: {frames} frames")
    assert stream.durations is None and frames > 24  # (at least three chunks)
    chunks = list(stream)
    assert len(chunks) == len(ev._stream_plan(frames, _out(ev, kw), 8, 16, 14))
    assert _same(chunks, ref, "predicted")
    assert same_state(np.random.get_state(), state)
    assert any(k[0] == "front" and k[1] != "ctl" for k in ev._graphs)


def test_eager_engine_streams_the_same_bytes(ev_base, device):
    """graph=False: the same plan through the eager functions."""
    ev = ev_base
    call = _call(device, 256, 12, 1)
    ev.graph = False
    try:
        ref, state, stream = _pair(ev, call, 7, target_frames=61, **SIZES, **CALLS[1])
        assert _same(list(stream), ref, "eager")
        assert same_state(np.random.get_state(), state)
    finally:
        ev.graph = True


# -- the tiny config in fp16, graphs on --------------------------------------------


@pytest.fixture(scope="module")
def ev_tiny(device, tmp_path_factory):
    c = tiny_cfg()
    ev = _emovits(device, build_model(c["model"], c["data"], device),
                  tmp_path_factory.mktemp("st_tiny"), c["data"]["text_channels"])
    yield ev
    _quiesce(ev)


def test_tiny_fp16_graphs_bytes_replays_and_early_close(ev_tiny, device):
    ev = ev_tiny
    assert ev.dtype == torch.float16 and ev.graph
    call = _call(device, 16, 12, 4)
    kw = dict(target_frames=61, **SIZES, **CALLS[1])
    ref, state, stream = _pair(ev, call, 3, **kw)
    chunks = list(stream)
    assert len(chunks) == 5 and np.abs(ref).max() > 0
    assert _same(chunks, ref, "tiny fp16")
    # a second call replays the cached graphs: nothing is captured
    graphs = dict(ev._graphs)
    assert ("dec", 64) in graphs
    ref2, _, stream2 = _pair(ev, call, 5, **kw)
    assert _same(list(stream2), ref2, "tiny fp16, second call")
    assert set(ev._graphs) == set(graphs) and all(ev._graphs[k] is graphs[k] for k in graphs)
    # closed at the first chunk: the engine goes on as after a complete call
    np.random.seed(3)
    ev.infer_pcm(*call, **{k: v for k, v in kw.items() if k not in SIZES})
    after = ev.infer_pcm(*call, **CALLS[1])[0]
    np.random.seed(3)
    stream = ev.infer_pcm_stream(*call, **kw)
    first = next(stream)
    stream.close()
    assert np.array_equal(first, chunks[0])
    assert same_state(np.random.get_state(), state)
    assert np.array_equal(ev.infer_pcm(*call, **CALLS[1])[0], after)
    # two streams taken in turns do not disturb each other
    np.random.seed(3)
    a = ev.infer_pcm_stream(*call, **kw)
    b = ev.infer_pcm_stream(*call, **dict(kw, target_frames=40))
    got_a, got_b = [], []
    for x in a:
        got_a.append(x)
        got_b += [y for y in [next(b, None)] if y is not None]
    got_b += list(b)
    assert _same(got_a, ref, "tiny fp16, interleaved")
    assert sum(len(x) for x in got_b) == b.n_samples


@pytest.mark.parametrize("batch", [False, True], ids=["one by one", "batch_segments"])
def test_speaking_stream_equals_speaking(ev_tiny, batch):
    from vits_amd import vits_wrap

    bank = np.random.RandomState(0).randn(3, 1024).astype(np.float32)

    class Parser:
        max_utt_length = 10

        def __call__(self, utt_id, text):
            rs = np.random.RandomState(len(text))
            return utt_id, text, rs.randn(max(1, len(text)), 16).astype(np.float32)

    def request():
        # (no emotion id: the lookup draws it, before every noise draw)
        return {"id": "u", "text": "abcdefghi。jklmnopq。rstu", "spkid": 1, "emotion": (bank,),
                "sampling_rate": 22050, "pitch": 1.2, "tail_silence": 0.02, **SIZES}

    wrap = vits_wrap.VITSWrap(textparser=Parser(), speecher=ev_tiny, device_post=True,
                              batch_segments=batch)
    assert wrap.batch_segments is batch
    np.random.seed(23)
    want = wrap.speaking(request())
    state = np.random.get_state()
    assert len(want["segment_info"]) == 3
    np.random.seed(23)
    items = list(wrap.speaking_stream(request()))
    assert same_state(np.random.get_state(), state)
    assert items[0] == want["wav"][:44] and items[0][:4] == b"RIFF" and len(items) > 4
    assert all(isinstance(i, bytes) for i in items)
    assert b"".join(items) == want["wav"]
    # one segment under a duration control
    np.random.seed(24)
    want = wrap.speaking(dict(request(), text="abcdefghi", duration_s=61 * HOP / 16000))
    np.random.seed(24)
    items = list(wrap.speaking_stream(dict(request(), text="abcdefghi",
                                           duration_s=61 * HOP / 16000)))
    assert len(items) == 6 and b"".join(items) == want["wav"]
    plain = vits_wrap.VITSWrap(textparser=Parser(), speecher=ev_tiny)
    with pytest.raises(ValueError, match="device_post"):
        plain.speaking_stream(request())


# -- the base config in fp16: the front is exact, the decoder to its rounding ------


def test_base_fp16_front_and_windows_are_the_whole_calls_z(device, monkeypatch):
    """The 16-bit decoder depends on where a frame lies in its row (DESIGN.md
    4t, up to 3.8e-4), and a streamed window starts at another row position
    than the whole utterance, so the PCM is not asserted here: what is
    asserted is everything in front of the decoder.  The z the whole call
    hands its decoder, the front's z and the windows that reach the decode
    graph's input are the same bits.  The PCM difference is printed and
    recorded in profiles/stream_latency.txt."""
    from vits_amd import engine, ops

    model = base_model(device)
    model.remove_weight_norm()
    model = model.half().eval()
    t_x, t_y, C = 12, 256, 192
    g = torch.Generator().manual_seed(11)
    x = torch.zeros(1, 32, 256)
    x[:, :t_x] = torch.randn(1, t_x, 256, generator=g)
    x = x.half().to(device)
    emo = torch.randn(1, 1024, generator=g).half().to(device)
    sid = torch.tensor([5], device=device)
    noise = (torch.randn(1, C, t_y, generator=g) * 0.667).to(device)
    xl = torch.tensor([t_x], dtype=torch.int32, device=device)
    ctl = dict(target=torch.tensor([61], dtype=torch.int32, device=device))
    seen = []
    run = engine.GeneratorPlan.run

    def spy(self, z, *a, **k):
        seen.append(z.clone())
        return run(self, z, *a, **k)

    monkeypatch.setattr(engine.GeneratorPlan, "run", spy)
    wav, y_len, _, _ = model.infer_bucketed(x, emo, sid, noise, t_y, x_lengths=xl, control=ctl)
    monkeypatch.undo()
    z, gg, y_len_f, _, _ = model.infer_front_bucketed(x, emo, sid, noise, t_y, x_lengths=xl,
                                                      control=ctl)
    torch.cuda.synchronize()
    assert int(y_len[0]) == int(y_len_f[0]) == 61 and len(seen) == 1
    assert z.dtype == torch.float32 and torch.equal(z, seen[0])
    assert z[:, :, :61].abs().max() > 0.1 and not z[:, :, 61:].any()

    class Ev:  # (the plan needs the hop alone)
        hop_size = HOP

    from vits_amd.infer import EmoVITS, _Output

    plan = EmoVITS._stream_plan(Ev, 61, _Output(1.0, 16000, 1.0, 0.0, 0, []), 8, 16, 14)
    worst, bad, total = 0.0, 0, 0
    for c in plan:
        w = c.b - c.a
        z_win = torch.full((1, C, 64), float("nan"), device=device)
        ops.copy_windows(z, z_win, [(c.a, 0, w, 64)], channels=C, src_rstride=t_y, dst_rstride=64)
        assert torch.equal(z_win[:, :, :w], seen[0][:, :, c.a:c.b]) and not z_win[:, :, w:].any()
        o = model.decode_window_bucketed(z_win, torch.tensor([w], dtype=torch.int32, device=device),
                                         gg)
        assert o.dtype == torch.float16 and tuple(o.shape) == (1, 1, 64 * HOP)
        lo, hi = c.core_lo * HOP, c.core_hi * HOP
        d = (o[0, 0, lo - c.a * HOP:hi - c.a * HOP].float() - wav[0, 0, lo:hi].float()).abs()
        worst, bad, total = max(worst, d.max().item()), bad + int((d > 0).sum()), total + d.numel()
    print(f"base fp16, 61 frames: streamed against whole waveform, max difference {worst:.3e}, "
          f"{bad} of {total} samples differ")
    assert np.isfinite(worst)

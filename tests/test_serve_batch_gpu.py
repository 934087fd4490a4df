"""Batched serving on the GPU: all segments of a request in one utterance
graph (ops.draw_starts, vits_expand_durations mode 2, ops.pack_pcm,
SynthesizerTrn.capture_infer_bucketed(batch=...), EmoVITS.infer_batch /
infer_pcm_batch, VITSWrap(batch_segments=True)).

Every kernel on the path maps one utterance to its own workgroups, so a row
of a batch is computed exactly as the same utterance alone: the comparisons
with the B = 1 paths are BITWISE, and numpy's generator must end in the state
the one-by-one calls leave it in."""
import json
import math

import numpy as np
import pytest
import torch

from common import base_model, build_model, tiny_cfg
from serve_batch_common import same_state, shared_pool_draw

pytestmark = pytest.mark.gpu


# -- kernels -------------------------------------------------------------------

def _draw_case(device):
    """B = 5, C = 8, t_x = 6: y_len = [48, 12, 1, 40, 33]."""
    logw = torch.empty(5, 1, 6, device=device)
    logw[0] = math.log(7.5)            # 6 x 8
    logw[1] = math.log(1.5)            # 6 x 2
    logw[2] = float("-inf")            # 6 x 0 -> clamped to 1
    logw[3] = math.log(7.5)            # x_len 5: 5 x 8
    logw[4] = math.log(10.5)           # x_len 3: 3 x 11
    x_len = torch.tensor([6, 6, 6, 5, 3], dtype=torch.int32, device=device)
    return logw, x_len, [48, 12, 1, 40, 33]


def test_draw_starts_equals_sequential_numpy_randint(device):
    from vits_amd import ops

    logw, x_len, want_len = _draw_case(device)
    C, noise_len = 8, 8 * 48 + 1  # row 0: one possible start, no word consumed
    highs = [noise_len - C * n for n in want_len]
    np.random.seed(3)
    want = [np.random.randint(h) for h in highs]
    want_state = np.random.get_state()
    np.random.seed(3)
    pool, state = ops.numpy_draw_pool(32 * 5)
    pool_d = torch.from_numpy(pool).to(device)
    starts, y_len, status, used = ops.draw_starts(logw, C, noise_len, pool_d, x_len=x_len)
    assert y_len.tolist() == want_len
    assert starts.dtype == torch.int64 and starts.tolist() == want
    status = status.tolist()
    assert status[0] == 0 and min(status) >= 0 and sum(status) == int(used)
    assert (starts.tolist(), status, int(used)) == shared_pool_draw(pool, highs)
    ops.numpy_draw_commit(state, int(used))
    assert same_state(np.random.get_state(), want_state)
    # rows 3 and 4 as the padding of a batch bucket: they draw nothing
    for n_rows in (3, torch.tensor([3], dtype=torch.int32, device=device)):
        s3, y3, st3, used3 = ops.draw_starts(logw, C, noise_len, pool_d, x_len=x_len, n_rows=n_rows)
        assert s3.tolist()[:3] == want[:3] and y3.tolist() == want_len
        assert st3.tolist() == status[:3] + [0, 0] and int(used3) == sum(status[:3])


def _guarded_noise(device, noise_len, guard=256):
    full = torch.full((guard + noise_len + guard,), 1e30, device=device)
    full[guard:guard + noise_len] = torch.randn(noise_len, device=device)
    return full, full[guard:guard + noise_len], guard


def _check_guards(full, guard, z):
    assert torch.all(full[:guard] == 1e30) and torch.all(full[-guard:] == 1e30)
    assert torch.isfinite(z).all() and z.abs().max().item() < 1e6  # no guard value was read


def test_draw_status_pool_exhausted(device):
    """Every word 0xFFFFFFFF with rng = 5 (mask 7 -> 7 > 5): all rejected, the
    pool runs out: status -2, z = 0, no noise element read."""
    from vits_amd import ops

    B, C, t_x, t_y = 2, 8, 6, 64
    logw = torch.full((B, 1, t_x), math.log(1.5), device=device)  # 12 frames each
    noise_len = C * 12 + 6
    full, noise, guard = _guarded_noise(device, noise_len)
    pool = torch.full((16,), -1, dtype=torch.int32, device=device)
    starts, y_len, status, used = ops.draw_starts(logw, C, noise_len, pool)
    assert y_len.tolist() == [12, 12] and status.tolist() == [-2, -2]
    assert starts.tolist() == [-1, -1]
    m_p = torch.randn(B, C, t_x, device=device)
    s_p = torch.rand(B, C, t_x, device=device) + 0.5
    z, lens = ops.expand_durations(logw, m_p, s_p, noise, t_y, starts=starts, stage_mult=(1, 2))
    assert lens.shape == (2, B) and lens[0].tolist() == [12, 12] and lens[1].tolist() == [24, 24]
    assert torch.count_nonzero(z).item() == 0
    _check_guards(full, guard, z)


def test_draw_status_slice_does_not_fit(device):
    """A row whose C * y_len > noise_len: status -1, nothing consumed, z = 0;
    the row after it draws from where the row before it stopped."""
    from vits_amd import ops

    B, C, t_x, t_y = 3, 8, 6, 64
    logw = torch.full((B, 1, t_x), math.log(1.5), device=device)  # 12 frames
    logw[1] = math.log(7.5)                                        # 48 frames
    noise_len = C * 40
    full, noise, guard = _guarded_noise(device, noise_len)
    np.random.seed(8)
    want = [np.random.randint(noise_len - C * 12) for _ in range(2)]
    want_state = np.random.get_state()
    np.random.seed(8)
    pool, state = ops.numpy_draw_pool(32 * B)
    starts, y_len, status, used = ops.draw_starts(logw, C, noise_len,
                                                  torch.from_numpy(pool).to(device))
    assert y_len.tolist() == [12, 48, 12]
    assert starts.tolist() == [want[0], -1, want[1]]
    assert status.tolist()[1] == -1 and int(used) == status[0].item() + status[2].item()
    ops.numpy_draw_commit(state, int(used))
    assert same_state(np.random.get_state(), want_state)
    m_p = torch.randn(B, C, t_x, device=device)
    s_p = torch.rand(B, C, t_x, device=device) + 0.5
    z, _ = ops.expand_durations(logw, m_p, s_p, noise, t_y, starts=starts)
    _check_guards(full, guard, z)
    assert torch.count_nonzero(z[1]).item() == 0
    tok = torch.arange(12, device=device) // 2  # 2 frames per token
    for b, s in ((0, want[0]), (2, want[1])):
        n = noise[s:s + C * 12].view(C, 12)
        ref = m_p[b][:, tok] + n * s_p[b][:, tok]
        assert torch.allclose(z[b, :, :12], ref, rtol=1e-6, atol=1e-6)  # (fma contraction)
        assert torch.count_nonzero(z[b, :, 12:]).item() == 0


def test_expand_durations_explicit_start_equals_device_draw(device):
    from vits_amd import ops

    B, C, t_x, t_y = 1, 8, 37, 256
    g = torch.Generator().manual_seed(4)
    logw = (torch.rand(B, 1, t_x, generator=g) * 2 - 0.5).to(device)
    m_p = torch.randn(B, C, t_x, generator=g).to(device)
    s_p = (torch.rand(B, C, t_x, generator=g) + 0.5).to(device)
    noise = torch.randn(C * 4096, generator=g).to(device)
    np.random.seed(6)
    pool, _ = ops.numpy_draw_pool()
    kw = dict(rate=1.1, noise_scale=0.9, stage_mult=(1, 1, 8))
    z1, lens1 = ops.expand_durations(logw, m_p, s_p, noise, t_y,
                                     noise_start=torch.from_numpy(pool).to(device).view(1, -1), **kw)
    y_len, used = int(lens1[0, 0]), int(lens1[3, 0])
    assert 1 < y_len <= t_y and used >= 1
    start, status, _ = shared_pool_draw(pool, [noise.numel() - C * y_len])
    assert status == [used]
    z2, lens2 = ops.expand_durations(logw, m_p, s_p, noise, t_y,
                                     starts=torch.tensor(start, dtype=torch.int64, device=device),
                                     **kw)
    assert lens2.shape == (3, 1) and torch.equal(lens2, lens1[:3])
    assert torch.equal(z1, z2) and torch.count_nonzero(z2).item() > 0


@pytest.mark.parametrize("tail", [0, 7])
@pytest.mark.parametrize("passes", [[], [(5, 6)], [(5, 6), (1, 2)]], ids=["none", "one", "two"])
def test_pack_pcm(device, passes, tail):
    from vits_amd import ops

    B, hop, cap = 3, 192, 3 * 192 + 24
    g = torch.Generator().manual_seed(9)
    rows = torch.randint(-30000, 30000, (B, cap), generator=g, dtype=torch.int16).to(device)
    y_len = torch.tensor([3, 1, 2], dtype=torch.int32, device=device)
    n_rows = torch.tensor([B], dtype=torch.int32, device=device)
    header = ops.pack_header_len(B)
    out = torch.empty(header + B * (cap + tail) + 64, dtype=torch.int16, device=device)

    def expect(frames, n):
        offs, parts = [0], []
        for b in range(B):
            if b < n:
                n_out = frames[b] * hop
                for up, down in passes:
                    n_out = ops.resample_out_len(n_out, up, down)
                parts += [rows[b, :n_out].cpu(), torch.zeros(tail, dtype=torch.int16)]
                offs.append(offs[-1] + n_out + tail)
            else:
                offs.append(offs[-1])
        return offs, torch.cat(parts)

    def body():
        return ops.pack_pcm(rows, y_len, hop, passes, tail, n_rows=n_rows, out=out)

    body()  # (eager once: nothing in it allocates with out given)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, offsets, stream = body()
    for frames, n in (([3, 1, 2], 3), ([1, 3, 2], 3), ([2, 3, 1], 2)):
        y_len.copy_(torch.tensor(frames, dtype=torch.int32))
        n_rows.fill_(n)
        out.fill_(12345)
        graph.replay()
        offs, want = expect(frames, n)
        assert offsets.tolist() == offs
        got = stream.cpu()
        assert torch.equal(got[:offs[-1]], want)
        assert torch.all(got[offs[-1]:] == 12345)             # nothing past offset[B]
        assert torch.all(out[2 * (B + 1):header] == 12345)     # nor between offsets and stream


# -- model ---------------------------------------------------------------------

def _quiesce():
    """Leave the process as the module found it: graphs destroyed, no work
    in flight, cached device memory returned."""
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def base(device):
    yield base_model(device)
    _quiesce()


def _rows(device, lengths, seed0):
    """Padded [n, max, 256] text, emo [n, 1024], sid [n] and the B = 1 pieces."""
    from test_infer_bucketed_gpu import _inputs

    ones = [_inputs(device, t, seed0 + i)[:3] for i, t in enumerate(lengths)]
    x = torch.zeros(len(lengths), max(lengths), 256, device=device)
    for i, (xi, _, _) in enumerate(ones):
        x[i, :lengths[i]] = xi[0]
    return x, torch.cat([o[1] for o in ones]), torch.cat([o[2] for o in ones]), ones


def test_infer_bucketed_batch_rows_equal_single_utterances(base, device):
    from test_infer_bucketed_gpu import _eager

    lengths, t_y = [37, 12, 23], 512
    x, emo, sid, ones = _rows(device, lengths, 40)
    xp = torch.zeros(3, 64, 256, device=device)
    xp[:, :x.shape[1]] = x
    noise = (torch.randn(3, 192, t_y, generator=torch.Generator().manual_seed(1)) * 0.707).to(device)
    wav, yl = base.infer_bucketed(xp, emo, sid, noise, t_y,
                                  x_lengths=torch.tensor(lengths, dtype=torch.int32))
    torch.cuda.synchronize()
    assert wav.shape == (3, 1, t_y * 192)
    for i, (xi, ei, si) in enumerate(ones):
        ref, y_len = _eager(base, xi, ei, si, noise[i:i + 1])
        assert int(yl[i]) == y_len <= t_y
        assert torch.equal(wav[i:i + 1, :, :y_len * 192], ref), i


def test_batched_graph_rows_equal_single_graph(base, device):
    """One graph for up to 4 utterances, replayed with 3 rows then with 2
    shorter ones: each row is bitwise the B = 1 graph's result from the same
    words, padding rows draw nothing, nothing stale leaks in."""
    from vits_amd import ops

    noise_len = 192 * 4096
    noise = torch.randn(noise_len, generator=torch.Generator().manual_seed(2)).to(device) * 0.707
    run4 = base.capture_infer_bucketed(64, 512, batch=4, padded_text=True, noise_len=noise_len)
    run1 = base.capture_infer_bucketed(64, 512, padded_text=True, noise_len=noise_len)
    run4.static["noise"].copy_(noise)
    run1.static["noise"].copy_(noise)
    assert run4.pool_len == ops.ED_DRAWS * 4
    np.random.seed(5)
    for lengths, seed0 in (([37, 12, 23], 50), ([9, 17], 60)):
        n = len(lengths)
        x, emo, sid, ones = _rows(device, lengths, seed0)
        pool, state = ops.numpy_draw_pool(run4.pool_len)
        wav, y_len, status, used = run4(x, emo, sid, lengths, pool, n)
        wav, y_len, status = wav.clone(), y_len.tolist(), status.tolist()
        assert y_len[n:] == [1] * (4 - n) and status[n:] == [0] * (4 - n)
        assert min(status[:n]) >= 1 and int(used) == sum(status[:n])
        pos = 0
        for i, (xi, ei, si) in enumerate(ones):
            words = np.zeros(ops.ED_DRAWS, dtype=np.int32)
            part = pool[pos:pos + ops.ED_DRAWS]
            words[:len(part)] = part
            ref, yl = run1(xi, ei, si, noise_start=words, x_length=lengths[i])
            assert yl[:, 0].tolist() == [y_len[i], status[i]]
            assert 1 < y_len[i] <= 512
            assert torch.equal(wav[i:i + 1, :, :y_len[i] * 192], ref[:, :, :y_len[i] * 192]), i
            pos += status[i]
        ops.numpy_draw_commit(state, int(used))


# -- EmoVITS / VITSWrap on the tiny checkpoint -----------------------------------

@pytest.fixture(scope="module")
def tts(tmp_path_factory, device):
    """tests/test_wrappers.py's tiny checkpoint: 16 kHz, hop 192."""
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import deterministic_fill_

    root = tmp_path_factory.mktemp("serve_ckpt")
    c = tiny_cfg()
    hps = {"train": {"segment_size": c["data"]["segment_size"] * 192},
           "data": {"text_channels": c["data"]["text_channels"],
                    "filter_length": (c["data"]["spec_channels"] - 1) * 2, "hop_length": 192,
                    "n_speakers": c["data"]["n_speakers"], "sampling_rate": 16000,
                    "noise_scale": 0.707},
           "model": c["model"]}
    with open(root / "config.json", "w") as f:
        json.dump(hps, f)
    m = build_model(c["model"], c["data"], fill=False)
    deterministic_fill_(m, seed=100)
    torch.save({"model": m.state_dict(), "iteration": 0}, root / "G_1000.pth")
    np.random.RandomState(0).randn(3, 1024).astype(np.float32).tofile(root / "1.emo")
    ev = EmoVITS(str(root / "G_1000.pth"), device)
    yield ev
    ev._graphs.clear()
    ev._pinned.clear()
    del ev
    _quiesce()


def _items(device, lengths=(9, 4, 14)):
    channels = tiny_cfg()["data"]["text_channels"]
    rs = np.random.RandomState(17)
    return [(1, rs.randn(n, channels).astype(np.float32),
             torch.from_numpy(rs.randn(1, 1024).astype(np.float32)).half().to(device))
            for n in lengths]


@pytest.mark.parametrize("max_batch", [16, 2])
def test_infer_batch_equals_the_loop_over_infer(tts, device, monkeypatch, max_batch):
    items = _items(device)
    np.random.seed(21)
    want = [tts.infer(*it) for it in items]
    want_state = np.random.get_state()
    monkeypatch.setattr(type(tts), "MAX_BATCH", max_batch)
    np.random.seed(21)
    got = tts.infer_batch(items)
    assert same_state(np.random.get_state(), want_state)
    assert len(got) == len(want)
    for (w, e), (gw, ge), it in zip(want, got, items):
        assert gw.dtype == np.float32 and gw.shape == w.shape and len(w) % 192 == 0 and len(w) > 0
        assert np.array_equal(gw, w) and np.abs(w).max() > 0
        assert torch.equal(ge, e) and torch.equal(ge, it[2])
    assert any(len(k) == 4 for k in tts._graphs)  # a batched graph was used


def test_exhausted_pool_reruns_with_a_pool_twice_as_long(tts, device, monkeypatch):
    """A first pool whose every word is rejected (0xFFFFFFFF: the masked
    value exceeds any range that is not 2^k - 1): status -2, the generator is
    restored and the group runs again on 2 P real words - same result, same
    final state as the loop."""
    from vits_amd import ops

    items = _items(device)
    np.random.seed(24)
    want = [tts.infer(*it)[0] for it in items]
    want_state = np.random.get_state()
    real, calls = ops.numpy_draw_pool, []

    def draw_pool(n=ops.ED_DRAWS):
        words, state = real(n)
        calls.append(n)
        return (np.full(n, -1, dtype=np.int32) if len(calls) == 1 else words), state

    monkeypatch.setattr(ops, "numpy_draw_pool", draw_pool)
    np.random.seed(24)
    got = tts.infer_batch(items)
    assert calls == [ops.ED_DRAWS * 4, ops.ED_DRAWS * 8]
    assert same_state(np.random.get_state(), want_state)
    assert all(np.array_equal(g, w) for (g, _), w in zip(got, want))


def test_a_segment_that_does_not_fit_the_noise_buffer_raises(tts, device, monkeypatch):
    items = _items(device)
    np.random.seed(25)
    state = np.random.get_state()
    monkeypatch.setattr(tts, "noise", tts.noise[:8])  # no slice fits 8 samples
    monkeypatch.setattr(tts, "_graphs", {})
    with pytest.raises(ValueError, match="does not fit"):
        tts.infer_batch(items)
    assert same_state(np.random.get_state(), state)


@pytest.mark.parametrize("kw", [{}, dict(pitch=1.2, sampling_rate=8000, volume=0.7,
                                         tail_silence=0.01)], ids=["defaults", "resampled"])
def test_infer_pcm_batch_equals_the_loop_over_infer_pcm(tts, device, kw):
    items = _items(device)
    np.random.seed(22)
    want = [tts.infer_pcm(*it, **kw) for it in items]
    want_state = np.random.get_state()
    np.random.seed(22)
    pcm, offsets, emos, n_model = tts.infer_pcm_batch(items, **kw)
    assert same_state(np.random.get_state(), want_state)
    assert pcm.dtype == np.int16 and pcm.ndim == 1
    assert offsets.tolist() == np.cumsum([0] + [len(w[0]) for w in want]).tolist()
    assert n_model == [w[2] for w in want]
    for i, (w, e, _) in enumerate(want):
        seg = pcm[offsets[i]:offsets[i + 1]]
        assert np.array_equal(seg, w) and np.abs(seg).max() > 0
        assert torch.equal(emos[i], e)
    assert len(pcm) == offsets[-1]


def test_vitswrap_batch_segments_equals_device_post(tts, monkeypatch):
    from vits_amd import vits_wrap

    channels = tiny_cfg()["data"]["text_channels"]

    class Parser:
        max_utt_length = 10

        def __call__(self, utt_id, text):
            rs = np.random.RandomState(len(text))
            return utt_id, text, rs.randn(max(1, len(text)), channels).astype(np.float32)

    def request():
        return {"id": "u", "text": "abcdefghi。jklmnopq。rstu", "spkid": 1, "sampling_rate": 22050,
                "pitch": 1.2, "tail_silence": 0.02}

    seq = vits_wrap.VITSWrap(textparser=Parser(), speecher=tts, device_post=True)
    bat = vits_wrap.VITSWrap(textparser=Parser(), speecher=tts, batch_segments=True)
    assert seq.batch_segments is False and bat.batch_segments is True and bat.device_post is True
    np.random.seed(23)
    a = seq.speaking(request())
    state_a = np.random.get_state()

    def no_host_resampling(*args, **kwargs):
        raise AssertionError("batch_segments=True must not resample on the host")

    monkeypatch.setattr(vits_wrap, "_resample", no_host_resampling)
    np.random.seed(23)
    b = bat.speaking(request())
    assert same_state(np.random.get_state(), state_a)
    assert a["wav"] == b["wav"] and len(b["wav"]) > 44
    assert a["segment_info"] == b["segment_info"] and len(b["segment_info"]) == 3
    assert a["sr"] == b["sr"] == 22050
    assert b["rtf"] > 0 and b["time_used_backend"] > 0 and b["time_used_frontend"] >= 0
    assert set(a) == set(b)
    assert np.abs(np.frombuffer(b["wav"][44:], dtype=np.int16)).max() > 0

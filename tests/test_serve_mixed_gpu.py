"""Mixed requests in one graph: per-row speed (ops.expand_durations /
draw_starts with ``rate`` as a tensor), the per-row output stage
(ops.resample_rows, ops.pack_pcm_rows), EmoVITS.infer_pcm_requests and
VITSWrap.speaking_many.

The reference of every per-row kernel is the existing uniform kernel called
once per row (tests/test_post_gpu.py and tests/test_serve_batch_gpu.py pin
those to the float64 closed form, the host expression and numpy's generator).
The per-row kernels run the same code on the same operands, so every
comparison here is BITWISE."""
import json

import numpy as np
import pytest
import torch

from common import build_model, tiny_cfg
from serve_batch_common import same_state, shared_pool_draw

pytestmark = pytest.mark.gpu


# -- per-row speed ------------------------------------------------------------------

RATES = (0.5, 1.0, 1.37, 2.0)


@pytest.mark.parametrize("half_round", [False, True], ids=["fp32", "half_round"])
def test_rate_tensor_rows_equal_the_scalar_calls(device, half_round):
    """B = 4, t_x = 12, C = 4, t_y = 64; exp(logw) <= 2.46, so a row has at
    most 12 * ceil(2.46 * 2) = 60 frames.  Row 3 is the padding of the batch
    (n_rows = 3): it draws nothing, its length and its z are still its own."""
    from vits_amd import ops

    B, t_x, C, t_y, n_rows, guard = 4, 12, 4, 64, 3, 256
    g = torch.Generator().manual_seed(31)
    logw = (torch.rand(B, 1, t_x, generator=g) * 1.4 - 0.5).to(device)
    m_p = torch.randn(B, C, t_x, generator=g).to(device)
    s_p = (torch.rand(B, C, t_x, generator=g) + 0.5).to(device)
    x_len = torch.tensor([12, 7, 12, 9], dtype=torch.int32, device=device)
    noise_len = C * t_y + 37
    full = torch.full((guard + noise_len + guard,), 1e30, device=device)
    full[guard:guard + noise_len] = torch.randn(noise_len, generator=g).to(device)
    noise = full[guard:guard + noise_len]
    rates = torch.tensor(RATES, dtype=torch.float32, device=device)
    np.random.seed(32)
    pool, _ = ops.numpy_draw_pool(ops.ED_DRAWS * B)
    pool_d = torch.from_numpy(pool).to(device)
    kw = dict(half_round=half_round)

    starts, y_len, status, used = ops.draw_starts(logw, C, noise_len, pool_d, rate=rates,
                                                  x_len=x_len, n_rows=n_rows, **kw)
    z, lens = ops.expand_durations(logw, m_p, s_p, noise, t_y, rate=rates, x_len=x_len,
                                   starts=starts, stage_mult=(1, 2), noise_scale=0.9, **kw)
    assert lens.shape == (2, B) and torch.equal(lens[0], y_len) and torch.equal(lens[1], 2 * y_len)
    pos, y_rows = 0, []
    for b, r in enumerate(RATES):
        one = slice(b, b + 1)
        s1, y1, st1, u1 = ops.draw_starts(logw[one], C, noise_len, pool_d[pos:], rate=r,
                                          x_len=x_len[one], n_rows=1 if b < n_rows else 0, **kw)
        assert (starts[b].item(), y_len[b].item(), status[b].item()) == \
            (s1.item(), y1.item(), st1.item()), b
        assert st1.item() >= (1 if b < n_rows else 0)
        z1, l1 = ops.expand_durations(logw[one], m_p[one], s_p[one], noise, t_y, rate=r,
                                      x_len=x_len[one], starts=s1, stage_mult=(1, 2),
                                      noise_scale=0.9, **kw)
        assert torch.equal(z[one], z1) and torch.equal(lens[:, one], l1), b
        assert torch.count_nonzero(z1).item() > 0 and 1 < y1.item() <= t_y
        pos += int(u1)  # words this row used
        y_rows.append(y1.item())
    assert int(used) == pos
    y_at_1 = ops.draw_starts(logw, C, noise_len, pool_d, x_len=x_len, **kw)[1].tolist()
    assert y_rows[0] < y_at_1[0] and y_rows[1] == y_at_1[1] and y_rows[3] > y_at_1[3]
    # ... and the host restatement of the shared-pool draw
    want = shared_pool_draw(pool, [noise_len - C * n for n in y_rows], n_rows)
    assert (starts.tolist(), status.tolist(), int(used)) == want
    assert torch.all(full[:guard] == 1e30) and torch.all(full[-guard:] == 1e30)
    assert torch.isfinite(z).all() and z.abs().max().item() < 1e6  # no guard value was read


def test_rate_tensor_of_equal_rates_is_the_scalar_batch_call(device):
    from vits_amd import ops

    B, t_x, C, t_y = 3, 12, 4, 64
    g = torch.Generator().manual_seed(33)
    logw = (torch.rand(B, 1, t_x, generator=g) * 1.4 - 0.5).to(device)
    m_p = torch.randn(B, C, t_x, generator=g).to(device)
    s_p = (torch.rand(B, C, t_x, generator=g) + 0.5).to(device)
    noise = torch.randn(B, C, t_y, generator=g).to(device)
    za, la = ops.expand_durations(logw, m_p, s_p, noise, t_y, rate=1.37)
    zb, lb = ops.expand_durations(logw, m_p, s_p, noise, t_y,
                                  rate=torch.full((B,), 1.37, dtype=torch.float32, device=device))
    assert torch.equal(za, zb) and torch.equal(la, lb)


# -- resample_rows --------------------------------------------------------------------

RATIOS = [(1, 1), (11, 10), (1, 2), (3, 1), (160, 441)]
X_CAP = 768
# (len_scale, device lengths, n_out of the five rows).  At len_scale 1 the
# n_out values cover 0, 1, 255, 256 and 257.  At len_scale 4 the row lengths
# are multiples of 4, for which none of the five ratios gives 1 or 255 (n, 2
# k, 12 k, ceil(4.4 k) and ceil(640 k / 441) skip them): 0, 256 and 257 remain.
LENGTH_CASES = [
    (1, [257, 233, 1, 85, 702], [257, 257, 1, 255, 255]),
    (1, [0, 232, 511, 0, 2], [0, 256, 256, 0, 1]),
    (4, [64, 58, 128, 0, 177], [256, 256, 256, 0, 257]),
    (4, [0, 1, 192, 21, 1], [0, 5, 384, 252, 2]),
]
CASE_IDS = ["s1-257-1-255", "s1-0-256-1", "s4-256-0-257", "s4-0-small"]


def _filled_rows(lengths, scale, dtype, device):
    """[B, X_CAP]: each row's signal, 1e3 from its length on."""
    x = np.full((len(lengths), X_CAP), 1e3, dtype=np.float32)
    for b, n in enumerate(lengths):
        x[b, :n * scale] = np.random.RandomState(50 + b).uniform(-1, 1, n * scale)
    return torch.from_numpy(x).to(device=device, dtype=dtype)


def test_length_cases_cover_the_edge_lengths():
    from vits_amd import ops

    seen = set()
    for scale, lens, n_out in LENGTH_CASES:
        assert [ops.resample_out_len(n * scale, u, d) for n, (u, d) in zip(lens, RATIOS)] == n_out
        seen |= set(n_out)
    assert {0, 1, 255, 256, 257} <= seen


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("scale,lens,n_out", LENGTH_CASES, ids=CASE_IDS)
def test_resample_rows_equals_resample_poly_row_by_row(device, scale, lens, n_out, dtype):
    from vits_amd import ops

    B = len(RATIOS)
    x = _filled_rows(lens, scale, dtype, device)
    lengths = torch.tensor(lens, dtype=torch.int32, device=device)
    out_lengths = torch.full((B,), -7, dtype=torch.int32, device=device)
    out = ops.resample_rows(x, RATIOS, lengths=lengths, length_scale=scale,
                            out_lengths=out_lengths)
    cap = max(ops.resample_out_len(X_CAP, u, d) for u, d in RATIOS)
    assert out.shape == (B, cap) and out.dtype == torch.float32
    assert out_lengths.tolist() == n_out
    for b, (up, down) in enumerate(RATIOS):
        one = slice(b, b + 1)
        ol = torch.zeros(1, dtype=torch.int32, device=device)
        ref = ops.resample_poly(x[one], up, down, lengths=lengths[one], length_scale=scale,
                                out_lengths=ol)
        assert ol.item() == n_out[b]
        assert torch.equal(out[one, :ref.shape[1]], ref), (b, up, down)
        assert torch.count_nonzero(out[b, n_out[b]:]).item() == 0  # zero up to the shared cap
        if n_out[b] > 8:
            assert torch.count_nonzero(ref[0, :n_out[b]]).item() > n_out[b] // 2
        assert out[b].abs().max().item() < 8.0  # nothing of the 1e3 fill came through


VOLUMES = (1.0, 0.8, 0.0, 0.5, 0.3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_resample_rows_int16_equals_the_uniform_epilogue(device, dtype):
    from vits_amd import ops

    scale, lens, n_out = LENGTH_CASES[0]
    B = len(RATIOS)
    x = _filled_rows(lens, scale, dtype, device)
    lengths = torch.tensor(lens, dtype=torch.int32, device=device)
    cap = max(ops.resample_out_len(X_CAP, u, d) for u, d in RATIOS) + 9  # (a tail)
    out = torch.full((B, cap), 12345, dtype=torch.int16, device=device)
    ops.resample_rows(x, RATIOS, lengths=lengths, volumes=VOLUMES, pcm=True, out=out)
    for b, (up, down) in enumerate(RATIOS):
        one = slice(b, b + 1)
        if up == down:
            ref = ops.pcm16(x[one], VOLUMES[b], lengths=lengths[one])
        else:
            ref = ops.resample_pcm16(x[one], up, down, VOLUMES[b], lengths=lengths[one])
        assert ref.dtype == torch.int16
        assert torch.equal(out[one, :ref.shape[1]], ref), (b, up, down)
        assert torch.count_nonzero(out[b, n_out[b]:]).item() == 0
        assert (torch.count_nonzero(ref).item() > 0) == (VOLUMES[b] > 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_two_launch_chain_with_identity_slots(device, dtype):
    """Two launches over four rows: (identity, 11/10), (11/10, identity),
    (5/6, 1/2) and (identity, identity).  A pass next to an identity is the
    single direct pass; two real passes are the uniform two-pass chain."""
    from vits_amd import ops

    hop, frames = 4, [60, 60, 45, 30]
    first = [(1, 1), (11, 10), (5, 6), (1, 1)]
    second = [(11, 10), (1, 1), (1, 2), (1, 1)]
    volumes = (0.9, 0.9, 0.6, 1.0)
    B = 4
    x = _filled_rows(frames, hop, dtype, device)[:, :256]
    y_len = torch.tensor(frames, dtype=torch.int32, device=device)
    n1 = torch.empty(B, dtype=torch.int32, device=device)
    mid = ops.resample_rows(x, first, lengths=y_len, length_scale=hop, out_lengths=n1)
    pcm = ops.resample_rows(mid, second, lengths=n1, volumes=volumes, pcm=True)
    direct = {0: (11, 10), 1: (11, 10)}
    for b in range(B):
        one = slice(b, b + 1)
        if b in direct:
            ref = ops.resample_pcm16(x[one], *direct[b], volumes[b], lengths=y_len[one],
                                     length_scale=hop)
        elif b == 2:
            l1 = torch.empty(1, dtype=torch.int32, device=device)
            m1 = ops.resample_poly(x[one], 5, 6, lengths=y_len[one], length_scale=hop,
                                   out_lengths=l1)
            ref = ops.resample_pcm16(m1, 1, 2, volumes[b], lengths=l1)
        else:
            ref = ops.pcm16(x[one], volumes[b], lengths=y_len[one], length_scale=hop)
        n = min(ref.shape[1], pcm.shape[1])
        assert torch.equal(pcm[one, :n], ref[:, :n]), b
        assert torch.count_nonzero(ref[:, n:]).item() == 0
        assert torch.count_nonzero(pcm[one, n:]).item() == 0
        assert torch.count_nonzero(ref).item() > 8


# -- pack_pcm_rows ----------------------------------------------------------------------

def test_pack_pcm_rows(device):
    from vits_amd import ops

    B, hop, cap = 4, 192, 3 * 192 + 24
    passes = [[], [(5, 6)], [(5, 6), (1, 2)], [(3, 1)]]
    tails = [0, 7, 3, 5]
    g = torch.Generator().manual_seed(9)
    rows = torch.randint(-30000, 30000, (B, cap), generator=g, dtype=torch.int16).to(device)
    header = ops.pack_header_len(B)
    big = torch.empty(header + B * (cap + 7) + 64, dtype=torch.int16, device=device)

    def expect(frames, n):
        offs, parts = [0], [torch.zeros(0, dtype=torch.int16)]
        for b in range(B):
            if b < n:
                n_out = frames[b] * hop
                for up, down in passes[b]:
                    n_out = ops.resample_out_len(n_out, up, down)
                parts += [rows[b, :n_out].cpu(), torch.zeros(tails[b], dtype=torch.int16)]
                offs.append(offs[-1] + n_out + tails[b])
            else:
                offs.append(offs[-1])
        return offs, torch.cat(parts)

    word = torch.tensor([3], dtype=torch.int32, device=device)  # n_rows as a graph holds it
    for frames, n_rows, n in (([3, 1, 2, 1], 3, 3), ([1, 3, 2, 1], 3, 3), ([2, 3, 1, 1], 2, 2),
                              ([2, 2, 3, 1], word, 3), ([1, 2, 1, 1], None, 4)):
        y_len = torch.tensor(frames, dtype=torch.int32, device=device)
        big.fill_(12345)
        _, offsets, stream = ops.pack_pcm_rows(rows, y_len, hop, passes, tails, n_rows=n_rows,
                                               out=big)
        offs, want = expect(frames, n)
        assert offsets.tolist() == offs and offs[-1] > 0
        got = stream.cpu()
        assert torch.equal(got[:offs[-1]], want)
        assert torch.all(got[offs[-1]:] == 12345)               # nothing past offset[B]
        assert torch.all(big[2 * (B + 1):header] == 12345)       # nor between offsets and stream
    # a stream too short for the rows: nothing is written at or past its capacity
    frames, short = [3, 1, 2, 1], 600
    offs, want = expect(frames, 3)
    assert offs[-1] > short
    big.fill_(12345)
    ops.pack_pcm_rows(rows, torch.tensor(frames, dtype=torch.int32, device=device), hop, passes,
                      tails, n_rows=3, out=big[:header + short])
    assert torch.equal(big[header:header + short].cpu(), want[:short])
    assert torch.all(big[header + short:] == 12345)
    # the default buffer holds every row at its longest
    out, offsets, stream = ops.pack_pcm_rows(rows, torch.tensor(frames, dtype=torch.int32,
                                                                device=device), hop, passes, tails)
    assert out.numel() == header + B * (cap + 7)
    assert offsets.tolist() == expect(frames, 4)[0]


# -- EmoVITS / VITSWrap on the tiny checkpoint ------------------------------------------

def _quiesce():
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tts(tmp_path_factory, device):
    """The tiny checkpoint of tests/test_serve_batch_gpu.py: 16 kHz, hop 192."""
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import deterministic_fill_

    root = tmp_path_factory.mktemp("serve_mixed_ckpt")
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


CONTROLS = [{}, dict(duration_rate=0.8, pitch=1.2, sampling_rate=8000, volume=0.7,
                     tail_silence=0.01), dict(duration_rate=1.3, sampling_rate=24000)]
SEGMENTS = [(9,), (4, 14), (7, 11, 5)]


def _requests(device):
    from vits_amd.infer import PcmRequest

    channels = tiny_cfg()["data"]["text_channels"]
    rs = np.random.RandomState(17)
    return [PcmRequest([(1, rs.randn(n, channels).astype(np.float32),
                         torch.from_numpy(rs.randn(1, 1024).astype(np.float32)).half().to(device))
                        for n in lengths], **kw)
            for lengths, kw in zip(SEGMENTS, CONTROLS)]


@pytest.fixture(scope="module")
def in_order(tts, device):
    """The in-order loop over infer_pcm_batch from seed 41, and numpy's state
    behind it: computed once, read-only."""
    np.random.seed(41)
    want = [tts.infer_pcm_batch(r.items, **kw) for r, kw in zip(_requests(device), CONTROLS)]
    return want, np.random.get_state()


@pytest.mark.parametrize("max_batch", [16, 2])
def test_infer_pcm_requests_equals_the_loop_over_infer_pcm_batch(tts, device, monkeypatch,
                                                                 in_order, max_batch):
    want, want_state = in_order
    monkeypatch.setattr(type(tts), "MAX_BATCH", max_batch)  # 2: request 1 straddles two groups
    reqs = _requests(device)
    np.random.seed(41)
    got = tts.infer_pcm_requests(reqs)
    assert same_state(np.random.get_state(), want_state)
    assert len(got) == len(want) == 3
    lengths = []
    for (pcm, offs, emos, n_model), (wp, wo, we, wn), r in zip(got, want, reqs):
        assert pcm.dtype == np.int16 and pcm.ndim == 1 and offs.dtype == np.int64
        assert offs.tolist() == wo.tolist() and len(offs) == len(r.items) + 1
        assert np.array_equal(pcm, wp) and len(pcm) == offs[-1]
        assert n_model == wn and all(n % 192 == 0 and n > 0 for n in n_model)
        for i, (e, w_e) in enumerate(zip(emos, we)):
            assert torch.equal(e, w_e)
            assert np.abs(pcm[offs[i]:offs[i + 1]]).max() > 0
        lengths.append(len(pcm))
    # the controls took effect: 8 kHz is about half, 24 kHz about 1.5 x the samples per frame
    per_frame = [n / sum(g[3]) for n, g in zip(lengths, got)]
    assert per_frame[1] < 0.7 * per_frame[0] and per_frame[2] > 1.3 * per_frame[0]
    assert any(k[0] == "rows" for k in tts._graphs)  # a rate-free batched graph was used


def test_one_graph_serves_every_speed(tts, device, monkeypatch):
    from vits_amd.infer import PcmRequest

    items = _requests(device)[1].items
    monkeypatch.setattr(tts, "_graphs", {})
    monkeypatch.setattr(tts, "_ty_bucket", {})
    real, calls = tts.model.capture_infer_bucketed, []

    def counting(*args, **kwargs):
        calls.append((args, kwargs))
        return real(*args, **kwargs)

    monkeypatch.setattr(tts.model, "capture_infer_bucketed", counting)
    frames = []
    for speed in (0.8, 1.0, 1.25):
        np.random.seed(43)
        (pcm, offs, _, n_model), = tts.infer_pcm_requests([PcmRequest(items, duration_rate=speed)])
        np.random.seed(43)
        wp, wo, _, wn = tts.infer_pcm_batch(items, duration_rate=speed)
        assert np.array_equal(pcm, wp) and n_model == wn
        assert max(n_model) <= 256 * 192  # the 256-frame bucket holds it
        frames.append(sum(n_model))
    assert frames[0] < frames[1] < frames[2]
    rows = [c for c in calls if isinstance(c[1]["length_scale"], torch.Tensor)]
    assert len(rows) == 1                       # one capture for the three speeds ...
    assert len(calls) == 1 + 3                  # ... against one per speed of infer_pcm_batch
    assert list(tts._ty_bucket) == [] and sum(k[0] == "rows" for k in tts._graphs) == 1


def test_single_utterance_graph_with_the_rate_as_an_input(tts, device):
    """capture_infer_bucketed(batch=1, length_scale=tensor): replay takes the
    speed; the result is the graph captured at that speed."""
    from vits_amd import ops

    channels = tiny_cfg()["data"]["text_channels"]
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.randn(1, 11, channels).astype(np.float32)).half().to(device)
    emo = torch.from_numpy(rs.randn(1, 1024).astype(np.float32)).half().to(device)
    sid = torch.tensor([1], device=device)
    kw = dict(noise_len=tts.noise.numel(), padded_text=True)
    free = tts.model.capture_infer_bucketed(32, 256, length_scale=torch.ones(1), **kw)
    free.static["noise"].copy_(tts.noise.float())
    np.random.seed(44)
    pool, _ = ops.numpy_draw_pool()
    lens = []
    for speed in (1.3, 0.7):
        fixed = tts.model.capture_infer_bucketed(32, 256, length_scale=speed, **kw)
        fixed.static["noise"].copy_(tts.noise.float())
        want, want_len = fixed(x, emo, sid, noise_start=pool, x_length=11)
        got, got_len = free(x, emo, sid, noise_start=pool, x_length=11, rate=speed)
        assert torch.equal(got_len, want_len) and 1 < int(got_len[0, 0]) <= 256
        n = int(got_len[0, 0]) * 192
        assert torch.equal(got[..., :n], want[..., :n]) and torch.count_nonzero(got).item() > 0
        lens.append(int(got_len[0, 0]))
        with pytest.raises(ValueError, match="fixed length_scale"):
            fixed(x, emo, sid, noise_start=pool, x_length=11, rate=speed)
    assert lens[0] > lens[1]


def test_speaking_many_equals_the_loop_over_speaking(tts, monkeypatch):
    from vits_amd import vits_wrap

    channels = tiny_cfg()["data"]["text_channels"]

    class Parser:
        max_utt_length = 10

        def __call__(self, utt_id, text):
            rs = np.random.RandomState(len(text))
            return utt_id, text, rs.randn(max(1, len(text)), channels).astype(np.float32)

    def inputs():
        return [{"id": "a", "text": "abcdefghi。jklmnopq。rstu", "spkid": 1, "emotion": (1, 0),
                 "sampling_rate": 22050, "pitch": 1.2, "tail_silence": 0.02},
                {"id": "b", "text": "hello", "spkid": 1, "emotion": (1, 1), "speed": 0.8,
                 "sampling_rate": 8000, "volume": 0.7},
                {"id": "c", "text": "xyzw", "spkid": 1, "emotion": (1, 2), "speed": 1.3,
                 "pitch": 0.9}]

    seq = vits_wrap.VITSWrap(textparser=Parser(), speecher=tts, device_post=True)
    bat = vits_wrap.VITSWrap(textparser=Parser(), speecher=tts, batch_segments=True)

    def no_host_resampling(*args, **kwargs):
        raise AssertionError("the output stage must stay on the device")

    monkeypatch.setattr(vits_wrap, "_resample", no_host_resampling)
    np.random.seed(45)
    want = [seq.speaking(i) for i in inputs()]
    want_state = np.random.get_state()
    np.random.seed(45)
    got = bat.speaking_many(inputs())
    assert same_state(np.random.get_state(), want_state)  # (explicit emotions: same draw order)
    assert [len(b["segment_info"]) for b in got] == [3, 1, 1]
    for a, b in zip(want, got):
        assert a["wav"] == b["wav"] and len(b["wav"]) > 44
        assert a["sr"] == b["sr"] and a["segment_info"] == b["segment_info"]
        assert set(a) == set(b)
        assert np.abs(np.frombuffer(b["wav"][44:], dtype=np.int16)).max() > 0
        assert b["time_used_backend"] == got[0]["time_used_backend"] > 0
        assert b["time_used_frontend"] == got[0]["time_used_frontend"] >= 0 and b["rtf"] > 0
    assert [b["sr"] for b in got] == [22050, 8000, 16000]
    # without batch_segments it is the loop; so is a call below MANY_MIN_ROWS segments
    np.random.seed(45)
    loop = seq.speaking_many(inputs())
    assert [b["wav"] for b in loop] == [a["wav"] for a in want]
    assert bat.MANY_MIN_ROWS == 2

    def not_batched(*args, **kwargs):
        raise AssertionError("one segment in all must go through speaking")

    monkeypatch.setattr(tts, "infer_pcm_requests", not_batched)
    np.random.seed(45)
    one, = bat.speaking_many([inputs()[1]])
    np.random.seed(45)
    assert one["wav"] == seq.speaking(inputs()[1])["wav"]
    assert bat.speaking_many([]) == []

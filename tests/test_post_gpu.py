"""Device-side PCM output stage: ops.resample_poly / pcm16 / resample_pcm16,
EmoVITS.infer_pcm and VITSWrap(device_post=True).

The resampler's reference is the closed form of scipy.signal.resample_poly
(zero extension, float32 filter h of ops.resample_filter's design),
    out[n] = sum_i x[i] * h[n * down - i * up + half_len],
evaluated in float64.  Per output sample the kernel may differ from it by at
most E[n] = (K + 2) * 2^-24 * sum_i |x[i]| * |h[j]|, K the number of taps
summed: the standard bound of an fp32 dot product of K terms (any order, with
or without FMA), derived and not measured.
"""
import functools
import json

import numpy as np
import pytest
import torch

from common import build_model, tiny_cfg

pytestmark = pytest.mark.gpu

RATIOS = [(11, 10), (5, 6), (320, 441), (160, 441), (160, 147), (2, 1), (1, 2)]
LENGTH_PAIRS = [(1, 300), (7, 1999)]  # B = 2 rows of different lengths
NP_DT = {torch.float32: np.float32, torch.float16: np.float16}


@functools.lru_cache(maxsize=None)
def _signal(n_in, dtype):
    """|x| <= 1, already rounded to the input dtype (read-only)."""
    x = np.random.RandomState(1000 + n_in).uniform(-1, 1, n_in).astype(NP_DT[dtype])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(up, down, n_in, dtype):
    """(float64 closed form, bound E) for _signal(n_in, dtype); computed once
    and shared by the tests (read-only)."""
    from scipy.signal import firwin

    m = max(up, down)
    half = 10 * m
    h = (firwin(2 * half + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32)
         * np.float32(up)).astype(np.float64)
    x = _signal(n_in, dtype).astype(np.float64)
    n_out = -(-n_in * up // down)
    j = (np.arange(n_out, dtype=np.int64)[:, None] * down + half
         - np.arange(n_in, dtype=np.int64)[None, :] * up)
    valid = (j >= 0) & (j <= 2 * half)
    taps = np.where(valid, h[np.clip(j, 0, 2 * half)], 0.0)
    ref = taps @ x
    bound = (valid.sum(1) + 2) * 2.0 ** -24 * (np.abs(taps) @ np.abs(x))
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def _rows(lengths, dtype, device, pad=37, fill=1e3):
    """[B, max(lengths) + pad] with each row's signal, `fill` past its length."""
    buf = np.full((len(lengths), max(lengths) + pad), fill, dtype=NP_DT[dtype])
    for b, n in enumerate(lengths):
        buf[b, :n] = _signal(n, dtype)
    return torch.from_numpy(buf).to(device)


def _lens(values, device):
    return torch.tensor(values, dtype=torch.int32, device=device)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_matches_float64_closed_form(device, up, down, dtype):
    from vits_amd import ops

    for lengths in LENGTH_PAIRS:
        x = _rows(lengths, dtype, device)
        out_lens = torch.full((2,), -1, dtype=torch.int32, device=device)
        out = ops.resample_poly(x, up, down, lengths=_lens(lengths, device), out_lengths=out_lens)
        assert out.dtype == torch.float32
        assert out.shape == (2, ops.resample_out_len(x.shape[1], up, down))
        out = out.cpu().numpy()
        n_outs = [ops.resample_out_len(n, up, down) for n in lengths]
        assert out_lens.tolist() == n_outs
        for b, n_in in enumerate(lengths):
            ref, bound = _reference(up, down, n_in, dtype)
            assert len(ref) == n_outs[b]
            err = np.abs(out[b, :n_outs[b]].astype(np.float64) - ref)
            worst = int(np.argmax(err - bound))
            print(f"{up}/{down} n_in={n_in}: max err {err.max():.3g}, bound there "
                  f"{bound[int(np.argmax(err))]:.3g}, max bound {bound.max():.3g}")
            assert (err <= bound).all(), (n_in, worst, err[worst], bound[worst])
            assert not out[b, n_outs[b]:].any()  # zero to the end of the buffer


def test_device_and_host_lengths_agree_bitwise(device):
    from vits_amd import ops

    for up, down in ((320, 441), (11, 10)):
        for frames, n_in in ((75, 300), (499, 1996)):
            x = _rows((1999, 1999), torch.float32, device, fill=7.0)
            a = ops.resample_poly(x, up, down, lengths=_lens([frames, frames], device),
                                  length_scale=4)
            b = torch.full_like(a, 5.0)
            ops.resample_poly(x, up, down, lengths=n_in, out=b)
            assert torch.equal(a, b)
            assert a[:, :ops.resample_out_len(n_in, up, down)].abs().sum() > 0
            # a host length allocates exactly n_out, and all of x when none is given
            assert ops.resample_poly(x, up, down, lengths=n_in).shape[1] == \
                ops.resample_out_len(n_in, up, down)
    x1 = x[0, :300].contiguous()
    assert torch.equal(ops.resample_poly(x1, 2, 1), ops.resample_poly(x1.view(1, -1), 2, 1)[0])


def test_host_length_must_fit_the_buffers(device):
    from vits_amd import _lib, ops

    x = _rows((300,), torch.float32, device)
    with pytest.raises(_lib.VitsAmdError):
        ops.resample_poly(x, 2, 1, lengths=x.shape[1] + 1)
    with pytest.raises(_lib.VitsAmdError):
        ops.resample_poly(x, 2, 1, lengths=300, out=torch.empty(1, 599, device=device))
    with pytest.raises(_lib.VitsAmdError):
        ops.resample_poly(x.cpu(), 2, 1)


def test_resample_is_deterministic_and_reduces_the_ratio(device):
    from vits_amd import ops

    x = _rows((300, 1999), torch.float16, device)
    lens = _lens([300, 1999], device)
    a = ops.resample_poly(x, 160, 441, lengths=lens)
    b = ops.resample_poly(x, 160, 441, lengths=lens)
    c = ops.resample_poly(x, 320, 882, lengths=lens)
    assert torch.equal(a, b) and torch.equal(a, c)
    # up == down: a masked copy
    d = ops.resample_poly(x, 3, 3, lengths=lens)
    assert d.shape == x.shape and torch.equal(d[1, :1999], x[1, :1999].float())
    assert not d[0, 300:].any() and not d[1, 1999:].any()


@pytest.mark.parametrize("volume", [1.0, 0.8, 0.0])
def test_pcm16_is_the_host_expression_bitwise(device, volume):
    from vits_amd import ops

    edge = [1.5, 1.0, 0.99997, 0.6 / 32767]
    special = np.array(edge + [-v for v in edge] + [0.0, 32767.5 / 32767, -32768.5 / 32767],
                       dtype=np.float32)
    rnd = np.random.RandomState(3).uniform(-1.2, 1.2, 1501).astype(np.float32)
    x = np.concatenate([special, rnd, np.full(100, 0.5, np.float32)])
    n = len(special) + len(rnd)
    want = np.clip(x[:n] * volume * 32767, -32768, 32767).astype(np.int16)
    xd = torch.from_numpy(x).to(device)
    for got in (ops.pcm16(xd, volume, lengths=n),
                ops.pcm16(xd.view(1, -1), volume, lengths=_lens([n // 2], device), length_scale=2,
                          out=torch.full((1, len(x)), 77, dtype=torch.int16, device=device))[0]):
        assert got.dtype == torch.int16
        got = got.cpu().numpy()
        assert np.array_equal(got[:n], want)
        assert not got[n:].any()
    assert len(ops.pcm16(xd, volume)) == len(x)


@pytest.mark.parametrize("up,down", [(11, 10), (160, 441)])
def test_fused_resample_pcm16_quantises_the_reference(device, up, down):
    """Every sample equals trunc(clip(v')) for some v' within e of v = the
    float64 reference times float32(0.8) * 32767 (the volume the kernel is
    given is the float32 one), e = E * 0.8 * 32767 + 2^-22 * |v| (the bound of
    the resampler scaled, plus the two fp32 roundings of the multiplies):
    the float64 quantisation, except where v is within e of an integer or of
    a clip edge.  A systematic off-by-one cannot pass."""
    from vits_amd import ops

    n_in, volume = 1999, 0.8
    ref, bound = _reference(up, down, n_in, torch.float32)
    x = _rows((n_in,), torch.float32, device)
    out_lens = torch.zeros(1, dtype=torch.int32, device=device)
    pcm = ops.resample_pcm16(x, up, down, volume, lengths=_lens([n_in], device),
                             out_lengths=out_lens)
    assert pcm.dtype == torch.int16 and out_lens.item() == len(ref)
    pcm = pcm[0].cpu().numpy().astype(np.int64)
    scale = float(np.float32(volume)) * 32767
    v = ref * scale
    e = bound * scale + 2.0 ** -22 * np.abs(v)
    lo = np.trunc(np.clip(v - e, -32768, 32767)).astype(np.int64)
    hi = np.trunc(np.clip(v + e, -32768, 32767)).astype(np.int64)
    got = pcm[:len(ref)]
    exact = np.trunc(np.clip(v, -32768, 32767)).astype(np.int64)
    print(f"{up}/{down}: {int((got != exact).sum())} of {len(ref)} samples differ from the "
          f"float64 quantisation, {int((lo != hi).sum())} are ambiguous within e")
    assert ((got >= lo) & (got <= hi)).all()
    assert np.abs(got).max() > 10000  # the signal is there
    assert not pcm[len(ref):].any()
    # the unfused pair of calls gives the same PCM
    two = ops.pcm16(ops.resample_poly(x, up, down, lengths=n_in), volume)
    assert np.array_equal(two[0].cpu().numpy(), got)


def test_resample_pcm16_under_graph_capture(device):
    from vits_amd import ops

    up, down, volume = 320, 441, 0.9
    x = _rows((1999,), torch.float16, device)
    lens = _lens([0], device)
    out = torch.empty(1, ops.resample_out_len(x.shape[1], up, down) + 50, dtype=torch.int16,
                      device=device)
    out_lens = torch.zeros(1, dtype=torch.int32, device=device)

    def body():
        ops.resample_pcm16(x, up, down, volume, lengths=lens, length_scale=3, out=out,
                           out_lengths=out_lens)

    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        body()  # designs and caches the filter outside the capture
    torch.cuda.current_stream(device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for frames in (100, 666, 41):
        lens.fill_(frames)
        out.fill_(-1)
        graph.replay()
        eager = ops.resample_pcm16(x, up, down, volume, lengths=3 * frames,
                                   out=torch.empty_like(out))
        assert torch.equal(out, eager)
        assert out_lens.item() == ops.resample_out_len(3 * frames, up, down)
        assert out[0, :out_lens.item()].abs().max() > 1000


# -- EmoVITS.infer_pcm / VITSWrap(device_post=True) on the tiny checkpoint -----

@pytest.fixture(scope="module")
def tts(tmp_path_factory, device):
    """tests/test_wrappers.py's tiny checkpoint: 16 kHz, hop 192."""
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import deterministic_fill_

    root = tmp_path_factory.mktemp("post_ckpt")
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
    return EmoVITS(str(root / "G_1000.pth"), device)


def _text(n=9):
    return np.random.RandomState(7).randn(n, tiny_cfg()["data"]["text_channels"]).astype(np.float32)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_infer_pcm_defaults_are_infer_quantised(tts):
    np.random.seed(11)
    wav, _ = tts.infer(1, _text(), None)
    state = np.random.get_state()
    np.random.seed(11)
    pcm, emo, n_model = tts.infer_pcm(1, _text(), None)
    assert pcm.dtype == np.int16 and pcm.ndim == 1 and emo.shape == (1, 1024)
    assert n_model == len(wav) and len(wav) % 192 == 0 and len(wav) > 0
    assert np.array_equal(pcm, np.clip(wav * 32767, -32768, 32767).astype(np.int16))
    assert np.abs(pcm).max() > 0
    assert _same_state(np.random.get_state(), state)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_infer_pcm_matches_the_host_chain(tts, graph, monkeypatch):
    """Both chains are within about 0.2 LSB of the exact value (E through two
    passes, scaled by 0.7 * 32767), so the values they truncate differ by
    less than 1 and the int16 samples by at most 1."""
    from vits_amd import ops, vits_wrap

    monkeypatch.setattr(tts, "graph", graph)
    kw = dict(pitch=1.2, sampling_rate=8000, volume=0.7, tail_silence=0.01)
    np.random.seed(12)
    wav, _ = tts.infer(1, _text(), None)
    state = np.random.get_state()
    want = vits_wrap.host_pcm(wav, tts.sampling_rate, kw["pitch"], kw["sampling_rate"],
                              kw["volume"], kw["tail_silence"])
    np.random.seed(12)
    pcm, _, n_model = tts.infer_pcm(1, _text(), None, **kw)
    assert _same_state(np.random.get_state(), state)
    assert n_model == len(wav)
    n_out = len(wav)
    for up, down in (ops.resample_ratio(int(16000 / 1.2), 16000), ops.resample_ratio(16000, 8000)):
        n_out = ops.resample_out_len(n_out, up, down)
    assert len(pcm) == len(want) == n_out + 80
    diff = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
    print(f"graph={graph}: {int((diff > 0).sum())} of {len(pcm)} samples differ, max {diff.max()}")
    assert diff.max() <= 1
    assert np.abs(pcm[:n_out]).max() > 0 and not pcm[n_out:].any()


def test_vitswrap_device_post_matches_the_host_path(tts, monkeypatch):
    from vits_amd import vits_wrap

    channels = tiny_cfg()["data"]["text_channels"]

    class Parser:
        max_utt_length = 10

        def __call__(self, utt_id, text):
            rs = np.random.RandomState(len(text))
            return utt_id, text, rs.randn(max(1, len(text)), channels).astype(np.float32)

    def request():
        return {"id": "u", "text": "abcdefghij。klmnopq", "spkid": 1, "sampling_rate": 22050,
                "pitch": 1.2, "tail_silence": 0.02}

    with pytest.raises(TypeError):
        vits_wrap.VITSWrap(None, None, 0, Parser(), tts, True)  # keyword-only
    host = vits_wrap.VITSWrap(textparser=Parser(), speecher=tts)
    dev = vits_wrap.VITSWrap(textparser=Parser(), speecher=tts, device_post=True)
    assert host.device_post is False and dev.device_post is True
    np.random.seed(13)
    a = host.speaking(request())

    def no_host_resampling(*args, **kwargs):
        raise AssertionError("device_post=True must not resample on the host")

    monkeypatch.setattr(vits_wrap, "_resample", no_host_resampling)
    np.random.seed(13)
    b = dev.speaking(request())
    assert a["sr"] == b["sr"] == 22050
    assert a["wav"][:44] == b["wav"][:44] and len(a["wav"]) == len(b["wav"])
    assert a["segment_info"] == b["segment_info"] and len(b["segment_info"]) == 2
    assert b["rtf"] > 0 and b["time_used_backend"] > 0
    pa = np.frombuffer(a["wav"][44:], dtype=np.int16).astype(np.int32)
    pb = np.frombuffer(b["wav"][44:], dtype=np.int16).astype(np.int32)
    assert np.abs(pa - pb).max() <= 1 and np.abs(pb).max() > 0
    tail = int(0.02 * 22050)
    assert not pb[-tail:].any()

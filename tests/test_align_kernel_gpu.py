"""vits_maximum_path_durations on the GPU (ops.maximum_path_durations): the
durations epilogue of the MAS kernel against the CPU oracle (oracle/mas.py)
reduced in numpy (tests/align_common.py).  Everything is integer or a
sequential float32 sum, so every comparison is exact.

Shapes (frames, tokens): the smallest ones, tokens == frames, one and two
32-row decision blocks and one row past them, a full and a just-exceeded
64-column wave row (XPL 1 -> 2), more than one streamed chunk, and 1500 /
1600 x 129 on either side of the switch of the decision words from LDS to the
global workspace."""
import numpy as np
import pytest
import torch

import align_common as A
from oracle import mas as mas_oracle

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 1), (7, 7), (31, 9), (32, 9), (33, 9), (64, 17), (65, 64), (70, 65),
          (300, 129), (1500, 129), (1600, 129)]
GUARD = 64
I_SENT, F_SENT = -77, -12345.5


def _neg_cent(B, Tt, Ts, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Tt, Ts, generator=g) * 3.0 - 1.0


def _call_guarded(lib_ops, nc, tt, ts, scores=True, frame_token=True):
    """The C entry on sentinel-filled outputs with guard bands on both sides:
    (durations, scores | None, frame_token | None) as numpy, after checking
    that nothing outside [B, Ts] / [B, Tt] was written."""
    from vits_amd import _lib

    B, Tt, Ts = nc.shape
    dev = nc.device

    def band(n, dtype, fill):
        return torch.full((GUARD + n + GUARD,), fill, device=dev, dtype=dtype)

    dur = band(B * Ts, torch.int32, I_SENT)
    sc = band(B * Ts, torch.float32, F_SENT) if scores else None
    ft = band(B * Tt, torch.int32, I_SENT) if frame_token else None
    lib = _lib.load()
    wsb = int(lib.vits_maximum_path_workspace(B, Tt, Ts))
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)

    def ptr(t):
        return None if t is None else t.data_ptr() + GUARD * 4

    _lib.check(lib.vits_maximum_path_durations(
        nc.data_ptr(), tt.data_ptr(), ts.data_ptr(), ptr(dur), ptr(sc), ptr(ft), B, Tt, Ts,
        ws.data_ptr(), ws.numel(), lib_ops._stream_ptr(dev)), "vits_maximum_path_durations")
    torch.cuda.synchronize()
    out = []
    for t, n, fill in ((dur, B * Ts, I_SENT), (sc, B * Ts, F_SENT), (ft, B * Tt, I_SENT)):
        if t is None:
            out.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all(), "guard band written"
        body = h[GUARD:GUARD + n]
        assert not (body == fill).any(), "an output element was left unwritten"
        out.append(body.reshape(B, -1))
    return out


def _oracle(nc, tt, ts):
    rows = [A.mas_reduce(nc[b], int(tt[b]), int(ts[b])) for b in range(nc.shape[0])]
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


@pytest.mark.parametrize("Tt,Ts", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_durations_equal_oracle(device, Tt, Ts):
    from vits_amd import _lib, ops

    B = 2
    nc = _neg_cent(B, Tt, Ts, 100 * Tt + Ts)
    # row 0 fills the buffer, row 1 is ragged (never shorter than one token)
    tt = np.array([Tt, max(1, Tt - Tt // 3)], dtype=np.int32)
    ts = np.array([Ts, max(1, min(Ts - Ts // 4, tt[1]))], dtype=np.int32)
    want = _oracle(nc.numpy(), tt, ts)
    assert want[0][0].sum() == Tt and want[0][1].sum() == tt[1]
    ncd = nc.to(device)
    ttd, tsd = torch.from_numpy(tt).to(device), torch.from_numpy(ts).to(device)
    dur, sc, ft = _call_guarded(ops, ncd, ttd, tsd)
    assert np.array_equal(dur, want[0])
    assert np.array_equal(ft, want[2])
    assert np.array_equal(sc, want[1])
    # the public op returns the same, and each optional output can be left out
    d2, s2, f2 = ops.maximum_path_durations(ncd, ttd, tsd, frame_token=True)
    assert d2.dtype == torch.int32 and s2.dtype == torch.float32 and f2.dtype == torch.int32
    assert np.array_equal(d2.cpu().numpy(), dur) and np.array_equal(s2.cpu().numpy(), sc)
    assert np.array_equal(f2.cpu().numpy(), ft)
    d3, s3, f3 = ops.maximum_path_durations(ncd, ttd, tsd, scores=False)
    assert s3 is None and f3 is None and np.array_equal(d3.cpu().numpy(), dur)
    # the path entry is untouched by the new epilogue: still the oracle's path
    path = ops.maximum_path_lengths(ncd, ttd, tsd, dtype=torch.int32).cpu().numpy()
    assert np.array_equal(path, mas_oracle.maximum_path_lengths(nc.numpy(), tt, ts))
    if (Tt, Ts) in ((1500, 129), (1600, 129)):
        lib = _lib.load()
        base = 2 * 4 * B + 256
        assert (int(lib.vits_maximum_path_workspace(B, Tt, Ts)) > base) == (Tt == 1600)


def test_optional_outputs_guarded(device):
    """scores = NULL and frame_token = NULL each work, alone and together, and
    leave the other outputs as they are."""
    from vits_amd import ops

    nc = _neg_cent(3, 70, 33, 5)
    tt = np.array([70, 41, 33], dtype=np.int32)
    ts = np.array([33, 20, 33], dtype=np.int32)
    want = _oracle(nc.numpy(), tt, ts)
    ncd = nc.to(device)
    ttd, tsd = torch.from_numpy(tt).to(device), torch.from_numpy(ts).to(device)
    for scores, tokens in ((True, False), (False, True), (False, False)):
        dur, sc, ft = _call_guarded(ops, ncd, ttd, tsd, scores=scores, frame_token=tokens)
        assert np.array_equal(dur, want[0])
        assert (sc is None) == (not scores) and (ft is None) == (not tokens)
        if scores:
            assert np.array_equal(sc, want[1])
        if tokens:
            assert np.array_equal(ft, want[2])


def test_ragged_batch_and_rows_without_alignment(device):
    """Five rows in a 96 x 40 buffer: full, t_t == t_s, t_t < t_s, length 0,
    ragged; NaN past every row's lengths is never read into a result, and
    the rows without an alignment come back as defined: durations 0, scores 0,
    tokens -1 over the whole row."""
    from vits_amd import ops

    Tt, Ts = 96, 40
    tt = np.array([96, 23, 17, 0, 64], dtype=np.int32)
    ts = np.array([40, 23, 18, 12, 7], dtype=np.int32)
    B = len(tt)
    nc = _neg_cent(B, Tt, Ts, 9)
    want = _oracle(nc.numpy(), tt, ts)  # (the oracle reads the live corner only)
    for b in range(B):
        nc[b, tt[b]:, :] = float("nan")
        nc[b, :, ts[b]:] = float("nan")
    ncd = nc.to(device)
    ttd, tsd = torch.from_numpy(tt).to(device), torch.from_numpy(ts).to(device)
    dur, sc, ft = _call_guarded(ops, ncd, ttd, tsd)
    for b in (2, 3):
        assert not dur[b].any() and (sc[b] == 0).all() and (ft[b] == -1).all(), b
    assert dur[1, :23].tolist() == [1] * 23 and ft[1, :23].tolist() == list(range(23))
    assert np.isfinite(sc).all()
    assert np.array_equal(dur, want[0])
    assert np.array_equal(ft, want[2])
    assert np.array_equal(sc, want[1])
    for b in (0, 1, 4):
        assert dur[b, :ts[b]].min() >= 1 and dur[b].sum() == tt[b]


def test_capture_safe(device):
    """No host sync: the op can be captured, and the replay reads new lengths."""
    from vits_amd import ops

    nc = _neg_cent(2, 64, 17, 3)
    ncd = nc.to(device)
    ttd = torch.tensor([64, 30], dtype=torch.int32, device=device)
    tsd = torch.tensor([17, 9], dtype=torch.int32, device=device)
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        ops.maximum_path_durations(ncd, ttd, tsd, frame_token=True)
    torch.cuda.current_stream(device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.maximum_path_durations(ncd, ttd, tsd, frame_token=True)
    # (second replay: row 1 has frames but no tokens: no alignment)
    for tt, ts in (([64, 30], [17, 9]), ([40, 30], [17, 0])):
        ttd.copy_(torch.tensor(tt, dtype=torch.int32))
        tsd.copy_(torch.tensor(ts, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want = _oracle(nc.numpy(), tt, ts)
        for got, w in zip(out, want):
            assert np.array_equal(got.cpu().numpy(), w)

"""The panelled, stripped MAS (vits_mas_long_*, ops.maximum_path_durations_panels
/ _long) on the GPU against the CPU oracle (oracle/mas.py) reduced in numpy
(tests/align_common.py).  Everything is integer or a sequential float32 sum,
so every comparison is exact.

strip = 64 and panel = 32 make small shapes cross every seam: tokens 1, 63,
64, 65, 128, 129, 150 are one strip, exactly full strips, one column into the
next strip and a partial last strip; frames t_s, t_s + 1, 32, 33, 64, 95, 97,
200 are D = 0, a path on the diagonal, a panel ending on and off a decision
word, and seven panels."""
import numpy as np
import pytest
import torch

import align_common as A

pytestmark = pytest.mark.gpu

TOKENS = [1, 63, 64, 65, 128, 129, 150]
FRAMES = ["ts", "ts+1", 32, 33, 64, 95, 97, 200]
GUARD = 64
I_SENT, F_SENT = -77, -12345.5


def _frames(spec, ts):
    return ts if spec == "ts" else ts + 1 if spec == "ts+1" else spec


SHAPES = sorted({(_frames(f, s), s) for s in TOKENS for f in FRAMES if _frames(f, s) >= s})


def _neg_cent(B, Tt, Ts, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Tt, Ts, generator=g) * 3.0 - 1.0


def _oracle(nc, tt, ts):
    rows = [A.mas_reduce(nc[b], int(tt[b]), int(ts[b])) for b in range(nc.shape[0])]
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def _dev(device, *arrays):
    return [torch.as_tensor(np.asarray(a)).to(device) for a in arrays]


def _np(outs):
    return [None if o is None else o.cpu().numpy() for o in outs]


def _call_guarded(nc, tt, ts, strip, panel, scores=True, frame_token=True):
    """The C entries on sentinel-filled outputs with guard bands on both
    sides: (durations, scores | None, frame_token | None) as numpy, after
    checking that nothing outside [B, Ts] / [B, Tt] was written and every
    element inside was."""
    from vits_amd import _lib, ops

    B, Tt, Ts = nc.shape
    dev = nc.device

    def band(n, dtype, fill):
        return torch.full((GUARD + n + GUARD,), fill, device=dev, dtype=dtype)

    dur = band(B * Ts, torch.int32, I_SENT)
    sc = band(B * Ts, torch.float32, F_SENT) if scores else None
    ft = band(B * Tt, torch.int32, I_SENT) if frame_token else None
    lib = _lib.load()
    strip, panel = ops.mas_long_plan(Tt, Ts, strip, panel)
    wsb = int(lib.vits_mas_long_workspace(B, Tt, Ts, strip, panel))
    assert wsb > 0
    # the workspace between guard bands of its own, filled with NaN bits: it
    # needs no initialisation
    ws = torch.full((256 + wsb + 256,), 0xFF, device=dev, dtype=torch.uint8)
    wsp = ws.data_ptr() + 256

    def ptr(t):
        return None if t is None else t.data_ptr() + GUARD * 4

    dims = (B, Tt, Ts, strip, panel)
    tail = (wsp, wsb, ops._stream_ptr(dev))
    spans = [(y0, min(panel, Tt - y0)) for y0 in range(0, Tt, panel)]
    for y0, rows in spans:
        _lib.check(lib.vits_mas_long_panel(nc.data_ptr() + 4 * y0 * Ts, Tt * Ts, tt.data_ptr(),
                                           ts.data_ptr(), *dims, y0, rows, *tail), "panel")
    _lib.check(lib.vits_mas_long_backtrack(tt.data_ptr(), ts.data_ptr(), ptr(dur), ptr(ft),
                                           *dims, *tail), "backtrack")
    if scores:
        for y0, rows in reversed(spans):  # (any order)
            _lib.check(lib.vits_mas_long_gather(nc.data_ptr() + 4 * y0 * Ts, Tt * Ts,
                                                tt.data_ptr(), ts.data_ptr(), *dims, y0, rows,
                                                *tail), "gather")
        _lib.check(lib.vits_mas_long_scores(tt.data_ptr(), ts.data_ptr(), ptr(sc), *dims, *tail),
                   "scores")
    torch.cuda.synchronize()
    h = ws.cpu().numpy()
    assert (h[:256] == 0xFF).all() and (h[256 + wsb:] == 0xFF).all(), "workspace guard written"
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


def _check(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"durations {what}"
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), f"frame_token {what}"
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), f"scores {what}"


@pytest.mark.parametrize("Tt,Ts", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_panels_equal_oracle(device, Tt, Ts):
    """Two rows (a full one, a ragged one) at strip 64, panel 32: the oracle,
    and ops.maximum_path_durations, which accepts every one of these shapes."""
    from vits_amd import ops

    B = 2
    nc = _neg_cent(B, Tt, Ts, 100 * Tt + Ts)
    tt = np.array([Tt, max(1, Tt - Tt // 3)], dtype=np.int32)
    ts = np.array([Ts, max(1, min(Ts - Ts // 4, tt[1]))], dtype=np.int32)
    want = _oracle(nc.numpy(), tt, ts)
    assert want[0][0].sum() == Tt and want[0][1].sum() == tt[1]
    ncd, ttd, tsd = _dev(device, nc, tt, ts)
    _check(_call_guarded(ncd, ttd, tsd, 64, 32), want, "C entries")
    got = ops.maximum_path_durations_panels(ncd, ttd, tsd, strip=64, panel=32, frame_token=True)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert got[2].dtype == torch.int32
    _check(_np(got), want, "op")
    short = _np(ops.maximum_path_durations(ncd, ttd, tsd, frame_token=True))
    _check(_np(got), short, "vs maximum_path_durations")


def test_ragged_batch_in_one_buffer(device):
    """Three rows in a [3, 200, 150] buffer, NaN past each row's lengths: a
    row whose frames end two panels early, a row whose tokens end a strip
    early, a row without an alignment."""
    from vits_amd import ops

    Tt, Ts = 200, 150
    tt = np.array([200 - 2 * 32 - 5, 200, 40], dtype=np.int32)
    ts = np.array([129, 150 - 64 - 3, 41], dtype=np.int32)
    nc = _neg_cent(3, Tt, Ts, 11)
    want = _oracle(nc.numpy(), tt, ts)  # (the oracle reads the live corner only)
    for b in range(3):
        nc[b, tt[b]:, :] = float("nan")
        nc[b, :, ts[b]:] = float("nan")
    ncd, ttd, tsd = _dev(device, nc, tt, ts)
    got = _call_guarded(ncd, ttd, tsd, 64, 32)
    assert not got[0][2].any() and (got[1][2] == 0).all() and (got[2][2] == -1).all()
    assert np.isfinite(got[1]).all()
    _check(got, want)
    for b in (0, 1):
        assert got[0][b, :ts[b]].min() >= 1 and got[0][b].sum() == tt[b]
    _check(_np(ops.maximum_path_durations(ncd, ttd, tsd, frame_token=True)), want, "short")
    # more rows without an alignment: an empty side each
    tt2 = np.array([0, 200, 17], dtype=np.int32)
    ts2 = np.array([12, 0, 18], dtype=np.int32)
    ttd2, tsd2 = _dev(device, tt2, ts2)
    got = _call_guarded(ncd, ttd2, tsd2, 64, 32)
    assert not got[0].any() and (got[1] == 0).all() and (got[2] == -1).all()


def test_one_token_holds_three_thousand_frames(device):
    """Column 0 favoured: token 0 keeps about 3000 of 3100 frames, across the
    LDS windows of the score sum (and a 100-token tail after it)."""
    from vits_amd import ops

    Tt, Ts = 3100, 101
    nc = _neg_cent(1, Tt, Ts, 21)
    nc[0, :3000, 0] += 50.0
    tt, ts = np.array([Tt], dtype=np.int32), np.array([Ts], dtype=np.int32)
    want = _oracle(nc.numpy(), tt, ts)
    assert want[0][0, 0] > 2900
    ncd, ttd, tsd = _dev(device, nc, tt, ts)
    for strip, panel in ((64, 32), (128, 4096)):
        got = _np(ops.maximum_path_durations_panels(ncd, ttd, tsd, strip=strip, panel=panel,
                                                    frame_token=True))
        _check(got, want, f"strip {strip} panel {panel}")
    # ... and a token in the middle that crosses the 8192-frame window
    Tt, Ts = 9000, 40
    nc = _neg_cent(1, Tt, Ts, 22)
    nc[0, 6000:8800, 17] += 50.0
    tt, ts = np.array([Tt], dtype=np.int32), np.array([Ts], dtype=np.int32)
    want = _oracle(nc.numpy(), tt, ts)
    assert want[2][0, 8191] == 17 and want[2][0, 8192] == 17
    ncd, ttd, tsd = _dev(device, nc, tt, ts)
    got = _np(ops.maximum_path_durations_panels(ncd, ttd, tsd, strip=64, panel=4096,
                                                frame_token=True))
    _check(got, want, "9000 x 40")


WIDE = [(2100, 2049, 128, 64), (2100, 2049, 2048, 4096), (4200, 100, 128, 64),
        (4200, 100, 2048, 4096)]


@pytest.mark.parametrize("Tt,Ts,strip,panel", WIDE, ids=[f"{a}x{b}-s{c}-p{d}" for a, b, c, d in WIDE])
def test_wide_strips_and_tall_panels(device, Tt, Ts, strip, panel):
    """2100 x 2049: two real strips of 2048 in one panel (and 17 strips of 128
    in 33 panels); 4200 x 100: two panels of 4096."""
    from vits_amd import ops

    nc = _neg_cent(1, Tt, Ts, Tt + Ts)
    tt, ts = np.array([Tt], dtype=np.int32), np.array([Ts], dtype=np.int32)
    want = _oracle(nc.numpy(), tt, ts)
    ncd, ttd, tsd = _dev(device, nc, tt, ts)
    got = _np(ops.maximum_path_durations_panels(ncd, ttd, tsd, strip=strip, panel=panel,
                                                frame_token=True))
    _check(got, want)
    if Ts <= 2048:
        _check(got, _np(ops.maximum_path_durations(ncd, ttd, tsd, frame_token=True)), "short")


def test_optional_outputs(device):
    """scores and frame_token can each be left out, alone and together."""
    nc = _neg_cent(3, 97, 70, 5)
    tt = np.array([97, 41, 70], dtype=np.int32)
    ts = np.array([70, 20, 70], dtype=np.int32)
    want = _oracle(nc.numpy(), tt, ts)
    ncd, ttd, tsd = _dev(device, nc, tt, ts)
    for scores, tokens in ((True, False), (False, True), (False, False)):
        got = _call_guarded(ncd, ttd, tsd, 64, 32, scores=scores, frame_token=tokens)
        assert (got[1] is None) == (not scores) and (got[2] is None) == (not tokens)
        _check(got, want)
    from vits_amd import ops

    d, s, f = ops.maximum_path_durations_panels(ncd, ttd, tsd, strip=64, panel=32, scores=False)
    assert s is None and f is None and np.array_equal(d.cpu().numpy(), want[0])


def test_capture_safe(device):
    """The whole sequence under graph capture: the replay equals eager and
    reads new lengths."""
    from vits_amd import ops

    nc = _neg_cent(2, 97, 70, 3)
    ncd = nc.to(device)
    ttd = torch.tensor([97, 30], dtype=torch.int32, device=device)
    tsd = torch.tensor([70, 9], dtype=torch.int32, device=device)
    kw = dict(strip=64, panel=32, frame_token=True)
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        ops.maximum_path_durations_panels(ncd, ttd, tsd, **kw)
    torch.cuda.current_stream(device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.maximum_path_durations_panels(ncd, ttd, tsd, **kw)
    for tt, ts in (([97, 30], [70, 9]), ([66, 30], [65, 0])):
        ttd.copy_(torch.tensor(tt, dtype=torch.int32))
        tsd.copy_(torch.tensor(ts, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        replay = _np(out)
        _check(replay, _oracle(nc.numpy(), tt, ts), "replay vs oracle")
        _check(replay, _np(ops.maximum_path_durations_panels(ncd, ttd, tsd, **kw)), "vs eager")


def _latents(B, C, Tt, Ts, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, Tt, generator=g)
    m = torch.randn(B, C, Ts, generator=g) * 0.5
    lg = torch.randn(B, C, Ts, generator=g) * 0.2
    return z, m, lg


def test_neg_cent_of_a_panel_is_the_whole_matrix_rows(device):
    """200 frames x 150 tokens x 192 channels: the scores of panels of 32 and
    96 rows, as maximum_path_durations_long produces them (copy_windows into a
    contiguous slice, then the neg_cent kernel), equal the same rows of
    ops.neg_cent of the whole recording in every bit."""
    from vits_amd import ops

    C, Tt, Ts = 192, 200, 150
    z, m, lg = [t.to(device) for t in _latents(2, C, Tt, Ts, 31)]
    whole = ops.neg_cent(z, m, lg)
    for panel in (32, 96):
        spans = [(y0, min(panel, Tt - y0)) for y0 in range(0, Tt, panel)]
        assert spans[-1][1] < panel  # a partial last panel
        for y0, rows in spans:
            zp = torch.empty(2, C, rows, device=device)
            ops.copy_windows(z, zp, [(b * C * Tt + y0, b * C * rows, rows, rows) for b in range(2)],
                             channels=C, src_rstride=Tt, dst_rstride=rows)
            assert torch.equal(zp, z[:, :, y0:y0 + rows])
            assert torch.equal(ops.neg_cent(zp, m, lg), whole[:, y0:y0 + rows]), (panel, y0)


def test_long_from_latents_past_2048_tokens(device):
    """2300 frames against 2100 tokens, wider than maximum_path_durations
    takes: the long entry from the latents (one strip of 2048 and a second of
    52 columns, one panel at the defaults, 24 at panels of 96) equals the
    oracle's path on ops.neg_cent of the whole."""
    from vits_amd import ops

    C, Tt, Ts = 192, 2300, 2100
    z, m, lg = [t.to(device) for t in _latents(1, C, Tt, Ts, 33)]
    nc = ops.neg_cent(z, m, lg)
    tt, ts = np.array([Tt], dtype=np.int32), np.array([Ts], dtype=np.int32)
    want = _oracle(nc.cpu().numpy(), tt, ts)
    ttd, tsd = _dev(device, tt, ts)
    with pytest.raises(Exception):
        ops.maximum_path_durations(nc, ttd, tsd)
    for kw in (dict(), dict(strip=512, panel=96)):
        got = _np(ops.maximum_path_durations_long(z, m, lg, ttd, tsd, frame_token=True, **kw))
        _check(got, want, str(kw))


def test_long_from_latents_equals_short_on_the_matrix(device):
    """maximum_path_durations_long never holds the matrix; its outputs equal
    maximum_path_durations on ops.neg_cent of the whole, bit for bit, ragged
    rows included, at panels of 32 and 96 rows and at the defaults."""
    from vits_amd import ops

    C, Tt, Ts = 192, 200, 150
    z, m, lg = [t.to(device) for t in _latents(3, C, Tt, Ts, 32)]
    ttd = torch.tensor([200, 131, 40], dtype=torch.int32, device=device)
    tsd = torch.tensor([150, 83, 41], dtype=torch.int32, device=device)
    want = _np(ops.maximum_path_durations(ops.neg_cent(z, m, lg), ttd, tsd, frame_token=True))
    assert want[0][0].sum() == 200 and want[0][1].sum() == 131 and not want[0][2].any()
    for kw in (dict(strip=64, panel=32), dict(strip=64, panel=96), dict()):
        got = _np(ops.maximum_path_durations_long(z, m, lg, ttd, tsd, frame_token=True, **kw))
        _check(got, want, str(kw))
    d, s, f = ops.maximum_path_durations_long(z, m, lg, ttd, tsd, strip=64, panel=96,
                                              scores=False)
    assert s is None and f is None and np.array_equal(d.cpu().numpy(), want[0])

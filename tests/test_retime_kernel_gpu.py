"""The retiming kernels (csrc/retime.hip) against the numpy oracle of
tests/retime_common.py: integers exact, floats compared as bit patterns.
Outputs are pre-filled with NaN / a sentinel (every element must be written)
inside guard bands (nothing around them may be), NaN sits in z_p_rec past each
row's length (it may not be read), rows are ragged."""
import numpy as np
import pytest
import torch

import retime_common as RC

pytestmark = pytest.mark.gpu
I32 = torch.int32
GUARD = 64
SENT = -77777


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device)


def _guarded(shape, dtype, fill, device, off=0):
    """(view of ``shape`` inside a flat buffer with GUARD elements on each
    side, the buffer); ``off`` shifts the view by that many elements (off a
    16-byte boundary)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 4,), fill, dtype=dtype, device=device)
    return buf[GUARD + off:GUARD + off + n].view(*shape), buf


def _guards_intact(buf, n, fill, off=0):
    b = buf.cpu()
    lo, hi = b[:GUARD + off], b[GUARD + off + n:]
    if isinstance(fill, float) and np.isnan(fill):
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


# -- the plan ---------------------------------------------------------------------------

def _plan_rows(rng, t_x, big):
    """Ragged rows of one t_x: (dur_old [B, t_x + 3], x_len, y_len)."""
    B = 6
    hi = (1 << 18) // t_x if big else 9
    dur = rng.randint(0, max(hi, 2), (B, t_x + 3)).astype(np.int32)
    xl = np.array([t_x, t_x, max(t_x - 1, 1), max(t_x // 2, 1), 1, t_x], np.int32)
    if big:  # the last shape: row 0 is 4096 tokens of exactly 4096 frames
        dur[0, :t_x] = 1
    yl = np.array([dur[b, :xl[b]].sum() for b in range(B)], np.int32)
    return dur, xl, yl


@pytest.mark.parametrize("t_x", [1, 255, 256, 257, 4096])
def test_retime_plan(device, t_x):
    from vits_amd import ops

    rng = np.random.RandomState(t_x)
    dur, xl, yl = _plan_rows(rng, t_x, t_x == 4096)
    B = dur.shape[0]
    if t_x == 4096:
        assert yl[0] == 4096
    given = np.where(rng.rand(B, t_x) < 0.2, rng.randint(0, 12, (B, t_x)), -1).astype(np.int32)
    given[1] = -1
    scale = rng.choice([1.0, 0.5, 2.0, 1.1, 0.3, 3.7], (B, t_x)).astype(np.float32)
    rate = np.array([1.0, 1.1, 0.8, 2.0, 0.07, 1.0], np.float32)
    target = np.array([0, int(yl[1] * 1.3) + 1, 0, int(given[3, :xl[3]].clip(0).sum()) + 5, 0, 7],
                      np.int32)
    d = _dev(dur, device)[:, :t_x]
    assert d.stride(0) == t_x + 3
    dx, dy = _dev(xl, device), _dev(yl, device)
    n_served = 0
    for use in range(16):  # every subset of the four optional arguments
        g = given if use & 1 else None
        s = scale if use & 2 else None
        r = rate if use & 4 else None
        tg = target if use & 8 else None
        out, obuf = _guarded((B, t_x), I32, SENT, device)
        meta, mbuf = _guarded((2, B), I32, SENT, device)
        dn, total, status = ops.retime_plan(
            d, dy, x_len=dx, given=None if g is None else _dev(g, device),
            tok_scale=None if s is None else _dev(s, device),
            rate=None if r is None else _dev(r, device),
            target=None if tg is None else _dev(tg, device), dur=out, meta=meta)
        torch.cuda.synchronize()
        w_dn, w_total, w_st = RC.plan(dur[:, :t_x], xl, yl, g, s, r, tg)
        assert dn.data_ptr() == out.data_ptr() and dn.dtype == I32
        assert np.array_equal(dn.cpu().numpy(), w_dn), use
        assert total.cpu().tolist() == w_total.tolist() and status.cpu().tolist() == w_st.tolist()
        assert _guards_intact(obuf, B * t_x, SENT) and _guards_intact(mbuf, 2 * B, SENT)
        n_served += int((w_st == 0).sum())
        if use == 0:  # no control: the identity
            assert not w_st.any()
            for b in range(B):
                assert w_dn[b, :xl[b]].tolist() == dur[b, :xl[b]].tolist()
                assert not w_dn[b, xl[b]:].any()
        if tg is not None:
            for b in range(B):
                if tg[b] and not w_st[b]:
                    assert w_total[b] == tg[b]
    assert n_served > 60


def test_retime_plan_no_optional_argument_and_refusals(device):
    """x_len left out too; then every status-1 case, an Inf / NaN scale and
    pins above 2^18 in one ragged batch."""
    from vits_amd import ops

    rng = np.random.RandomState(3)
    dur = rng.randint(0, 9, (3, 12)).astype(np.int32)
    yl = dur.sum(1).astype(np.int32)
    dn, total, status = ops.retime_plan(_dev(dur, device), _dev(yl, device))
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy(), dur) and total.cpu().tolist() == yl.tolist()
    assert status.cpu().tolist() == [0, 0, 0]

    t_x = 8
    d = [4, 0, 6, 5, 3, 7, 2, 9]  # 36 frames
    rows = [  # (dur_old, x_len, y_len_old, given, tok_scale, rate, target) -> status
        (d, 8, 35, None, None, 1.0, 0, 1),                                  # sum != y_len_old
        (d, 7, 36, None, None, 1.0, 0, 1),                                  # (x_len cuts the sum)
        (d, 8, 36, [-1, 40, -1, -1, -1, -1, -1, -1], None, 1.0, 39, 1),     # E < 0
        (d, 8, 36, None, None, 1.0, (1 << 24) + 1, 1),                      # target > 2^24
        (d, 8, 36, [3, -1, 3, 3, 3, 3, 3, 3], None, 1.0, 22, 1),            # Qtot == 0, E != 0
        (d, 8, 36, [3, -1, 3, 3, 3, 3, 3, 3], None, 1.0, 21, 0),            # Qtot == 0, E == 0
        (d, 8, 36, None, [np.nan, np.inf, -np.inf, 1, 1e30, -1e30, 0, 1], np.nan, 0, 0),
        (d, 8, 36, None, [np.nan, np.inf, 1, 1, 1, 1, 1, 1], np.inf, 50, 0),
        (d, 8, 36, [(1 << 18) + 5, -1, -1, 1 << 30, -1, -1, -1, -1], None, 1.0, 0, 0),  # pins > 2^18
        ([(1 << 18) + 9, -3, 6, 5, 3, 7, 2, 9], 8, (1 << 18) + 32, None, None, 1.0, 0, 1),
        ([(1 << 18) + 9, -3, 6, 5, 3, 7, 2, 9], 2, 1 << 18, None, None, 0.5, 0, 0),  # clamped durs
        (d, 8, 36, None, None, 1.0, 1 << 24, 0),                            # the largest target
    ]
    B = len(rows)
    dur = np.array([r[0] for r in rows], np.int32)
    xl = np.array([r[1] for r in rows], np.int32)
    yl = np.array([r[2] for r in rows], np.int32)
    given = np.array([r[3] or [-1] * t_x for r in rows], np.int32)
    scale = np.array([r[4] or [1.0] * t_x for r in rows], np.float32)
    rate = np.array([r[5] for r in rows], np.float32)
    target = np.array([r[6] for r in rows], np.int32)
    dn, total, status = ops.retime_plan(
        _dev(dur, device), _dev(yl, device), x_len=_dev(xl, device), given=_dev(given, device),
        tok_scale=_dev(scale, device), rate=_dev(rate, device), target=_dev(target, device))
    torch.cuda.synchronize()
    w_dn, w_total, w_st = RC.plan(dur, xl, yl, given, scale, rate, target)
    assert w_st.tolist() == [r[7] for r in rows]
    assert np.array_equal(dn.cpu().numpy(), w_dn)
    assert total.cpu().tolist() == w_total.tolist() and status.cpu().tolist() == w_st.tolist()
    assert w_total[11] == 1 << 24 and w_dn[8, 0] == 1 << 18 and w_dn[8, 3] == 1 << 18
    for b in range(B):  # a refused row keeps its (clamped) durations
        if w_st[b]:
            assert w_dn[b].tolist() == [min(max(v, 0), 1 << 18) if x < xl[b] else 0
                                        for x, v in enumerate(dur[b])]


# -- the warp ---------------------------------------------------------------------------

# (dur_old, dur_new, x_len): one-token rows, then many-token rows with tokens
# going 0 -> n and n -> 0, then the refusals
WARP_ROWS = [
    ([1], [1], 1),
    ([67], [33], 1),
    ([67], [67], 1),
    ([67], [134], 1),
    ([67], [135], 1),
    ([30, 0, 41, 7, 0, 26, 50, 40], [30, 5, 41, 0, 3, 52, 25, 41], 8),    # 0 -> n, n -> 0
    ([0, 0, 60, 0, 61, 0, 0, 9], [4, 0, 30, 7, 90, 0, 2, 0], 8),          # at both ends
    ([10, 20, 30, 40, 9, 9, 9, 9], [20, 10, 60, 20, 9, 9, 9, 9], 4),      # x_len < tokens given
    ([50, 60, 70, 0, 0, 0, 0, 0], [50, 60, 70, 0, 0, 0, 0, 0], 3),        # the copy
    ([100, 50, 0, 0, 0, 0, 0, 0], [200, 101, 0, 0, 0, 0, 0, 0], 2),       # y_new > t_y
    ([0, 0, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0], 8),              # y_len_old = 0
    ([0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], 0),              # an empty row
]


def _warp_inputs(rng, C, t_rec):
    B, t_x = len(WARP_ROWS), 8
    do = np.zeros((B, t_x + 2), np.int32)  # rows strided
    dn = np.zeros((B, t_x + 5), np.int32)
    xl = np.zeros(B, np.int32)
    for b, (o, n, nx) in enumerate(WARP_ROWS):
        do[b, :len(o)], dn[b, :len(n)], xl[b] = o, n, nx
        do[b, len(o):], dn[b, len(n):] = 99, 99  # (past the tokens given: x_len hides them)
        if nx == 1:
            xl[b] = 1
    yl = np.array([do[b, :xl[b]].sum() for b in range(B)], np.int32)
    z_rec = rng.randn(B, C, t_rec).astype(np.float32)
    for b in range(B):
        z_rec[b, :, yl[b]:] = np.nan
    return do, dn, xl, yl, z_rec


@pytest.mark.parametrize("C,t_rec,t_y,off", [(6, 300, 256, 0), (192, 300, 256, 0),
                                             (6, 301, 255, 0), (6, 300, 256, 1),
                                             (192, 301, 255, 3)])
def test_retime_warp(device, C, t_rec, t_y, off):
    """t_rec != t_y; buckets that are no multiple of four; z and z_p_rec
    starting off a 16-byte boundary (off elements past one)."""
    from vits_amd import ops

    rng = np.random.RandomState(C + t_y + off)
    do, dn, xl, yl, z_rec = _warp_inputs(rng, C, t_rec)
    B, t_x = len(WARP_ROWS), 8
    mult = (1, 1, 8, 48)
    out, obuf = _guarded((B, C, t_y), torch.float32, float("nan"), device, off)
    rec, _ = _guarded((B, C, t_rec), torch.float32, float("nan"), device, off)
    rec.copy_(_dev(z_rec, device))
    assert out.data_ptr() % 16 == rec.data_ptr() % 16 == 4 * off
    d_old, d_new = _dev(do, device)[:, :t_x], _dev(dn, device)[:, :t_x]
    z, lens, meta = ops.retime_warp(rec, d_old, d_new, _dev(yl, device), t_y,
                                    x_len=_dev(xl, device), stage_mult=mult, out=out)
    torch.cuda.synchronize()
    assert z.data_ptr() == out.data_ptr()
    w_z, w_lens, w_meta = RC.warp(z_rec, do[:, :t_x], dn[:, :t_x], xl, yl, t_y, stage_mult=mult)
    assert w_meta[1].tolist() == [0] * 9 + [-1, -1, -1]
    assert w_meta[0, 9] == 301 and w_meta[0, 10] == 3  # y_new is still reported
    assert np.array_equal(meta.cpu().numpy(), w_meta) and np.array_equal(lens.cpu().numpy(), w_lens)
    got = z.cpu().numpy()
    assert np.isfinite(got).all()  # every element written, no NaN of the recording read
    assert got.view(np.int32).tolist() == w_z.view(np.int32).tolist()
    assert _guards_intact(obuf, B * C * t_y, float("nan"), off)
    assert got[2, :, :67].tobytes() == z_rec[2, :, :67].tobytes()  # 67 -> 67 copies
    assert got[8, :, :180].tobytes() == z_rec[8, :, :180].tobytes()
    for b in (9, 10, 11):
        assert not got[b].any() and not w_lens[:, b].any()


def test_retime_warp_without_x_len_and_large_tokens(device):
    """x_len left out; 4096 tokens over more than one workgroup of frames, a
    long row stretched and squeezed token by token."""
    from vits_amd import ops

    rng = np.random.RandomState(9)
    B, C, t_x = 2, 6, 4096
    do = rng.randint(0, 2, (B, t_x)).astype(np.int32)
    do[:, 0] = 1
    dn = rng.randint(0, 3, (B, t_x)).astype(np.int32)
    yl = do.sum(1).astype(np.int32)
    t_rec = int(yl.max()) + 1
    t_y = int(dn.sum(1).max()) + 7
    z_rec = rng.randn(B, C, t_rec).astype(np.float32)
    for b in range(B):
        z_rec[b, :, yl[b]:] = np.nan
    z, lens, meta = ops.retime_warp(_dev(z_rec, device), _dev(do, device), _dev(dn, device),
                                    _dev(yl, device), t_y)
    torch.cuda.synchronize()
    w_z, w_lens, w_meta = RC.warp(z_rec, do, dn, None, yl, t_y)
    assert not w_meta[1].any()
    assert np.array_equal(meta.cpu().numpy(), w_meta) and np.array_equal(lens.cpu().numpy(), w_lens)
    assert z.cpu().numpy().view(np.int32).tolist() == w_z.view(np.int32).tolist()


# -- under capture ------------------------------------------------------------------------

def test_retime_kernels_under_capture(device):
    """Plan and warp in one graph; the controls and the recording change
    between replays, nothing else: each replay equals the oracle."""
    from vits_amd import ops

    rng = np.random.RandomState(17)
    B, C, t_x, t_rec, t_y = 3, 6, 8, 300, 384
    do = np.array([[30, 0, 41, 7, 0, 26, 50, 40], [67, 0, 0, 0, 0, 0, 0, 0],
                   [10, 20, 30, 40, 9, 9, 9, 9]], np.int32)
    xl = np.array([8, 1, 4], np.int32)
    yl = np.array([do[b, :xl[b]].sum() for b in range(B)], np.int32)
    st = dict(do=_dev(do, device), xl=_dev(xl, device), yl=_dev(yl, device),
              given=torch.full((B, t_x), -1, dtype=I32, device=device),
              scale=torch.ones(B, t_x, device=device), rate=torch.ones(B, device=device),
              target=torch.zeros(B, dtype=I32, device=device),
              rec=torch.zeros(B, C, t_rec, device=device))

    def body():
        dn, total, status = ops.retime_plan(st["do"], st["yl"], x_len=st["xl"], given=st["given"],
                                            tok_scale=st["scale"], rate=st["rate"],
                                            target=st["target"])
        z, lens, meta = ops.retime_warp(st["rec"], st["do"], dn, st["yl"], t_y, x_len=st["xl"],
                                        stage_mult=(1, 8))
        return dn, total, status, z, lens, meta

    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream(device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    controls = [
        (None, None, [1.0, 1.0, 1.0], [0, 0, 0]),
        ([[-1, 4, -1, -1, -1, -1, -1, 12], [-1] * 8, [-1] * 8],
         [[1, 1, 2, 1, 1, 1, 0.5, 1], [1.0] * 8, [1, 3, 1, 1, 1, 1, 1, 1]],
         [1.1, 2.0, 0.7], [0, 0, 0]),
        (None, None, [1.0, 1.0, 1.0], [250, 135, 33]),
    ]
    for given, scale, rate, target in controls:
        z_rec = rng.randn(B, C, t_rec).astype(np.float32)
        for b in range(B):
            z_rec[b, :, yl[b]:] = np.nan
        given = np.full((B, t_x), -1, np.int32) if given is None else np.array(given, np.int32)
        scale = np.ones((B, t_x), np.float32) if scale is None else np.array(scale, np.float32)
        st["given"].copy_(_dev(given, device))
        st["scale"].copy_(_dev(scale, device))
        st["rate"].copy_(_dev(np.array(rate, np.float32), device))
        st["target"].copy_(_dev(np.array(target, np.int32), device))
        st["rec"].copy_(_dev(z_rec, device))
        for o in out:
            o.fill_(-1)  # poisoned: the replay must rewrite all of it
        graph.replay()
        torch.cuda.synchronize()
        dn, total, status, z, lens, meta = out
        w_dn, w_total, w_st = RC.plan(do, xl, yl, given, scale, np.array(rate, np.float32),
                                      np.array(target, np.int32))
        w_z, w_lens, w_meta = RC.warp(z_rec, do, w_dn, xl, yl, t_y, stage_mult=(1, 8))
        assert not w_st.any() and not w_meta[1].any()
        assert np.array_equal(dn.cpu().numpy(), w_dn) and total.cpu().tolist() == w_total.tolist()
        assert np.array_equal(meta.cpu().numpy(), w_meta)
        assert np.array_equal(lens.cpu().numpy(), w_lens)
        assert z.cpu().numpy().view(np.int32).tolist() == w_z.view(np.int32).tolist()
    assert w_total.tolist() == [250, 135, 33]

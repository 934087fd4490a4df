"""The duration-control kernels on the GPU (csrc/misc.hip): vits_duration_plan
against the numpy oracle of tests/duration_common.py, EXACTLY (dur, total,
status are integers), and the integer-duration forms of the expansion and the
start draw against numpy, bitwise.

The oracle takes w from the kernel's own w_out (no transcendental is
recomputed on the host for the comparison); w_out itself is held to numpy's
exp within a few ulp, which is what shows whether the rate, the scale and the
fp16 roundings were applied where they belong.

Bitwise expansion: the kernel computes m + (noise * s) * noise_scale.  With
noise_scale 1 or 0.5 the product by noise_scale is exact, so a fused
multiply-add of it with m rounds once, exactly as numpy's separate add does;
those are the scales used here."""
import math

import numpy as np
import pytest
import torch

import duration_common as DC
from serve_batch_common import same_state, shared_pool_draw

pytestmark = pytest.mark.gpu

SENT = -777
GUARD = 64
SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (3, 700), (2, 4096)]
KINDS = ("none", "pins_ends", "pins_zero", "single_free", "all_pinned_T_eq_P", "E_eq_0",
         "T_4096", "target_mid", "infeasible_E_lt_0", "infeasible_all_pinned", "mixed_rows")


def _guarded(device, shape, dtype, fill):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), fill, device=device, dtype=dtype)
    return full, full[GUARD:GUARD + n].view(*shape)


def _guards_intact(full, fill):
    return bool((full[:GUARD] == fill).all()) and bool((full[-GUARD:] == fill).all())


def _x_len(B, t_x):
    """Ragged rows for B > 1: the full row, about two thirds, one token."""
    return [t_x, max(1, (2 * t_x) // 3 + 1), 1][:B] if B > 1 else [t_x]


def _controls(kind, rng, logw, xl, rate_rows):
    """(given or None, target or None) of one case; rows follow xl."""
    B, t_x = logw.shape
    given = np.full((B, t_x), -1, np.int64)
    target = np.zeros(B, np.int64)
    for b, nx in enumerate(xl):
        natural = int(np.ceil(np.exp(logw[b, :nx].astype(np.float64)) * rate_rows[b]).sum())
        k = kind
        if kind == "mixed_rows":
            k = ("target_mid", "none", "infeasible_E_lt_0")[b % 3]
        if k == "pins_ends":
            given[b, 0], given[b, nx - 1] = 3, 5
        elif k == "pins_zero":
            pin = rng.random(nx) < 0.4
            pin[0] = True
            given[b, :nx][pin] = 0
        elif k == "single_free":
            given[b, :nx] = rng.integers(0, 4, nx)
            given[b, nx // 2] = -1
            target[b] = int(given[b, :nx][given[b, :nx] >= 0].sum()) + 9
        elif k in ("all_pinned_T_eq_P", "infeasible_all_pinned"):
            given[b, :nx] = rng.integers(0, 4, nx)
            given[b, 0] = 2
            target[b] = int(given[b, :nx].sum()) + (k == "infeasible_all_pinned")
        elif k in ("E_eq_0", "infeasible_E_lt_0", "target_mid"):
            pin = rng.random(nx) < 0.25
            pin[nx - 1] = nx > 1  # (one token: it stays free)
            if k == "target_mid":
                pin[0] = False     # a free token, so that every target above P + |F| fits
            given[b, :nx][pin] = rng.integers(0, 6, nx)[pin]
            P = int(given[b, :nx][pin].sum())
            nF = int((~pin).sum())
            if k == "E_eq_0":
                target[b] = P + nF
            elif k == "infeasible_E_lt_0":
                target[b] = P + nF - 1  # (0 for a lone free token: then no target at all)
            else:
                target[b] = P + nF + int(rng.integers(1, 2 * natural + 2))
        elif k == "T_4096":
            target[b] = 4096  # no pins: feasible at every t_x <= 4096
        # row padding beyond nx: pins there must be ignored
        given[b, nx:] = 7
    return given, target


def _w_ref(logw, rate_rows, scale, fit_rows, half):
    """numpy's w: exp(logw) * rate (not on fitted rows) * scale, with the fp16
    roundings of half_round."""
    w = np.exp(logw.astype(np.float32))
    r = np.where(fit_rows, 1.0, rate_rows).astype(np.float32)[:, None]
    if half:
        w = w.astype(np.float16).astype(np.float32)
        w = np.where(np.asarray(fit_rows)[:, None], w, (w * r).astype(np.float16).astype(np.float32))
        if scale is not None:
            w = (w * scale).astype(np.float16).astype(np.float32)
        return w
    w = w * r
    return w if scale is None else w * scale


def _run_case(device, rng, B, t_x, kind, use_scale, per_row_rate, half):
    from vits_amd import ops

    xl = _x_len(B, t_x)
    pad = 5
    logw_full = np.full((B, t_x + pad), np.nan, np.float32)  # strided rows, NaN behind them
    for b, nx in enumerate(xl):
        logw_full[b, :nx] = rng.normal(0.6, 0.9, nx)
    logw = logw_full[:, :t_x]
    rate_rows = (rng.uniform(0.6, 1.7, B) if per_row_rate else np.full(B, 1.25)).astype(np.float32)
    given, target = _controls(kind, rng, logw, xl, rate_rows)
    scale = None
    if use_scale:
        scale = rng.uniform(0.0, 2.5, (B, t_x)).astype(np.float32)
        scale[:, ::7] = 1.0
        if t_x > 3:
            scale[:, 3] = 0.0

    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device)
    logw_d = d(logw_full, torch.float32)[:, :t_x]
    assert logw_d.stride(0) == t_x + pad
    dur_full, dur = _guarded(device, (B, t_x), torch.int32, SENT)
    meta_full, meta = _guarded(device, (2, B), torch.int32, SENT)
    w_full, w_buf = _guarded(device, (B, t_x), torch.float32, float(SENT))
    ragged = B > 1
    rate = d(rate_rows, torch.float32) if per_row_rate else float(rate_rows[0])
    has_given = kind != "none"
    has_target = bool(np.any(target > 0)) or kind == "infeasible_E_lt_0"
    out = ops.duration_plan(
        logw_d, rate=rate, x_len=d(xl, torch.int32) if ragged else None, half_round=half,
        given=d(given, torch.int32) if has_given else None,
        tok_scale=d(scale, torch.float32) if use_scale else None,
        target=d(target, torch.int32) if has_target else None,
        w_out=w_buf, dur=dur, meta=meta)
    torch.cuda.synchronize()
    got_d, got_total, got_status, got_w = (t.cpu().numpy() for t in out)
    tag = (B, t_x, kind, use_scale, per_row_rate, half)
    assert _guards_intact(dur_full, SENT) and _guards_intact(meta_full, SENT), tag
    assert _guards_intact(w_full, float(SENT)), tag
    assert not np.any(got_d == SENT) and not np.any(got_w == SENT), tag
    assert not np.any(meta.cpu().numpy() == SENT), tag

    # w_out: 0 where nothing is free, numpy's w (a few ulp) where it is
    g_eff = given if has_given else np.full((B, t_x), -1, np.int64)
    free = np.zeros((B, t_x), bool)
    fit_rows = np.zeros(B, bool)
    for b, nx in enumerate(xl):
        free[b, :nx] = g_eff[b, :nx] < 0
        fit_rows[b] = DC.feasible(g_eff[b], target[b] if has_target else 0, nx)[1]
    assert np.all(got_w[~free] == 0), tag
    w_ref = _w_ref(np.where(free, logw, 0).astype(np.float32), rate_rows, scale, fit_rows, half)
    # fp32: expf against numpy's exp, a few ulp.  half: an ulp of exp can flip
    # an fp16 rounding (2^-11 relative), up to three roundings in a row
    tol = 2.0 ** -8 if half else 1e-5
    assert np.allclose(got_w[free], w_ref[free], rtol=tol, atol=1e-6 if half else 1e-30), tag

    want_d, want_total, want_status = DC.plan(got_w, g_eff, target if has_target else None, xl)
    assert np.array_equal(got_d, want_d), tag
    assert np.array_equal(got_total, want_total), tag
    assert np.array_equal(got_status, want_status), tag
    return got_d, got_total, got_status, target, fit_rows


@pytest.mark.parametrize("B,t_x", SHAPES, ids=[f"{b}x{t}" for b, t in SHAPES])
def test_duration_plan_equals_the_oracle(device, B, t_x):
    rng = np.random.default_rng(1000 * B + t_x)
    seen = set()
    for kind in KINDS:
        if kind == "mixed_rows" and B == 1:
            continue
        for use_scale in (False, True):
            for per_row_rate in (False, True):
                got_d, total, status, target, fit = _run_case(device, rng, B, t_x, kind, use_scale,
                                                              per_row_rate, half=False)
                if kind == "none":
                    assert not status.any()
                if kind in ("E_eq_0", "T_4096", "all_pinned_T_eq_P", "single_free", "target_mid"):
                    assert not status.any() and np.array_equal(total, target), (kind, total, target)
                if kind == "infeasible_all_pinned":
                    assert status.all()
                if kind == "infeasible_E_lt_0":
                    assert np.array_equal(status, (target > 0).astype(status.dtype))
                seen.add((kind, bool(status.any()), bool(fit.any())))
    assert any(s for _, s, _ in seen) and any(f for _, _, f in seen)


@pytest.mark.parametrize("kind", ["none", "pins_zero", "target_mid", "infeasible_all_pinned"])
def test_duration_plan_half_round(device, kind):
    """The fp16 roundings of the half model: exp, the rate, the scale."""
    rng = np.random.default_rng(5)
    for use_scale in (False, True):
        for per_row_rate in (False, True):
            _run_case(device, rng, 3, 300, kind, use_scale, per_row_rate, half=True)


def test_duration_plan_without_the_optional_arguments(device):
    """Every optional input and output left out, one at a time: the plain
    call is ceil(exp(logw) * rate) and equals the existing kernels' y_len."""
    from vits_amd import ops

    torch.manual_seed(3)
    B, t_x = 2, 41
    logw = torch.randn(B, 1, t_x, device=device) * 0.7 + 0.5
    dur, total, status = ops.duration_plan(logw, rate=1.3)
    assert dur.shape == (B, t_x) and dur.dtype == torch.int32
    assert status.tolist() == [0, 0] and torch.equal(total, dur.sum(1).to(torch.int32))
    pool = torch.zeros(64, dtype=torch.int32, device=device)
    assert torch.equal(ops.draw_starts(logw, 4, 1 << 20, pool, rate=1.3)[1], total)
    given = torch.full((B, t_x), -1, dtype=torch.int32, device=device)
    given[:, 5] = 0
    scale = torch.ones(B, t_x, device=device)
    target = torch.tensor([0, 200], dtype=torch.int32, device=device)
    x_len = torch.tensor([t_x, 30], dtype=torch.int32, device=device)
    full = dict(given=given, tok_scale=scale, target=target, x_len=x_len)
    ref = ops.duration_plan(logw, rate=1.3, w_out=True, **full)
    assert len(ref) == 4 and ref[1].tolist()[1] == 200 and ref[0][1, 30:].sum().item() == 0
    for drop in full:
        kw = {k: v for k, v in full.items() if k != drop}
        got = ops.duration_plan(logw, rate=1.3, **kw)
        assert len(got) == 3
        want = ops.duration_plan(logw, rate=1.3, **dict(
            kw, **{drop: {"given": torch.full_like(given, -1), "tok_scale": scale,
                          "target": torch.zeros_like(target),
                          "x_len": torch.full_like(x_len, t_x)}[drop]}))
        for a, b in zip(got, want):
            assert torch.equal(a, b), drop
    # scale 1 and all-free pins change nothing
    plain = ops.duration_plan(logw, rate=1.3)
    neutral = ops.duration_plan(logw, rate=1.3, given=torch.full_like(given, -1), tok_scale=scale,
                                target=torch.zeros_like(target))
    for a, b in zip(plain, neutral):
        assert torch.equal(a, b)


def test_duration_plan_under_graph_capture(device):
    """Captured once, replayed with other controls in the static buffers:
    every replay equals the eager call."""
    from vits_amd import ops

    torch.manual_seed(11)
    B, t_x = 3, 97
    st = dict(logw=torch.randn(B, t_x, device=device) * 0.6 + 0.4,
              given=torch.full((B, t_x), -1, dtype=torch.int32, device=device),
              scale=torch.ones(B, t_x, device=device),
              target=torch.zeros(B, dtype=torch.int32, device=device),
              rates=torch.ones(B, device=device),
              x_len=torch.tensor([97, 60, 1], dtype=torch.int32, device=device),
              dur=torch.zeros(B, t_x, dtype=torch.int32, device=device),
              meta=torch.zeros(2, B, dtype=torch.int32, device=device))

    def body():
        return ops.duration_plan(st["logw"], rate=st["rates"], x_len=st["x_len"],
                                 given=st["given"], tok_scale=st["scale"], target=st["target"],
                                 dur=st["dur"], meta=st["meta"])

    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream(device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    gen = torch.Generator().manual_seed(4)
    for it in range(3):
        given = torch.randint(-6, 5, (B, t_x), generator=gen, dtype=torch.int32)
        st["given"].copy_(given if it else torch.full_like(given, -1))
        st["scale"].copy_(torch.rand(B, t_x, generator=gen) * 2)
        st["target"].copy_(torch.tensor([0, 300 * it, 5 * it], dtype=torch.int32))
        st["rates"].copy_(torch.rand(B, generator=gen) + 0.5)
        graph.replay()
        got = [st["dur"].clone(), st["meta"].clone()]
        st["dur"].fill_(SENT)
        st["meta"].fill_(SENT)
        body()
        assert torch.equal(got[0], st["dur"]) and torch.equal(got[1], st["meta"])
    assert st["meta"][0].tolist()[1] == 600 and st["meta"][1].tolist()[1] == 0


# -- the integer-duration forms ---------------------------------------------------

def _int_case(device, seed=0):
    """B = 4, C = 6, t_x = 70 (ragged), bucket 192 > 64-frame tiles: durations
    with zeros, a row that sums to 0 (y_len 1, no frame) and a row longer
    than the bucket."""
    rng = np.random.default_rng(seed)
    B, C, t_x, t_y = 4, 6, 70, 192
    dur = rng.integers(0, 5, (B, t_x)).astype(np.int32)
    dur[:, ::9] = 0
    dur[1] = 0
    dur[3, 10] = 130                      # row 3: more frames than the bucket
    x_len = np.array([70, 70, 33, 64], np.int32)
    dur[2, 33:] = 9                       # behind x_len: ignored
    m = rng.normal(size=(B, C, t_x)).astype(np.float32)
    s = (rng.random((B, C, t_x)) + 0.5).astype(np.float32)
    y_len = [max(int(dur[b, :x_len[b]].sum()), 1) for b in range(B)]
    return B, C, t_x, t_y, dur, x_len, m, s, y_len


@pytest.mark.parametrize("noise_scale", [1.0, 0.5])
def test_expand_durations_int_equals_numpy_bitwise(device, noise_scale):
    from vits_amd import ops

    B, C, t_x, t_y, dur, x_len, m, s, y_len = _int_case(device)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    dur_d, xl_d, m_d, s_d = d(dur), d(x_len), d(m), d(s)
    rng = np.random.default_rng(1)
    masked = [np.where(np.arange(t_x) < x_len[b], dur[b], 0) for b in range(B)]

    # mode 0: noise [B, C, t_y]
    noise = rng.normal(size=(B, C, t_y)).astype(np.float32)
    zf, z = _guarded(device, (B, C, t_y), torch.float32, 1e30)
    _, lens = ops.expand_durations(None, m_d, s_d, d(noise), t_y, durations=dur_d, x_len=xl_d,
                                   noise_scale=noise_scale, stage_mult=(1, 3), out=z)
    assert lens[0].tolist() == y_len and lens[1].tolist() == [3 * v for v in y_len]
    assert _guards_intact(zf, 1e30)
    for b in range(B):
        want, yl = DC.expand(masked[b], m[b], s[b], noise[b], t_y, noise_scale)
        assert yl == y_len[b]
        assert np.array_equal(z[b].cpu().numpy(), want), ("mode 0", b)
    assert torch.count_nonzero(z[1]).item() == 0  # all-zero durations: y_len 1, no frame

    # mode 2: flat buffer at the starts of draw_starts(durations=)
    noise_len = C * 200  # rows 0 - 2 fit, row 3 (> 230 frames) does not
    flat = rng.normal(size=noise_len).astype(np.float32)
    np.random.seed(21)
    highs = [noise_len - C * v for v in y_len]
    want_starts = [np.random.randint(h) if h >= 1 else -1 for h in highs]
    want_state = np.random.get_state()
    np.random.seed(21)
    pool, state = ops.numpy_draw_pool(32 * B)
    starts, yl_d, status, used = ops.draw_starts(None, C, noise_len, d(pool), durations=dur_d,
                                                 x_len=xl_d)
    assert yl_d.tolist() == y_len
    assert starts.tolist() == want_starts and status.tolist()[3] == -1
    assert (starts.tolist(), status.tolist(), int(used)) == shared_pool_draw(pool, highs)
    ops.numpy_draw_commit(state, int(used))
    assert same_state(np.random.get_state(), want_state)
    z2, lens2 = ops.expand_durations(None, m_d, s_d, d(flat), t_y, durations=dur_d, x_len=xl_d,
                                     noise_scale=noise_scale, starts=starts)
    assert lens2.shape == (1, B) and lens2[0].tolist() == y_len
    for b in range(B):
        if want_starts[b] < 0:
            assert torch.count_nonzero(z2[b]).item() == 0
            continue
        n = flat[want_starts[b]:want_starts[b] + C * y_len[b]].reshape(C, y_len[b])
        want, _ = DC.expand(masked[b], m[b], s[b], n, t_y, noise_scale)
        assert np.array_equal(z2[b].cpu().numpy(), want), ("mode 2", b)

    # mode 1: a pool of raw words per row, the draw made in the expansion
    pools = rng.integers(0, 2 ** 32, (B, ops.ED_DRAWS), dtype=np.uint64).astype(np.uint32)
    z1, lens1 = ops.expand_durations(None, m_d, s_d, d(flat), t_y, durations=dur_d, x_len=xl_d,
                                     noise_scale=noise_scale,
                                     noise_start=d(pools.view(np.int32)))
    assert lens1.shape == (2, B) and lens1[0].tolist() == y_len
    for b in range(B):
        st, used_b, _ = shared_pool_draw(pools[b], [highs[b]])
        assert lens1[1].tolist()[b] == used_b[0]
        if st[0] < 0:
            assert torch.count_nonzero(z1[b]).item() == 0
            continue
        n = flat[st[0]:st[0] + C * y_len[b]].reshape(C, y_len[b])
        want, _ = DC.expand(masked[b], m[b], s[b], n, t_y, noise_scale)
        assert np.array_equal(z1[b].cpu().numpy(), want), ("mode 1", b)


def test_draw_starts_int_padding_rows_draw_nothing(device):
    from vits_amd import ops

    B, C, t_x, t_y, dur, x_len, m, s, y_len = _int_case(device, seed=2)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    noise_len = C * 400
    np.random.seed(5)
    pool, _ = ops.numpy_draw_pool(64)
    highs = [noise_len - C * v for v in y_len]
    for n_rows in (2, torch.tensor([2], dtype=torch.int32, device=device)):
        starts, yl, status, used = ops.draw_starts(None, C, noise_len, d(pool), durations=d(dur),
                                                   x_len=d(x_len), n_rows=n_rows)
        assert yl.tolist() == y_len
        assert (starts.tolist(), status.tolist(), int(used)) == shared_pool_draw(pool, highs, 2)


def test_int_forms_equal_the_logw_forms_bit_for_bit(device):
    """durations = ceil(w) from the plan: the int entries compute what the
    logw entries compute (totals <= 2048), in every noise mode, with a
    scalar and a per-row rate."""
    from vits_amd import ops

    torch.manual_seed(9)
    B, C, t_x, t_y = 3, 8, 150, 1024
    logw = torch.randn(B, 1, t_x, device=device) * 0.5 + 0.9
    x_len = torch.tensor([150, 101, 7], dtype=torch.int32, device=device)
    m = torch.randn(B, C, t_x, device=device)
    s = torch.rand(B, C, t_x, device=device) + 0.5
    noise = torch.randn(B, C, t_y, device=device)
    flat = torch.randn(C * 1100, device=device)
    pool = torch.randint(-2 ** 31, 2 ** 31 - 1, (B * ops.ED_DRAWS,), dtype=torch.int64,
                         device=device).to(torch.int32)
    for rate in (1.2, torch.tensor([0.8, 1.0, 1.9], device=device)):
        dur, total, status = ops.duration_plan(logw, rate=rate, x_len=x_len)
        assert int(total.max()) <= 2048 and int(total.max()) > 64 and not status.any()
        kw = dict(x_len=x_len, noise_scale=0.8, stage_mult=(1, 1, 8))
        a, la = ops.expand_durations(logw, m, s, noise, t_y, rate=rate, **kw)
        b, lb = ops.expand_durations(None, m, s, noise, t_y, durations=dur, **kw)
        assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(la[0], total)
        sa = ops.draw_starts(logw, C, flat.numel(), pool, rate=rate, x_len=x_len, n_rows=3)
        sb = ops.draw_starts(None, C, flat.numel(), pool, durations=dur, x_len=x_len, n_rows=3)
        for u, v in zip(sa, sb):
            assert torch.equal(u, v)
        assert int(sa[2].min()) >= 0
        a, la = ops.expand_durations(logw, m, s, flat, t_y, rate=rate, starts=sa[0], **kw)
        b, lb = ops.expand_durations(None, m, s, flat, t_y, durations=dur, starts=sb[0], **kw)
        assert torch.equal(a, b) and torch.equal(la, lb) and a.abs().sum().item() > 0
        ns = pool.view(B, ops.ED_DRAWS)
        a, la = ops.expand_durations(logw, m, s, flat, t_y, rate=rate, noise_start=ns, **kw)
        b, lb = ops.expand_durations(None, m, s, flat, t_y, durations=dur, noise_start=ns, **kw)
        assert torch.equal(a, b) and torch.equal(la, lb) and int(la[-1].min()) >= 0


def test_duration_plan_domain_is_clamped(device):
    """Inf, huge, NaN and negative w, and pins above 2^18: every duration lands
    in [0, 2^18], total is their sum, and the _int forms' y_len agrees with it."""
    from vits_amd import ops

    logw = torch.tensor([[100.0, 20.0, float("nan"), -200.0, 0.0, 0.0, 1.0, 1.0]], device=device)
    scale = torch.tensor([[1.0, 3e38, 1.0, 1.0, 3e38, 1.0, 1.0, 1.0]], device=device)
    given = torch.tensor([[-1, -1, -1, -1, -1, 1 << 20, 2147483647, 3]], dtype=torch.int32,
                         device=device)
    dur, total, status, w = ops.duration_plan(logw, given=given, tok_scale=scale, w_out=True)
    big = DC.MAX_DUR
    assert dur.tolist() == [[big, big, 0, 0, big, big, big, 3]]
    assert total.tolist() == [5 * big + 3] and status.tolist() == [0]
    want = DC.plan(w.cpu().numpy(), given.cpu().numpy())
    assert np.array_equal(dur.cpu().numpy(), want[0]) and want[1].tolist() == total.tolist()
    pool = torch.zeros(32, dtype=torch.int32, device=device)
    y_len = ops.draw_starts(None, 1, 1 << 30, pool, durations=dur)[1]
    assert y_len.tolist() == total.tolist()

"""The numpy oracle of retiming a recording (csrc/retime.hip; include/
vits_amd.h states the rules): the plan and the warp restated with array
operations in the kernels' integer and fp32 arithmetic, shared by the CPU and
GPU tests, plus the brute-force restatements the oracle itself is checked
against (tests/test_retime.py: Python big integers and fractions.Fraction for
the plan, a per-frame loop for the warp) and the shape of the golden fixture
base_retime.npz (tests/golden/make_golden_retime.py)."""
from fractions import Fraction

import numpy as np

MAX_DUR = 1 << 18  # the clamp of every duration and pin
MAX_LEN = 1 << 18  # y_len_old of a row the plan serves
MAX_TARGET = 1 << 24

# base_retime.npz: 60 frames + 57 samples, 12 tokens, hand durations with a
# token of 0 frames; the plan's controls: one pin, one scaled token, a target
GOLDEN_L = 60 * 192 + 57
GOLDEN_SID_SRC = 23
GOLDEN_SID_TGT = 7
GOLDEN_DUR_OLD = [4, 6, 3, 7, 0, 5, 9, 4, 6, 7, 3, 6]  # 60 frames
GOLDEN_GIVEN = [-1, -1, -1, 11, -1, -1, -1, -1, -1, -1, -1, -1]
GOLDEN_TOK_SCALE = [1, 1, 1, 1, 1, 1, 2.5, 1, 1, 1, 1, 1]
GOLDEN_TARGET = 71


def _clamp(d):
    return np.clip(np.asarray(d, np.int64), 0, MAX_DUR)


def scale(tok_scale, rate):
    """s of the plan: one fp32 product, clamped to [2^-8, 2^8] with fmax /
    fmin (a NaN becomes 2^-8)."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(tok_scale, f) * f(rate)
    return np.fmin(np.fmax(s, f(2.0 ** -8)), f(256.0)).astype(f)


def plan_row(dur_old, nx, y_len_old, given=None, tok_scale=None, rate=None, target=0):
    """One row of vits_retime_plan: (dur_new int64 [t_x], total, status)."""
    t_x = len(dur_old)
    nx = min(max(int(nx), 0), t_x)
    d = _clamp(dur_old)
    d[nx:] = 0
    g = np.full(t_x, -1, np.int64) if given is None else np.asarray(given, np.int64).copy()
    g[nx:] = 0  # (past the row: neither pinned frames nor free weight)
    pin = g >= 0
    pin[nx:] = True
    T = int(target)
    has_target = T > 0
    r = 1.0 if has_target or rate is None else rate
    s = scale(np.ones(t_x, np.float32) if tok_scale is None else tok_scale, r)
    q = np.rint(d.astype(np.float64) * s.astype(np.float64) * 256.0).astype(np.int64)
    q[pin] = 0
    P = int(np.minimum(g[pin], MAX_DUR).sum())
    Q = np.cumsum(q)
    Qtot = int(Q[-1]) if t_x else 0
    E = T - P if has_target else (Qtot + 128) >> 8
    ty = int(y_len_old)
    bad = (int(d.sum()) != ty or ty > MAX_LEN or E < 0 or T > MAX_TARGET
           or (has_target and Qtot == 0 and E != 0))
    if bad:
        return d, int(d.sum()), 1
    qd = max(Qtot, 1)
    B = (Q * E + qd // 2) // qd  # (Q * E < 2^60)
    out = np.diff(np.concatenate([[0], B]))  # a pinned token: B unchanged, 0 here
    out[pin] = np.minimum(g[pin], MAX_DUR)
    out[nx:] = 0
    return out, int(out.sum()), 0


def plan(dur_old, x_len, y_len_old, given=None, tok_scale=None, rate=None, target=None):
    """vits_retime_plan: (dur_new int64 [B, t_x], total [B], status [B])."""
    dur_old = np.asarray(dur_old, np.int64)
    B, t_x = dur_old.shape
    out = np.zeros((B, t_x), np.int64)
    total = np.zeros(B, np.int64)
    status = np.zeros(B, np.int64)
    for b in range(B):
        out[b], total[b], status[b] = plan_row(
            dur_old[b], t_x if x_len is None else x_len[b], y_len_old[b],
            None if given is None else given[b], None if tok_scale is None else tok_scale[b],
            None if rate is None else rate[b], 0 if target is None else target[b])
    return out, total, status


def plan_brute(dur_old, nx, y_len_old, given=None, tok_scale=None, rate=None, target=0):
    """One row of the rule in Python big integers and Fractions, token by
    token, straight from the issue's sentences: (dur_new list, status)."""
    t_x = len(dur_old)
    nx = min(max(int(nx), 0), t_x)
    d = [min(max(int(v), 0), MAX_DUR) for v in dur_old[:nx]]
    T = int(target)
    free, P, q = [], 0, {}
    for x in range(nx):
        g = -1 if given is None else int(given[x])
        if g >= 0:
            P += min(g, MAX_DUR)
            continue
        free.append(x)
        ts = np.float32(1.0 if tok_scale is None else tok_scale[x])
        r = np.float32(1.0 if T > 0 or rate is None else rate)
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.float32(ts * r)
        s = np.float32(2.0 ** -8) if np.isnan(s) else min(max(s, np.float32(2.0 ** -8)),
                                                           np.float32(256.0))
        v = Fraction(d[x]) * Fraction(float(s)) * 256  # exact
        fl = v.numerator // v.denominator
        rem = v - fl
        q[x] = fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2) else 0)
    Qtot = sum(q.values())
    E = T - P if T > 0 else (Qtot + 128) // 256
    old = d + [0] * (t_x - nx)
    if (sum(d) != int(y_len_old) or int(y_len_old) > MAX_LEN or E < 0 or T > MAX_TARGET
            or (T > 0 and Qtot == 0 and E != 0)):
        return old, 1
    out = [0] * t_x
    for x in range(nx):
        if x not in q:
            out[x] = min(int(given[x]), MAX_DUR)
    acc, b_prev = 0, 0
    for x in free:
        acc += q[x]
        b_x = (acc * E + Qtot // 2) // Qtot if Qtot else 0
        out[x] = b_x - b_prev
        b_prev = b_x
    return out, 0


def warp_sources(dur_old, dur_new, nx, ty):
    """(j0, j1, r, den) int64 [y_new] of one row of vits_retime_warp: the two
    source frames and the weight r / den of every output frame."""
    t_x = len(dur_old)
    nx = min(max(int(nx), 0), t_x)
    do, dn = _clamp(dur_old), _clamp(dur_new)
    do[nx:] = 0
    dn[nx:] = 0
    c_old = np.cumsum(do) - do
    c_new = np.cumsum(dn) - dn
    i = np.repeat(np.arange(t_x), dn)  # the owner of every output frame
    t = np.arange(len(i), dtype=np.int64)
    k = t - c_new[i]
    num = (2 * k + 1) * do[i] - dn[i]
    den = 2 * dn[i]
    qf = num // den  # floor
    r = num - qf * den
    j0 = np.clip(c_old[i] + qf, 0, ty - 1)
    j1 = np.clip(c_old[i] + qf + 1, 0, ty - 1)
    return j0, j1, r, den


def warp(z_rec, dur_old, dur_new, x_len, y_len_old, t_y, stage_mult=(1,)):
    """vits_retime_warp: (z fp32 [B, C, t_y], lens [n_stage, B], meta [2, B] =
    y_new | status).  z_rec [B, C, t_rec] is read below y_len_old only."""
    f = np.float32
    B, C, t_rec = z_rec.shape
    t_x = np.asarray(dur_old).shape[1]
    z = np.zeros((B, C, t_y), f)
    lens = np.zeros((len(stage_mult), B), np.int64)
    meta = np.zeros((2, B), np.int64)
    for b in range(B):
        nx = t_x if x_len is None else min(max(int(x_len[b]), 0), t_x)
        ty = int(y_len_old[b])
        dn = _clamp(dur_new[b])
        dn[nx:] = 0
        y_new = int(dn.sum())
        meta[0, b] = y_new
        if y_new > t_y or ty <= 0 or ty > t_rec:
            meta[1, b] = -1
            continue
        j0, j1, r, den = warp_sources(dur_old[b], dur_new[b], nx, ty)
        w = r.astype(f) / den.astype(f)  # exact operands, one rounded division
        a = z_rec[b][:, j0].astype(f)
        with np.errstate(invalid="ignore"):
            lin = a + w[None, :] * (z_rec[b][:, j1].astype(f) - a)
        z[b, :, :y_new] = np.where(((r == 0) | (j0 == j1))[None, :], a, lin)
        lens[:, b] = [y_new * int(v) for v in stage_mult]
    return z, lens, meta


def warp_brute(z_rec, dur_old, dur_new, nx, ty):
    """One row of the warp frame by frame from the issue's formulas, the
    position as a Fraction; (z [C, y_new], positions) with positions the exact
    centre-aligned source position of every frame before the clamp."""
    f = np.float32
    do = [min(max(int(v), 0), MAX_DUR) if x < nx else 0 for x, v in enumerate(dur_old)]
    dn = [min(max(int(v), 0), MAX_DUR) if x < nx else 0 for x, v in enumerate(dur_new)]
    C = z_rec.shape[0]
    y_new = sum(dn)
    z = np.zeros((C, y_new), f)
    pos = []
    t = 0
    for i in range(len(dn)):
        for k in range(dn[i]):
            # the centre of new frame k of the token, mapped onto its old frames
            p = sum(do[:i]) + Fraction(2 * k + 1, 2) * Fraction(do[i], dn[i]) - Fraction(1, 2)
            pos.append(p)
            fl = p.numerator // p.denominator
            frac = p - fl
            j0 = min(max(fl, 0), ty - 1)
            j1 = min(max(fl + 1, 0), ty - 1)
            if frac == 0 or j0 == j1:
                z[:, t] = z_rec[:, j0]
            else:
                w = f(f(frac.numerator * (2 * dn[i] // frac.denominator)) / f(2 * dn[i]))
                for c in range(C):
                    a = f(z_rec[c, j0])
                    z[c, t] = a + f(w * f(f(z_rec[c, j1]) - a))
            t += 1
    return z, pos

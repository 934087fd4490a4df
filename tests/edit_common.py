"""The numpy oracle of speech editing (csrc/edit.hip; include/vits_amd.h
states the rules): pins, splice and patch restated with array operations in
the kernels' fp32 arithmetic, shared by the CPU and GPU tests, plus the
per-frame brute-force loops the oracle itself is checked against
(tests/test_edit.py) and the shape of the golden fixture base_edit.npz
(tests/golden/make_golden_edit.py)."""
import numpy as np

MAX_DUR = 1 << 18  # the clamp of every duration

# base_edit.npz: 60 frames + 57 samples, 12 -> 13 tokens, hand durations
GOLDEN_L = 60 * 192 + 57
GOLDEN_SID = 23
GOLDEN_SPAN = (4, 7, 8)  # old tokens [4, 7) become new tokens [4, 8)
GOLDEN_DUR_OLD = [4, 6, 3, 7, 5, 2, 9, 4, 6, 5, 3, 6]  # 60 frames; the old span: 16
GOLDEN_DUR_SPAN = [6, 0, 8, 3]  # the new span: 17 frames, so y_new = 61


def _clamp(d):
    return np.clip(np.asarray(d, np.int64), 0, MAX_DUR)


def pins(dur_old, x_len_old, x_len_new, t_x_new, spans, y_len_old, span_given=None,
         span_target=None):
    """vits_edit_pins: (given int64 [B, t_x_new], target [B], meta [3, B])."""
    dur_old = np.asarray(dur_old, np.int64)
    B, t_x_old = dur_old.shape
    given = np.zeros((B, t_x_new), np.int64)
    target = np.zeros(B, np.int64)
    meta = np.zeros((3, B), np.int64)
    for b in range(B):
        nxo, nxn = int(x_len_old[b]), int(x_len_new[b])
        a, bo, bn = (int(v) for v in spans[b])
        ty = int(y_len_old[b])
        d = _clamp(dur_old[b])
        d[min(max(nxo, 0), t_x_old):] = 0
        total = int(d.sum())
        ok = (0 <= nxo <= t_x_old and 0 <= nxn <= t_x_new and 0 <= a <= bo <= nxo
              and a <= bn <= nxn and nxo - bo == nxn - bn and not (nxo > 0 and total == 0)
              and total == ty)
        if not ok:
            meta[2, b] = 1
            continue
        f0, f1 = int(d[:a].sum()), int(d[:bo].sum())
        given[b, :a] = d[:a]
        given[b, a:bn] = -1 if span_given is None else np.asarray(span_given[b])[a:bn]
        given[b, bn:nxn] = d[bo:nxo]
        given[b, nxn:] = -1
        st = 0 if span_target is None else int(span_target[b])
        target[b] = ty - (f1 - f0) + st if st > 0 else (ty if st < 0 else 0)
        meta[0, b], meta[1, b] = f0, f1
    return given, target, meta


def splice_geometry(dur_new, nx, span, ty, t_rec, t_y):
    """(f0, n_new, f1, status, total) of one row, as vits_edit_splice derives
    them from dur_new alone."""
    d = _clamp(dur_new)
    d[nx:] = 0
    cum = np.concatenate([[0], np.cumsum(d)])
    total = int(cum[-1])
    a, bo, bn = (int(v) for v in span)
    if not (0 <= a <= bn <= nx and bo >= a and 0 <= ty <= t_rec):
        return 0, 0, 0, 1, total
    f0, e1 = int(cum[a]), int(cum[bn])
    f1 = ty - (total - e1)
    if f1 < f0:
        return 0, 0, 0, 1, total
    return f0, e1 - f0, f1, (-1 if total > t_y else 0), total


def splice(dur_new, x_len_new, spans, y_len_old, m, s, noise, z_rec, stage_mult=(1,)):
    """vits_edit_splice: (z fp32 [B, C, t_y], lens [n_stage, B], meta [4, B]).
    m, s [B, C, t_x]; noise [B, C, t_y]; z_rec [B, C, t_rec]."""
    f = np.float32
    B, C, t_y = noise.shape
    t_rec = z_rec.shape[2]
    t_x = m.shape[2]
    z = np.zeros((B, C, t_y), f)
    lens = np.zeros((len(stage_mult), B), np.int64)
    meta = np.zeros((4, B), np.int64)
    for b in range(B):
        nx = t_x if x_len_new is None else min(max(int(x_len_new[b]), 0), t_x)
        f0, n_new, f1, st, total = splice_geometry(dur_new[b], nx, spans[b], int(y_len_old[b]),
                                                   t_rec, t_y)
        meta[:, b] = f0, n_new, f1, st
        if st != 0:
            continue
        ty = int(y_len_old[b])
        d = _clamp(dur_new[b])
        d[nx:] = 0
        tok = np.repeat(np.arange(t_x), d)[f0:f0 + n_new]
        e0 = f0 + n_new
        z[b, :, :f0] = z_rec[b, :, :f0]
        z[b, :, f0:e0] = m[b][:, tok].astype(f) + noise[b, :, f0:e0].astype(f) * s[b][:, tok].astype(f)
        z[b, :, e0:total] = z_rec[b, :, f1:ty]
        lens[:, b] = [total * int(v) for v in stage_mult]
    return z, lens, meta


def splice_brute(dur_new, nx, span, ty, m, s, noise, z_rec):
    """One row of the definition frame by frame (ISSUE: the spliced z_p[:, t]),
    from f0 / f1 computed the long way; None for a row the kernel refuses."""
    f = np.float32
    C, t_y = noise.shape
    a, bo, bn = span
    d = [min(max(int(v), 0), MAX_DUR) if x < nx else 0 for x, v in enumerate(dur_new)]
    f0 = sum(d[:a])
    n_new = sum(d[a:bn])
    f1 = ty - sum(d[bn:])
    y_new = f0 + n_new + (ty - f1)
    if f1 < f0 or y_new > t_y:
        return None
    z = np.zeros((C, t_y), f)
    for t in range(y_new):
        if t < f0:
            z[:, t] = z_rec[:, t]
        elif t < f0 + n_new:
            x, acc = 0, d[0]
            while acc <= t:
                x += 1
                acc += d[x]
            for c in range(C):
                z[c, t] = f(m[c, x]) + f(f(noise[c, t]) * f(s[c, x]))
        else:
            z[:, t] = z_rec[:, t - n_new + (f1 - f0)]
    return z, (f0, n_new, f1)


def patch_bounds(f0, n_new, f1, ty, hop, margin, fade):
    """(L, lo, hi, shift, fade_in, fade_out) of vits_edit_patch."""
    y_new = f0 + n_new + ty - f1
    L = y_new * hop
    lo = max(f0 - margin, 0) * hop
    hi = min(f0 + n_new + margin, y_new) * hop
    fade_in = fade > 0 and lo - fade >= 0
    fade_out = fade > 0 and hi + fade <= L
    if fade > 0 and not fade_in:
        lo = 0
    if fade > 0 and not fade_out:
        hi = L
    return L, lo, hi, (y_new - ty) * hop, fade_in, fade_out


def patch(orig, o, y_len_old, smeta, hop, margin, fade, out_cap=None):
    """vits_edit_patch: (out fp32 [B, out_cap], out_len [B]); orig [B, n], o [B, n_o]."""
    f = np.float32
    B = o.shape[0]
    out_cap = o.shape[1] if out_cap is None else out_cap
    out = np.zeros((B, out_cap), f)
    out_len = np.zeros(B, np.int64)
    for b in range(B):
        f0, n_new, f1, st = (int(v) for v in smeta[:, b])
        ty = int(y_len_old[b])
        L, lo, hi, shift, fin, fout = patch_bounds(f0, n_new, f1, ty, hop, margin, fade)
        if (st != 0 or ty < 0 or min(f0, n_new) < 0 or not f0 <= f1 <= ty
                or ty * hop > orig.shape[1] or L > o.shape[1] or L > out_cap):
            continue
        out_len[b] = L
        g, s = orig[b].astype(f), o[b].astype(f)
        row = out[b]
        row[:lo] = g[:lo]
        row[lo:hi] = s[lo:hi]
        row[hi:L] = g[hi - shift:L - shift]
        if fin:
            w = (np.arange(fade, dtype=f) + f(0.5)) / f(fade)
            i = np.arange(lo - fade, lo)
            row[i] = g[i] * (f(1) - w) + s[i] * w
        if fout:
            w = (np.arange(fade - 1, -1, -1, dtype=f) + f(0.5)) / f(fade)
            i = np.arange(hi, hi + fade)
            row[i] = g[i - shift] * (f(1) - w) + s[i] * w
    return out, out_len


def patch_brute(orig, o, ty, f0, n_new, f1, hop, margin, fade):
    """One row of the patch sample by sample, from the issue's formulas."""
    f = np.float32
    y_new = f0 + n_new + ty - f1
    L = y_new * hop
    lo = max(f0 - margin, 0) * hop
    hi = min(f0 + n_new + margin, y_new) * hop
    shift = (y_new - ty) * hop
    fin, fout = fade, fade
    if lo - fade < 0:
        lo, fin = (0, 0) if fade > 0 else (lo, 0)
    if hi + fade > L:
        hi, fout = (L, 0) if fade > 0 else (hi, 0)
    out = np.zeros(L, f)
    for i in range(L):
        if i < lo - fin:
            out[i] = orig[i]
        elif i < lo:
            w = f(f(i - (lo - fin)) + f(0.5)) / f(fade)
            out[i] = f(f(orig[i]) * f(f(1) - w)) + f(f(o[i]) * w)
        elif i < hi:
            out[i] = o[i]
        elif i < hi + fout:
            w = f(f(hi + fade - 1 - i) + f(0.5)) / f(fade)
            out[i] = f(f(orig[i - shift]) * f(f(1) - w)) + f(f(o[i]) * w)
        else:
            out[i] = orig[i - shift]
    return out

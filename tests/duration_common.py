"""The numpy oracle of the duration plan (csrc/misc.hip duration_plan_kernel,
include/vits_amd.h vits_duration_plan), shared by the CPU and GPU tests.

The oracle takes ``w`` as given (the GPU tests hand it the kernel's own
``w_out``), so no transcendental is recomputed on the host: what it restates is
the ceil, the integer fit and the infer_path-style expansion."""
import numpy as np

MAX_TARGET = 1 << 24  # the range of the kernel's int64 fit
MAX_DUR = 1 << 18     # the clamp of a pin and of ceil(w)


def ceil_frames(w):
    """ceil(w) as the kernel takes it: within [0, MAX_DUR], a NaN w -> 0."""
    w = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.ceil(np.clip(np.nan_to_num(w, nan=0.0, posinf=MAX_DUR, neginf=0.0), 0, MAX_DUR))
    return c.astype(np.int64)


def fit_weights(w):
    """q of the fit: max(llrint(clamp(w, 2^-8, 2^15) * 256) - 128, 1), int64.
    fmax / fmin, as the kernel's fmaxf / fminf: a NaN w counts as 2^-8."""
    w = np.asarray(w, np.float32)
    c = np.fmin(np.fmax(w, np.float32(2.0 ** -8)), np.float32(2.0 ** 15))
    q = np.rint(c * np.float32(256)).astype(np.int64) - 128  # rint: half to even, as llrint
    return np.maximum(q, 1)


def feasible(given_row, target, nx):
    """(has_target, fit) of one row: fit = the target can be met."""
    g = np.minimum(np.asarray(given_row[:nx], np.int64), MAX_DUR)
    free = g < 0
    P = int(g[~free].sum())
    nF = int(free.sum())
    T = int(target)
    if T <= 0:
        return False, False
    ok = T <= MAX_TARGET and ((T - P - nF) >= 0 if nF else T == P)
    return True, ok


def plan_row(w_row, given_row, target, nx):
    """One row: (dur int64 [t_x], total, status).  ``w_row``: the w of the
    free tokens (fitted rows: without the rate)."""
    t_x = len(w_row)
    g = (np.full(t_x, -1, np.int64) if given_row is None else np.asarray(given_row, np.int64))
    g = np.minimum(g, MAX_DUR)
    d = np.zeros(t_x, np.int64)
    has_t, fit = feasible(g, target, nx)
    free = np.zeros(t_x, bool)
    free[:nx] = g[:nx] < 0
    pinned = np.zeros(t_x, bool)
    pinned[:nx] = g[:nx] >= 0
    d[pinned] = g[pinned]
    if fit:
        E = int(target) - int(g[pinned].sum()) - int(free.sum())
        if free.any():
            q = fit_weights(np.asarray(w_row)[free])
            Q = np.cumsum(q)
            Qtot = int(Q[-1])
            B = (Q * E + Qtot // 2) // Qtot  # < 2^60: exact in int64
            d[free] = 1 + np.diff(np.concatenate([[0], B]))
    else:
        d[free] = ceil_frames(np.asarray(w_row, np.float32)[free])
    return d, int(d.sum()), int(has_t and not fit)


def plan(w, given=None, target=None, x_len=None):
    """Rows of plan_row: (dur int64 [B, t_x], total [B], status [B])."""
    w = np.asarray(w, np.float32)
    B, t_x = w.shape
    out = [plan_row(w[b], None if given is None else given[b],
                    0 if target is None else target[b],
                    t_x if x_len is None else min(max(int(x_len[b]), 0), t_x)) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64),
            np.array([o[2] for o in out], np.int64))


def plan_bigint(w_row, given_row, target):
    """The fit restated with Python integers and exact fractions of q (no
    numpy, no fixed width): the brute-force check of plan_row on small
    cases.  Returns (dur list, status)."""
    n = len(w_row)
    g = [-1] * n if given_row is None else [min(int(v), MAX_DUR) for v in given_row]
    free = [i for i in range(n) if g[i] < 0]
    P = sum(v for v in g if v >= 0)
    T = int(target)
    ok = T > 0 and T <= MAX_TARGET and ((T - P - len(free)) >= 0 if free else T == P)
    d = [max(v, 0) for v in g]
    if not ok:
        for i in free:
            d[i] = int(ceil_frames(w_row[i]))
        return d, int(T > 0)
    E = T - P - len(free)
    q = []
    for i in free:
        wf = float(np.float32(w_row[i]))
        c = 2.0 ** -8 if wf != wf else min(max(wf, 2.0 ** -8), 2.0 ** 15)  # NaN: the smallest
        # round half to even of c * 256 (exact: a power-of-two scale of an fp32)
        v = c * 256
        r = int(np.floor(v))
        frac = v - r
        if frac > 0.5 or (frac == 0.5 and r % 2 == 1):
            r += 1
        q.append(max(r - 128, 1))
    Qtot = sum(q)
    acc, prev = 0, 0
    for i, qi in zip(free, q):
        acc += qi
        b_i = (acc * E + Qtot // 2) // Qtot
        d[i] = 1 + b_i - prev
        prev = b_i
    return d, 0


def expand(dur_row, m, s, noise, t_y, noise_scale=1.0):
    """infer_path-style expansion of one row in the kernel's fp32 arithmetic:
    frame t belongs to the token x with cum[x - 1] <= t < cum[x]; z[c][t] =
    m[c][x] + (noise[c][t] * s[c][x]) * noise_scale for t < y_len, 0 past it.
    m, s [C, t_x]; noise [C, y_len] (already the row's slice).  Returns (z [C,
    t_y] fp32, y_len)."""
    d = np.clip(np.asarray(dur_row, np.int64), 0, 1 << 18)
    total = int(d.sum())
    y_len = max(total, 1)
    tok = np.repeat(np.arange(len(d)), d)[:t_y]
    z = np.zeros((m.shape[0], t_y), np.float32)
    n = len(tok)
    f = np.float32
    z[:, :n] = m[:, tok].astype(f) + (noise[:, :n].astype(f) * s[:, tok].astype(f)) * f(noise_scale)
    return z, y_len

"""Host side of duration control: the duration plan's rule in numpy (for paths
that have the durations on the host anyway: eager, CPU) and the checks a caller
makes before anything is uploaded.  The device side is ops.duration_plan
(csrc/misc.hip duration_plan_kernel); the two are held to one oracle
(tests/duration_common.py)."""
from __future__ import annotations

import numpy as np

MAX_FRAMES = 4096       # the longest utterance a control may ask for
MAX_TARGET = 1 << 24    # the range of the int64 fit (vits_duration_plan)
MAX_DUR = 1 << 18       # the clamp of a pin and of ceil(w) (vits_duration_plan)


def _weights(w):
    c = np.fmin(np.fmax(np.asarray(w, np.float32), np.float32(2.0 ** -8)), np.float32(2.0 ** 15))
    return np.maximum(np.rint(c * np.float32(256)).astype(np.int64) - 128, 1)


def plan_durations(w, given=None, target=0):
    """One utterance's integer durations under controls, as vits_duration_plan
    computes them.  ``w`` fp32 [t_x]: exp(logw) * tok_scale of every token,
    times the speed when there is no target (the caller applies it, with the
    half model's roundings); ``given``: None or [t_x] ints, >= 0 pins a token,
    < 0 leaves it free; ``target``: > 0 = the total to fit.  Returns (dur
    int64 [t_x], status): status 1 = the target cannot be met and ``dur`` holds
    ceil(w) for the free tokens (``w`` is used as passed)."""
    w = np.asarray(w, np.float32).reshape(-1)
    g = np.full(w.shape, -1, np.int64) if given is None else np.asarray(given, np.int64).reshape(-1)
    if g.shape != w.shape:
        raise ValueError(f"plan_durations: {g.size} pins for {w.size} tokens")
    free = g < 0
    d = np.where(free, 0, np.minimum(g, MAX_DUR))
    T, P, nF = int(target), int(d.sum()), int(free.sum())
    fit = 0 < T <= MAX_TARGET and (T - P - nF >= 0 if nF else T == P)
    if fit and nF:
        Q = np.cumsum(_weights(w[free]))
        B = (Q * (T - P - nF) + int(Q[-1]) // 2) // int(Q[-1])
        d[free] = 1 + np.diff(np.concatenate([[0], B]))
    elif not fit:
        c = np.nan_to_num(w[free], nan=0.0, posinf=MAX_DUR, neginf=0.0)
        d[free] = np.ceil(np.clip(c, 0, MAX_DUR)).astype(np.int64)
    return d, int(T > 0 and not fit)


def check_controls(t_x, durations=None, token_scale=None, target_frames=None):
    """Refuse controls that cannot be served, before anything is uploaded
    (ValueError): a length other than ``t_x``, a negative or non-finite
    scale, a target below P + |F| or (nothing free) other than P, a known
    total over MAX_FRAMES.  Returns (given int32 [t_x] or None, scale fp32
    [t_x] or None, target int, known_total or None): known_total is the
    utterance's frame count when the host already knows it (a target, or
    every token pinned), else None."""
    given = scale = None
    if durations is not None:
        given = np.asarray(durations)
        if given.ndim != 1 or given.size != t_x:
            raise ValueError(f"durations: need one value per token ({t_x}), got shape "
                             f"{given.shape}")
        if not np.issubdtype(given.dtype, np.integer):
            if not np.all(np.isfinite(given)) or np.any(given != np.round(given)):
                raise ValueError("durations: frames per token must be integers (< 0: free)")
        given = np.where(given < 0, -1, given).astype(np.int64)
        if given.max(initial=0) > MAX_FRAMES:
            raise ValueError(f"durations: a token of more than {MAX_FRAMES} frames")
        given = given.astype(np.int32)
    if token_scale is not None:
        scale = np.asarray(token_scale, np.float32)
        if scale.ndim != 1 or scale.size != t_x:
            raise ValueError(f"token_scale: need one value per token ({t_x}), got shape "
                             f"{scale.shape}")
        if not np.all(np.isfinite(scale)) or np.any(scale < 0):
            raise ValueError("token_scale: factors must be finite and >= 0")
    P = int(given[given >= 0].sum()) if given is not None else 0
    nF = int((given < 0).sum()) if given is not None else int(t_x)
    T = 0
    known = P if nF == 0 else None
    if target_frames is not None:
        T = int(target_frames)
        if T <= 0:
            raise ValueError(f"target_frames: must be > 0, got {target_frames}")
        if nF and T < P + nF:
            raise ValueError(f"target_frames: {T} frames cannot hold {P} pinned frames and "
                             f"{nF} free tokens of at least 1 frame each")
        if not nF and T != P:
            raise ValueError(f"target_frames: every token is pinned to a total of {P} frames, "
                             f"not {T}")
        known = T
    if known is not None and known > MAX_FRAMES:
        raise ValueError(f"an utterance of {known} frames is over the limit of {MAX_FRAMES}")
    return given, scale, T, known

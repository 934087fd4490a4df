"""Host restatements for the batched-serving tests (CPU and GPU files)."""
import numpy as np


def shared_pool_draw(words: np.ndarray, highs, n_rows=None):
    """misc.hip draw_starts_kernel's draw phase, line by line: row b's
    np.random.randint(highs[b]) taken with numpy's legacy masked rejection
    from ONE pool of raw MT19937 words, starting where row b - 1 stopped.
    Returns (starts, status, used_total): status = words consumed, -1 = the
    range is empty (nothing consumed), -2 = the pool ran out at this row;
    start = -1 for both.  Rows at or past n_rows draw nothing (0, 0)."""
    words = np.asarray(words).view(np.uint32)
    n_rows = len(highs) if n_rows is None else n_rows
    starts, status, pos = [], [], 0
    for b, high in enumerate(highs):
        start, used = 0, 0
        if b < n_rows:
            high = int(high)
            if high < 1 or high - 1 > 0xFFFFFFFF:
                used = -1
            elif high > 1:
                rng = high - 1
                mask = rng
                for sh in (1, 2, 4, 8, 16):
                    mask |= mask >> sh
                used = -2
                for i in range(pos, len(words)):
                    if (int(words[i]) & mask) <= rng:
                        start, used = int(words[i]) & mask, i + 1 - pos
                        break
                pos = pos + used if used > 0 else len(words)
            if used < 0:
                start = -1
        starts.append(start)
        status.append(used)
    return starts, status, pos


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]

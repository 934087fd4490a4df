"""Host side of the PCM output stage (ops.resample_* / pcm16): the filter
design, the output length, the wrappers' ratios and the C-ABI's argument
checks.  No GPU: nothing here launches a kernel."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
from scipy.signal import firwin, resample_poly

RATIOS = [(11, 10), (320, 441), (1, 2), (2, 1)]


@pytest.mark.parametrize("up,down", RATIOS)
def test_filter_is_scipys_bitwise(up, down):
    from vits_amd import ops

    table, half_len = ops.resample_filter(up, down, "cpu")
    m = max(up, down)
    assert half_len == 10 * m
    want = firwin(2 * half_len + 1, 1.0 / m, window=("kaiser", 5.0)).astype(np.float32) * np.float32(up)
    k = -(-(2 * half_len + 1) // up)
    assert tuple(table.shape) == (up, k) and table.dtype.is_floating_point and table.is_contiguous()
    flat = table.t().reshape(-1).numpy()  # flat[r + k * up] = table[r, k]
    assert np.array_equal(flat[:want.size].view(np.uint32), want.view(np.uint32))
    assert not flat[want.size:].any()
    # designed once: the same tensor on the next call, also for an unreduced ratio
    assert ops.resample_filter(up, down, "cpu")[0] is table
    assert ops.resample_filter(3 * up, 3 * down, "cpu")[0] is table


@pytest.mark.parametrize("up,down", RATIOS)
def test_out_len_is_scipys(up, down):
    from vits_amd import ops

    for n in (1, 2, 7, 255, 256, 257, 1999):
        assert ops.resample_out_len(n, up, down) == len(resample_poly(np.zeros(n), up, down)), n
    assert ops.resample_out_len(100, 7, 7) == 100


def test_ratio_helper_reproduces_the_wrappers_fractions():
    from vits_amd import ops

    sr = 22050
    steps = [(int(sr / p), sr) for p in (0.5, 0.9, 1.1, 1.3, 2.0)]
    steps += [(sr, r) for r in (8000, 16000, 24000, 44100, 48000)]
    for orig, target in steps:
        fr = Fraction(int(target), int(orig)).limit_denominator(1000)
        assert ops.resample_ratio(orig, target) == (fr.numerator, fr.denominator), (orig, target)
    assert ops.resample_ratio(22050, 16000) == (320, 441)
    assert ops.resample_ratio(int(22050 / 1.1), 22050) == (11, 10)


def test_bad_arguments_are_refused():
    from vits_amd import _lib, ops

    with pytest.raises(_lib.VitsAmdError):
        ops.resample_out_len(10, 0, 1)
    with pytest.raises(_lib.VitsAmdError):
        ops.resample_filter(1, -2)
    with pytest.raises(_lib.VitsAmdError):
        ops.resample_filter(5, 5)


def test_capi_refuses_before_launching():
    """Every invalid call returns an error code from the host-side checks (a
    GPU-less host would fail differently had anything been launched)."""
    from vits_amd import _lib

    lib = _lib.load()
    up, down, half = 2, 1, 20
    k = (2 * half + 1 + up - 1) // up
    buf = (ctypes.c_float * 4096)()
    tab = (ctypes.c_float * (up * k))()
    pcm = (ctypes.c_int16 * 4096)()
    p, t, q = (ctypes.addressof(v) for v in (buf, tab, pcm))

    def rs(x=p, dt=_lib.DT_F32, x_cap=100, lens=None, scale=1, n=100, table=t, rows=up, tk=k,
           up_=up, down_=down, half_=half, out=p, pcm_=None, out_cap=200, batch=1):
        return lib.vits_resample_poly(x, dt, x_cap, x_cap, lens, scale, n, table, rows, tk, up_,
                                      down_, half_, out, pcm_, out_cap, out_cap, 1.0, None, batch,
                                      None)

    assert rs(up_=0) == _lib.VITS_E_ARG and rs(down_=-1) == _lib.VITS_E_ARG
    assert rs(x=None) == _lib.VITS_E_ARG and rs(table=None) == _lib.VITS_E_ARG
    assert rs(out=None) == _lib.VITS_E_ARG and rs(pcm_=q) == _lib.VITS_E_ARG  # none / both
    assert rs(dt=_lib.DT_I32) == _lib.VITS_E_ARG and rs(batch=0) == _lib.VITS_E_ARG
    assert rs(lens=p, scale=0) == _lib.VITS_E_ARG
    # a table of another ratio
    assert rs(rows=up + 1) == _lib.VITS_E_SHAPE and rs(tk=k + 1) == _lib.VITS_E_SHAPE
    assert rs(half_=half + 1) == _lib.VITS_E_SHAPE
    # host length: longer than the input buffer, or n_out past the output buffer
    assert rs(n=101) == _lib.VITS_E_SHAPE and rs(out_cap=199) == _lib.VITS_E_SHAPE
    assert rs(n=-1) == _lib.VITS_E_SHAPE

    def pc(x=p, x_cap=100, n=100, out=q, out_cap=100):
        return lib.vits_pcm16(x, _lib.DT_F32, x_cap, x_cap, None, 1, n, 1.0, out, out_cap,
                              out_cap, 1, None)

    assert pc(x=None) == _lib.VITS_E_ARG and pc(out=None) == _lib.VITS_E_ARG
    assert pc(n=101) == _lib.VITS_E_SHAPE and pc(out_cap=99) == _lib.VITS_E_SHAPE

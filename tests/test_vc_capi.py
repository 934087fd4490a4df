"""Argument checks of the two voice-conversion entry points of the C ABI
(vits_stft_mag_forward_rows in csrc/stft.hip, vits_posterior_sample in
csrc/misc.hip): every call here is invalid and must come back with VITS_E_ARG
/ VITS_E_SHAPE from the host-side checks before anything is launched (the
buffers are host memory).  No GPU."""
import ctypes

import pytest

from vits_amd import _lib

ARG, SHAPE = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 8192)()
    return keep, ctypes.addressof(keep)


ROWS_GOOD = dict(x_bstride=1000, batch=2, cap=1000, n_fft=128, hop=32, win=128, pad=64,
                 frames_cap=30)
ROWS_BAD = [
    ("null x", dict(x=None), ARG),
    ("null mag", dict(mag=None), ARG),
    ("null lens", dict(lens=None), ARG),
    ("null window", dict(window=None), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("hop = 0", dict(hop=0), ARG),
    ("frames_cap = 0", dict(frames_cap=0), SHAPE),
    ("frames_cap < 0", dict(frames_cap=-3), SHAPE),
    ("pad == cap", dict(cap=64, x_bstride=64), SHAPE),
    ("pad > cap", dict(cap=50, x_bstride=50), SHAPE),
    ("win > n_fft", dict(win=129), SHAPE),
    ("n_fft not a power of two", dict(n_fft=100, win=100, pad=50), SHAPE),
    ("rows overlap", dict(x_bstride=999), SHAPE),
]


@pytest.mark.parametrize("what,over,code", ROWS_BAD, ids=[c[0] for c in ROWS_BAD])
def test_stft_rows_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(ROWS_GOOD, x=p, mag=p, lens=p, window=p)
    c.update(over)
    rc = lib.vits_stft_mag_forward_rows(c["x"], c["x_bstride"], c["batch"], c["cap"], c["lens"],
                                        c["window"], c["n_fft"], c["hop"], c["win"], c["pad"],
                                        1e-6, c["mag"], c["frames_cap"], None, None)
    assert rc == code, what


PS_GOOD = dict(ms_bstride=2 * 4 * 64, ms_cstride=64, batch=2, channels=4, t_len=64, n_stage=2)
PS_BAD = [
    ("null m", dict(m=None), ARG),
    ("null s", dict(s=None), ARG),
    ("null lens", dict(lens=None), ARG),
    ("null z", dict(z=None), ARG),
    ("batch = 0", dict(batch=0), SHAPE),
    ("channels = 0", dict(channels=0), SHAPE),
    ("t_len = 0", dict(t_len=0), SHAPE),
    ("rows of m shorter than t_len", dict(ms_cstride=63), SHAPE),
    ("stage lengths without multipliers", dict(stage_mult=None), ARG),
    ("too many stages", dict(n_stage=9), ARG),
    ("no stage", dict(n_stage=0), ARG),
]


@pytest.mark.parametrize("what,over,code", PS_BAD, ids=[c[0] for c in PS_BAD])
def test_posterior_sample_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(PS_GOOD, m=p, s=p, lens=p, z=p, stage_lens=p, stage_mult=p)
    c.update(over)
    rc = lib.vits_posterior_sample(c["m"], c["s"], c["ms_bstride"], c["ms_cstride"], None, 1.0,
                                   c["lens"], c["z"], c["batch"], c["channels"], c["t_len"],
                                   c["stage_lens"], c["stage_mult"], c["n_stage"], None)
    assert rc == code, what


def test_symbols_exported():
    assert "vits_stft_mag_forward_rows" in _lib.EXPORTED_SYMBOLS
    assert "vits_posterior_sample" in _lib.EXPORTED_SYMBOLS

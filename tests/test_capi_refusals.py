"""Argument checks of the STFT and the small inference kernels' C ABI: every
call here is invalid and must come back with VITS_E_ARG / VITS_E_SHAPE from the
host-side checks, before anything is launched (the buffers are host memory).
No GPU.  Each case names the check it exercises in csrc/stft.hip,
csrc/misc.hip or csrc/layernorm.hip."""
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


# (what, overrides, expected code): make_job's checks in csrc/stft.hip
STFT_BAD = [
    ("n_fft not a power of two", dict(n_fft=100, win=100, pad=50), SHAPE),
    ("n_fft = 4096", dict(n_fft=4096, length=8192, pad=2048), SHAPE),
    ("n_fft = 1", dict(n_fft=1, win=1, pad=0), SHAPE),
    ("win > n_fft", dict(win=129), SHAPE),
    ("pad == length", dict(length=64, pad=64), SHAPE),
    ("pad > length", dict(length=50, pad=64), SHAPE),
    ("pad < 0", dict(pad=-1), SHAPE),
    ("no frame fits, pad 0", dict(length=100, pad=0, hop=32), SHAPE),
    ("no frame fits, padded", dict(length=60, pad=32), SHAPE),
    ("one sample short", dict(length=127, pad=0), SHAPE),
    ("hop = 0", dict(hop=0), ARG),
    ("hop < 0", dict(hop=-32), ARG),
    ("null window", dict(window=None), ARG),
    ("win = 0", dict(win=0), ARG),
    ("length = 0", dict(length=0), ARG),
    ("batch = 0", dict(batch=0), ARG),
]
GOOD = dict(batch=1, length=1000, n_fft=128, hop=32, win=128, pad=64)
IDS = [c[0] for c in STFT_BAD]


def _cfg(over, p):
    c = dict(GOOD, window=p)
    c.update(over)
    return c


@pytest.mark.parametrize("what,over,code", STFT_BAD, ids=IDS)
def test_stft_forward_refuses(lib, buf, what, over, code):
    _, p = buf
    c = _cfg(over, p)
    rc = lib.vits_stft_mag_forward(p, c["batch"], c["length"], c["window"], c["n_fft"], c["hop"],
                                   c["win"], c["pad"], 1e-7, p, None, None, None)
    assert rc == code, what


def test_stft_forward_null_pointers(lib, buf):
    _, p = buf
    g = GOOD
    for x, mag in ((None, p), (p, None)):
        assert lib.vits_stft_mag_forward(x, g["batch"], g["length"], p, g["n_fft"], g["hop"],
                                         g["win"], g["pad"], 1e-7, mag, None, None, None) == ARG


@pytest.mark.parametrize("what,over,code", STFT_BAD, ids=IDS)
def test_stft_backward_refuses(lib, buf, what, over, code):
    _, p = buf
    c = _cfg(over, p)
    rc = lib.vits_stft_mag_backward(p, p, p, p, c["window"], c["batch"], c["length"], c["n_fft"],
                                    c["hop"], c["win"], c["pad"], p, p, 1 << 40, None)
    assert rc == code, what


def test_stft_backward_small_workspace(lib, buf):
    _, p = buf
    g = GOOD
    need = lib.vits_stft_workspace(g["batch"], g["length"], g["n_fft"], g["hop"], g["pad"])
    assert need > 0
    assert lib.vits_stft_mag_backward(p, p, p, p, p, g["batch"], g["length"], g["n_fft"], g["hop"],
                                      g["win"], g["pad"], p, p, need - 1, None) == ARG


def _jobs(cfgs, p):
    jobs = (_lib.StftJob * len(cfgs))()
    for j, c in zip(jobs, cfgs):
        j.x = j.grad_mag = j.mag = j.re = j.im = j.grad_x = p
        j.window = c["window"]
        j.batch, j.length, j.n_fft, j.hop, j.win, j.pad = (c[k] for k in (
            "batch", "length", "n_fft", "hop", "win", "pad"))
        j.eps, j.layout = 1e-7, 1
    return jobs


@pytest.mark.parametrize("what,over,code", STFT_BAD, ids=IDS)
def test_stft_multi_refuses(lib, buf, what, over, code):
    """A valid job followed by the invalid one: both entry points build the
    whole job table before their first launch, so the bad job refuses the call."""
    _, p = buf
    jobs = _jobs([_cfg({}, p), _cfg(over, p)], p)
    assert lib.vits_stft_mag_forward_multi(jobs, 2, None) == code, what
    assert lib.vits_stft_mag_backward_multi(jobs, 2, p, 1 << 40, None) == code, what


def test_stft_multi_job_count(lib, buf):
    _, p = buf
    jobs = _jobs([_cfg({}, p)] * 17, p)
    assert lib.vits_stft_mag_forward_multi(jobs, 0, None) == ARG
    assert lib.vits_stft_mag_forward_multi(jobs, 17, None) == ARG
    assert lib.vits_stft_mag_forward_multi(None, 1, None) == ARG
    assert lib.vits_stft_mag_backward_multi(jobs, 17, p, 1 << 40, None) == ARG
    assert lib.vits_stft_mag_backward_multi(jobs, 1, None, 1 << 40, None) == ARG
    # a workspace smaller than vits_stft_workspace_multi says
    need = lib.vits_stft_workspace_multi(jobs, 2)
    assert need == 2 * lib.vits_stft_workspace(*(GOOD[k] for k in (
        "batch", "length", "n_fft", "hop", "pad")))
    assert lib.vits_stft_mag_backward_multi(jobs, 2, p, need - 1, None) == ARG


def test_stft_workspace_counts_frames_like_python(lib):
    """batch * frames * n_fft with floor division; 0 when no frame fits (C
    division of the negative numerator gave one frame)."""
    assert lib.vits_stft_workspace(1, 100, 128, 32, 0) == 0
    assert lib.vits_stft_workspace(3, 60, 128, 32, 32) == 0
    assert lib.vits_stft_workspace(2, 127, 128, 1, 0) == 0
    assert lib.vits_stft_workspace(2, 128, 128, 1, 0) == 2 * 128
    for batch in (1, 3):
        for length in (1, 65, 100, 127, 128, 129, 333, 1000):
            for n_fft in (16, 128, 256, 1024):
                for hop in (1, 32, 100, 300):
                    for pad in (0, 8, n_fft // 2, (n_fft - hop) // 2):
                        if pad < 0:
                            continue
                        padded = length + 2 * pad
                        want = 0 if padded < n_fft else batch * ((padded - n_fft) // hop + 1) * n_fft
                        got = lib.vits_stft_workspace(batch, length, n_fft, hop, pad)
                        assert got == want, (batch, length, n_fft, hop, pad)
    assert lib.vits_stft_workspace(0, 1000, 128, 32, 64) == 0
    assert lib.vits_stft_workspace(1, 1000, 128, 0, 64) == 0


def test_stft_wrapper_frame_count():
    """The frame count both autograd wrappers allocate by: Python floor
    division, and a VitsAmdError naming the shape when no frame fits (the
    wrappers themselves are run on the device in test_stft_edges_gpu.py)."""
    from vits_amd import ops

    assert ops._stft_frames("t", 2, 128, 128, 32, 128, 0) == 1
    assert ops._stft_frames("t", 2, 1111, 1024, 192, 768, 416) == 5
    with pytest.raises(_lib.VitsAmdError, match=r"stft_mag: .*\[2, 100\].*n_fft 128"):
        ops._stft_frames("stft_mag", 2, 100, 128, 32, 128, 0)
    with pytest.raises(_lib.VitsAmdError, match=r"job 3.*\[3, 60\] with pad 32.*n_fft 128"):
        ops._stft_frames("stft_mag_multi job 3", 3, 60, 128, 32, 128, 32)


def test_expand_prior_refuses(lib, buf):
    _, p = buf

    def ep(attn=p, channels=192, t_y=8, t_x=4, batch=1):
        return lib.vits_expand_prior(attn, p, p, p, p, batch, channels, t_y, t_x, 0, 1.0, None)

    assert ep(channels=257) == SHAPE
    assert ep(attn=None) == ARG and ep(channels=0) == ARG and ep(t_x=0) == ARG
    assert ep(t_y=0) == ARG and ep(batch=0) == ARG


def test_expand_durations_refuses(lib, buf):
    _, p = buf
    mult = (ctypes.c_int32 * 9)(*([1] * 9))

    def ed(t_x=10, cstride=None, mode=0, start=None, n_stage=1, stage_mult=mult, lens=p):
        cs = t_x if cstride is None else cstride
        return lib.vits_expand_durations(p, t_x, None, t_x, 1.0, 0, p, p, 4 * cs, cs, p, mode,
                                         start, 4096, 1.0, p, 1, 4, 64, lens, stage_mult, n_stage,
                                         None)

    assert ed(t_x=4097) == SHAPE
    assert ed(cstride=9) == SHAPE  # rows of m / s shorter than t_x
    assert ed(n_stage=0) == ARG and ed(n_stage=9) == ARG
    assert ed(n_stage=2, stage_mult=None) == ARG
    assert ed(mode=1) == ARG and ed(mode=2) == ARG  # no noise_start
    assert ed(mode=3, start=p) == ARG
    assert ed(lens=None) == ARG


def test_conv_post_tanh_refuses(lib, buf):
    _, p = buf

    def cp(x=p, channels=32, t_len=64, ksize=7, cstride=64, xdtype=_lib.WDT_F32):
        return lib.vits_conv_post_tanh_lowp(x, channels * cstride, cstride, p, p, 1, channels,
                                            t_len, ksize, xdtype, None)

    assert cp(ksize=4) == SHAPE and cp(ksize=259) == SHAPE
    assert cp(cstride=63) == SHAPE
    assert cp(channels=64, ksize=9) == SHAPE  # the staged window exceeds 64 KiB of LDS
    assert cp(xdtype=7) == ARG and cp(xdtype=_lib.WDT_F32S) == ARG
    assert cp(x=None) == ARG and cp(ksize=0) == ARG and cp(t_len=0) == ARG


def test_linear_forward_refuses(lib, buf):
    _, p = buf

    def lin(g=p, g_bstride=8, n_in=8, n_out=3, batch=2):
        return lib.vits_linear_forward(g, g_bstride, p, None, p, n_out, batch, n_out, n_in, None)

    # the 16-byte row loads of n_in % 4 == 0 need rows that stay aligned
    assert lin(g_bstride=9) == SHAPE and lin(g_bstride=10) == SHAPE
    assert lin(g=p + 4) == SHAPE
    assert lin(g=None) == ARG and lin(n_in=0) == ARG and lin(n_out=0) == ARG and lin(batch=0) == ARG


def test_layer_norm_refuses(lib, buf):
    _, p = buf

    def ln(x=p, pos=None, alpha=None, channels=4, t_len=8, batch=1):
        return lib.vits_layer_norm_channels(x, None, None, None, p, batch, channels, t_len, 1e-5,
                                            None, None, 0, 1.0, pos, alpha, None)

    assert ln(pos=p) == ARG  # pos without pos_alpha
    assert ln(x=None) == ARG and ln(channels=0) == ARG and ln(t_len=0) == ARG and ln(batch=0) == ARG

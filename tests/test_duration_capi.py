"""Argument checks of the duration-control entry points of the C ABI
(vits_duration_plan, vits_expand_durations_int, vits_draw_starts_int in
csrc/misc.hip): every call here is invalid and must come back with VITS_E_ARG /
VITS_E_SHAPE / VITS_E_UNSUP from the host-side checks before anything is
launched (the buffers are host memory).  No GPU."""
import ctypes

import pytest
import torch

from vits_amd import _lib, ops

ARG, SHAPE, UNSUP = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE, _lib.VITS_E_UNSUP
NEW = ("vits_duration_plan", "vits_expand_durations_int", "vits_draw_starts_int")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 8192)()
    return keep, ctypes.addressof(keep)


def test_symbols_exported(lib):
    raw = ctypes.CDLL(_lib.lib_path())
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(raw, name)


PLAN_BAD = [
    ("null logw", dict(logw=None), ARG),
    ("null dur", dict(dur=None), ARG),
    ("null meta", dict(meta=None), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("batch < 0", dict(batch=-2), ARG),
    ("t_x = 0", dict(t_x=0, stride=12), ARG),
    ("t_x < 0", dict(t_x=-4, stride=12), ARG),
    ("row stride below t_x", dict(stride=11), SHAPE),
    ("t_x = 4097", dict(t_x=4097, stride=4097), UNSUP),
    ("t_x far beyond the limit", dict(t_x=1 << 20, stride=1 << 20), UNSUP),
]


@pytest.mark.parametrize("what,over,code", PLAN_BAD, ids=[c[0] for c in PLAN_BAD])
def test_duration_plan_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(logw=p, dur=p, meta=p, batch=2, t_x=12, stride=12)
    c.update(over)
    for opt in (p, None):  # with and without every optional pointer
        rc = lib.vits_duration_plan(c["logw"], c["stride"], opt, c["t_x"], 1.0, opt, 0, opt, opt,
                                    opt, c["dur"], c["meta"], opt, c["batch"], None)
        assert rc == code, what


EXPAND_BAD = [
    ("null dur", dict(dur=None), ARG),
    ("null m", dict(m=None), ARG),
    ("null s", dict(s=None), ARG),
    ("null noise", dict(noise=None), ARG),
    ("null z", dict(z=None), ARG),
    ("null lens", dict(lens=None), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("channels = 0", dict(channels=0), ARG),
    ("t_y = 0", dict(t_y=0), ARG),
    ("t_x = 0", dict(t_x=0), ARG),
    ("n_stage = 0", dict(n_stage=0), ARG),
    ("n_stage = 9", dict(n_stage=9), ARG),
    ("two stages without multipliers", dict(n_stage=2), ARG),
    ("mode 1 without the pool", dict(mode=1), ARG),
    ("mode 2 without starts", dict(mode=2), ARG),
    ("mode 3", dict(mode=3, start="p"), ARG),
    ("mode 2 with misaligned starts", dict(mode=2, start="p+4"), ARG),
    ("t_x = 5000", dict(t_x=5000, stride=5000, cs=5000), SHAPE),
    ("channel stride below t_x", dict(cs=11), SHAPE),
    ("row stride below t_x", dict(stride=11), SHAPE),
]


@pytest.mark.parametrize("what,over,code", EXPAND_BAD, ids=[c[0] for c in EXPAND_BAD])
def test_expand_durations_int_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(dur=p, m=p, s=p, noise=p, z=p, lens=p, batch=2, channels=4, t_y=64, t_x=12,
             stride=12, cs=12, n_stage=1, mode=0, start=None)
    c.update(over)
    start = {"p": p, "p+4": p + 4, None: None}[c["start"]]
    rc = lib.vits_expand_durations_int(c["dur"], c["stride"], None, c["t_x"], c["m"], c["s"],
                                       4 * c["cs"], c["cs"], c["noise"], c["mode"], start, 1024,
                                       1.0, c["z"], c["batch"], c["channels"], c["t_y"],
                                       c["lens"], None, c["n_stage"], None)
    assert rc == code, what


DRAW_BAD = [
    ("null dur", dict(dur=None), ARG),
    ("null pool", dict(pool=None), ARG),
    ("null starts", dict(starts=None), ARG),
    ("null meta", dict(meta=None), ARG),
    ("misaligned starts", dict(starts="p+4"), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("channels = 0", dict(channels=0), ARG),
    ("t_x = 0", dict(t_x=0), ARG),
    ("empty pool", dict(pool_n=0), ARG),
    ("noise_len = 0", dict(noise_len=0), ARG),
    ("t_x = 5000", dict(t_x=5000, stride=5000), SHAPE),
    ("batch = 1025", dict(batch=1025), SHAPE),
    ("row stride below t_x", dict(stride=11), SHAPE),
]


@pytest.mark.parametrize("what,over,code", DRAW_BAD, ids=[c[0] for c in DRAW_BAD])
def test_draw_starts_int_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(dur="p", pool="p", starts="p", meta="p", batch=2, channels=4, t_x=12, stride=12,
             pool_n=64, noise_len=1024)
    c.update(over)
    ptr = {"p": p, "p+4": p + 4, None: None}
    rc = lib.vits_draw_starts_int(ptr[c["dur"]], c["stride"], None, c["t_x"], c["channels"],
                                  c["noise_len"], ptr[c["pool"]], c["pool_n"], None, c["batch"],
                                  ptr[c["starts"]], ptr[c["meta"]], None)
    assert rc == code, what


def test_ops_refuse_durations_next_to_a_rate():
    """durations already hold the speed: a rate (or half_round) next to them is
    a caller's mistake, refused before any device is touched."""
    m = torch.zeros(2, 4, 12)
    dur = torch.ones(2, 12, dtype=torch.int32)
    for kw in (dict(rate=1.5), dict(rate=torch.ones(2)), dict(half_round=True)):
        with pytest.raises(_lib.VitsAmdError, match="not both"):
            ops.expand_durations(None, m, m, torch.zeros(2, 4, 64), 64, durations=dur, **kw)
        with pytest.raises(_lib.VitsAmdError, match="not both"):
            ops.draw_starts(None, 4, 1024, torch.zeros(64, dtype=torch.int32), durations=dur, **kw)
    for bad in (dur.long(), dur[:, :11], dur.t().contiguous().t()):
        with pytest.raises(_lib.VitsAmdError, match="int32"):
            ops.expand_durations(None, m, m, torch.zeros(2, 4, 64), 64, durations=bad)
    # and everything on the host is refused as such, not computed
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ops.duration_plan(torch.zeros(2, 12))
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ops.expand_durations(None, m, m, torch.zeros(2, 4, 64), 64, durations=dur)

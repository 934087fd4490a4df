"""Argument checks of the retiming entry points of the C ABI
(vits_retime_plan, vits_retime_warp in csrc/retime.hip): every call here is
invalid and must come back with VITS_E_ARG / VITS_E_SHAPE / VITS_E_UNSUP from
the host-side checks before anything is launched (the buffers are host
memory).  No GPU."""
import ctypes

import pytest
import torch

from vits_amd import _lib, ops

ARG, SHAPE, UNSUP = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE, _lib.VITS_E_UNSUP
NEW = ("vits_retime_plan", "vits_retime_warp")


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
    ("null dur_old", dict(dur_old=None), ARG),
    ("null y_len_old", dict(yl=None), ARG),
    ("null dur_new", dict(dur_new=None), ARG),
    ("null meta", dict(meta=None), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("batch < 0", dict(batch=-1), ARG),
    ("t_x = 0", dict(t_x=0), ARG),
    ("row stride below t_x", dict(stride=11), SHAPE),
    ("t_x = 4097", dict(t_x=4097, stride=4097), UNSUP),
]


@pytest.mark.parametrize("what,over,code", PLAN_BAD, ids=[c[0] for c in PLAN_BAD])
def test_retime_plan_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(dur_old=p, yl=p, dur_new=p, meta=p, batch=2, t_x=12, stride=12)
    c.update(over)
    for opt in (p, None):  # with and without the optional pointers
        rc = lib.vits_retime_plan(c["dur_old"], c["stride"], opt, c["t_x"], c["yl"], opt, opt, opt,
                                  opt, c["dur_new"], c["meta"], c["batch"], None)
        assert rc == code, what


WARP_BAD = [
    ("null z_p_rec", dict(rec=None), ARG),
    ("null dur_old", dict(do=None), ARG),
    ("null dur_new", dict(dn=None), ARG),
    ("null y_len_old", dict(yl=None), ARG),
    ("null z", dict(z=None), ARG),
    ("null lens", dict(lens=None), ARG),
    ("null meta", dict(meta=None), ARG),
    ("z off a 4-byte boundary", dict(z="p+2"), ARG),
    ("z_p_rec off a 4-byte boundary", dict(rec="p+1"), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("channels = 0", dict(channels=0), ARG),
    ("t_y = 0", dict(t_y=0), ARG),
    ("t_rec = 0", dict(t_rec=0), ARG),
    ("t_x = 0", dict(t_x=0), ARG),
    ("n_stage = 0", dict(n_stage=0), ARG),
    ("n_stage = 9", dict(n_stage=9), ARG),
    ("two stages without multipliers", dict(n_stage=2), ARG),
    ("old row stride below t_x", dict(so=11), SHAPE),
    ("new row stride below t_x", dict(sn=11), SHAPE),
    ("batch = 65536", dict(batch=65536), SHAPE),
    ("t_x = 4097", dict(t_x=4097, so=4097, sn=4097), UNSUP),
    ("t_rec = 2^18 + 1", dict(t_rec=(1 << 18) + 1), UNSUP),
    ("t_y = 2^18 + 1", dict(t_y=(1 << 18) + 1), UNSUP),
]


@pytest.mark.parametrize("what,over,code", WARP_BAD, ids=[c[0] for c in WARP_BAD])
def test_retime_warp_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(rec="p", do="p", dn="p", yl="p", z="p", lens="p", meta="p", batch=2, channels=4,
             t_y=64, t_rec=60, t_x=12, so=12, sn=12, n_stage=1)
    c.update(over)
    ptr = {"p": p, "p+1": p + 1, "p+2": p + 2, None: None}
    for xl in (p, None):
        rc = lib.vits_retime_warp(ptr[c["rec"]], c["t_rec"], ptr[c["do"]], c["so"], ptr[c["dn"]],
                                  c["sn"], xl, c["t_x"], ptr[c["yl"]], ptr[c["z"]], c["batch"],
                                  c["channels"], c["t_y"], ptr[c["lens"]], None, c["n_stage"],
                                  ptr[c["meta"]], None)
        assert rc == code, what


def test_ops_refuse_host_tensors_and_bad_shapes():
    """The wrappers check dtypes and shapes on the host, and everything on the
    host is refused as such, not computed."""
    i32 = torch.int32
    dur = torch.full((2, 12), 5, dtype=i32)
    yl = torch.full((2,), 60, dtype=i32)
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ops.retime_plan(dur, yl)
    with pytest.raises(_lib.VitsAmdError, match="int32"):
        ops.retime_plan(dur.long(), yl)
    with pytest.raises(_lib.VitsAmdError, match="int32"):
        ops.retime_plan(dur.t(), yl)  # rows not contiguous
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ops.retime_warp(torch.zeros(2, 4, 60), dur, dur, yl, 64)
    with pytest.raises(_lib.VitsAmdError, match="fp32"):
        ops.retime_warp(torch.zeros(2, 4, 60, dtype=torch.float64), dur, dur, yl, 64)

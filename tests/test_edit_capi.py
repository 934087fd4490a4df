"""Argument checks of the speech-editing entry points of the C ABI
(vits_edit_pins, vits_edit_splice, vits_edit_patch in csrc/edit.hip): every
call here is invalid and must come back with VITS_E_ARG / VITS_E_SHAPE /
VITS_E_UNSUP from the host-side checks before anything is launched (the
buffers are host memory).  No GPU."""
import ctypes

import pytest
import torch

from vits_amd import _lib, ops

ARG, SHAPE, UNSUP = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE, _lib.VITS_E_UNSUP
NEW = ("vits_edit_pins", "vits_edit_splice", "vits_edit_patch")


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


PINS_BAD = [
    ("null dur_old", dict(dur_old=None), ARG),
    ("null x_len_old", dict(xlo=None), ARG),
    ("null x_len_new", dict(xln=None), ARG),
    ("null spans", dict(spans=None), ARG),
    ("null y_len_old", dict(yl=None), ARG),
    ("null given", dict(given=None), ARG),
    ("null target", dict(target=None), ARG),
    ("null meta", dict(meta=None), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("batch < 0", dict(batch=-1), ARG),
    ("t_x_old = 0", dict(t_old=0), ARG),
    ("t_x_new = 0", dict(t_new=0), ARG),
    ("row stride below t_x_old", dict(stride=11), SHAPE),
    ("t_x_old = 4097", dict(t_old=4097, stride=4097), UNSUP),
    ("t_x_new = 4097", dict(t_new=4097), UNSUP),
]


@pytest.mark.parametrize("what,over,code", PINS_BAD, ids=[c[0] for c in PINS_BAD])
def test_edit_pins_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(dur_old=p, xlo=p, xln=p, spans=p, yl=p, given=p, target=p, meta=p, batch=2,
             t_old=12, t_new=13, stride=12)
    c.update(over)
    for opt in (p, None):  # with and without the optional pointers
        rc = lib.vits_edit_pins(c["dur_old"], c["stride"], c["xlo"], c["t_old"], c["xln"],
                                c["t_new"], c["spans"], opt, opt, c["yl"], c["given"],
                                c["target"], c["meta"], c["batch"], None)
        assert rc == code, what


SPLICE_BAD = [
    ("null dur_new", dict(dur=None), ARG),
    ("null spans", dict(spans=None), ARG),
    ("null y_len_old", dict(yl=None), ARG),
    ("null m", dict(m=None), ARG),
    ("null s", dict(s=None), ARG),
    ("null noise", dict(noise=None), ARG),
    ("null z_p_rec", dict(rec=None), ARG),
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
    ("row stride below t_x", dict(stride=11), SHAPE),
    ("channel stride below t_x", dict(cs=11), SHAPE),
    ("negative batch stride of m", dict(bs=-1), SHAPE),
    ("batch = 65536", dict(batch=65536), SHAPE),
    ("t_x = 4097", dict(t_x=4097, stride=4097, cs=4097), UNSUP),
]


@pytest.mark.parametrize("what,over,code", SPLICE_BAD, ids=[c[0] for c in SPLICE_BAD])
def test_edit_splice_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(dur="p", spans="p", yl="p", m="p", s="p", noise="p", rec="p", z="p", lens="p",
             meta="p", batch=2, channels=4, t_y=64, t_rec=60, t_x=12, stride=12, cs=12, bs=48,
             n_stage=1)
    c.update(over)
    ptr = {"p": p, "p+1": p + 1, "p+2": p + 2, None: None}
    for xl in (p, None):
        rc = lib.vits_edit_splice(ptr[c["dur"]], c["stride"], xl, c["t_x"], ptr[c["spans"]],
                                  ptr[c["yl"]], ptr[c["m"]], ptr[c["s"]], c["bs"], c["cs"],
                                  ptr[c["noise"]], ptr[c["rec"]], c["t_rec"], ptr[c["z"]],
                                  c["batch"], c["channels"], c["t_y"], ptr[c["lens"]], None,
                                  c["n_stage"], ptr[c["meta"]], None)
        assert rc == code, what


PATCH_BAD = [
    ("null orig", dict(orig=None), ARG),
    ("null o", dict(o=None), ARG),
    ("null y_len_old", dict(yl=None), ARG),
    ("null meta", dict(meta=None), ARG),
    ("null out", dict(out=None), ARG),
    ("null out_len", dict(out_len=None), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("orig_cap = 0", dict(orig_cap=0), ARG),
    ("o_cap = 0", dict(o_cap=0), ARG),
    ("out_cap = 0", dict(out_cap=0), ARG),
    ("hop = 0", dict(hop=0), ARG),
    ("margin < 0", dict(margin=-1), ARG),
    ("fade < 0", dict(fade=-1), ARG),
    ("orig stride below its cap", dict(orig_bs=99), SHAPE),
    ("o stride below its cap", dict(o_bs=99), SHAPE),
    ("out stride below its cap", dict(out_bs=99), SHAPE),
    ("batch = 65536", dict(batch=65536), SHAPE),
]


@pytest.mark.parametrize("what,over,code", PATCH_BAD, ids=[c[0] for c in PATCH_BAD])
def test_edit_patch_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(orig=p, o=p, yl=p, meta=p, out=p, out_len=p, batch=2, orig_cap=100, o_cap=100,
             out_cap=100, orig_bs=100, o_bs=100, out_bs=100, hop=4, margin=2, fade=8)
    c.update(over)
    rc = lib.vits_edit_patch(c["orig"], c["orig_bs"], c["orig_cap"], c["o"], c["o_bs"], c["o_cap"],
                             c["yl"], c["meta"], c["hop"], c["margin"], c["fade"], c["out"],
                             c["out_bs"], c["out_cap"], c["out_len"], c["batch"], None)
    assert rc == code, what


def test_ops_refuse_host_tensors_and_bad_shapes():
    """The wrappers check dtypes and shapes on the host, and everything on the
    host is refused as such, not computed."""
    i32 = torch.int32
    dur = torch.ones(2, 12, dtype=i32)
    xl = torch.full((2,), 12, dtype=i32)
    spans = torch.tensor([[4, 7, 8], [0, 0, 1]], dtype=i32)
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ops.edit_pins(dur, xl, xl, 13, spans, xl)
    with pytest.raises(_lib.VitsAmdError, match="int32"):
        ops.edit_pins(dur.long(), xl, xl, 13, spans, xl)
    m = torch.zeros(2, 4, 12)
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ops.edit_splice(dur, spans, xl, m, m, torch.zeros(2, 4, 64), torch.zeros(2, 4, 60))
    with pytest.raises(_lib.VitsAmdError, match="ROCm GPU"):
        ops.edit_patch(torch.zeros(2, 100), torch.zeros(2, 100), xl,
                       torch.zeros(4, 2, dtype=i32), 4, margin=2, fade=8)

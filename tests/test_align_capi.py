"""Argument checks of the forced-alignment entry point of the C ABI
(vits_maximum_path_durations in csrc/mas.hip): every call here is invalid and
must come back with VITS_E_ARG / VITS_E_UNSUP from the host-side checks before
anything is launched (the buffers are host memory).  No GPU."""
import ctypes

import pytest

from vits_amd import _lib

ARG, UNSUP = _lib.VITS_E_ARG, _lib.VITS_E_UNSUP


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 8192)()
    return keep, ctypes.addressof(keep)


GOOD = dict(batch=2, t_t=40, t_s=12)
BAD = [
    ("null neg_cent", dict(neg_cent=None), ARG),
    ("null t_t_len", dict(tt=None), ARG),
    ("null t_s_len", dict(ts=None), ARG),
    ("null durations", dict(dur=None), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("batch < 0", dict(batch=-1), ARG),
    ("t_t = 0", dict(t_t=0), ARG),
    ("t_s = 0", dict(t_s=0), ARG),
    ("t_s < 0", dict(t_s=-5), ARG),
    ("null workspace", dict(ws=None), ARG),
    ("workspace one byte short", dict(ws_short=1), ARG),
    ("no workspace bytes", dict(ws_bytes=0), ARG),
    ("global decision words, workspace one byte short", dict(t_t=1600, t_s=129, ws_short=1), ARG),
    ("t_s beyond the widest kernel", dict(t_s=2049), UNSUP),
    ("t_s far beyond the widest kernel", dict(t_s=1 << 20), UNSUP),
]


@pytest.mark.parametrize("what,over,code", BAD, ids=[c[0] for c in BAD])
def test_maximum_path_durations_refuses(lib, buf, what, over, code):
    _, p = buf
    c = dict(GOOD, neg_cent=p, tt=p, ts=p, dur=p, ws=p, ws_short=0)
    c.update(over)
    need = int(lib.vits_maximum_path_workspace(c["batch"], c["t_t"], c["t_s"]))
    ws_bytes = c.get("ws_bytes", need - c["ws_short"])
    for scores, tokens in ((p, p), (None, None)):
        rc = lib.vits_maximum_path_durations(c["neg_cent"], c["tt"], c["ts"], c["dur"], scores,
                                             tokens, c["batch"], c["t_t"], c["t_s"], c["ws"],
                                             ws_bytes, None)
        assert rc == code, what


def test_workspace_switch_sits_between_the_kernel_test_shapes(lib):
    """(1500, 129) keeps the decision words in LDS, (1600, 129) puts them in
    the workspace: the two shapes of tests/test_align_kernel_gpu.py take the
    kernel's two instantiations."""
    small = int(lib.vits_maximum_path_workspace(4, 1500, 129))
    large = int(lib.vits_maximum_path_workspace(4, 1600, 129))
    assert small == 2 * 4 * 4 + 256
    assert large == small + 4 * (1600 // 32) * 256 * 4


def test_symbol_exported():
    assert "vits_maximum_path_durations" in _lib.EXPORTED_SYMBOLS

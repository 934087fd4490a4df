"""Argument checks and the workspace layout of the long MAS entries of the C
ABI (vits_mas_long_* in csrc/mas_long.hip): every call here is invalid and
must come back with VITS_E_ARG / VITS_E_UNSUP from the host-side checks before
anything is launched (the buffers are host memory).  No GPU."""
import ctypes

import pytest

from vits_amd import _lib

ARG, UNSUP = _lib.VITS_E_ARG, _lib.VITS_E_UNSUP
NAMES = ("vits_mas_long_workspace", "vits_mas_long_panel", "vits_mas_long_backtrack",
         "vits_mas_long_gather", "vits_mas_long_scores")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 64)()
    p = ctypes.addressof(keep)
    return keep, (p + 15) & ~15


GOOD = dict(batch=2, t_t=200, t_s=150, strip=64, panel=32, y0=64, rows=32, bstride=200 * 150)
# (what, overrides, code, entries it applies to: p panel, b backtrack, g gather, s scores)
BAD = [
    ("null scores matrix", dict(nc=None), ARG, "pg"),
    ("null t_t_len", dict(tt=None), ARG, "pbgs"),
    ("null t_s_len", dict(ts=None), ARG, "pbgs"),
    ("null durations", dict(dur=None), ARG, "b"),
    ("null token scores", dict(sc=None), ARG, "s"),
    ("null workspace", dict(ws=None), ARG, "pbgs"),
    ("batch = 0", dict(batch=0), ARG, "pbgs"),
    ("batch < 0", dict(batch=-3), ARG, "pbgs"),
    ("t_t = 0", dict(t_t=0), ARG, "pbgs"),
    ("t_s = 0", dict(t_s=0), ARG, "pbgs"),
    ("t_s < 0", dict(t_s=-5), ARG, "pbgs"),
    ("strip = 0", dict(strip=0), ARG, "pbgs"),
    ("panel = 0", dict(panel=0), ARG, "pbgs"),
    ("panel < 0", dict(panel=-32), ARG, "pbgs"),
    ("panel no multiple of 32", dict(panel=48, y0=48), ARG, "pbgs"),
    ("panel 33", dict(panel=33, y0=0), ARG, "pbgs"),
    ("strip 32", dict(strip=32), ARG, "pbgs"),
    ("strip 96", dict(strip=96), ARG, "pbgs"),
    ("strip 192 = 64 * 3", dict(strip=192), ARG, "pbgs"),
    ("strip 4096 = 64 * 2^6", dict(strip=4096), ARG, "pbgs"),
    ("strip 2049", dict(strip=2049), ARG, "pbgs"),
    ("y0 no multiple of panel", dict(y0=16), ARG, "pg"),
    ("y0 one past a multiple", dict(y0=65), ARG, "pg"),
    ("y0 < 0", dict(y0=-32), ARG, "pg"),
    ("y0 past the frames", dict(y0=224), ARG, "pg"),
    ("rows = 0", dict(rows=0), ARG, "pg"),
    ("rows < 0", dict(rows=-1), ARG, "pg"),
    ("rows above panel", dict(rows=33), ARG, "pg"),
    ("rows past the frames", dict(y0=192, rows=9), ARG, "pg"),
    ("a short panel that is not the last", dict(rows=31), ARG, "pg"),
    ("batch stride below one panel", dict(bstride=32 * 150 - 1), ARG, "pg"),
    ("workspace one byte short", dict(ws_short=1), ARG, "pbgs"),
    ("no workspace bytes", dict(ws_bytes=0), ARG, "pbgs"),
    ("workspace not 16-byte aligned", dict(ws_off=4), ARG, "pbgs"),
    ("panel beyond the LDS", dict(panel=1 << 20, y0=0, rows=200), UNSUP, "pbgs"),
]


def _calls(lib, c, ws_bytes):
    dims = (c["batch"], c["t_t"], c["t_s"], c["strip"], c["panel"])
    ws = None if c["ws"] is None else c["ws"] + c.get("ws_off", 0)
    tail = (ws, ws_bytes, None)
    return {
        "p": lambda: lib.vits_mas_long_panel(c["nc"], c["bstride"], c["tt"], c["ts"], *dims,
                                             c["y0"], c["rows"], *tail),
        "b": lambda: lib.vits_mas_long_backtrack(c["tt"], c["ts"], c["dur"], c["ft"], *dims,
                                                 *tail),
        "g": lambda: lib.vits_mas_long_gather(c["nc"], c["bstride"], c["tt"], c["ts"], *dims,
                                              c["y0"], c["rows"], *tail),
        "s": lambda: lib.vits_mas_long_scores(c["tt"], c["ts"], c["sc"], *dims, *tail),
    }


@pytest.mark.parametrize("what,over,code,entries", BAD, ids=[c[0] for c in BAD])
def test_long_entries_refuse(lib, buf, what, over, code, entries):
    _, p = buf
    c = dict(GOOD, nc=p, tt=p, ts=p, dur=p, ft=p, sc=p, ws=p, ws_short=0)
    c.update(over)
    need = int(lib.vits_mas_long_workspace(c["batch"], c["t_t"], c["t_s"], c["strip"],
                                           c["panel"]))
    if need == 0:  # sizes no plan exists for: the calls still see a large workspace
        need = 1 << 40
    ws_bytes = c.get("ws_bytes", need - c["ws_short"])
    calls = _calls(lib, c, ws_bytes)
    for e in entries:
        assert calls[e]() == code, (what, e)
    if "b" in entries:  # frame_token is optional and does not change a refusal
        c["ft"] = None
        assert _calls(lib, c, ws_bytes)["b"]() == code, what


def _up256(n):
    return (n + 255) // 256 * 256


def _layout_bytes(batch, t_t, t_s, strip):
    """include/vits_amd.h: the five sections, each rounded up to 256 bytes."""
    ws = -(-t_s // strip) * strip
    nblk = -(-t_t // 32)
    return (_up256(4 * 2 * batch * ws) + _up256(4 * batch * nblk * ws) + _up256(4 * batch * t_t)
            + _up256(4 * batch * (ws + 1)) + _up256(4 * batch * t_t))


SIZES = [(1, 1, 1, 64, 32), (2, 200, 150, 64, 32), (3, 200, 150, 128, 64),
         (1, 2100, 2049, 2048, 4096), (1, 4200, 100, 128, 4096), (1, 50000, 8300, 2048, 4096),
         (4, 97, 65, 64, 96)]


@pytest.mark.parametrize("batch,t_t,t_s,strip,panel", SIZES)
def test_workspace_is_the_documented_layout(lib, batch, t_t, t_s, strip, panel):
    got = int(lib.vits_mas_long_workspace(batch, t_t, t_s, strip, panel))
    assert got == _layout_bytes(batch, t_t, t_s, strip)


def test_workspace_of_ten_minutes_stays_far_below_the_matrix(lib):
    """50 000 frames against 8 192 tokens: the decision words are 1/32 of the
    1.6 GB matrix, the rest is a few hundred KB."""
    got = int(lib.vits_mas_long_workspace(1, 50000, 8192, 2048, 4096))
    words = 4 * 1563 * 8192
    assert words <= got <= words + (1 << 20)
    assert got < 50000 * 8192 * 4 // 30


@pytest.mark.parametrize("over", [dict(batch=0), dict(t_t=0), dict(t_s=-1), dict(strip=96),
                                  dict(strip=4096), dict(panel=40), dict(panel=0),
                                  dict(panel=1 << 20)])
def test_workspace_is_zero_for_what_the_calls_refuse(lib, over):
    c = dict(batch=1, t_t=100, t_s=70, strip=64, panel=32)
    c.update(over)
    assert lib.vits_mas_long_workspace(c["batch"], c["t_t"], c["t_s"], c["strip"],
                                       c["panel"]) == 0


def test_symbols_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS

"""vits_resample_poly_span's C ABI: the export, and every refusal of its
header comment, returned by the host-side checks before anything is launched
(the buffers are host memory).  No GPU."""
import ctypes

import pytest

from vits_amd import _lib, ops

ARG, SHAPE = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE
UP, DOWN, HL = 1, 2, 20
K = (2 * HL + UP) // UP


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 8192)()
    return keep, ctypes.addressof(keep)


# a signal of 1000 samples, the window [100, 400): outputs [80, 180) of the
# 1:2 pass need the inputs [140, 379)
GOOD = dict(dt=_lib.DT_F32, x_lo=100, x_len=300, n_in=1000, rows=UP, k=K, up=UP, down=DOWN, hl=HL,
            out_lo=80, out_len=100, volume=1.0)


def _call(lib, p, null=(), pcm=False, both=False, **over):
    c = dict(GOOD, **over)
    out = None if ("out" in null or (pcm and not both)) else p
    return lib.vits_resample_poly_span(
        None if "x" in null else p, c["dt"], c["x_lo"], c["x_len"], c["n_in"],
        None if "table" in null else p, c["rows"], c["k"], c["up"], c["down"], c["hl"], out,
        p if (pcm or both) else None, c["out_lo"], c["out_len"], c["volume"], None)


def test_symbol():
    assert "vits_resample_poly_span" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "vits_resample_poly_span")
    for name in ("resample_poly_span", "resample_pcm16_span", "resample_span_input"):
        assert callable(getattr(ops, name))


def test_the_good_call_needs_what_the_helper_says():
    """GOOD is refused by nothing below but its own override: its window
    holds resample_span_input's range with room on both sides."""
    lo, hi = ops.resample_span_input(80, 180, 1000, UP, DOWN, HL)
    assert (lo, hi) == (140, 379)
    assert GOOD["x_lo"] < lo and hi < GOOD["x_lo"] + GOOD["x_len"]


BAD = [
    ("negative x_lo", dict(x_lo=-1), ARG),
    ("negative x_len", dict(x_len=-1), ARG),
    ("negative n_in", dict(n_in=-1), ARG),
    ("negative out_lo", dict(out_lo=-1), ARG),
    ("negative out_len", dict(out_len=-1), ARG),
    ("up = 0", dict(up=0), ARG),
    ("down = 0", dict(down=0), ARG),
    ("unknown dtype", dict(dt=99), ARG),
    ("table of another up", dict(rows=2), SHAPE),
    ("half_len of another ratio", dict(hl=10), SHAPE),
    ("table_k of another ratio", dict(k=K + 1), SHAPE),
    ("window starts one sample late", dict(x_lo=141, x_len=259), SHAPE),
    ("window ends one sample early", dict(x_lo=100, x_len=278), SHAPE),
    ("window elsewhere", dict(x_lo=500, x_len=300), SHAPE),
    ("empty window", dict(x_len=0), SHAPE),
    ("span to the signal's end, window not", dict(out_lo=400, out_len=200), SHAPE),
    ("x_lo + x_len overflows", dict(x_lo=2 ** 63 - 10, x_len=300), SHAPE),
    ("out_lo + out_len overflows", dict(out_lo=2 ** 63 - 10, out_len=100), SHAPE),
    ("n * down overflows", dict(out_lo=2 ** 62, out_len=100), SHAPE),
    ("n_in * up overflows", dict(n_in=2 ** 63 - 1, up=3, down=2, rows=3, hl=30, k=21), SHAPE),
    ("a grid past 2^31 blocks", dict(out_lo=0, out_len=2 ** 40, n_in=0), SHAPE),
]


@pytest.mark.parametrize("what,over,code", BAD, ids=[c[0] for c in BAD])
def test_span_refuses(lib, buf, what, over, code):
    assert _call(lib, buf[1], **over) == code, what
    assert _call(lib, buf[1], pcm=True, **over) == code, what


def test_span_null_pointers_and_outputs(lib, buf):
    p = buf[1]
    assert _call(lib, p, null=("x",)) == ARG
    assert _call(lib, p, null=("table",)) == ARG
    assert _call(lib, p, null=("out",)) == ARG  # neither output
    assert _call(lib, p, both=True) == ARG  # both outputs


def test_copy_form_refusals(lib, buf):
    """up == down == 1: no table is needed, the window must hold the span
    itself, cut at the signal's end."""
    p = buf[1]
    copy = dict(up=1, down=1, rows=0, k=0, hl=0)
    assert _call(lib, p, null=("table",), out_lo=150, out_len=100, x_lo=151, **copy) == SHAPE
    assert _call(lib, p, null=("table",), out_lo=150, out_len=100, x_lo=100, x_len=149,
                 **copy) == SHAPE
    assert _call(lib, p, null=("table",), out_lo=950, out_len=100, x_lo=900, x_len=99,
                 **copy) == SHAPE


def test_nothing_to_compute_launches_nothing(lib, buf):
    """A span of no samples is VITS_OK without a launch (there is no GPU here
    to launch on), with or without a window."""
    assert _call(lib, buf[1], out_len=0) == _lib.VITS_OK
    assert _call(lib, buf[1], null=("x",), x_len=0, out_len=0) == _lib.VITS_OK

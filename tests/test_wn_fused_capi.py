"""Argument checks of the fused WN layer's C ABI (csrc/wn_f32p.hip,
vits_wn_layers_f32p_forward and the mixed vits_conv1d_wn_seq_forward): every
call here is invalid and must come back with VITS_E_ARG / VITS_E_SHAPE from the
host-side checks, before anything is launched (the buffers are host memory).
No GPU."""
import ctypes

import pytest

from vits_amd import _lib
from vits_amd._lib import ConvDesc, WnLayerDesc

ARG, SHAPE = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(keep) + 63) & ~63  # 64-byte aligned
    return keep, base


def _good(p, last=False):
    """A descriptor that passes every check (never launched: host memory)."""
    d = WnLayerDesc()
    d.h, d.h_bstride, d.h_cstride, d.t_len = p, 256 * 64, 64, 64
    d.hidden, d.k, d.dil, d.last = 256, 5, 1, int(last)
    d.w1, d.m_pad1, d.cin_pad1 = p + 1024, 512, 256
    d.w2, d.m_pad2, d.cin_pad2 = p + 2048, 256 if last else 512, 256
    if not last:
        d.h_out, d.ho_bstride, d.ho_cstride = p + 4096, 256 * 64, 64
    d.skip, d.skip_bstride, d.skip_cstride = p + 8192, 256 * 64, 64
    return d


def _call(lib, d, n=1, batch=1):
    return lib.vits_wn_layers_f32p_forward(ctypes.byref(d) if d is not None else None, n, batch,
                                           None)


BAD = [
    ("null h", dict(h=None), ARG),
    ("null w1", dict(w1=None), ARG),
    ("null w2", dict(w2=None), ARG),
    ("null skip", dict(skip=None), ARG),
    ("null h_out on a middle layer", dict(h_out=None), ARG),
    ("h updated in place", dict(h_out="h"), ARG),
    ("skip aliases h", dict(skip="h"), ARG),
    ("tile columns 48", dict(ng=48), ARG),
    ("H = 192", dict(hidden=192), SHAPE),
    ("H = 512", dict(hidden=512), SHAPE),
    ("even k", dict(k=4), SHAPE),
    ("window too wide", dict(k=15, dil=5), SHAPE),
    ("T % 4 != 0", dict(t_len=62), SHAPE),
    ("channel stride % 4 != 0", dict(h_cstride=66), SHAPE),
    ("batch stride % 4 != 0", dict(h_bstride=256 * 64 + 2), SHAPE),
    ("channel stride < T", dict(h_cstride=60), SHAPE),
    ("skip stride < T", dict(skip_cstride=60), SHAPE),
    ("h not 16-byte aligned", dict(h="+4"), SHAPE),
    ("w1 not 16-byte aligned", dict(w1="+8"), SHAPE),
    ("m_pad1 < 2H", dict(m_pad1=256), SHAPE),
    ("cin_pad2 != H", dict(cin_pad2=128), SHAPE),
    ("32-bit lane offsets", dict(h_cstride=1 << 23, h_bstride=1 << 31), SHAPE),
]


@pytest.mark.parametrize("what,over,code", BAD, ids=[c[0] for c in BAD])
def test_wn_layer_refuses(lib, buf, what, over, code):
    _, p = buf
    d = _good(p)
    for key, val in over.items():
        if val == "h":
            val = d.h
        elif isinstance(val, str):
            val = getattr(d, key) + int(val)
        setattr(d, key, val)
    assert _call(lib, d) == code, what


def test_wn_layers_refuse_null_and_empty(lib, buf):
    _, p = buf
    d = _good(p)
    assert _call(lib, None) == ARG
    assert _call(lib, d, n=0) == ARG
    assert _call(lib, d, n=-1) == ARG
    assert _call(lib, d, batch=0) == ARG


def test_last_layer_takes_no_h_out(lib, buf):
    _, p = buf
    d = _good(p, last=True)
    d.h_out = p + 4096
    assert _call(lib, d) == ARG


def test_a_bad_layer_refuses_the_whole_stack(lib, buf):
    """Every descriptor is checked before the first launch: a stack whose
    second layer is invalid returns its error (a launch of the first on host
    memory would not return)."""
    _, p = buf
    arr = (WnLayerDesc * 2)(_good(p), _good(p))
    arr[1].hidden = 192
    assert lib.vits_wn_layers_f32p_forward(arr, 2, 1, None) == SHAPE


def test_mixed_sequence_refuses(lib, buf):
    _, p = buf
    wn = (WnLayerDesc * 1)(_good(p))
    conv = (ConvDesc * 1)()  # all zero: null pointers
    kinds = (ctypes.c_int32 * 2)(0, 1)
    f = lib.vits_conv1d_wn_seq_forward
    assert f(conv, 1, wn, 1, None, 2, 1, None) == ARG          # null kinds
    assert f(conv, 1, wn, 1, kinds, 0, 1, None) == ARG         # n = 0
    assert f(conv, 1, wn, 1, kinds, 1, 1, None) == ARG         # counts do not add up
    assert f(None, 1, wn, 1, kinds, 2, 1, None) == ARG         # null conv array
    assert f(conv, 1, None, 1, kinds, 2, 1, None) == ARG       # null WN array
    assert f(conv, 1, wn, 1, kinds, 2, 1, None) == ARG         # the conv's null pointers
    bad = (ctypes.c_int32 * 2)(1, 1)                            # more WN items than given
    assert f(conv, 1, wn, 1, bad, 2, 1, None) == ARG
    wn[0].hidden = 192
    only = (ctypes.c_int32 * 1)(1)
    assert f(None, 0, wn, 1, only, 1, 1, None) == SHAPE        # unsupported H


def test_struct_layout_matches_header():
    """ctypes WnLayerDesc equals the C vits_wn_layer_desc (size and the offsets
    of fields behind each change of alignment), checked by compiling a probe."""
    import os
    import subprocess
    import tempfile

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ("w1", "b1", "cond_bstride", "w2", "h_out", "accumulate", "skip", "len_skip", "ng",
              "lengths")
    probe = ('#include <stdio.h>\n#include <stddef.h>\n#include "vits_amd.h"\n'
             'int main(){printf("%zu", sizeof(vits_wn_layer_desc));\n'
             + "".join(f'printf(" %zu", offsetof(vits_wn_layer_desc, {f}));\n' for f in fields)
             + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(WnLayerDesc)
    for f, off in zip(fields, out[1:]):
        assert int(off) == getattr(WnLayerDesc, f).offset, f

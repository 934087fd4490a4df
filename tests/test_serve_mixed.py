"""Mixed-request serving without a GPU: the per-row entry points are declared,
exported and bound; every invalid call comes back from the host-side checks of
csrc/post.hip and csrc/misc.hip before anything is launched (the buffers are
host memory); ops refuses a per-row rate that is not fp32; and
VITSWrap.speaking_many on a CPU speecher is the loop over speaking."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import HERE
from vits_amd import _lib

ARG, SHAPE = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE
NEW = ("vits_expand_durations_rows", "vits_draw_starts_rows", "vits_resample_poly_rows",
       "vits_pack_pcm_rows")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 8192)()
    return keep, ctypes.addressof(keep)


def test_new_symbols_declared_exported_and_bound():
    with open(os.path.join(os.path.dirname(HERE), "include", "vits_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    raw = ctypes.CDLL(_lib.lib_path())
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert "vits_post_row;" in header
    # the per-row launches count under no family, as vits_resample_poly: the
    # families of the header and of the binding are the ten there were
    assert len(_lib.CNT_NAMES) == int(re.search(r"#define VITS_CNT_N (\d+)", header).group(1)) == 10
    from vits_amd import ops
    from vits_amd.infer import EmoVITS, PcmRequest
    from vits_amd.vits_wrap import VITSWrap

    assert callable(ops.resample_rows) and callable(ops.pack_pcm_rows)
    assert callable(EmoVITS.infer_pcm_requests) and callable(VITSWrap.speaking_many)
    r = PcmRequest(items=[])
    assert (r.duration_rate, r.pitch, r.sampling_rate, r.volume, r.tail_silence) == (1, 1, None, 1, 0)


def test_post_row_layout_matches_header(tmp_path):
    import subprocess

    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vits_amd.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(vits_post_row), '
                   'offsetof(vits_post_row, up), offsetof(vits_post_row, table_k), '
                   'offsetof(vits_post_row, volume)); return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    P = _lib.PostRow
    assert [int(v) for v in out] == [ctypes.sizeof(P), P.up.offset, P.table_k.offset,
                                     P.volume.offset]


# -- vits_resample_poly_rows ------------------------------------------------------

def _row(p, up=11, down=10, half_len=None, k=None, table=True, volume=1.0):
    half_len = 10 * max(up, down) if half_len is None else half_len
    k = (2 * half_len + up) // max(1, up) if k is None else k
    return _lib.PostRow(p if table else None, up, down, half_len, k, volume, 0)


def _resample_rows(lib, p, rows, **over):
    a = dict(x=p, dt=_lib.DT_F32, xs=64, xc=64, lens=p, scale=1, out=p, pcm=None, os=128, oc=128,
             olens=None, batch=len(rows))
    a.update(over)
    arr = (_lib.PostRow * max(1, len(rows)))(*rows)
    return lib.vits_resample_poly_rows(a["x"], a["dt"], a["xs"], a["xc"], a["lens"], a["scale"],
                                       None if over.get("rows_null") else arr, a["out"], a["pcm"],
                                       a["os"], a["oc"], a["olens"], a["batch"], None)


RESAMPLE_ROWS_BAD = [
    ("null x", dict(x=None), ARG),
    ("null lens (device lengths are required)", dict(lens=None), ARG),
    ("null rows", dict(rows_null=True), ARG),
    ("no output", dict(out=None), ARG),
    ("two outputs", dict(pcm="p"), ARG),
    ("batch = 0", dict(batch=0), ARG),
    ("len_scale = 0", dict(scale=0), ARG),
    ("int32 input", dict(dt=_lib.DT_I32), ARG),
    ("batch above the limit", dict(batch=65), SHAPE),
    ("row stride below the capacity", dict(xs=63), SHAPE),
    ("out stride below the capacity", dict(os=127), SHAPE),
]


@pytest.mark.parametrize("what,over,code", RESAMPLE_ROWS_BAD, ids=[c[0] for c in RESAMPLE_ROWS_BAD])
def test_resample_rows_refuses(lib, buf, what, over, code):
    _, p = buf
    over = {k: (p if v == "p" else v) for k, v in over.items()}
    assert _resample_rows(lib, p, [_row(p), _row(p, 1, 1, table=False)], **over) == code, what


ROW_BAD = [
    ("K of another ratio", dict(k=20), SHAPE),            # 11 / 10: K = (220 + 11) // 11 = 21
    ("half_len of another ratio", dict(half_len=100), SHAPE),
    ("a ratio without its table", dict(table=False), ARG),
    ("up = 0", dict(up=0), ARG),
    ("down < 0", dict(down=-1), ARG),
]


@pytest.mark.parametrize("what,over,code", ROW_BAD, ids=[c[0] for c in ROW_BAD])
def test_resample_rows_refuses_a_bad_row(lib, buf, what, over, code):
    """The descriptor of the LAST row is wrong; the rows before it are fine."""
    _, p = buf
    good = _row(p)
    assert (good.half_len, good.table_k) == (110, 21)
    assert _resample_rows(lib, p, [good, _row(p, 1, 1, table=False), _row(p, **over)]) == code, what


# -- vits_pack_pcm_rows -------------------------------------------------------------

def _pack_rows(lib, p, batch=3, ups=None, downs=None, tails=None, **over):
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    a = dict(rows=p, bs=64, cap=64, y=p, hop=4, up=i32(ups or [1] * 2 * batch),
             down=i32(downs or [1] * 2 * batch), tail=i32(tails or [0] * batch), nr=None,
             batch=batch, offs=p, out=p, oc=1024)
    a.update(over)
    return lib.vits_pack_pcm_rows(a["rows"], a["bs"], a["cap"], a["y"], a["hop"], a["up"],
                                  a["down"], a["tail"], a["nr"], a["batch"], a["offs"], a["out"],
                                  a["oc"], None)


def test_pack_pcm_rows_refuses(lib, buf):
    _, p = buf
    for name in ("rows", "y", "offs", "out", "up", "down", "tail"):
        assert _pack_rows(lib, p, **{name: None}) == ARG, name
    assert _pack_rows(lib, p, hop=0) == ARG
    assert _pack_rows(lib, p, oc=0) == ARG
    assert _pack_rows(lib, p, cap=0) == ARG
    assert _pack_rows(lib, p, batch=65) == SHAPE        # above the pack limit of 64
    assert _pack_rows(lib, p, bs=63) == SHAPE
    assert _pack_rows(lib, p, ups=[1, 1, 0, 1, 1, 1]) == ARG
    assert _pack_rows(lib, p, downs=[1, 1, 1, 1, 1, -2]) == ARG
    assert _pack_rows(lib, p, tails=[0, -1, 0]) == ARG
    assert _pack_rows(lib, p, cap=2 ** 31 - 8, bs=2 ** 31, tails=[0, 16, 0]) == SHAPE


# -- per-row speed --------------------------------------------------------------------

def test_rows_entry_points_refuse_null_rates(lib, buf):
    _, p = buf
    mult = (ctypes.c_int32 * 1)(1)
    assert lib.vits_expand_durations_rows(p, 12, None, 12, None, 0, p, p, 48, 12, p, 0, None, 64,
                                          1.0, p, 2, 4, 64, p, mult, 1, None) == ARG
    assert lib.vits_draw_starts_rows(p, 12, None, 12, None, 0, 4, 1024, p, 64, None, 2, p, p,
                                     None) == ARG
    # with rates given the other checks are the scalar entry points'
    assert lib.vits_expand_durations_rows(p, 12, None, 5000, p, 0, p, p, 48, 5000, p, 0, None, 64,
                                          1.0, p, 2, 4, 64, p, mult, 1, None) == SHAPE
    assert lib.vits_draw_starts_rows(p, 12, None, 12, p, 0, 4, 1024, None, 64, None, 2, p, p,
                                     None) == ARG


def test_ops_refuse_a_rate_that_is_no_fp32_row_tensor():
    """Checked before anything else, so it needs no GPU: the tensors here are
    on the CPU and a valid rate would be refused for that instead."""
    from vits_amd import ops

    logw = torch.zeros(4, 1, 12)
    m = torch.zeros(4, 4, 12)
    bad = [torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float16),
           torch.ones(4, dtype=torch.int32), torch.ones(3), torch.ones(4, 1), torch.ones(8)[::2],
           "1.0", None, [1.0] * 4]
    for rate in bad:
        with pytest.raises(_lib.VitsAmdError, match="rate"):
            ops.expand_durations(logw, m, m, torch.zeros(4, 4, 64), 64, rate=rate)
        with pytest.raises(_lib.VitsAmdError, match="rate"):
            ops.draw_starts(logw, 4, 1024, torch.zeros(64, dtype=torch.int32), rate=rate)
    with pytest.raises(_lib.VitsAmdError, match="fp32"):
        ops._rate_arg(torch.ones(4, dtype=torch.float64), 4, "draw_starts")
    assert ops._rate_arg(2, 4, "x") == (2.0, None)
    assert ops._rate_arg(np.float32(0.5), 4, "x") == (0.5, None)
    with pytest.raises(_lib.VitsAmdError, match="GPU"):  # right form, wrong device
        ops._rate_arg(torch.ones(4), 4, "x")


def test_row_wrappers_refuse_bad_arguments_without_a_gpu():
    from vits_amd import ops

    with pytest.raises(_lib.VitsAmdError):
        ops.resample_rows(torch.zeros(2, 8), [(1, 1), (1, 2)],
                          lengths=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.VitsAmdError):
        ops.pack_pcm_rows(torch.zeros(2, 8, dtype=torch.int16), torch.zeros(2, dtype=torch.int32),
                          4, [[], []], [0, 0])


# -- VITSWrap.speaking_many on a CPU speecher -------------------------------------------

class _CpuSpeecher:
    """EmoVITS's interface as far as VITSWrap's host path uses it."""
    device = torch.device("cpu")
    sampling_rate = 16000

    def infer(self, spkid, text, emo, *, duration_rate=1.0):
        n = max(1, int(round(text.shape[0] * 40 * duration_rate)))
        rs = np.random.RandomState(int(abs(float(text.sum())) * 1000) % 2 ** 31)
        return rs.uniform(-1, 1, n).astype(np.float32), (spkid, 0) if emo is None else emo

    def update(self):
        pass


class _Parser:
    max_utt_length = 10

    def __call__(self, utt_id, text):
        rs = np.random.RandomState(len(text))
        return utt_id, text, rs.randn(max(1, len(text)), 8).astype(np.float32)


def _inputs():
    return [{"id": "a", "text": "abcdefghi。jklmnopq。rstu", "spkid": 1, "emotion": (1, 0)},
            {"id": "b", "text": "hello", "spkid": 2, "speed": 0.8, "pitch": 1.2,
             "sampling_rate": 8000, "volume": 0.7, "tail_silence": 0.01, "emotion": (1, 1)},
            {"id": "c", "text": "xyz", "speed": 1.3, "sampling_rate": 24000, "emotion": (1, 2)}]


def test_speaking_many_on_a_cpu_model_is_the_loop():
    from vits_amd.vits_wrap import VITSWrap

    wrap = VITSWrap(textparser=_Parser(), speecher=_CpuSpeecher(), batch_segments=True)
    assert wrap.batch_segments is False  # (CUDA only)
    want = [wrap.speaking(i) for i in _inputs()]
    got = wrap.speaking_many(_inputs())
    assert len(got) == len(want) == 3
    for a, b in zip(want, got):
        assert a["wav"] == b["wav"] and len(b["wav"]) > 44 and a["sr"] == b["sr"]
        assert a["segment_info"] == b["segment_info"]
        assert set(a) == set(b)
    assert [len(b["segment_info"]) for b in got] == [3, 1, 1]
    assert wrap.speaking_many([]) == []

"""Voice conversion of long recordings, CPU side: the window plan
(EmoVITS._long_plan), the context a window needs
(SynthesizerTrn.vc_context_frames against a restatement from the config's
numbers, its decoder part against a reach measured on a random-weight
Generator), the limits of the long entry points and the refusals of
vits_copy_windows' C ABI.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from common import BASE_DATA, BASE_MODEL, build_model, tiny_cfg
from vits_amd import _lib

N_FFT, HOP, WIN = 1024, 192, 768
STFT = (N_FFT, HOP, WIN)
ARG, SHAPE = _lib.VITS_E_ARG, _lib.VITS_E_SHAPE


@pytest.fixture(scope="module")
def ev_cpu(tmp_path_factory):
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    c = tiny_cfg()
    data = dict(c["data"], spec_channels=N_FFT // 2 + 1)
    hps = get_hparams_from_dict({
        "data": {"sampling_rate": 16000, "filter_length": N_FFT, "hop_length": HOP,
                 "win_length": WIN, "text_channels": data["text_channels"],
                 "n_speakers": data["n_speakers"], "noise_scale": 0.667},
        "model": c["model"]})
    model = build_model(c["model"], data, "cpu")
    return EmoVITS(str(tmp_path_factory.mktemp("vcl") / "ckpt.pth"), "cpu", hps=hps, model=model)


# -- the plan ---------------------------------------------------------------------


def _check_plan(plan, n, wf, ctx):
    F, cf = n // HOP, wf - 2 * ctx
    assert len(plan) == math.ceil(F / cf)
    nxt = 0
    for i, w in enumerate(plan):
        # the cores tile [0, F) exactly once, in order, and none is empty
        assert w.core_lo == nxt and w.core_lo < w.core_hi <= F
        nxt = w.core_hi
        # the row holds its core and fits the window
        assert 0 <= w.a <= w.core_lo and w.core_hi <= w.b <= F
        assert w.b - w.a <= wf
        assert w.s0 == w.a * HOP and w.core_off == (w.core_lo - w.a) * HOP
        # a row that reaches the last frame runs to the last sample (the
        # reflection at its end is then the recording's), the others end on a frame
        assert w.s1 == (n if w.b == F else w.b * HOP)
        assert w.b == F or i < len(plan) - 1
        assert w.s1 - w.s0 <= wf * HOP + HOP - 1
        assert (w.s1 - w.s0) // HOP == w.b - w.a  # the frames the row's STFT gives
        # an artificial edge lies at least ctx frames from the core; the others are true
        assert w.a == 0 or w.core_lo - w.a >= ctx
        assert w.b == F or w.b - w.core_hi >= ctx
    assert nxt == F
    assert plan[0].s0 == 0 and plan[0].a == 0  # the recording's true start
    assert plan[-1].s1 == n and plan[-1].b == F  # and its true end, remainder included


def test_plan_properties(ev_cpu):
    """Every F in 1 .. 3 * Cf + 2 and F = 50 000 at window_frames 256 and a
    context of 113 (Cf = 30), each with n % hop in {0, 1, hop - 1}.  At these
    F a row reaches both true ends (F < 2 * 113), so F in 257 .. 257 + 3 * Cf
    + 2, where rows have artificial edges on one side or on both, runs too."""
    wf, ctx = 256, 113
    cf = wf - 2 * ctx
    both = 0
    for F in list(range(1, 3 * cf + 3)) + list(range(257, 257 + 3 * cf + 3)) + [50000]:
        for rem in (0, 1, HOP - 1):
            n = F * HOP + rem
            plan = ev_cpu._long_plan(n, wf, ctx)
            _check_plan(plan, n, wf, ctx)
            both += sum(1 for w in plan if w.a > 0 and w.b < F)
    assert both > 0  # (the property on artificial edges was exercised on both sides at once)
    # the serving default and a recording of ten minutes
    ctx = 113
    _check_plan(ev_cpu._long_plan(16000 * 600 + 5, 4096, ctx), 16000 * 600 + 5, 4096, ctx)
    assert ev_cpu._long_plan(HOP - 1, wf, 113) == []


def test_plan_refuses_window_without_core(ev_cpu):
    with pytest.raises(ValueError):
        ev_cpu._long_plan(1000 * HOP, 256, 128)  # Cf = 0
    with pytest.raises(ValueError):
        ev_cpu._long_plan(1000 * HOP, 256, 200)
    assert len(ev_cpu._long_plan(1000 * HOP, 256, 127)) == 500  # Cf = 2


# -- the context ------------------------------------------------------------------


def _context_ref(cfg):
    """The four parts restated from the config's numbers, the decoder
    FORWARDS (which samples does one input frame reach?), where the model
    goes backwards (which input frames does one frame of samples need?)."""
    pad = (N_FFT - HOP) // 2
    rows = 64  # frames of a row long enough that its two ends do not meet
    left = sum(1 for j in range(rows) if j * HOP - pad < 0)
    right = sum(1 for j in range(rows) if j * HOP - pad + N_FFT > rows * HOP)
    enc_q = sum((cfg["kernel_size_q"] - 1) // 2 for _ in range(cfg["n_layers_q"]))  # dilation 1
    flow = sum((5 - 1) // 2 * dr ** i for dr in cfg["dilation_rate"] for i in range(4))
    lo, hi = -3, 3  # conv_pre, kernel 7, around input frame 0
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        p = (k - u) // 2
        lo, hi = lo * u - p, hi * u - p + k - 1  # input i reaches i * u - p + [0, k)
        r = max(sum((kr - 1) // 2 * d + (kr - 1) // 2 for d in ds)
                for kr, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
        lo, hi = lo - r, hi + r
    lo, hi = lo - 3, hi + 3  # conv_post, kernel 7
    dec = max(-(lo // HOP), hi // HOP)  # frames of samples reached on either side
    return max(left, right), enc_q, 2 * flow, dec


@pytest.mark.parametrize("which", ["base", "tiny"])
def test_context_matches_restatement(which):
    if which == "base":
        cfg, data = BASE_MODEL, BASE_DATA
    else:
        c = tiny_cfg()
        cfg, data = c["model"], dict(c["data"], spec_channels=N_FFT // 2 + 1)
    model = build_model(cfg, data, "cpu", fill=False)
    parts = _context_ref(cfg)
    print(f"{which}: stft {parts[0]} + enc_q {parts[1]} + flows {parts[2]} + decoder {parts[3]}")
    assert model.dec.context_frames() == parts[3]
    assert model.vc_context_frames(STFT) == sum(parts)
    if which == "base":
        assert parts == (3, 32, 64, 14)  # the figures of the design note
    model.remove_weight_norm()  # (the serving model: the same modules without weight norm)
    assert model.vc_context_frames(STFT) == sum(parts)
    with pytest.raises(ValueError):
        model.vc_context_frames((N_FFT, HOP // 2, WIN))


def test_decoder_context_is_the_measured_reach():
    """A random-weight Generator of the tiny config in float64 on its CPU
    (autograd) path: the gradient of the sum of frame f's hop samples with
    respect to z is non-zero exactly on the input frames that frame depends
    on (all weights, inputs and so every partial product are positive: no
    cancellation; a derivative is a product, never absorbed by a sum of
    larger terms, which is what a finite change of z would suffer).  The
    derived reach is at least the measured one and at most one frame more."""
    from vits_amd.models import Generator

    c = tiny_cfg()["model"]
    torch.manual_seed(0)
    dec = Generator(c["inter_channels"], c["resblock"], c["resblock_kernel_sizes"],
                    c["resblock_dilation_sizes"], c["upsample_rates"],
                    c["upsample_initial_channel"], c["upsample_kernel_sizes"],
                    gin_channels=c["gin_channels"]).double()
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if name.endswith("weight_g"):
                # w = g * v / |v| ~ 1 / fan: every layer's output is of the order of its input
                fan = dec.get_parameter(name[:-1] + "v")[0].numel()
                p.uniform_(0.5, 1.5).div_(fan ** 0.5)
            elif name.endswith("weight_v"):
                p.uniform_(0.5, 1.5)
            elif name.endswith("bias"):
                p.zero_()
            else:  # conv_pre / conv_post: plain weights
                p.uniform_(0.5, 1.5).div_(p[0].numel())
    hop = math.prod(c["upsample_rates"])
    derived = dec.context_frames()
    T, f = 2 * derived + 9, derived + 4
    z = torch.rand(1, c["inter_channels"], T, dtype=torch.float64).add_(0.5).requires_grad_()
    g = torch.rand(1, c["gin_channels"], dtype=torch.float64) * 0.1
    out = dec(z, g)
    assert out.shape == (1, 1, T * hop)
    out[0, 0, f * hop:(f + 1) * hop].sum().backward()
    touched = torch.nonzero(z.grad[0].abs().amax(0)).flatten()
    measured = max(f - int(touched.min()), int(touched.max()) - f)
    print(f"decoder reach: derived {derived}, measured {measured} frames "
          f"(frames {int(touched.min())} .. {int(touched.max())} around {f})")
    assert 0 < int(touched.min()) and int(touched.max()) < T - 1  # (not cut by the ends)
    assert measured <= derived <= measured + 1


# -- the limits of the long entry points ----------------------------------------


def test_long_limits_and_cpu_refusal(ev_cpu):
    from vits_amd._lib import VitsAmdError

    big = ev_cpu.LONG_MAX_SAMPLES
    assert big == 2 ** 31 - 1
    assert ev_cpu._long_check(big, None) == big // HOP
    with pytest.raises(ValueError):
        ev_cpu._long_check(big + 1, None)
    with pytest.raises(ValueError):
        ev_cpu._long_check(416, None)  # _vc_lengths' refusal: at most pad samples
    # twice the rate out doubles the samples; the tail counts
    with pytest.raises(ValueError):
        ev_cpu._long_check(big // 2 + HOP, None, ev_cpu._output(1.0, 32000, 1.0, 0.0))
    n = 1000 * HOP
    assert ev_cpu._long_check(n, None, ev_cpu._output(1.0, 32000, 1.0, 0.0)) == 1000
    with pytest.raises(ValueError):
        ev_cpu._long_check(n, None, ev_cpu._output(1.0, 16000, 1.0, float(big) / 16000))
    # 4097 frames: past convert's cap, fine here
    assert ev_cpu._vc_lengths(4097 * HOP)[2] == 4097
    wav = np.zeros(4097 * HOP, dtype=np.int16)
    with pytest.raises(VitsAmdError):
        ev_cpu.convert_long(wav, 1, 2)
    with pytest.raises(VitsAmdError):
        ev_cpu.convert_pcm_long(wav, 1, 2)


# -- vits_copy_windows: every call is refused before anything is launched --------


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    keep = (ctypes.c_float * 4096)()
    return keep, ctypes.addressof(keep)


def _jobs(*jobs):
    return (_lib.WindowJob * len(jobs))(*[_lib.WindowJob(*j) for j in jobs])


GOOD = dict(src_numel=4096, src_rstride=0, dst_numel=4096, dst_rstride=0, jobs=[(0, 0, 16, 32)],
            channels=1)
COPY_BAD = [
    ("no job", dict(jobs=[]), ARG),
    ("negative len", dict(jobs=[(0, 0, -1, 8)]), ARG),
    ("fill_len < len", dict(jobs=[(0, 0, 16, 15)]), ARG),
    ("negative src_off", dict(jobs=[(-1, 0, 16, 16)]), ARG),
    ("negative dst_off", dict(jobs=[(0, -4, 16, 16)]), ARG),
    ("channels = 0", dict(channels=0), ARG),
    ("negative stride", dict(channels=2, src_rstride=-1, dst_rstride=64), ARG),
    ("negative size", dict(dst_numel=-1), ARG),
    ("65 jobs", dict(jobs=[(0, 32 * j, 16, 32) for j in range(65)]), SHAPE),
    ("channels > 65535", dict(channels=65536), SHAPE),
    ("read past src", dict(jobs=[(4090, 0, 16, 16)]), SHAPE),
    ("write past dst", dict(jobs=[(0, 4080, 16, 32)]), SHAPE),
    ("last channel reads past src", dict(channels=5, src_rstride=1024, dst_rstride=64,
                                         jobs=[(0, 0, 16, 16)], src_numel=4 * 1024 + 15), SHAPE),
    ("last channel writes past dst", dict(channels=5, src_rstride=64, dst_rstride=1024,
                                          jobs=[(0, 1, 16, 16)], dst_numel=4 * 1024 + 16), SHAPE),
    ("offset overflows int64", dict(jobs=[(2 ** 63 - 1, 0, 16, 16)]), SHAPE),
    ("stride overflows int64", dict(channels=3, src_rstride=2 ** 62, dst_rstride=64), SHAPE),
    ("channels overlap in dst", dict(channels=2, src_rstride=64, dst_rstride=31), SHAPE),
]


def _call(lib, p, null=(), **over):
    c = dict(GOOD, **over)
    table = _jobs(*c["jobs"]) if c["jobs"] else _jobs((0, 0, 0, 0))
    return lib.vits_copy_windows(None if "src" in null else p, c["src_numel"], c["src_rstride"],
                                 None if "dst" in null else p, c["dst_numel"], c["dst_rstride"],
                                 None if "jobs" in null else table, len(c["jobs"]),
                                 c["channels"], None)


@pytest.mark.parametrize("what,over,code", COPY_BAD, ids=[c[0] for c in COPY_BAD])
def test_copy_windows_refuses(lib, buf, what, over, code):
    assert _call(lib, buf[1], **over) == code, what


def test_copy_windows_null_and_misaligned_pointers(lib, buf):
    p = buf[1]
    for which in ("src", "dst", "jobs"):
        assert _call(lib, p, null=(which,)) == ARG, which
    assert _call(lib, p + 2) == ARG  # (fp32 elements lie on 4-byte boundaries)


def test_copy_windows_nothing_to_write_launches_nothing(lib, buf):
    """Jobs whose fill_len is 0 write nothing: VITS_OK with no launch (there
    is no GPU here to launch on)."""
    assert _call(lib, buf[1], jobs=[(0, 0, 0, 0), (5, 7, 0, 0)]) == _lib.VITS_OK


def test_symbol_and_struct(lib):
    assert "vits_copy_windows" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "vits_copy_windows")
    assert ctypes.sizeof(_lib.WindowJob) == 32 and _lib.WindowJob.fill_len.offset == 24
    from vits_amd import ops

    assert ops.COPY_MAX_JOBS == 64

"""vits_resample_poly_span on the GPU: a span of the output stage computed
from a window of its input against the SAME samples of the whole-signal
kernels (ops.resample_poly / resample_pcm16 / pcm16), bitwise.

Shapes.  A signal of 3001 samples (odd, twelve workgroups of the whole-signal
kernel); the ratios of pitch 1.1 at 16 kHz (3200 / 2909: 3200 phase rows of
21 taps), a halving, a doubling and the copy; spans of one sample, of one
workgroup and a sample, an interior one of two workgroups and a sample at an
offset that is no multiple of anything, the signal's end with 100 samples of
silence behind it, and silence alone.  The window is exactly what
ops.resample_span_input asks for, inside an allocation of NaN: a read outside
it, or a zero tap multiplied with it, shows in the result."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_IN = 3001
RATIOS = [(3200, 2909), (1, 2), (2, 1), (1, 1)]
DTYPES = [torch.float32, torch.float16]
VOLUME = 0.8
PAST = 200  # zeros the whole-signal reference carries behind n_out
_REFS = {}


def _case(device, up, down, dtype):
    """(signal, fp32 reference, int16 reference), computed once per case."""
    from vits_amd import ops

    key = (up, down, dtype)
    if key not in _REFS:
        g = torch.Generator().manual_seed(up + down)
        x = (torch.randn(N_IN, generator=g) * 0.4).to(dtype).to(device)
        n_out = ops.resample_out_len(N_IN, up, down)
        f = torch.full((n_out + PAST,), float("nan"), device=device)
        p = torch.full((n_out + PAST,), 77, device=device, dtype=torch.int16)
        ops.resample_poly(x, up, down, out=f)
        if up == down:
            ops.pcm16(x, VOLUME, out=p)
        else:
            ops.resample_pcm16(x, up, down, VOLUME, out=p)
        torch.cuda.synchronize()
        assert not torch.isnan(f).any() and f[:n_out].abs().max() > 0.1
        assert not f[n_out:].any() and not p[n_out:].any() and p[:n_out].abs().max() > 1000
        _REFS[key] = (x, f, p)
    return _REFS[key]


def _spans(n_out):
    return [(0, 1), (0, 257), (1000, 1513), (n_out - 300, n_out + 100), (n_out + 5, n_out + 50)]


def _window(x, lo, hi):
    """x[lo:hi] with 32 NaN on each side in its allocation."""
    buf = torch.full((hi - lo + 64,), float("nan"), device=x.device, dtype=x.dtype)
    buf[32:32 + hi - lo] = x[lo:hi]
    return buf[32:32 + hi - lo]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("up,down", RATIOS, ids=[f"{u}:{d}" for u, d in RATIOS])
def test_span_equals_the_whole_signal_bitwise(device, up, down, dtype):
    from vits_amd import ops

    x, ref_f, ref_p = _case(device, up, down, dtype)
    n_out = ops.resample_out_len(N_IN, up, down)
    seen_offset = False
    for lo, hi in _spans(n_out):
        i_lo, i_hi = ops.resample_span_input(lo, hi, N_IN, up, down)
        seen_offset |= i_lo > 0
        assert (i_lo < i_hi) == (lo < n_out)
        win = _window(x, i_lo, i_hi)
        out = ops.resample_poly_span(win, i_lo, N_IN, up, down, lo, hi - lo)
        pcm = ops.resample_pcm16_span(win, i_lo, N_IN, up, down, lo, hi - lo, VOLUME)
        torch.cuda.synchronize()
        assert out.dtype == torch.float32 and pcm.dtype == torch.int16
        assert tuple(out.shape) == tuple(pcm.shape) == (hi - lo,)
        assert not torch.isnan(out).any(), (lo, hi)
        assert torch.equal(out, ref_f[lo:hi]), (lo, hi)
        assert torch.equal(pcm, ref_p[lo:hi]), (lo, hi)
        # into a given buffer: nothing behind the span is written
        buf = torch.full((hi - lo + 3,), 55, device=device, dtype=torch.int16)
        got = ops.resample_pcm16_span(win, i_lo, N_IN, up, down, lo, hi - lo, VOLUME, out=buf)
        assert got.data_ptr() == buf.data_ptr() and torch.equal(got, ref_p[lo:hi])
        assert buf[hi - lo:].tolist() == [55] * 3
    assert seen_offset  # (a window that does not start at sample 0 was used)


@pytest.mark.parametrize("up,down", RATIOS, ids=[f"{u}:{d}" for u, d in RATIOS])
def test_a_window_one_sample_short_is_refused(device, up, down):
    from vits_amd import ops

    x, _, _ = _case(device, up, down, torch.float32)
    lo, hi = 1000, 1300
    i_lo, i_hi = ops.resample_span_input(lo, hi, N_IN, up, down)
    for a, b in ((i_lo + 1, i_hi), (i_lo, i_hi - 1)):
        with pytest.raises(ops._lib.VitsAmdError):
            ops.resample_poly_span(x[a:b].clone(), a, N_IN, up, down, lo, hi - lo)
        with pytest.raises(ops._lib.VitsAmdError):
            ops.resample_pcm16_span(x[a:b].clone(), a, N_IN, up, down, lo, hi - lo, VOLUME)
    # a wider window than needed, at another offset, is the same samples
    wide = ops.resample_poly_span(x[i_lo - 7:i_hi + 9].clone(), i_lo - 7, N_IN, up, down, lo, hi - lo)
    exact = ops.resample_poly_span(x[i_lo:i_hi].clone(), i_lo, N_IN, up, down, lo, hi - lo)
    assert torch.equal(wide, exact)
    with pytest.raises(ops._lib.VitsAmdError):
        ops.resample_poly_span(x[i_lo:i_hi].cpu(), i_lo, N_IN, up, down, lo, hi - lo)

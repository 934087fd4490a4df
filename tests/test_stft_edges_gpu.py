"""STFT magnitude and its adjoint (csrc/stft.hip) at the shapes the kernels can
go wrong at, against a float64 CPU reference of the same fp32 inputs.

The reference reflect-pads by ``pad`` in float64, runs ``torch.stft(center=
False, win_length=win)`` with the fp32 Hann window converted up, and takes
``sqrt(re^2 + im^2 + eps)``; the gradient is float64 autograd of ``(mag *
gm).sum()`` for a fixed random ``gm``.

Which forward each case runs (read from ``use_fwd2`` in csrc/stft.hip: the
two-pass register FFT serves n_fft 128..2048 with hop <= n_fft, the Stockham
LDS FFT everything else):

  two-pass  (333, 128, 32, 128, 64)      11 frames in one partial block of 32
            (65, 128, 32, 128, 64)       L = pad + 1: both reflections in every frame
            (1111, 1024, 192, 768, 416)  the spectrogram configuration, ragged
            (700, 512, 128, 400, 256)    win < n_fft
            (1000, 256, 64, 255, 128)    odd window: left offset (n - win) // 2
            (2049, 2048, 512, 2048, 1024) split pass 2, last block partial
            (1000, 256, 100, 256, 0)     no padding: a tail no frame covers
  Stockham  (1000, 64, 16, 64, 32)       63 frames, 16 per block
            (300, 32, 8, 32, 16), (200, 16, 4, 16, 8)   odd and even log2 n
            (1500, 256, 300, 256, 128)   hop > n_fft on a two-pass size
            (500, 64, 16, 50, 32)        win < n_fft: the window offset of this forward

The backward is the same two kernels for every case.  Tolerance: the 2e-5 the
project already uses for the STFT, applied per (utterance, frame) against that
frame's largest bin, and per utterance for the gradient."""
import pytest
import torch
import torch.nn.functional as F

from vits_amd import _lib, ops

pytestmark = pytest.mark.gpu

TOL = 2e-5
EPS = 1e-7

TWO_PASS = [
    (333, 128, 32, 128, 64),
    (65, 128, 32, 128, 64),
    (1111, 1024, 192, 768, 416),
    (700, 512, 128, 400, 256),
    (1000, 256, 64, 255, 128),
    (2049, 2048, 512, 2048, 1024),
    (1000, 256, 100, 256, 0),
]
STOCKHAM = [
    (1000, 64, 16, 64, 32),
    (300, 32, 8, 32, 16),
    (200, 16, 4, 16, 8),
    (1500, 256, 300, 256, 128),
    (500, 64, 16, 50, 32),
]
CASES = TWO_PASS + STOCKHAM


def _frames(L, n_fft, hop, pad):
    return (L + 2 * pad - n_fft) // hop + 1


def _signal(case, B):
    L, n_fft, hop, win, pad = case
    g = torch.Generator().manual_seed(1000 * n_fft + L)
    x = (torch.randn(B, L, generator=g) * 0.5).clamp(-1, 1)
    gm = torch.randn(B, n_fft // 2 + 1, _frames(L, n_fft, hop, pad), generator=g)
    return x, gm


def _stft_cpu(x, window, n_fft, hop, win, pad, gm, eps=EPS):
    """(mag, d (mag * gm).sum() / dx) on the CPU in x's precision."""
    xr = x.clone().requires_grad_(True)
    xp = F.pad(xr.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1) if pad else xr
    spec = torch.stft(xp, n_fft, hop, win, window.to(x.dtype), center=False, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + eps)
    (mag * gm.to(x.dtype)).sum().backward()
    return mag.detach(), xr.grad


def _uncovered(L, n_fft, hop, pad):
    """Samples of the signal that no frame reads, directly or reflected."""
    frames = _frames(L, n_fft, hop, pad)
    read = torch.zeros(L + 2 * pad, dtype=torch.bool)
    for f in range(frames):
        read[f * hop:f * hop + n_fft] = True
    idx = torch.arange(-pad, L + pad).abs()
    idx = torch.where(idx >= L, 2 * (L - 1) - idx, idx)
    hit = torch.zeros(L, dtype=torch.bool)
    hit[idx[read]] = True
    return ~hit


_cache = {}


def _run(case, device):
    """Reference and kernel results of one case, computed once per session."""
    if case in _cache:
        return _cache[case]
    L, n_fft, hop, win, pad = case
    B = 3 if n_fft < 1024 else 2
    x, gm = _signal(case, B)
    window = torch.hann_window(win)
    ref, gref = _stft_cpu(x.double(), window, n_fft, hop, win, pad, gm)
    xd = x.to(device).requires_grad_(True)
    mag = ops.stft_mag(xd, window.to(device), n_fft, hop, win, pad=pad, eps=EPS)
    loss = (mag * gm.to(device)).sum()
    g1, = torch.autograd.grad(loss, xd, retain_graph=True)
    g2, = torch.autograd.grad(loss, xd)
    out = dict(B=B, x=x, gm=gm, window=window, ref=ref, gref=gref, mag=mag.detach().cpu(),
               g1=g1.cpu(), g2=g2.cpu())
    _cache[case] = out
    return out


def _frame_err(mag, ref):
    """max over (b, frame) of max_k |mag - ref| / max_k ref."""
    err = (mag.double() - ref).abs().amax(1)
    return (err / ref.amax(1)).max().item()


def _row_err(g, gref):
    err = (g.double() - gref).abs().amax(1)
    return (err / gref.abs().amax(1)).max().item()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_stft_forward_edges(device, case):
    L, n_fft, hop, win, pad = case
    r = _run(case, device)
    assert tuple(r["mag"].shape) == (r["B"], n_fft // 2 + 1, (L + 2 * pad - n_fft) // hop + 1)
    assert tuple(r["mag"].shape) == tuple(r["ref"].shape)
    err = _frame_err(r["mag"], r["ref"])
    print(f"stft fwd {case}: worst per-frame rel err {err:.3e} (tol {TOL:.0e})")
    assert err <= TOL, f"{case}: per-frame err {err:.3e}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_stft_backward_edges(device, case):
    L, n_fft, hop, win, pad = case
    r = _run(case, device)
    g1, gref = r["g1"], r["gref"]
    assert tuple(g1.shape) == (r["B"], L)
    err = _row_err(g1, gref)
    if err > TOL:
        # the ill-conditioned-input rule: fp32 CPU autograd on the same input
        _, g32 = _stft_cpu(r["x"], r["window"], n_fft, hop, win, pad, r["gm"])
        print(f"stft bwd {case}: CPU fp32 autograd row err {_row_err(g32, gref):.3e}")
    print(f"stft bwd {case}: worst per-row rel err {err:.3e} (tol {TOL:.0e})")
    assert err <= TOL, f"{case}: gradient err {err:.3e}"
    # samples no frame reads get exactly zero, as in float64
    dead = _uncovered(L, n_fft, hop, pad)
    if hop > n_fft or pad == 0:
        assert dead.any()
    assert (gref[:, dead] == 0).all()
    zero = gref == 0
    assert (g1[zero] == 0).all(), f"{case}: {int((g1[zero] != 0).sum())} nonzero where the gradient is 0"
    # no atomics: the same bits every time
    assert torch.equal(g1, r["g2"])


def test_stft_multi_mixed_kinds_and_lengths(device):
    """One launch each way over jobs of both forward kinds, four lengths and
    two batch sizes (the job table's block prefix, per_b and the shared LDS
    size are all different per job)."""
    cases = [(1000, 64, 16, 64, 32), (333, 128, 32, 128, 64), (1500, 256, 300, 256, 128),
             (1111, 1024, 192, 768, 416)]
    batches = [2, 3, 2, 3]
    xs, gms, specs = [], [], []
    for case, B in zip(cases, batches):
        L, n_fft, hop, win, pad = case
        x, gm = _signal(case, 3)
        xs.append(x[:B].contiguous())
        gms.append(gm[:B].contiguous())
        specs.append((torch.hann_window(win).to(device), n_fft, hop, win, pad, EPS))
    xd = [x.to(device).requires_grad_(True) for x in xs]
    mags = ops.stft_mag_multi(xd, specs)
    grads = torch.autograd.grad(sum((m * gm.to(device)).sum() for m, gm in zip(mags, gms)), xd)
    for case, x, gm, m, gx, sp in zip(cases, xs, gms, mags, grads, specs):
        L, n_fft, hop, win, pad = case
        single = ops.stft_mag(x.to(device), sp[0], n_fft, hop, win, pad=pad, eps=EPS)
        assert torch.equal(m, single), case
        ref, gref = _stft_cpu(x.double(), torch.hann_window(win), n_fft, hop, win, pad, gm)
        assert tuple(m.shape) == tuple(ref.shape)
        ferr, gerr = _frame_err(m.detach().cpu(), ref), _row_err(gx.cpu(), gref)
        print(f"stft multi {case}: fwd {ferr:.3e} bwd {gerr:.3e} (tol {TOL:.0e})")
        assert ferr <= TOL and gerr <= TOL, (case, ferr, gerr)
        assert (gx.cpu()[gref == 0] == 0).all(), case


def test_stft_wrappers_refuse_a_signal_without_frames(device):
    """length + 2 pad < n_fft: torch.stft raises, and so do both wrappers,
    with the shape in the message (C division used to count one frame)."""
    x = torch.zeros(2, 100, device=device)
    w = torch.hann_window(128).to(device)
    with pytest.raises(_lib.VitsAmdError, match=r"\[2, 100\].*n_fft 128"):
        ops.stft_mag(x, w, 128, 32, 128, pad=0)
    ok = torch.zeros(2, 333, device=device)
    with pytest.raises(_lib.VitsAmdError, match=r"job 1.*\[2, 100\].*n_fft 128"):
        ops.stft_mag_multi([ok, x], [(w, 128, 32, 128, None, EPS), (w, 128, 32, 128, 0, EPS)])

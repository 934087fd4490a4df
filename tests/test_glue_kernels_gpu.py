"""The small inference kernels (csrc/layernorm.hip, csrc/misc.hip) at their
edge shapes and with every optional operand, against float64 CPU references
computed from the same fp32 (or 16-bit) inputs converted up.

Dot-product kernels (linear_rows, expand_prior) are held to the fp32
dot-product bound tests/test_post_gpu.py uses, derived and not measured:
|err| <= (K + 2) * 2^-24 * sum |a_i * b_i| for K summed terms in any order,
with or without FMA.  Layer norm is held to the larger of the project's 1e-5 *
max |ref| and 4x the error of CPU fp32 on the same input (the kernel sums four
wave partials in another order); the test prints both figures."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vits_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------
# layer_norm_channels
# ---------------------------------------------------------------------------
LN_SHAPES = [(256, 77), (192, 64), (192, 65), (5, 37), (3, 1), (2, 130)]
LN_SETS = ["plain", "residual", "no_affine", "lengths", "post_add", "scale", "pos", "all", "inplace"]
LN_B = 3


def _ln_formula(x, r, gamma, beta, lengths, post_add, scale, pos, alpha, dtype):
    """The documented formula in ``dtype`` on the CPU: ((LN(x + r) * gamma +
    beta) + post_add[b]) * scale + pos[t] * alpha, zero at t >= lengths[b]."""
    B, C, T = x.shape
    c = lambda t: None if t is None else t.to(dtype)
    v = c(x) if r is None else c(x) + c(r)
    y = F.layer_norm(v.transpose(1, 2), (C,), c(gamma), c(beta), 1e-5).transpose(1, 2)
    if post_add is not None:
        y = y + c(post_add)[:, :, None]
    if scale != 1.0:
        y = y * torch.tensor(np.float32(scale).item(), dtype=dtype)
    if pos is not None:
        y = y + c(pos)[:T].t()[None] * c(alpha)
    if lengths is not None:
        y = y * (torch.arange(T)[None, None, :] < lengths[:, None, None]).to(dtype)
    return y


def _ln_operands(C, T, kind, mean=0.0):
    g = _gen(C, T, 17)
    o = dict(x=torch.randn(LN_B, C, T, generator=g) + mean, r=None,
             gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g), lengths=None,
             post_add=None, scale=1.0, pos=None, alpha=None)
    wide = torch.randn(LN_B, 3 * C, generator=g)
    every = kind == "all"
    if kind in ("residual", "inplace") or every:
        o["r"] = torch.randn(LN_B, C, T, generator=g)
    if kind == "no_affine":
        o["gamma"] = o["beta"] = None
    if kind == "lengths" or every:
        o["lengths"] = torch.tensor([T, T // 2, 0], dtype=torch.int32)
    if kind == "post_add" or every:
        o["post_add"] = wide  # the kernel gets the column slice [:, C:2C] of it
    if kind == "scale" or every:
        o["scale"] = 1.7
    if kind == "pos" or every:
        o["pos"] = torch.randn(T + 5, C, generator=g)
        o["alpha"] = torch.tensor([0.37])
    return o


def _ln_run(o, device, C, **over):
    d = lambda t: None if t is None else t.to(device)
    pa = None
    if o["post_add"] is not None:
        pa = d(o["post_add"])[:, C:2 * C]
        assert pa.stride(0) == 3 * C
    kw = dict(residual=d(o["r"]), lengths=d(o["lengths"]), post_add=pa, scale=o["scale"],
              pos=d(o["pos"]), pos_alpha=d(o["alpha"]))
    kw.update(over)
    return ops.layer_norm_channels(kw.pop("x", d(o["x"])), d(o["gamma"]), d(o["beta"]), **kw)


def _ln_check(o, out, C, what):
    pa = None if o["post_add"] is None else o["post_add"][:, C:2 * C]
    args = (o["x"], o["r"], o["gamma"], o["beta"], o["lengths"], pa, o["scale"], o["pos"], o["alpha"])
    ref = _ln_formula(*args, torch.float64)
    cpu32 = _ln_formula(*args, torch.float32)
    cpu_err = (cpu32.double() - ref).abs().max().item()
    tol = max(1e-5 * ref.abs().max().item(), 4 * cpu_err)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"LN {what}: kernel err {err:.3e}, CPU fp32 err {cpu_err:.3e}, tol {tol:.3e}")
    assert err <= tol, f"{what}: err {err:.3e} > tol {tol:.3e}"
    return ref


@pytest.mark.parametrize("kind", LN_SETS)
@pytest.mark.parametrize("C,T", LN_SHAPES)
def test_layer_norm_operands(device, C, T, kind):
    o = _ln_operands(C, T, kind)
    if kind == "inplace":
        want = _ln_run(o, device, C)
        x = o["x"].to(device)
        got = _ln_run(o, device, C, x=x, out=x)
        assert got is x
        assert torch.equal(got, want)
        _ln_check(o, got, C, f"C={C} T={T} {kind}")
        return
    out = _ln_run(o, device, C)
    _ln_check(o, out, C, f"C={C} T={T} {kind}")
    if o["lengths"] is not None:
        out = out.cpu()
        free = _ln_run(o, device, C, lengths=None).cpu()
        for b, n in enumerate(o["lengths"].tolist()):
            assert not out[b, :, n:].any()  # exact zeros past the length
            assert torch.equal(out[b, :, :n], free[b, :, :n])  # and nothing else changed


def test_layer_norm_large_mean(device):
    """Mean 1e3, std 1: a one-pass variance (E[x^2] - mean^2) is off by about
    0.5 here, the two-pass one by about 1e-4 (CPU fp32); the 4x-CPU rule
    separates them by three orders of magnitude."""
    C, T = 192, 65
    o = _ln_operands(C, T, "plain", mean=1e3)
    _ln_check(o, _ln_run(o, device, C), C, "mean 1e3")


# ---------------------------------------------------------------------------
# linear_rows
# ---------------------------------------------------------------------------
LIN_SHAPES = [(5, 1024, 3000), (1, 1022, 7), (3, 4, 1), (2, 256, 1026), (2, 63, 130)]


def _lin_data(B, n_in, n_out):
    g = _gen(B, n_in, n_out)
    x = torch.randn(B, n_in, generator=g)
    w = torch.randn(n_out, n_in, generator=g) * 0.03
    b = torch.randn(n_out, generator=g)
    return x, w, b


def _lin_check(out, x, w, b, what):
    ref = x.double() @ w.double().t()
    mass = x.double().abs() @ w.double().abs().t()
    if b is not None:
        ref = ref + b.double()
        mass = mass + b.double().abs()
    bound = (x.shape[1] + 2) * U * mass
    err = (out.cpu().double() - ref).abs()
    print(f"linear {what}: max err {err.max():.3e}, max err/bound {(err / bound).max():.3f}")
    assert tuple(out.shape) == tuple(ref.shape)
    assert (err <= bound).all(), f"{what}: worst err/bound {(err / bound).max():.3f}"


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,n_in,n_out", LIN_SHAPES)
def test_linear_rows_edges(device, B, n_in, n_out, bias):
    x, w, b = _lin_data(B, n_in, n_out)
    if not bias:
        b = None
    out = ops.linear_rows(x.to(device), w.to(device), None if b is None else b.to(device))
    _lin_check(out, x, w, b, f"{B}x{n_in}->{n_out} bias={bias}")


@pytest.mark.parametrize("B,n_in,n_out", LIN_SHAPES)
def test_linear_rows_strided_out(device, B, n_in, n_out):
    """y as a column slice of a wider buffer: y_bstride != n_out, and the
    columns on both sides keep their contents."""
    x, w, b = _lin_data(B, n_in, n_out)
    wide = torch.full((B, n_out + 8), -777.0, device=device)
    view = wide[:, 3:3 + n_out]
    got = ops.linear_rows(x.to(device), w.to(device), b.to(device), out=view)
    assert got.data_ptr() == view.data_ptr()
    _lin_check(view, x, w, b, f"{B}x{n_in}->{n_out} strided")
    assert (wide[:, :3] == -777.0).all() and (wide[:, 3 + n_out:] == -777.0).all()
    assert torch.equal(view, ops.linear_rows(x.to(device), w.to(device), b.to(device)))


# ---------------------------------------------------------------------------
# expand_prior
# ---------------------------------------------------------------------------
EP_SHAPES = [(192, 37, 110), (80, 150, 333), (256, 65, 64), (1, 1, 1)]
EP_B = 2


def _ep_weights(kind, t_x, t_y, g):
    attn = torch.zeros(EP_B, t_y, t_x)
    for b in range(EP_B):
        y_len = t_y if b == 0 else max(t_y - 5, 1)  # the second row ends early: empty frames
        if kind == "onehot":
            tok = torch.sort(torch.randint(0, t_x, (y_len,), generator=g)).values
            tok[-1] = t_x - 1
            attn[b, torch.arange(y_len), tok] = 1.0
        else:
            for t in range(y_len):
                nnz = 2 + (t + b) % 2
                c0 = (t * max(t_x - nnz, 0)) // max(y_len - 1, 1)
                if t_x > 64 and t % 7 == 3:
                    c0 = 64 * (1 + (t // 7) % ((t_x - 1) // 64)) - 1 - (t // 7) % 2  # straddles a chunk edge
                cols = [c for c in range(c0, c0 + nnz) if c < t_x]
                attn[b, t, cols] = torch.rand(len(cols), generator=g) * 0.6 + 0.05
    return attn


@pytest.mark.parametrize("exp_s", [False, True])
@pytest.mark.parametrize("kind", ["onehot", "soft"])
@pytest.mark.parametrize("C,t_x,t_y", EP_SHAPES)
def test_expand_prior_edges(device, C, t_x, t_y, kind, exp_s):
    g = _gen(C, t_x, t_y, kind == "soft")
    attn = _ep_weights(kind, t_x, t_y, g)
    if kind == "soft" and t_x > 64:
        cols = attn[0].ne(0)
        assert (cols[:, 63] & cols[:, 64]).any()  # some frame spans two ballot chunks
    m = torch.randn(EP_B, C, t_x, generator=g)
    s = torch.rand(EP_B, C, t_x, generator=g) - 0.7  # log-std: |sum a s| < 1.4
    noise = torch.randn(EP_B, C, t_y, generator=g)
    ns = 0.667 if exp_s else 1.0
    d = lambda t: t.to(device)
    out = ops.expand_prior(d(attn), d(m), d(s), d(noise), exp_s=exp_s, noise_scale=ns)
    assert tuple(out.shape) == (EP_B, C, t_y)
    a64, n64 = attn.double(), noise.double()
    M = torch.matmul(a64, m.double().transpose(1, 2)).transpose(1, 2)
    Ssum = torch.matmul(a64, s.double().transpose(1, 2)).transpose(1, 2)
    Mabs = torch.matmul(a64.abs(), m.double().abs().transpose(1, 2)).transpose(1, 2)
    if exp_s:
        S = torch.exp(Ssum) * float(np.float32(ns))
        ref = M + n64 * S
    else:
        S = torch.matmul(a64.abs(), s.double().abs().transpose(1, 2)).transpose(1, 2)
        ref = M + n64 * Ssum
    nnz = attn.ne(0).sum(-1).double()[:, None, :]  # [B, 1, t_y]
    bound = (nnz + 2) * U * (Mabs + n64.abs() * S) + 8 * U * n64.abs() * S
    err = (out.cpu().double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"expand_prior C={C} t_x={t_x} t_y={t_y} {kind} exp_s={exp_s}: max err {err.max():.3e}, "
          f"max err/bound {ratio:.3f}")
    assert (err <= bound).all(), f"worst err/bound {ratio:.3f}"


# ---------------------------------------------------------------------------
# expand_durations (noise mode 0)
# ---------------------------------------------------------------------------
def _draw_logw(B, t_x, lo, hi, rate, g):
    """logw with exp(logw) * rate in (lo, hi) and at least 1e-3 away from an
    integer in float64, so the fp32 ceil is unambiguous; offenders are redrawn."""
    w = torch.rand(B, t_x, generator=g, dtype=torch.float64) * (hi - lo) + lo
    logw = torch.log(w / rate).float()
    for _ in range(100):
        v = torch.exp(logw.double()) * rate
        bad = (v - v.round()).abs() < 1e-3
        if not bad.any():
            break
        redo = torch.rand(int(bad.sum()), generator=g, dtype=torch.float64) * (hi - lo) + lo
        logw[bad] = torch.log(redo / rate).float()
    v = torch.exp(logw.double()) * rate
    assert ((v - v.round()).abs() >= 1e-3).all()
    return logw


ED_CASES = [
    # B, C, t_x, t_y, x_len, (lo, hi) of exp(logw) * rate, rate
    (3, 8, 300, 1024, [300, 257, 1], (0.2, 4.8), 1.0),
    (2, 4, 4096, 8192, None, (0.1, 1.9), 1.3),
    (1, 192, 1, 64, None, (2.1, 6.9), 1.0),
    (2, 16, 50, 64, [50, 40], (1.2, 4.8), 0.9),  # totals exceed t_y: truncated at the bucket
]


@pytest.mark.parametrize("B,C,t_x,t_y,x_len,span,rate", ED_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}" for c in ED_CASES])
def test_expand_durations_edges(device, B, C, t_x, t_y, x_len, span, rate):
    g = _gen(B, C, t_x, t_y)
    rate32 = float(np.float32(rate))
    ns32 = float(np.float32(0.667))
    logw = _draw_logw(B, t_x, span[0], span[1], rate32, g)
    m = torch.randn(B, C, t_x, generator=g)
    s = torch.rand(B, C, t_x, generator=g) + 0.5
    noise = torch.randn(B, C, t_y, generator=g)
    mult = (1, 8, 256)
    d = lambda t: t.to(device)
    xl = None if x_len is None else torch.tensor(x_len, dtype=torch.int32, device=device)
    z, lens = ops.expand_durations(d(logw).unsqueeze(1), d(m), d(s), d(noise), t_y, rate=rate,
                                   noise_scale=0.667, x_len=xl, stage_mult=mult)
    assert tuple(z.shape) == (B, C, t_y) and tuple(lens.shape) == (3, B)
    z = z.cpu()
    dur = torch.ceil(torch.exp(logw.double()) * rate32).long()
    if x_len is not None:
        dur = dur * (torch.arange(t_x)[None, :] < torch.tensor(x_len)[:, None])
    cum = dur.cumsum(1)
    y_len = cum[:, -1].clamp_min(1)
    if t_x == 50:
        assert (y_len > t_y).all()
    if t_x == 4096:
        assert dur.min() == 1 and dur.max() == 2 and (y_len <= t_y).all()
    assert lens.cpu().tolist() == [(y_len * k).tolist() for k in mult]
    ref = torch.zeros(B, C, t_y, dtype=torch.float64)
    mass = torch.zeros(B, C, t_y, dtype=torch.float64)
    for b in range(B):
        n = min(int(y_len[b]), t_y)
        tok = torch.searchsorted(cum[b], torch.arange(n), right=True)
        assert int(tok.max()) < t_x
        nz = noise[b, :, :n].double() * s[b].double()[:, tok] * ns32
        ref[b, :, :n] = m[b].double()[:, tok] + nz
        mass[b, :, :n] = m[b].double()[:, tok].abs() + nz.abs()
        assert not z[b, :, n:].any()  # exact zeros past y_len
        assert z[b, :, :n].ne(0).any(0).all()  # and every frame before it is written
    err = (z.double() - ref).abs()
    bound = 4 * U * mass
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"expand_durations t_x={t_x}: y_len {y_len.tolist()}, max err {err.max():.3e}, "
          f"max err/bound {ratio:.3f}")
    assert (err <= bound).all(), f"worst err/bound {ratio:.3f}"


def test_expand_durations_half_round(device):
    """The fp16 model's total length: 600 tokens of 4 frames and one of 3 sum
    to 2403, which torch.sum in half rounds to 2404 (even mantissa above 2048);
    lens follows the half arithmetic, the frames follow the integer durations."""
    B, C, t_x, t_y = 2, 2, 601, 2432
    logw = torch.full((B, t_x), math.log(3.5)).half()  # exactly representable inputs
    logw[:, -1] = math.log(2.5)
    x_len = torch.tensor([601, 300], dtype=torch.int32)
    w_ceil = torch.ceil(torch.exp(logw) * torch.tensor(1.0).half())
    w_ceil = w_ceil * (torch.arange(t_x)[None, :] < x_len[:, None]).half()
    assert w_ceil.dtype == torch.float16 and w_ceil[0, :3].tolist() == [4, 4, 4] and w_ceil[0, -1] == 3
    want = torch.clamp_min(torch.sum(w_ceil, 1), 1).long()
    assert want.tolist() == [2404, 1200]
    g = _gen(601)
    m = torch.randn(B, C, t_x, generator=g)
    s = torch.rand(B, C, t_x, generator=g) + 0.5
    noise = torch.randn(B, C, t_y, generator=g)
    d = lambda t: t.to(device)
    z, lens = ops.expand_durations(d(logw.float()), d(m), d(s), d(noise), t_y, x_len=d(x_len),
                                   half_round=True, stage_mult=(1, 256))
    assert lens.cpu().tolist() == [want.tolist(), (want * 256).tolist()]
    z = z.cpu()
    for b, total in enumerate((2403, 1200)):
        assert not z[b, :, total:].any() and z[b, :, :total].ne(0).any(0).all()
    # frame 2402 is the last token's third frame
    nz = noise[0, :, 2402].double() * s[0, :, 600].double()
    ref = m[0, :, 600].double() + nz
    assert ((z[0, :, 2402].double() - ref).abs() <= 4 * U * (m[0, :, 600].double().abs() + nz.abs())).all()
    # without half_round the same durations report 2403
    _, lens32 = ops.expand_durations(d(logw.float()), d(m), d(s), d(noise), t_y, x_len=d(x_len))
    assert lens32.cpu().tolist() == [[2403, 1200]]


# ---------------------------------------------------------------------------
# conv_post_tanh
# ---------------------------------------------------------------------------
CP_GENERIC = [(16, 7, 1234), (48, 3, 257), (32, 11, 1000), (8, 1, 5), (32, 7, 255)]
CP_ALIGNED = [(32, k, T) for k in (1, 3, 5, 9) for T in (4, 256, 260, 1236)]
CP_TOL = 1e-4


def _cp_data(C, k, T, dt=torch.float32, B=2):
    g = _gen(C, k, T)
    x = torch.randn(B, C, T, generator=g).to(dt)
    w = torch.randn(1, C, k, generator=g) * 0.2
    ref = torch.tanh(F.conv1d(F.leaky_relu(x.double(), 0.01), w.double(), None, padding=(k - 1) // 2))
    return x, w, ref


def _cp_check(out, ref, what):
    assert tuple(out.shape) == tuple(ref.shape)
    err = (out.cpu().double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"conv_post {what}: max err {err:.3e}, scale {scale:.3e}, tol {CP_TOL * scale:.3e}")
    assert err <= CP_TOL * scale, f"{what}: err {err:.3e}"


@pytest.mark.parametrize("C,k,T", CP_GENERIC + CP_ALIGNED)
def test_conv_post_tanh_shapes(device, C, k, T):
    """Generic kernel: other channel counts, kernel sizes and a T below one
    tile.  Aligned kernel (C = 32, T % 4 == 0, k <= 9): every k, T below,
    equal to and just past a 256-sample tile."""
    x, w, ref = _cp_data(C, k, T)
    _cp_check(ops.conv_post_tanh(x.to(device), w.to(device)), ref, f"C={C} k={k} T={T}")


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,k,T", [(16, 7, 1234), (32, 5, 260)])
def test_conv_post_tanh_dtypes(device, C, k, T, dt):
    x, w, ref = _cp_data(C, k, T, dt)
    _cp_check(ops.conv_post_tanh(x.to(device), w.to(device)), ref, f"C={C} k={k} T={T} {dt}")


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("k,T", [(7, 256), (9, 1236)])
def test_conv_post_tanh_strided_and_misaligned(device, k, T, dt):
    """Rows of a wider buffer (x_cstride = T + 8, still 4-element aligned: the
    aligned kernel) and the same data one element further in (misaligned: the
    generic kernel): the same values, to tolerance."""
    x, w, ref = _cp_data(32, k, T, dt)
    B = x.shape[0]
    buf = torch.full((B, 32, T + 8), 50.0, dtype=dt, device=device)  # a read past a row would show
    view = buf[:, :, :T]
    view.copy_(x)
    assert view.stride(1) == T + 8 and view.data_ptr() % (16 if dt == torch.float32 else 8) == 0
    a = ops.conv_post_tanh(view, w.to(device))
    _cp_check(a, ref, f"k={k} T={T} {dt} strided")
    buf2 = torch.full((B, 32, T + 8), 50.0, dtype=dt, device=device)
    off = buf2[:, :, 1:T + 1]
    off.copy_(x)
    assert off.data_ptr() % (16 if dt == torch.float32 else 8) != 0
    b = ops.conv_post_tanh(off, w.to(device))
    _cp_check(b, ref, f"k={k} T={T} {dt} misaligned")
    assert (a - b).abs().max().item() <= 2 * CP_TOL * ref.abs().max().item()

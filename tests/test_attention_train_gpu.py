"""The differentiable HIP attention (csrc/attention.hip: training forward with
saved log-sum-exp, two-kernel backward, dropout) against the reference
arithmetic of attentions.py:85-100 in float64 on the CPU:
scores.masked_fill(mask == 0, -1e4) with mask the outer product of the length
masks, softmax, dropout, P V, and autograd for the gradients.

Shapes: T in {37, 77, 100} (no multiple of the 32-wide tile, 2 - 4 tiles on
both loop axes), lens [T, 20, 1] (a length below one tile, a length of 1,
fully masked query rows), H = 2, D in {96, 128} and once {16, 48} (partial
32-wide d tile).

Bars: forward and lse 2e-5 of max|ref| (test_kernels_gpu.test_attention's),
fp32 gradients RTOL = 1e-4 of max|ref| (test_kernels_gpu.RTOL), 16-bit:
error against float64 at most twice the torch autocast path's."""
import functools
import math

import pytest
import torch

from vits_amd import _lib, attentions, ops, train_ops

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
RTOL = 1e-4
H = 2
CASES = [(37, 96), (37, 128), (77, 96), (77, 128), (100, 96), (100, 128), (37, 16), (77, 48)]


def _lens(T):
    return [T, 20, 1]


def _ref_math(q, k, v, gy, lens, keep=None, p=0.0):
    """float64 reference: (out, lse, dq, dk, dv) of [B, H*D, T] q / k / v."""
    B, C, T = q.shape
    D = C // H
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    lm = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).double()
    am = (lm.unsqueeze(2) * lm.unsqueeze(1)).unsqueeze(1)
    qh, kh, vh = (t.view(B, H, D, T).transpose(2, 3) for t in (q, k, v))
    sc = torch.matmul(qh / math.sqrt(D), kh.transpose(-2, -1)).masked_fill(am == 0, -1e4)
    P = torch.softmax(sc, -1)
    if keep is not None:
        P = P * keep.double() / (1.0 - p)
    out = torch.matmul(P, vh).transpose(2, 3).reshape(B, C, T)
    out.backward(gy.double())
    return (out.detach(), torch.logsumexp(sc, -1).detach(), q.grad, k.grad, v.grad)


@functools.lru_cache(maxsize=None)
def _case(T, D, dtype=torch.float32):
    """Inputs (rounded to dtype) and their float64 reference, computed once."""
    g = torch.Generator().manual_seed(1000 * T + D)
    q, k, v, gy = (torch.randn(3, H * D, T, generator=g).to(dtype) for _ in range(4))
    return (q, k, v, gy), _ref_math(q, k, v, gy, _lens(T))


def _err(a, ref):
    return (a.detach().double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def _dev(device, T, *ts):
    return [t.to(device) for t in ts] + [torch.tensor(_lens(T), dtype=torch.int32, device=device)]


@pytest.mark.parametrize("T,D", CASES)
def test_forward_and_lse_fp32(device, T, D):
    (q, k, v, _), (ref, ref_lse, *_) = _case(T, D)
    qd, kd, vd, lens = _dev(device, T, q, k, v)
    out, lse = ops.attention_train_forward(qd, kd, vd, H, lens)
    e_out, e_lse = _err(out, ref), _err(lse, ref_lse)
    print(f"T={T} D={D} out {e_out:.2e} lse {e_lse:.2e}")
    assert out.dtype == torch.float32 and lse.shape == (3, H, T)
    assert e_out <= FWD_TOL
    assert e_lse <= FWD_TOL
    # (max|lse| is the fully masked rows' -1e4 + log T: the unmasked rows of
    # utterance 0 on their own scale too)
    assert _err(lse[0], ref_lse[0]) <= FWD_TOL
    # p = 0: the inference kernel's numerics exactly
    assert torch.equal(out, ops.attention(qd, kd, vd, H, lengths=lens))


@pytest.mark.parametrize("T,D", CASES)
def test_backward_fp32(device, T, D):
    (q, k, v, gy), (_, _, rq, rk, rv) = _case(T, D)
    qd, kd, vd, gd, lens = _dev(device, T, q, k, v, gy)
    out, lse = ops.attention_train_forward(qd, kd, vd, H, lens)
    dq, dk, dv = ops.attention_backward(qd, kd, vd, out, gd, lse, H, lens)
    errs = [_err(a, r) for a, r in ((dq, rq), (dk, rk), (dv, rv))]
    print(f"T={T} D={D} dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert max(errs) <= RTOL, errs
    # masked_fill passes no gradient: fully masked query rows of dq and masked
    # keys of dk are exactly zero (as the reference's are); dv is not
    for b, n in enumerate(_lens(T)):
        if n < T:
            assert rq[b, :, n:].abs().max() == 0 and rk[b, :, n:].abs().max() == 0
            assert dq[b, :, n:].abs().max().item() == 0
            assert dk[b, :, n:].abs().max().item() == 0
            assert rv[b, :, n:].abs().min() > 0
            assert dv[b, :, n:].abs().min().item() > 0


def test_ops_attention_alone_has_no_backward(device):
    """ops.attention (the inference entry) stays non-differentiable; the
    training op carries the graph."""
    (q, k, v, gy), (_, _, rq, _, _) = _case(37, 96)
    qd, kd, vd, gd, lens = _dev(device, 37, q, k, v, gy)
    qd.requires_grad_(True)
    assert ops.attention(qd, kd, vd, H, lengths=lens).grad_fn is None
    out = train_ops.attention(qd, kd, vd, H, lens, 0.0, True)
    out.backward(gd)
    assert _err(qd.grad, rq) <= RTOL


def test_fused_qkv_strides(device):
    """q / k / v as channel slices of one [B, 3C, T] buffer, dq / dk / dv
    written into the slices of one gradient buffer: bit-equal to the
    contiguous call."""
    T, D = 77, 96
    C = H * D
    (q, k, v, gy), _ = _case(T, D)
    qd, kd, vd, gd, lens = _dev(device, T, q, k, v, gy)
    out, lse = ops.attention_train_forward(qd, kd, vd, H, lens)
    grads = [torch.empty_like(qd) for _ in range(3)]
    ops.attention_backward(qd, kd, vd, out, gd, lse, H, lens, grads=grads)
    qkv = torch.cat([qd, kd, vd], 1)
    qs, ks, vs = qkv.split(C, 1)
    assert qs.stride(0) == 3 * C * T
    out2, lse2 = ops.attention_train_forward(qs, ks, vs, H, lens)
    gbuf = torch.full((3, 3 * C, T), float("nan"), device=device)
    ops.attention_backward(qs, ks, vs, out2, gd, lse2, H, lens, grads=gbuf.split(C, 1))
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    assert torch.equal(gbuf, torch.cat(grads, 1))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16bit_io_vs_torch_autocast(device, dtype):
    """Inputs rounded to the 16-bit type; the HIP op's error against the
    float64 reference of the rounded inputs is at most twice the torch
    path's under the same autocast dtype (a different rounding order of the
    same 16-bit products), for out, dq, dk and dv."""
    T, D = 77, 96
    (q, k, v, gy), (ref, _, rq, rk, rv) = _case(T, D, dtype)
    qd, kd, vd, gd, lens = _dev(device, T, q, k, v, gy)
    lm = (torch.arange(T, device=device)[None] < lens[:, None]).float()
    am = (lm.unsqueeze(2) * lm.unsqueeze(1)).unsqueeze(1)

    def run(hip):
        leaves = [t.clone().requires_grad_(True) for t in (qd, kd, vd)]
        with torch.autocast("cuda", dtype=dtype):
            if hip:
                out = train_ops.AttentionHip.apply(*leaves, H, lens, 0.0)
            else:
                out = train_ops._attention_torch(*leaves, H, am, 0.0, False)
        assert out.dtype == dtype
        out.backward(gd)
        return [out] + [t.grad for t in leaves]

    e_hip = [_err(a, r) for a, r in zip(run(True), (ref, rq, rk, rv))]
    e_torch = [_err(a, r) for a, r in zip(run(False), (ref, rq, rk, rv))]
    for name, a, b in zip(("out", "dq", "dk", "dv"), e_hip, e_torch):
        print(f"{dtype} {name}: err_hip {a:.3e} err_torch {b:.3e} ratio {a / b:.2f}")
    for name, a, b in zip(("out", "dq", "dk", "dv"), e_hip, e_torch):
        assert a <= 2 * b, (name, a, b)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout(device, p):
    T, D, B = 77, 96, 3
    (q, k, v, gy), _ = _case(T, D)
    qd, kd, vd, gd, lens = _dev(device, T, q, k, v, gy)
    seed = torch.tensor([1234567 + int(p * 10)], dtype=torch.int64, device=device)
    keep = ops.attention_dropout_mask(seed, B, H, T, p)
    assert keep.dtype == torch.uint8 and keep.shape == (B, H, T, T)
    ref, _, rq, rk, rv = _ref_math(q, k, v, gy, _lens(T), keep.cpu(), p)
    out, lse = ops.attention_train_forward(qd, kd, vd, H, lens, p, seed)
    dq, dk, dv = ops.attention_backward(qd, kd, vd, out, gd, lse, H, lens, p, seed)
    e_out = _err(out, ref)
    errs = [_err(a, r) for a, r in ((dq, rq), (dk, rk), (dv, rv))]
    print(f"p={p} out {e_out:.2e} dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")
    assert e_out <= FWD_TOL
    assert max(errs) <= RTOL, errs
    # the kept fraction of N Bernoulli(1 - p) draws, 5 sigma
    N = keep.numel()
    frac = keep.float().mean().item()
    print(f"p={p} kept {frac:.4f} of N={N}")
    assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / N)
    assert set(keep.unique().tolist()) == {0, 1}
    # the mask is a function of the seed
    assert torch.equal(keep, ops.attention_dropout_mask(seed.clone(), B, H, T, p))
    assert not torch.equal(keep, ops.attention_dropout_mask(seed + 1, B, H, T, p))
    # lse is the undropped normaliser's
    assert torch.equal(lse, ops.attention_train_forward(qd, kd, vd, H, lens)[1])


def test_dropout_reproducible_under_manual_seed(device):
    T, D = 37, 96
    (q, k, v, gy), _ = _case(T, D)
    qd, kd, vd, gd, lens = _dev(device, T, q, k, v, gy)

    def run(s):
        torch.manual_seed(s)
        leaves = [t.clone().requires_grad_(True) for t in (qd, kd, vd)]
        out = train_ops.attention(*leaves, H, lens, 0.1, True)
        out.backward(gd)
        return [out.detach()] + [t.grad for t in leaves]

    a, b, c = run(5), run(5), run(6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])
    # eval mode: no dropout
    torch.manual_seed(5)
    assert torch.equal(train_ops.attention(qd, kd, vd, H, lens, 0.1, False),
                       ops.attention(qd, kd, vd, H, lengths=lens))


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_backward_deterministic(device, p):
    T, D = 100, 128
    (q, k, v, gy), _ = _case(T, D)
    qd, kd, vd, gd, lens = _dev(device, T, q, k, v, gy)
    seed = torch.tensor([99], dtype=torch.int64, device=device)
    out, lse = ops.attention_train_forward(qd, kd, vd, H, lens, p, seed)
    a = ops.attention_backward(qd, kd, vd, out, gd, lse, H, lens, p, seed)
    b = ops.attention_backward(qd, kd, vd, out, gd, lse, H, lens, p, seed)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_torch_path_keeps_dtype_and_foreign_masks(device):
    """train_ops.attention stays on the torch chain, with the input dtype and
    the caller's mask, where the HIP op would change either: float64 tensors,
    16-bit tensors outside autocast (autocast casts neither), float64 inside
    autocast, and a mask that is not a [B, 1, T, T] one."""
    T, D = 37, 96
    (q, k, v, _), (ref, *_) = _case(T, D)
    qd, kd, vd, lens = _dev(device, T, q, k, v)
    lm = (torch.arange(T, device=device)[None] < lens[:, None]).float()
    am = (lm.unsqueeze(2) * lm.unsqueeze(1)).unsqueeze(1)

    def run(dtype, mask, autocast=None):
        _lib.dispatch_counts_reset()
        with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
            out = train_ops.attention(qd.to(dtype), kd.to(dtype), vd.to(dtype), H, lens, 0.0,
                                      True, mask=mask)
        return out, _lib.dispatch_counts()["attn"]

    out, n = run(torch.float64, am)
    assert out.dtype == torch.float64 and n == 0
    assert _err(out, ref) <= 1e-12
    out, n = run(torch.float64, am, autocast=torch.float16)
    assert out.dtype == torch.float64 and n == 0
    out, n = run(torch.float16, am)
    assert out.dtype == torch.float16 and n == 0
    # a causal mask shared by the batch: not the lengths' mask, so it is applied
    causal = torch.ones(T, T, device=device).tril()[None, None]
    out, n = run(torch.float32, causal)
    assert n == 0
    assert torch.equal(out, train_ops._attention_torch(qd, kd, vd, H, causal, 0.0, True))
    # and the HIP op where it applies: fp32 with the lengths' mask, fp32
    # tensors inside a 16-bit autocast region (cast as autocast casts them)
    out, n = run(torch.float32, am)
    assert out.dtype == torch.float32 and n == 1
    out, n = run(torch.float32, am, autocast=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and n == 1


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------

GIN = 16


def _module(kind):
    torch.manual_seed(3)
    if kind == "mha":
        return attentions.MultiHeadAttention(192, 192, 2, p_dropout=0.0).train()
    return attentions.Encoder(192, 768, 2, 2, kernel_size=5, gin_channels=GIN).train()


def _module_run(kind, m, x, lens, g, gy, autocast=None):
    """[output] + parameter gradients (in named_parameters order)."""
    T = x.shape[2]
    x_mask = (torch.arange(T, device=x.device)[None] < lens[:, None]).to(x.dtype).unsqueeze(1)
    for p in m.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
        if kind == "mha":
            am = x_mask.unsqueeze(2) * x_mask.unsqueeze(-1)
            y = m(x, x, am, lengths=None if x.device.type == "cpu" else lens.to(torch.int32))
        else:
            y = m(x, x_mask, g)
    y = y.to(x.dtype)
    y.backward(gy)
    return [y.detach()] + [p.grad for p in m.parameters()]


@functools.lru_cache(maxsize=None)
def _module_case(kind):
    T = 37
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 192, T, generator=g)
    gy = torch.randn(3, 192, T, generator=g)
    gin = torch.randn(3, GIN, generator=g)
    lens = torch.tensor([T, 20, 1])
    m64 = _module(kind).double()
    ref = _module_run(kind, m64, x.double(), lens, gin.double(), gy.double())
    return (x, gy, gin, lens), ref


def _grad_scales(kind, ref):
    """max|ref| per tensor.  conv_k.bias is the exception: a key bias shifts
    every score of a query by the same q . b_k, which the softmax ignores, so
    its gradient is identically zero and its float64 value rounding noise; it
    is d_k summed over (b, t) where conv_k.weight's gradient is d_k x^T with
    x of unit scale, so its error is measured on conv_k.weight's scale."""
    names = ["out"] + [n for n, _ in _module(kind).named_parameters()]
    scales = [r.abs().max().item() for r in ref]
    for i, n in enumerate(names):
        if n.endswith("conv_k.bias"):
            scales[i] = scales[names.index(n[:-4] + "weight")]
    return names, scales


@pytest.mark.parametrize("kind", ["mha", "encoder"])
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_module_hip_vs_torch_attention(device, monkeypatch, kind, mode):
    """MultiHeadAttention / a 2-layer Encoder in train mode at T = 37 with
    ragged lengths, ATTN_HIP on against off.  fp32: output and every parameter
    gradient agree at RTOL of the tensor's scale.  fp16 autocast: both paths'
    errors against a float64 CPU copy of the module, the HIP path's at most
    twice the torch path's (test_16bit_io_vs_torch_autocast's margin).

    conv_k.bias is held to an absolute bound instead, the same one for both
    paths: its true gradient is identically zero (see _grad_scales), so
    max|ref| is float64 noise and a ratio of two residuals compares noise
    with noise.  The bound: the gradient is sum_{b,t} dk[b, c, t] over the
    N = 58 unmasked positions, each term carrying k independent fp16
    roundings (dS, q / sqrt(D), the dk output, the sum's own adds; k <= 6)
    of relative size u = 2^-11, uniform, std u / sqrt(3): the residual's std
    is u sqrt(N k / 3) rms(dk), its maximum over 192 channels about 3 std.
    conv_k.weight's gradient sum_{b,t} dk x^T with unit-scale x has std
    sqrt(N) rms(dk), its maximum over 192^2 entries about 4.2 std.  So the
    residual is at most 3 sqrt(k / 3) / 4.2, about 1.0 u at k = 6, of
    conv_k.weight's gradient scale.  Measured (HIP / torch): MHA 2.8e-4 /
    1.4e-4 (0.57 u / 0.28 u), Encoder layers 2.7e-4 / 1.3e-4 and 1.8e-4 /
    1.7e-4."""
    (x, gy, gin, lens), ref = _module_case(kind)
    names, scales = _grad_scales(kind, ref)
    m = _module(kind).to(device)
    args = (x.to(device), lens.to(device), gin.to(device), gy.to(device))
    ac = torch.float16 if mode == "fp16" else None

    def run(on):
        monkeypatch.setattr(attentions, "ATTN_HIP", on)
        _lib.dispatch_counts_reset()
        res = _module_run(kind, m, *args, autocast=ac)
        return res, _lib.dispatch_counts()["attn"]

    hip, n_on = run(True)
    tor, n_off = run(False)
    layers = 1 if kind == "mha" else 2
    assert n_on == 3 * layers and n_off == 0, (n_on, n_off)
    for n, s, a, b, r in zip(names, scales, hip, tor, ref):
        ea = (a.double().cpu() - r).abs().max().item() / s
        eb = (b.double().cpu() - r).abs().max().item() / s
        d = (a.double() - b.double()).abs().max().item() / s
        print(f"{kind} {mode} {n}: err_hip {ea:.3e} err_torch {eb:.3e} hip-torch {d:.3e}")
    for n, s, a, b, r in zip(names, scales, hip, tor, ref):
        ea = (a.double().cpu() - r).abs().max().item() / s
        eb = (b.double().cpu() - r).abs().max().item() / s
        if mode == "fp32":
            assert (a.double() - b.double()).abs().max().item() / s <= RTOL, n
        elif n.endswith("conv_k.bias"):
            assert ea <= 2.0 ** -11 and eb <= 2.0 ** -11, (n, ea, eb)
        else:
            assert ea <= 2 * eb, (n, ea, eb)


# ---------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------


def _capture(device, p):
    T, D = 37, 96
    (q, k, v, gy), _ = _case(T, D)
    qd, kd, vd, gd, lens = _dev(device, T, q, k, v, gy)
    leaves = [t.requires_grad_(True) for t in (qd, kd, vd)]

    def step():
        out = train_ops.AttentionHip.apply(*leaves, H, lens, p)
        return [out] + list(torch.autograd.grad(out, leaves, gd))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    return graph, static, eager


def test_capture_replay_equals_eager(device):
    graph, static, eager = _capture(device, 0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), b) for a, b in zip(static, eager))


def test_capture_dropout_draws_per_replay(device):
    """The seed is device memory drawn from torch's generator inside the
    captured region: every replay drops another set of probabilities."""
    graph, static, _ = _capture(device, 0.1)
    graph.replay()
    first = [t.detach().clone() for t in static]
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(first[0], static[0].detach())
    assert all(torch.isfinite(t).all() for t in first + [s.detach() for s in static])

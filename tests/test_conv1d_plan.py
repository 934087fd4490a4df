"""vits_conv1d_plan (host only): every case of the conv-variant table plans to
the kernel it names, the table reaches every variant the pickers can produce,
the small-grid fallback switches where the library says it does, refusals are
refused - and the error bound the GPU tests apply is validated on the CPU:
wide enough for correct arithmetic, narrow enough to catch a lost tap.

No GPU: descriptors point at host allocations; the plan reads no memory."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_variants_common as cv
from vits_amd import _lib, ops
from vits_amd._lib import (VITS_E_UNSUP, VITS_OK, WDT_BF16, WDT_F16, WDT_F32, WDT_F32P,
                           WDT_F32S)

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def planned():
    """{case name: (rc, plan)} of the whole table, built once."""
    out = {}
    for c in cv.CASES:
        bt = cv.build(c, cv.make_inputs(c), CPU)
        out[c["name"]] = ops.conv1d_plan(bt.desc, c["B"])
    return out


@pytest.mark.parametrize("c", cv.CASES, ids=cv.CASE_IDS)
def test_case_plans_to_its_variant(planned, c):
    rc, plan = planned[c["name"]]
    assert rc == VITS_OK, rc
    want = cv.expected_plan(c)
    got = {f: plan[f] for f in want}
    assert got == want
    assert plan["grid"] == (-(-c["n_out"] // plan["bn"]), -(-c["m"] // plan["bm"]), c["B"])
    assert 0 < plan["lds_bytes"] <= 160 * 1024


def test_plan_bumps_no_counter(planned):
    _lib.dispatch_counts_reset()
    c = cv.CASES[0]
    bt = cv.build(c, cv.make_inputs(c), CPU)
    assert ops.conv1d_plan(bt.desc, c["B"])[0] == VITS_OK
    assert set(_lib.dispatch_counts().values()) == {0}


_TILES = {"32x256": (32, 256, 1, 4), "64x128": (64, 128, 2, 2), "128x128": (128, 128, 2, 2),
          "64x256": (64, 256, 1, 4), "64x256s": (64, 256, 2, 2)}
# (kind, global-A, tiles) the pickers can produce
_PICKED = [
    (WDT_F32, 0, ("32x256", "64x128", "64x256")),
    (WDT_BF16, 0, ("32x256", "64x128", "128x128", "64x256")),
    (WDT_BF16, 1, ("32x256", "64x128", "128x128", "64x256")),
    (WDT_F16, 0, ("32x256", "64x128", "128x128", "64x256")),
    (WDT_F16, 1, ("32x256", "64x128", "128x128", "64x256")),
    (WDT_F32S, 0, ("128x128", "64x128", "64x256s")),
    (WDT_F32P, 0, ("128x128", "64x128")),
]
# accepted by the C API, produced by no picker
_FORCED = [(WDT_F32, "128x128"), (WDT_F32P, "64x256s"), (WDT_F32P, "32x256"),
           (WDT_F32S, "32x256")]


def test_table_reaches_every_variant(planned):
    plans = [p for _, p in planned.values()]
    got = {cv.variant_key(p) for p in plans}
    # every picker variant, in both staging kinds
    req = {(wdt, ga) + _TILES[t] + (v4,) for wdt, ga, ts in _PICKED for t in ts for v4 in (0, 1)}
    assert got >= req, sorted(req - got)
    # the forced combinations, each at least once
    assert {k[:6] for k in got} >= {(wdt, 0) + _TILES[t] for wdt, t in _FORCED}
    # each epilogue (and the LDS-staged upsample store) at least once per kind
    epis = {(p["wdtype"], p["ga"], p["epi"], p["up_lds"]) for p in plans}
    for wdt, ga in ((WDT_F32, 0), (WDT_BF16, 0), (WDT_BF16, 1), (WDT_F16, 0), (WDT_F16, 1),
                    (WDT_F32S, 0), (WDT_F32P, 0)):
        for epi, ul in ((_lib.EPI_STORE, 0), (_lib.PLAN_EPI_STORE2, 0), (_lib.EPI_GATE, 0),
                        (_lib.EPI_UPSAMPLE, 0), (_lib.EPI_UPSAMPLE, 1)):
            assert (wdt, ga, epi, ul) in epis, (wdt, ga, epi, ul)
    # 16-bit activations: io16 = 1 (never global-A) and io16 = 2 (always)
    io = {(p["wdtype"], p["ga"]) for p in plans if p["io16"]}
    assert io >= {(WDT_BF16, 0), (WDT_BF16, 1), (WDT_F16, 0), (WDT_F16, 1)}


# ---------------------------------------------------------------------------
# the small-grid fallback
# ---------------------------------------------------------------------------


def _plain_desc(kind, tile, m, k, dil, tin, cin=16):
    c = cv.case("fallback", kind, "store", "0x0/0x0/v4", 1, cin, m, k, tile=tile, dil=dil, tin=tin)
    return cv.build(c, cv.make_inputs(c), CPU).desc


def _walk_threshold(d, per_batch, big):
    """Smallest workgroup count at which ``d`` (per_batch workgroups per
    utterance) plans to the ``big`` tile, walking the batch through the plan;
    every smaller launch must plan to 64x128 and every larger one to ``big``."""
    tiles = []
    for batch in range(1, 1200 // per_batch):
        rc, p = ops.conv1d_plan(d, batch)
        assert rc == VITS_OK and p["grid"][2] == batch
        tiles.append((p["bm"], p["bn"]))
    first = tiles.index(big)
    assert first > 0 and set(tiles[:first]) == {(64, 128)} and set(tiles[first:]) == {big}
    return per_batch * (first + 1)


@pytest.mark.parametrize("kind", ["f32", "bf16", "f32s", "f32p"])
def test_fallback_threshold_128x128(kind):
    """One workgroup per utterance, so the batch IS the workgroup count: 64x128
    up to one workgroup short of the threshold, 128x128 from the threshold on.
    The threshold is read off the plan, not written here; the same count
    reached through rows and columns switches at the same place."""
    thr = _walk_threshold(_plain_desc(kind, "128x128", 128, 3, 1, 128), 1, (128, 128))
    cols = -(-thr // 2)                                   # two row blocks (m = 130) x cols
    short = _plain_desc(kind, "128x128", 130, 3, 1, 128 * (cols - 1))
    at = _plain_desc(kind, "128x128", 130, 3, 1, 128 * (cols - 1) + 1)
    assert 2 * (cols - 1) < thr <= 2 * cols
    p = ops.conv1d_plan(short, 1)[1]
    assert (p["bm"], p["bn"]) == (64, 128)
    p = ops.conv1d_plan(at, 1)[1]
    assert (p["bm"], p["bn"]) == (128, 128) and p["grid"] == (cols, 2, 1)


def test_fallback_64x256_follows_fits128():
    """A 64x256 grid below the threshold falls back only when the chunk's
    window also fits the 128-column tile."""
    fits = _plain_desc("f32", "64x256", 66, 3, 1, 512)
    wide = _plain_desc("f32", "64x256", 66, 3, 40, 512, cin=20)
    assert wide.kc * ((128 + 2 * 40 + 3) // 4 * 4) > 2048 >= fits.kc * ((128 + 2 + 3) // 4 * 4)
    assert {ops.conv1d_plan(wide, b)[1]["bn"] for b in range(1, 300)} == {256}
    thr = _walk_threshold(fits, 4, (64, 256))             # 2 x 2 workgroups per utterance
    # the same threshold as the 128x128 rule
    assert thr == _walk_threshold(_plain_desc("f32", "128x128", 130, 3, 1, 256), 4, (128, 128))


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------


def test_mixed_staging_group_is_unsup():
    a = _plain_desc("f32p", "64x128", 66, 3, 1, 132)
    b = _plain_desc("f32p", "64x128", 66, 3, 1, 131)
    assert ops.conv1d_plan(a, 2)[1]["v4"] == 1 and ops.conv1d_plan(b, 2)[1]["v4"] == 0
    assert ops.conv1d_plan((a, a), 2)[0] == VITS_OK
    assert ops.conv1d_plan((a, b), 2) == (VITS_E_UNSUP, None)
    assert ops.conv1d_plan((b, a, b), 2) == (VITS_E_UNSUP, None)


def test_over_budget_chunk_is_unsup():
    d = _plain_desc("f32", "64x128", 66, 3, 1, 132, cin=64)
    assert ops.conv1d_plan(d, 2)[0] == VITS_OK
    d.kc, d.cin_pad = 64, 64                     # 64 * 3 * 64 floats of W per chunk > the stage
    assert ops.conv1d_plan(d, 2) == (VITS_E_UNSUP, None)
    p = _plain_desc("f32p", "64x128", 66, 3, 200, 132)   # window of 128 + 400 columns
    assert ops.conv1d_plan(p, 2) == (VITS_E_UNSUP, None)


@pytest.mark.parametrize("kind", ["f32", "f32s", "f32p"])
def test_io16_needs_a_16bit_kind(kind):
    d = _plain_desc(kind, "64x128", 66, 3, 1, 132)
    d.io16 = 1
    rc, plan = ops.conv1d_plan(d, 2)
    assert rc != VITS_OK and plan is None


def test_plan_argument_checks():
    d = _plain_desc("f32", "64x128", 66, 3, 1, 132)
    lib = _lib.load()
    out = _lib.ConvPlan()
    assert lib.vits_conv1d_plan(None, 1, 1, ctypes.byref(out)) == _lib.VITS_E_ARG
    assert lib.vits_conv1d_plan(ctypes.byref(d), 1, 1, None) == _lib.VITS_E_ARG
    assert lib.vits_conv1d_plan(ctypes.byref(d), 0, 1, ctypes.byref(out)) == _lib.VITS_E_ARG
    assert lib.vits_conv1d_plan(ctypes.byref(d), 1, 0, ctypes.byref(out)) == _lib.VITS_E_ARG


# ---------------------------------------------------------------------------
# the bound: wide enough for correct arithmetic, narrow enough to matter
# ---------------------------------------------------------------------------

SMALL = [c for c in cv.CASES if c["B"] * c["m"] * c["n_out"] <= 150_000]


def _acc_level(c):
    """(x' fp32, w fp32 in GEMM-row layout, float64 accumulator, A) of a conv case."""
    inp = cv.make_inputs(c)
    xp, w = cv.operands64(c, inp)
    return inp, xp, w, cv._conv64(c, xp, w), cv._conv64(c, np.abs(xp), np.abs(w))


@pytest.mark.parametrize("c", [c for c in cv.CASES if c["up"] is None], ids=lambda c: c["name"])
def test_bound_a_torch_fp32_conv_is_inside_exact_bound(c):
    """(a) torch's CPU fp32 convolution of the same (rounded) operands lies
    inside 2*K*u*A of the float64 accumulator."""
    inp, xp, w, acc, A = _acc_level(c)
    pl, n_out, tin = c["pad_left"], c["n_out"], c["tin"]
    pr = max(0, n_out - pl + (c["k"] - 1) * c["dil"] - tin)
    x32 = F.pad(torch.from_numpy(xp).float(), (max(pl, 0), pr))
    y = F.conv1d(x32, torch.from_numpy(w).float(), dilation=c["dil"])[:, :, :n_out]
    err = np.abs(y.double().numpy() - acc)
    assert (err <= 2 * c["cin"] * c["k"] * cv.U * A).all(), float((err / A).max())


@pytest.mark.parametrize("c", [c for c in cv.CASES if c["up"] is not None],
                         ids=lambda c: c["name"])
def test_bound_a_torch_fp32_conv_transpose_is_inside_exact_bound(c):
    """(a) for the polyphase cases: torch's CPU fp32 ConvTranspose1d."""
    inp = cv.make_inputs(c)
    xp, w = cv.operands64(c, inp)
    acc, A = cv._convT64(c, xp, w), cv._convT64(c, np.abs(xp), np.abs(w))
    K, u, pad = c["up"]
    y = F.conv_transpose1d(torch.from_numpy(xp).float(), torch.from_numpy(w).float(), stride=u,
                           padding=pad)[:, :, :c["t_out"]]
    err = np.abs(y.double().numpy() - acc)
    assert (err <= 2 * c["cin"] * c["k"] * cv.U * A).all()


# (b) runs on the conv cases of at most 150 000 outputs: the emulation is a
# Python loop over channels x taps x six products; the large-tile cases have
# the same K = cin * k as small ones
@pytest.mark.parametrize("c", [c for c in SMALL if c["up"] is None
                               and c["kind"] in ("f32s", "f32p")], ids=lambda c: c["name"])
def test_bound_b_six_term_split_is_inside_split_bound(c):
    """(b) the six kept bf16 x bf16 products, accumulated in fp32 term by
    term, lie inside (6*K*u + 2^-22)*A - and the plain fp32 sum does too."""
    inp, xp, w, acc, A = _acc_level(c)
    got = cv.conv_fp32_sequential(c, xp.astype(np.float32), w.astype(np.float32), split=True)
    err = np.abs(got.astype(np.float64) - acc)
    assert (err <= cv.coef(c) * A).all(), float((err / A).max())
    # the dropped terms are really there: the five-term sum is not exact either
    assert err.max() > 0


@pytest.mark.parametrize("c", cv.CASES, ids=cv.CASE_IDS)
def test_bound_c_lost_tap_falls_outside(c):
    """(c) a reference with one tap dropped leaves the bound of every case:
    each tap in turn on the small cases, the last tap on the large ones; so
    does one shifted by a column at a tile edge.  (A clamping activation, a
    masked column or a tap that reads only padding hides the tap from some
    elements, never from all.)"""
    inp = cv.make_inputs(c)
    ops64 = cv.operands64(c, inp)
    A = cv.abs_conv(c, ops64)
    ref, e = cv.reference(c, inp, operands=ops64, A=A)[0]
    assert (e > 0).any()
    taps = range(c["k"]) if c in SMALL else [c["k"] - 1]
    for j in taps:
        lo, hi = -c["pad_left"] + j * c["dil"], c["n_out"] - 1 - c["pad_left"] + j * c["dil"]
        if hi < 0 or lo >= c["tin"]:
            continue                              # this tap reads padding only
        mut, _ = cv.reference(c, inp, operands=ops64, A=A, drop_tap=j)[0]
        out = np.abs(mut - ref) > e
        assert out.mean() > 0.05, (j, float(out.mean()))
    if min(c["tin"], ref.shape[2]) > 129 and c["up"] is None and c["lengths"] is None:
        d = np.abs(ref[:, :, 127] - ref[:, :, 128]) > e[:, :, 128]
        assert d.mean() > 0.25, float(d.mean())

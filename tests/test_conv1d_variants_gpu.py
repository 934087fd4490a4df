"""Every conv1d kernel variant against a float64 reference, at the shapes
where kernels go wrong (conv_variants_common.py: case table, reference and
the derived per-element bound).

Each case asserts, in this order: the library plans the kernel variant the
case names (so a test knows which instantiation it ran); every output lies
inside the bound; the guard bands are intact.  Outputs are interior views of
sentinel-filled allocations (guard channels before and after, a channel
stride wider than the row, slack between utterances), so an overrun is a
failed assertion, not a fault.  Inputs are interior views of NaN-filled
allocations (channels >= cin, positions outside [0, tin), the slack), so a
padding read that is multiplied by a zero weight instead of masked shows as
a non-finite output."""
import ctypes

import numpy as np
import pytest
import torch

import conv_variants_common as cv
from vits_amd import _lib, ops
from vits_amd._lib import VITS_E_UNSUP, VITS_OK

pytestmark = pytest.mark.gpu


def _np64(t: torch.Tensor) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def _check_output(name, big, C_, T_, ypad, ref, bound, keep=None):
    """Region [B][GUARD_C : GUARD_C + C_][ypad : ypad + T_] of ``big`` inside
    the bound (or still the sentinel where ``keep``), everything else of the
    allocation bit-identical to the sentinel."""
    got = _np64(big)
    g = cv.GUARD_C
    region = got[:, g:g + C_, ypad:ypad + T_]
    assert np.isfinite(region).all(), f"{name}: non-finite output"
    err = np.abs(region - ref)
    if keep is not None:
        k3 = np.broadcast_to(keep[:, None, :], region.shape)
        assert (region[k3] == cv.SENTINEL).all(), f"{name}: a skipped tile was written"
        err = np.where(k3, 0.0, err)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} outside the bound; worst at "
                             f"{i}: got {region[i]!r} ref {ref[i]!r} bound {bound[i]:.3e}")
    outside = np.ones(got.shape, dtype=bool)
    outside[:, g:g + C_, ypad:ypad + T_] = False
    assert (got[outside] == cv.SENTINEL).all(), f"{name}: stray write outside the output region"


def _run_case(c, device, inp=None):
    inp = cv.make_inputs(c) if inp is None else inp
    bt = cv.build(c, inp, device)
    rc, plan = ops.conv1d_plan(bt.desc, c["B"])
    assert rc == VITS_OK, rc
    want = cv.expected_plan(c)
    assert {f: plan[f] for f in want} == want
    ops.conv1d_launch(bt.desc, c["B"], device)
    torch.cuda.synchronize(device)
    return inp, bt, plan


def _check_case(c, inp, bt, plan):
    refs = cv.reference(c, inp)
    keep = cv.untouched_columns(c, plan) if c["len_skip"] else None
    for i, ((C_, T_), (ref, bound)) in enumerate(zip(cv.out_shapes(c), refs)):
        _check_output(f"{c['name']} out{i}", bt.ybig[i], C_, T_, c["y_tpad"], ref, bound, keep)
    if c["len_skip"]:
        # [lengths[b], lengths[b] + len_skip) is written as exact zeros
        y = _np64(bt.yview[0])[:, cv.GUARD_C:cv.GUARD_C + cv.out_shapes(c)[0][0]]
        for b, ln in enumerate(c["lengths"]):
            z = y[b, :, ln:min(ln + c["len_skip"], y.shape[2])]
            assert (z == 0).all(), (b, ln)
        assert keep.any() and not keep.all()


@pytest.mark.parametrize("c", cv.CASES, ids=cv.CASE_IDS)
def test_variant(device, c):
    inp, bt, plan = _run_case(c, device)
    _check_case(c, inp, bt, plan)


def test_refusal_is_the_same_from_plan_and_launch(device):
    """A combination the library does not support (a 16-channel F32S chunk
    whose 128 + 96-column window exceeds the stage) is refused with UNSUP by
    the plan and by the launch alike, and nothing is written."""
    c = cv.case("f32s-halo96", "f32s", "store", "64x128/2x2/v4", 2, 16, 34, 3, tile="64x128",
                dil=48, tin=260)
    bt = cv.build(c, cv.make_inputs(c), device)
    assert ops.conv1d_plan(bt.desc, c["B"]) == (VITS_E_UNSUP, None)
    lib = _lib.load()
    rc = lib.vits_conv1d_forward(ctypes.byref(bt.desc), c["B"],
                                 torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    assert rc == VITS_E_UNSUP
    assert bool((bt.ybig[0] == cv.SENTINEL).all())


# ---------------------------------------------------------------------------
# grouped launches
# ---------------------------------------------------------------------------


def _group_cases(tins):
    """Three members of one kind with different k, dil, n_out and m (the
    second spans fewer column tiles than the grid)."""
    return [
        cv.case("grp-a", "f32p", "store", "64x128/2x2/v4", 2, 16, 66, 3, tile="64x128",
                tin=tins[0], res=True),
        cv.case("grp-b", "f32p", "store", "64x128/2x2/v4", 2, 32, 34, 7, tile="64x128", dil=3,
                tin=tins[1], act=cv.ACT_RELU),
        cv.case("grp-c", "f32p", "store", "64x128/2x2/v4", 2, 17, 130, 5, tile="64x128", dil=2,
                tin=tins[2], accumulate=True),
    ]


@pytest.mark.parametrize("tins,shared", [((260, 100, 384), True), ((260, 101, 384), False)])
def test_group_of_three(device, tins, shared):
    """A tuple through conv1d_launch_seq: one launch when the plan accepts the
    group (grid = the widest member's), three when the members' staging kinds
    differ (the plan refuses with UNSUP) - the same results either way."""
    cases = _group_cases(tins)
    if not shared:
        cases[1]["plan"] = "64x128/2x2/el"
    built = [(c, cv.make_inputs(c)) for c in cases]
    built = [(c, inp, cv.build(c, inp, device)) for c, inp in built]
    descs = tuple(bt.desc for _, _, bt in built)
    rc, plan = ops.conv1d_plan(descs, 2)
    singles = [ops.conv1d_plan(d, 2)[1] for d in descs]
    for (c, _, _), p in zip(built, singles):
        want = cv.expected_plan(c)
        assert {f: p[f] for f in want} == want
    if shared:
        assert rc == VITS_OK
        assert plan["grid"] == (max(p["grid"][0] for p in singles),
                                max(p["grid"][1] for p in singles), 3 * 2)
        assert plan["grid"][0] > singles[1]["grid"][0]
    else:
        assert rc == VITS_E_UNSUP and plan is None
    _lib.dispatch_counts_reset()
    ops.conv1d_launch_seq([descs], 2, device)
    torch.cuda.synchronize(device)
    assert _lib.dispatch_counts()["conv_split"] == (1 if shared else 3)
    for (c, inp, bt), p in zip(built, singles):
        _check_case(c, inp, bt, p)


# ---------------------------------------------------------------------------
# 16-bit consistency
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("tile,plan,m,tin", [("64x128", "64x128/2x2/v4", 66, 260),
                                            ("32x256", "32x256/1x4/v4", 30, 516)])
def test_io16_2_equals_fp32_io_rounded_once(device, kind, tile, plan, m, tin):
    """The 16-bit-activation inference kernel (io16 = 2, global-A) on 16-bit
    inputs against the fp32-I/O global-A kernel on the same values: the
    MFMAs and their order are the same and the epilogue runs in fp32 in
    both, so the outputs differ by the one rounding to the type - at most
    half an ulp of the output."""
    c16 = cv.case(f"io2-{kind}-{tile}", kind, "store", plan + "/ga", 2, 32, m, 5, tile=tile,
                  tin=tin, io16=2, res=True)
    c32 = dict(c16, io16=0)
    inp = cv.make_inputs(c16)                     # x and res hold 16-bit values
    _, b16, p16 = _run_case(c16, device, inp)
    _, b32, p32 = _run_case(c32, device, inp)
    assert p16["ga"] == p32["ga"] == 1 and (p16["bm"], p16["bn"]) == (p32["bm"], p32["bn"])
    g, yp = cv.GUARD_C, c16["y_tpad"]
    y16 = _np64(b16.ybig[0][:, g:g + m, yp:yp + tin])
    y32 = _np64(b32.ybig[0][:, g:g + m, yp:yp + tin])
    assert np.isfinite(y16).all()
    assert (np.abs(y16 - y32) <= cv._half_ulp16(y32, 0.0, cv.io_dtype(c16))).all()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("tile,plan,B,m,tin", [("64x128", "64x128/2x2/v4", 2, 66, 260),
                                              ("32x256", "32x256/1x4/v4", 2, 30, 516),
                                              ("128x128", "128x128/2x2/v4", 4, 130, 8192),
                                              ("64x256", "64x256/1x4/v4", 4, 66, 16384)])
def test_global_a_equals_lds_weights(device, kind, tile, plan, B, m, tin):
    """The global-A and the LDS-weight kernels of one 16-bit type on the same
    16-bit tensors, one shape per tile (the LDS-weight kernel through io16 =
    1, never global-A; the global-A one through io16 = 2).  With one
    16-channel slab per chunk (cin = 16) they issue the same MFMAs in the
    same order: bit-identical outputs."""
    ca = cv.case(f"ga-{kind}-{tile}", kind, "store", plan + "/ga", B, 16, m, 3, tile=tile, tin=tin,
                 io16=2, res=True)
    cl = dict(ca, io16=1, plan=plan)
    _, ba, pa = _run_case(ca, device)
    _, bl, pl = _run_case(cl, device)
    assert ba.layer.kc == bl.layer.kc == 16
    assert pa["ga"] == 1 and pl["ga"] == 0
    assert torch.equal(ba.ybig[0], bl.ybig[0])


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("io16,ga", [(1, ""), (2, "/ga")])
def test_two_slab_chunks_inside_the_bound(device, kind, io16, ga):
    """With two slabs per chunk (kc = 32) the two kernels are NOT bit-identical:
    the global-A kernel walks a chunk's k-steps slab-major (slab, then tap:
    the weight image read contiguously), the LDS-weight kernel tap-major (tap,
    then slab), so their fp32 sums round differently.  Each is held to the
    bound instead."""
    c = cv.case(f"kc32-{kind}-io{io16}", kind, "store", "64x128/2x2/v4" + ga, 2, 32, 66, 3,
                tile="64x128", tin=260, io16=io16, res=True)
    inp, bt, plan = _run_case(c, device)
    assert bt.layer.kc == 32
    _check_case(c, inp, bt, plan)

"""The speech-editing kernels (csrc/edit.hip) against the numpy oracle of
tests/edit_common.py: integers exact, floats compared as bit patterns.
Outputs are pre-filled with NaN (every element must be written), NaN sits in
z_p_rec past each row's length and in the noise outside the new span (neither
may be read)."""
import numpy as np
import pytest
import torch

import edit_common as EC

pytestmark = pytest.mark.gpu
I32 = torch.int32


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# rows of the pins test: (x_len_old, x_len_new, span, sum dur_old == y_len_old?)
PINS_ROWS = [
    (12, 13, (4, 7, 8), True),    # replacement
    (12, 14, (5, 5, 7), True),    # insertion
    (12, 9, (3, 6, 3), True),     # deletion
    (12, 12, (0, 2, 2), True),    # a = 0
    (12, 15, (9, 12, 15), True),  # b_old = Tx_old
    (7, 8, (2, 4, 5), True),      # a padded row
    (12, 12, (12, 12, 12), True), # an empty edit at the end
    (12, 13, (4, 7, 9), False),   # inconsistent: the suffixes differ
    (12, 13, (8, 7, 8), False),   # inconsistent: b_old < a
    (12, 13, (4, 7, 8), None),    # the durations do not sum to the recording
    (12, 13, (4, 7, 8), "zero"),  # no alignment
    (17, 13, (4, 7, 8), False),   # x_len_old past the bucket
]


@pytest.mark.parametrize("mode", ["none", "exact", "keep"])
def test_edit_pins(device, mode):
    from vits_amd import ops

    rng = np.random.RandomState(7)
    B, t_old, t_new = len(PINS_ROWS), 16, 15
    dur_old = rng.randint(0, 9, (B, t_old + 3)).astype(np.int32)  # rows strided: stride 19
    dur_old[:, 0] += 1
    xlo = np.array([r[0] for r in PINS_ROWS], np.int32)
    xln = np.array([r[1] for r in PINS_ROWS], np.int32)
    spans = np.array([r[2] for r in PINS_ROWS], np.int32)
    y_len = np.array([dur_old[b, :min(xlo[b], t_old)].sum() for b in range(B)], np.int32)
    for b, r in enumerate(PINS_ROWS):
        if r[3] is None:
            y_len[b] += 1
        if r[3] == "zero":
            dur_old[b] = 0
            y_len[b] = 0
    span_given = rng.randint(-1, 30, (B, t_new)).astype(np.int32)
    st = {"none": None, "exact": rng.randint(1, 40, B).astype(np.int32),
          "keep": np.full(B, -1, np.int32)}[mode]
    if mode == "exact":
        st[1] = 0  # (a row without a target among them)
    d = _dev(dur_old, device)[:, :t_old]
    assert d.stride(0) == t_old + 3
    for sg in (span_given, None):
        given, target, meta = ops.edit_pins(
            d, _dev(xlo, device), _dev(xln, device), t_new, _dev(spans, device),
            _dev(y_len, device), span_given=None if sg is None else _dev(sg, device),
            span_target=None if st is None else _dev(st, device))
        torch.cuda.synchronize()
        w_given, w_target, w_meta = EC.pins(dur_old[:, :t_old], xlo, xln, t_new, spans, y_len,
                                            span_given=sg, span_target=st)
        assert given.dtype == I32 and tuple(given.shape) == (B, t_new)
        assert np.array_equal(given.cpu().numpy(), w_given)
        assert np.array_equal(target.cpu().numpy(), w_target)
        assert np.array_equal(meta.cpu().numpy(), w_meta)
    want_status = [0 if r[3] is True else 1 for r in PINS_ROWS]
    assert w_meta[2].tolist() == want_status
    if mode == "keep":
        assert all(w_target[b] == y_len[b] for b in range(B) if want_status[b] == 0)
    for b in range(B):
        if want_status[b]:
            assert not w_given[b].any() and w_target[b] == 0


def _splice_case(rng, C, t_x, t_rec, t_y, rows):
    """rows = [(x_len, span, dur_new, y_len_old)] -> numpy inputs, NaN where
    nothing may be read."""
    B = len(rows)
    dur = np.zeros((B, t_x), np.int32)
    xl = np.zeros(B, np.int32)
    spans = np.zeros((B, 3), np.int32)
    yl = np.zeros(B, np.int32)
    for b, (n, span, d, ty) in enumerate(rows):
        dur[b, :len(d)] = d
        dur[b, n:] = 99  # (past x_len: not read as durations)
        xl[b], spans[b], yl[b] = n, span, ty
    m = rng.randn(B, C, t_x).astype(np.float32)
    s = rng.rand(B, C, t_x).astype(np.float32) + 0.1
    noise = rng.randn(B, C, t_y).astype(np.float32)
    z_rec = rng.randn(B, C, t_rec).astype(np.float32)
    for b in range(B):
        z_rec[b, :, yl[b]:] = np.nan
        f0, n_new, _, st, _ = EC.splice_geometry(dur[b], xl[b], spans[b], yl[b], t_rec, t_y)
        if st == 0:
            noise[b, :, :f0] = np.nan
            noise[b, :, f0 + n_new:] = np.nan
        else:
            noise[b] = np.nan
    return dur, xl, spans, yl, m, s, noise, z_rec


# (x_len, (a, b_old, b_new), dur_new, y_len_old); shift = n_new - (f1 - f0)
SPLICE_ROWS = [
    (6, (2, 4, 5), [30, 41, 7, 0, 26, 50, 40], 30 + 41 + 20 + 50 + 40),   # x_len < tokens given
    (7, (2, 4, 5), [30, 42, 7, 0, 25, 50, 41], 30 + 42 + 29 + 50 + 41),   # shift 3: one by one
    (7, (2, 4, 5), [32, 40, 8, 4, 24, 52, 40], 32 + 40 + 32 + 52 + 40),   # shift 4: vectors
    (7, (2, 4, 5), [32, 40, 8, 4, 24, 52, 40], 32 + 40 + 44 + 52 + 40),   # shift -8: vectors
    (5, (0, 1, 2), [9, 14, 60, 61, 62], 5 + 60 + 61 + 62),                # a = 0
    (5, (3, 5, 5), [60, 61, 62, 10, 13], 60 + 61 + 62 + 40),              # through the last token
    (5, (2, 2, 4), [70, 71, 6, 5, 72], 70 + 71 + 72),                     # insertion
    (4, (1, 3, 1), [40, 41, 42, 43], 40 + 50 + 41 + 42 + 43),             # deletion: n_new = 0
    (4, (1, 2, 3), [50, 0, 0, 60], 50 + 17 + 60),                         # n_new = 0 with tokens
    (3, (1, 2, 2), [100, 150, 120], 100 + 30 + 120),                      # overflow: 370 > t_y
    (3, (2, 1, 2), [10, 20, 30], 60),                                     # inconsistent: b_old < a
    (3, (1, 2, 2), [10, 20, 30], 25),                                     # inconsistent: f1 < f0
    (0, (0, 0, 0), [], 0),                                                # an empty row
]


@pytest.mark.parametrize("C,t_rec,t_y", [(6, 300, 256), (192, 300, 256), (6, 301, 255)])
def test_edit_splice(device, C, t_rec, t_y):
    """t_rec != t_y; rows whose suffix shift is and is not a multiple of four
    (both copy paths); buckets that are no multiple of four (no vectors)."""
    from vits_amd import ops

    rng = np.random.RandomState(C + t_y)
    t_x = 8
    dur, xl, spans, yl, m, s, noise, z_rec = _splice_case(rng, C, t_x, t_rec, t_y, SPLICE_ROWS)
    B = len(SPLICE_ROWS)
    mult = (1, 1, 8, 48)
    out = torch.full((B, C, t_y), float("nan"), device=device)
    z, lens, meta = ops.edit_splice(_dev(dur, device), _dev(spans, device), _dev(yl, device),
                                    _dev(m, device), _dev(s, device), _dev(noise, device),
                                    _dev(z_rec, device), x_len=_dev(xl, device), stage_mult=mult,
                                    out=out)
    torch.cuda.synchronize()
    assert z.data_ptr() == out.data_ptr()
    w_z, w_lens, w_meta = EC.splice(dur, xl, spans, yl, m, s, noise, z_rec, stage_mult=mult)
    assert np.array_equal(meta.cpu().numpy(), w_meta)
    assert np.array_equal(lens.cpu().numpy(), w_lens)
    assert w_meta[3].tolist() == [0] * 9 + [-1, 1, 1, 0]
    assert w_meta[1, 7] == 0 and w_meta[1, 8] == 0  # the two n_new = 0 rows
    assert torch.isfinite(z).all()  # every element written, no NaN read
    assert torch.equal(_bits(z), torch.from_numpy(w_z).view(torch.int32))
    for b in range(B):
        y_new = int(w_lens[0, b])
        assert torch.count_nonzero(z[b, :, y_new:]).item() == 0, b
        if w_meta[3, b] == 0 and y_new:
            assert z[b].abs().max().item() > 0
    # the overflow row reports its geometry, so the caller can size the next bucket
    f0, n_new, f1 = w_meta[:3, 9]
    assert f0 + n_new + yl[9] - f1 == 370


@pytest.mark.parametrize("z_off,rec_off", [(1, 0), (0, 3), (2, 2)])
def test_edit_splice_with_buffers_off_a_16_byte_boundary(device, z_off, rec_off):
    """z or z_p_rec (or both) start z_off / rec_off elements past a 16-byte
    boundary: the vector paths that would touch the misaligned buffer are not
    taken, and the result is the same bits."""
    from vits_amd import ops

    C, t_x, t_rec, t_y = 6, 8, 300, 256
    rng = np.random.RandomState(5)
    dur, xl, spans, yl, m, s, noise, z_rec = _splice_case(rng, C, t_x, t_rec, t_y, SPLICE_ROWS)
    B = len(SPLICE_ROWS)
    flat_z = torch.full((B * C * t_y + 4,), float("nan"), device=device)
    flat_r = torch.zeros(B * C * t_rec + 4, device=device)
    out = flat_z[z_off:z_off + B * C * t_y].view(B, C, t_y)
    rec = flat_r[rec_off:rec_off + B * C * t_rec].view(B, C, t_rec)
    rec.copy_(_dev(z_rec, device))
    assert out.data_ptr() % 16 == 4 * z_off and rec.data_ptr() % 16 == 4 * rec_off
    z, lens, meta = ops.edit_splice(_dev(dur, device), _dev(spans, device), _dev(yl, device),
                                    _dev(m, device), _dev(s, device), _dev(noise, device), rec,
                                    x_len=_dev(xl, device), out=out)
    torch.cuda.synchronize()
    w_z, w_lens, w_meta = EC.splice(dur, xl, spans, yl, m, s, noise, z_rec)
    assert np.array_equal(meta.cpu().numpy(), w_meta) and np.array_equal(lens.cpu().numpy(), w_lens)
    assert torch.equal(_bits(z), torch.from_numpy(w_z).view(torch.int32))
    # nothing was written outside the buffer
    assert torch.isnan(flat_z[:z_off]).all() and torch.isnan(flat_z[z_off + B * C * t_y:]).all()


def test_edit_splice_equals_expand_durations_on_the_new_span(device):
    """The new span is vits_expand_durations_int's expression and rounding: an
    edit that replaces everything is bit for bit the plain expansion."""
    from vits_amd import ops

    rng = np.random.RandomState(11)
    C, t_x, t_y = 192, 40, 336  # (40 tokens of at most 8 frames fit)
    dur = rng.randint(0, 9, (2, t_x)).astype(np.int32)
    xl = np.array([40, 33], np.int32)
    spans = np.array([[0, 3, 40], [0, 0, 33]], np.int32)
    yl = np.array([10, 0], np.int32)
    m, s = (rng.randn(2, C, t_x).astype(np.float32) for _ in range(2))
    noise = rng.randn(2, C, t_y).astype(np.float32)
    # row 0 replaces the 10 frames of 3 old tokens, row 1 inserts into an empty recording
    z, lens, meta = ops.edit_splice(_dev(dur, device), _dev(spans, device), _dev(yl, device),
                                    _dev(m, device), _dev(s, device), _dev(noise, device),
                                    torch.full((2, C, 16), float("nan"), device=device),
                                    x_len=_dev(xl, device))
    ref, ref_lens = ops.expand_durations(None, _dev(m, device), _dev(s, device),
                                         _dev(noise, device), t_y, x_len=_dev(xl, device),
                                         durations=_dev(dur, device))
    torch.cuda.synchronize()
    assert meta[3].tolist() == [0, 0] and lens[0].tolist() == ref_lens[0].tolist()
    assert torch.equal(_bits(z), _bits(ref))


PATCH_CASES = [  # (ty, f0, n_new, f1, status)
    (40, 12, 9, 17, 0),    # shift > 0
    (40, 12, 3, 20, 0),    # shift < 0
    (40, 12, 6, 18, 0),    # shift = 0
    (40, 1, 5, 4, 0),      # no room for the fade in
    (40, 36, 5, 39, 0),    # no room for the fade out
    (40, 0, 7, 40, 0),     # everything replaced: both fades dropped
    (40, 20, 0, 25, 0),    # deletion
    (40, 12, 9, 17, -1),   # a refused splice
    (70, 12, 9, 17, 0),    # the recording does not fit orig
]


@pytest.mark.parametrize("hop,margin,fade", [(7, 2, 10), (7, 0, 0), (8, 3, 13), (7, 3, 1)])
def test_edit_patch(device, hop, margin, fade):
    """Lengths that are no multiple of four (hop 7), dropped fades at both
    ends, shift < 0, = 0 and > 0, fade 0 and 1."""
    from vits_amd import ops

    rng = np.random.RandomState(hop + fade)
    B = len(PATCH_CASES)
    n_orig, n_o = 41 * hop + 3, 47 * hop + 1
    orig = rng.randn(B, n_orig + 5).astype(np.float32)  # rows strided
    o = rng.randn(B, n_o).astype(np.float32)
    yl = np.array([c[0] for c in PATCH_CASES], np.int32)
    smeta = np.array([[c[1] for c in PATCH_CASES], [c[2] for c in PATCH_CASES],
                      [c[3] for c in PATCH_CASES], [c[4] for c in PATCH_CASES]], np.int32)
    for b, (ty, f0, n_new, f1, st) in enumerate(PATCH_CASES):
        if st == 0 and ty * hop <= n_orig:
            orig[b, ty * hop:] = np.nan  # never read past the recording
            o[b, (f0 + n_new + ty - f1) * hop:] = np.nan
    out = torch.full((B, n_o), float("nan"), device=device)
    got, out_len = ops.edit_patch(_dev(orig, device)[:, :n_orig], _dev(o, device),
                                  _dev(yl, device), _dev(smeta, device), hop, margin=margin,
                                  fade=fade, out=out)
    torch.cuda.synchronize()
    want, want_len = EC.patch(orig[:, :n_orig], o, yl, smeta, hop, margin, fade)
    assert np.array_equal(out_len.cpu().numpy(), want_len)
    assert want_len.tolist()[-2:] == [0, 0] and all(v > 0 for v in want_len[:-2])
    assert torch.isfinite(got).all()
    assert torch.equal(_bits(got), torch.from_numpy(want).view(torch.int32))
    # which fades were dropped is what the cases say
    if fade == 10:
        b = [EC.patch_bounds(c[1], c[2], c[3], c[0], hop, margin, fade)[4:] for c in PATCH_CASES]
        assert b[0] == (True, True) and b[3] == (False, True) and b[4] == (True, False)
        assert b[5] == (False, False)

"""The pure host pieces under EmoVITS's serving paths, CPU: the packed
buffer's layout (written by _pack, read by _unpack), the most-recently-used
graph cache (_cached_graph) and the bucket rounding (_text_bucket,
_frame_bucket).  No model and no GPU: the object is made without __init__."""
import numpy as np
import pytest
import torch

from vits_amd.infer import EmoVITS


def _bare(**attrs):
    ev = EmoVITS.__new__(EmoVITS)
    for k, v in attrs.items():
        setattr(ev, k, v)
    return ev


@pytest.mark.parametrize("B", [2, 4, 8, 16])
@pytest.mark.parametrize("extra_per_row", [0, 32])
def test_packed_header_round_trip(B, extra_per_row):
    n_extra = B * extra_per_row
    header = EmoVITS._header(B, n_extra)
    assert header % 8 == 0 and header >= 2 * (3 * B + 2 + n_extra)
    assert header - 2 * (3 * B + 2 + n_extra) < 8  # rounded up, no further
    ev = _bare()
    ev._to_host = lambda t: t.numpy()
    row_cap = 24
    for n in sorted({1, B - 1, B}):
        lens = [(5 * i + 3) % row_cap for i in range(n)]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        samples = np.arange(1, offsets[-1] + 1, dtype=np.int16)
        y_len = torch.arange(100, 100 + B, dtype=torch.int32)
        status = torch.arange(B, dtype=torch.int32) % 3 - 2
        used = torch.tensor([7 * B + n], dtype=torch.int32)
        extra = (torch.arange(n_extra, dtype=torch.int32).reshape(B, -1) * 3 + 1
                 if n_extra else None)
        seen = []

        def pack(h):
            seen.append(h)
            out = torch.full((h + B * row_cap,), -1, dtype=torch.int16)
            out[:2 * (B + 1)].view(torch.int32)[:n + 1] = torch.from_numpy(offsets)
            out[h:h + len(samples)] = torch.from_numpy(samples)
            return out

        packed = EmoVITS._pack(B, pack, (y_len, status, used), extra)
        assert seen == [header] and packed.numel() == header + B * row_cap
        pcm, offs, y, st, used_total, dur = ev._unpack(packed, B, n, n_extra)
        assert np.array_equal(pcm, samples) and pcm.dtype == np.int16
        assert np.array_equal(offs, offsets) and len(offs) == n + 1
        assert y == y_len[:n].tolist() and st == status[:n].tolist()
        assert used_total == 7 * B + n and isinstance(used_total, int)
        if n_extra:
            assert dur.dtype == np.int32 and np.array_equal(dur, extra.reshape(-1).numpy())
        else:
            assert dur is None


def test_unpack_leaves_the_padding_rows_behind():
    B, n, row_cap = 4, 2, 16
    header = EmoVITS._header(B)
    ev = _bare()
    sizes = []
    ev._to_host = lambda t: sizes.append(t.numel()) or t.numpy()
    packed = torch.zeros(header + B * row_cap, dtype=torch.int16)
    ev._unpack(packed, B, n)
    assert sizes == [header + n * row_cap]  # one copy, of the rows in use


def test_graph_cache_is_most_recently_used():
    ev = _bare(_graphs={}, max_graphs=3, _p1_graphs={}, graph_cache=2)
    made = []

    def capture(key):
        def go():
            made.append(key)
            return ("run", key)
        return go

    for k in ("a", "b", "c"):
        assert ev._cached_graph(k, capture(k)) == ("run", k)
    assert made == ["a", "b", "c"] and list(ev._graphs) == ["a", "b", "c"]
    assert ev._cached_graph("a", capture("a")) == ("run", "a")  # a hit: no capture, moved last
    assert made == ["a", "b", "c"] and list(ev._graphs) == ["b", "c", "a"]
    ev._cached_graph("d", capture("d"))  # a miss at capacity evicts the first key
    assert made == ["a", "b", "c", "d"] and list(ev._graphs) == ["c", "a", "d"]
    ev.max_graphs = 1  # a smaller limit evicts down to it
    ev._cached_graph(("vc", 1, 256), capture("e"))
    assert list(ev._graphs) == [("vc", 1, 256)] and ev._p1_graphs == {}
    # the p1 cache obeys graph_cache the same way, apart from _graphs
    made.clear()
    for k in (10, 20, 10, 30):
        ev._cached_graph(k, capture(k), p1=True)
    assert made == [10, 20, 30] and list(ev._p1_graphs) == [10, 30]
    assert list(ev._graphs) == [("vc", 1, 256)]


def test_bucket_rounding():
    """Against the values of the expressions these helpers replaced
    (``-(-t // 32) * 32``; ``max(256, 1 << (n - 1).bit_length())``; where a
    bucket grows after a re-run, which happens above 256 frames only,
    ``min(4096, 1 << (n - 1).bit_length())``)."""
    ns = (1, 255, 256, 257, 4096, 4097)
    assert [EmoVITS._text_bucket(t) for t in ns] == [32, 256, 256, 288, 4096, 4128]
    assert [EmoVITS._frame_bucket(n) for n in ns] == [256, 256, 256, 512, 4096, 8192]
    assert [EmoVITS._frame_bucket(n, cap=4096) for n in ns] == [256, 256, 256, 512, 4096, 4096]
    assert EmoVITS._frame_bucket(0) == 256
    assert [EmoVITS._vc_bucket(n) for n in ns[:-1]] == [256, 256, 256, 512, 4096]
    with pytest.raises(ValueError, match="4097 frames exceeds the largest conversion bucket"):
        EmoVITS._vc_bucket(4097)

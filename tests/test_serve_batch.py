"""Host side of batched serving (EmoVITS.infer_batch / infer_pcm_batch), CPU.

A batch draws its noise-slice starts on the device from ONE pool of raw
MT19937 words, row after row (misc.hip draw_starts_kernel); the host then
re-advances numpy's generator by the total number of words consumed.
``shared_pool_draw`` restates the kernel's draw phase; with
ops.numpy_draw_commit it must give the values AND the final generator state
of the same randint calls made one after another."""
import numpy as np
import pytest

from serve_batch_common import same_state, shared_pool_draw

from vits_amd import ops


@pytest.mark.parametrize("seed", [0, 1, 7, 123])
def test_shared_pool_draws_are_consecutive_randint_calls(seed):
    highs = [700, 1, 513, 2 ** 20 + 3]
    np.random.seed(seed)
    want = [np.random.randint(h) for h in highs]
    want_state = np.random.get_state()
    np.random.seed(seed)
    pool, state = ops.numpy_draw_pool(ops.ED_DRAWS * len(highs))
    starts, status, used_total = shared_pool_draw(pool, highs)
    assert starts == want
    assert status[1] == 0 and min(status) >= 0  # high = 1 consumes no word
    assert used_total == sum(status)
    ops.numpy_draw_commit(state, used_total)
    assert same_state(np.random.get_state(), want_state)


def test_shared_pool_status_codes():
    pool = np.full(8, 0xFFFFFFFF, dtype=np.uint32)
    # rng = 5: mask 7, every word gives 7 > 5 -> the pool runs out at row 1
    starts, status, _ = shared_pool_draw(pool, [1, 6, 1, 6])
    assert status == [0, -2, 0, -2] and starts == [0, -1, 0, -1]
    np.random.seed(2)
    pool, _ = ops.numpy_draw_pool(16)
    a = shared_pool_draw(pool, [100, 0, 100])
    b = shared_pool_draw(pool, [100, 100])
    assert a[1][1] == -1 and a[0][1] == -1
    assert [a[0][0], a[0][2]] == b[0] and a[2] == b[2]  # -1 consumed nothing
    # padding rows draw nothing and do not move the rows before them
    c = shared_pool_draw(pool, [100, 100, 100], n_rows=2)
    assert c[0] == b[0] + [0] and c[1] == b[1] + [0] and c[2] == b[2]


def test_groups_and_batch_buckets(monkeypatch):
    from vits_amd.infer import EmoVITS

    assert EmoVITS.MAX_BATCH == 16
    assert EmoVITS._groups(19) == [(0, 16), (16, 19)]
    assert EmoVITS._groups(16) == [(0, 16)] and EmoVITS._groups(1) == [(0, 1)]
    assert [EmoVITS._batch_bucket(n) for n in (2, 3, 4, 5, 8, 9, 16)] == [2, 4, 4, 8, 8, 16, 16]
    with pytest.raises(ValueError):
        EmoVITS._batch_bucket(17)
    monkeypatch.setattr(EmoVITS, "MAX_BATCH", 2)
    assert EmoVITS._groups(5) == [(0, 2), (2, 4), (4, 5)]


def test_batch_entry_points_on_cpu_are_the_loop(tmp_path):
    """On a CPU device infer_batch / infer_pcm_batch are a loop over infer /
    infer_pcm behind the emotion lookups; here the model is never reached
    (no GPU): the entry points exist, resolve in item order and return the
    empty result for an empty request."""
    import torch

    from common import build_model, tiny_cfg
    from vits_amd.infer import EmoVITS
    from vits_amd.utils import get_hparams_from_dict

    c = tiny_cfg()
    hps = get_hparams_from_dict({"data": {"sampling_rate": 16000, "hop_length": 192,
                                          "text_channels": c["data"]["text_channels"],
                                          "n_speakers": c["data"]["n_speakers"],
                                          "noise_scale": 0.707},
                                 "model": c["model"]})
    ev = EmoVITS(str(tmp_path / "ckpt.pth"), torch.device("cpu"), hps=hps,
                 model=build_model(c["model"], c["data"]))
    assert ev.infer_batch([]) == []
    pcm, offsets, emos, n_model = ev.infer_pcm_batch([])
    assert pcm.dtype == np.int16 and len(pcm) == 0 and offsets.tolist() == [0]
    assert emos == [] and n_model == []
    emo = torch.zeros(1, 1024)
    texts, spkids, emos = ev._resolve_items([(1, np.zeros((3, 4), np.float32), emo),
                                             (0, np.zeros((5, 4), np.float32), emo)])
    assert spkids == [1, 0] and [t.shape[0] for t in texts] == [3, 5]
    assert all(e.dtype == torch.float16 and e.shape == (1, 1024) for e in emos)
    assert not ev._batchable(texts)  # CPU: the per-item path


def test_vitswrap_batch_segments_is_keyword_only_and_cuda_only():
    import inspect

    from vits_amd import vits_wrap

    p = inspect.signature(vits_wrap.VITSWrap.__init__).parameters["batch_segments"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert vits_wrap.VITSWrap.BATCH_MIN_SEGMENTS >= 2

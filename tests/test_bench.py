"""bench.py's plain run, --dump-outputs and the --full switch."""
import json
import sys

import numpy as np
import pytest
import torch


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """An output within the byte budget is written whole as float32; a larger
    one as the same seeded sample of its elements on every call."""
    import bench

    x = torch.arange(1000, dtype=torch.float16).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / "a"), {"wav": x})
    a = np.load(tmp_path / "a" / "wav.npy")
    assert a.dtype == np.float32 and a.shape == (10, 100) and np.array_equal(a, x.float().numpy())

    assert bench.DUMP_MAX_BYTES <= 64_000_000
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    y = torch.arange(1000, dtype=torch.float64)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"wav": y}, rank=1, world=2)
    b = np.load(tmp_path / "b" / "wav_rank1.npy")
    c = np.load(tmp_path / "c" / "wav_rank1.npy")
    # 4096 bytes over two ranks, the file's header included
    assert (tmp_path / "b" / "wav_rank1.npy").stat().st_size <= 2048
    assert b.dtype == np.float64 and b.size == (2048 - bench.NPY_HEADER_BYTES) // 8
    assert np.array_equal(b, c) and np.all(np.diff(b) > 0) and 0 <= b.min() and b.max() < 1000


def test_plain_run_drops_every_leg(monkeypatch, capsys):
    """Without --full every --no-<leg> switch is on before any device work
    (checked at the --dry-run exit, which needs no GPU)."""
    import bench

    seen = {}
    real = bench.dry_run_line

    def spy(args, *a):
        seen.update(vars(args))
        return real(args, *a)

    monkeypatch.setattr(bench, "dry_run_line", spy)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for full in (False, True):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--dry-run", "--steps", "2", "--warmup", "1"]
                            + (["--full"] if full else []))
        bench.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        for k in ("no_train", "no_roofline", "no_longform", "no_kernels", "no_cpu_baseline"):
            assert seen[k] is (not full), (full, k)


@pytest.mark.gpu
def test_plain_run_line_and_dump_repeatable(tmp_path, monkeypatch, capsys, device):
    """Two plain runs with the same arguments: one result line each (no
    kernel_table line, the --full legs null), --steps timed steps, and the
    dumped waveform bit-identical between them."""
    import bench

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    wavs = []
    for d in ("a", "b"):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                                          "--batch", "2", "--tx", "12", "--ty", "60",
                                          "--dump-outputs", str(tmp_path / d)])
        bench.main()
        out = capsys.readouterr().out.strip().splitlines()
        assert len(out) == 1, out
        line = json.loads(out[0])
        assert line["metric"] == bench.METRIC and line["unit"] == "output samples/s"
        assert line["higher_is_better"] is True and line["dtype"] == "fp32"
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(2 * 60 * 192 / (line["ms_per_step"] / 1e3), rel=1e-2)
        for k in ("roofline", "cpu_baseline", "kernels", "latency_b1", "longform", "train",
                  "train_c3"):
            assert line[k] is None, k
        wavs.append(np.load(tmp_path / d / "wav.npy"))
    assert wavs[0].dtype == np.float32 and wavs[0].shape == (2, 1, 60 * 192)
    assert np.isfinite(wavs[0]).all() and np.abs(wavs[0]).max() > 0
    assert np.array_equal(wavs[0], wavs[1])

"""Regenerate tests/golden/base_durations.npz: one base-config utterance of 20
tokens spoken by the REFERENCE model with hand-edited durations (a token of 0
frames, one of 30, 98 frames in all): the reference's infer_p1, a one-hot path
built here from the durations, the reference's infer_p2.

Runs only in the build container, on the CPU (it imports the read-only
reference the way make_golden.py does); the GPU box never runs it.  The file
holds inputs and outputs only: x, emo, sid, durations, noise (pre-scaled) and
the waveform."""
from __future__ import annotations

import os

import numpy as np
import torch

from make_golden import HERE, _ref, base_cfg, np32
from vits_amd.utils import deterministic_fill_

DURATIONS = [3, 5, 0, 7, 2, 30, 1, 4, 6, 2, 0, 3, 8, 1, 5, 4, 2, 9, 3, 3]


def main():
    models, _ = _ref()
    cfg = base_cfg()
    m = models.SynthesizerTrn(cfg["data"]["text_channels"], cfg["data"]["filter_length"] // 2 + 1,
                              cfg["train"]["segment_size"] // cfg["data"]["hop_length"],
                              n_speakers=cfg["data"]["n_speakers"], **cfg["model"]).eval()
    deterministic_fill_(m)
    g = torch.Generator().manual_seed(20261)
    t_x = len(DURATIONS)
    d = np.asarray(DURATIONS, np.int64)
    t_y = int(d.sum())
    assert t_x == 20 and t_y <= 100 and 0 in DURATIONS and 30 in DURATIONS
    x = torch.randn(1, t_x, 256, generator=g)
    emo = torch.randn(1, 1024, generator=g)
    sid = torch.tensor([11])
    noise = torch.randn(1, 192, t_y, generator=g) * 0.707
    # the path: frame t belongs to the token whose cumulative span holds it
    attn = np.zeros((1, t_y, t_x), np.float32)
    attn[0, np.arange(t_y), np.repeat(np.arange(t_x), d)] = 1.0
    with torch.no_grad():
        m_p, s_p, logw, gg = m.infer_p1(x, emo, sid)
        wav = m.infer_p2(torch.from_numpy(attn), m_p, s_p, gg, noise)
    assert wav.shape[-1] == t_y * 192 and torch.isfinite(wav).all()
    np.savez_compressed(os.path.join(HERE, "base_durations.npz"), x=np32(x), emo=np32(emo),
                        sid=sid.numpy(), durations=d.astype(np.int32), noise=np32(noise),
                        wav=np32(wav))
    print("base_durations.npz: %d tokens, %d frames, |wav| max %.4f" %
          (t_x, t_y, wav.abs().max().item()))


if __name__ == "__main__":
    main()

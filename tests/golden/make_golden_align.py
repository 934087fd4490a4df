"""Generate tests/golden/base_align.npz FROM THE REFERENCE ITSELF: forced
alignment of one short recording with its text through the reference's own
modules on the CPU.

Runs only in the build container, like make_golden_vc.py (whose helpers it
borrows): it imports the read-only reference.  Weights: configs/base.json with
vits_amd.utils.deterministic_fill_ (no checkpoint is shipped).

Composition (the reference aligns only inside its training forward, with
alignment noise; this is that forward's alignment without the noise):
  spec          = spectrogram_torch(wav)        restated in tests/vc_common.py
  _, m_p, logs_p, _ = enc_p(x, [Tx], emo, g)    models.py:167-178
  z             = enc_q.infer(spec, 0)          models.py:273-279: the mean
  z_p           = flow(z, ones, g)              models.py:219-222
  neg_cent      = the four terms                models.py:484-490
  path          = oracle/mas.py                 models.py:498
  durations     = path.sum(frames); scores = per-token float32 sums of
                  neg_cent along the path, in frame order

Contents: B = 1, generator seed 7, 61 * 192 + 57 samples (61 frames), 20
tokens, speaker 7; arrays wav, x, emo, sid, z_p, m_p, logs_p, neg_cent,
durations, scores.

Before writing, the path is checked to be stable: 20 random relative
perturbations neg_cent * (1 + 1e-3 * N(0, 1)) must all give the same path
(also run for two other input sets, which are not stored), so a test may ask
for exactly these durations from any implementation whose neg_cent is within
1e-4.

Usage: python tests/golden/make_golden_align.py
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (puts the repository root on sys.path)
import align_common as A  # noqa: E402
import vc_common as VC  # noqa: E402
from oracle import mas as mas_oracle  # noqa: E402


def compose(m, cfg, seed, n_samples, t_x, sid):
    wav, x, emo = A.golden_inputs(seed, n_samples, t_x, cfg["data"]["text_channels"])
    sid = torch.tensor([sid])
    with torch.no_grad():
        spec = VC.spectrogram(wav)
        g = m.emb_g(sid)
        _, m_p, logs_p, _ = m.enc_p(x, torch.tensor([t_x]), emo, g)
        z = m.enc_q.infer(spec, 0)
        z_p = m.flow(z, torch.ones(1, 1, z.shape[2]), g=g)
        s_p_sq_r = torch.exp(-2 * logs_p)
        nc1 = torch.sum(-0.5 * math.log(2 * math.pi) - logs_p, [1], keepdim=True)
        nc2 = torch.matmul(-0.5 * (z_p ** 2).transpose(1, 2), s_p_sq_r)
        nc3 = torch.matmul(z_p.transpose(1, 2), (m_p * s_p_sq_r))
        nc4 = torch.sum(-0.5 * (m_p ** 2) * s_p_sq_r, [1], keepdim=True)
        nc = nc1 + nc2 + nc3 + nc4
    return wav, x, emo, sid, z_p, m_p, logs_p, nc


def stable_path(nc, what):
    """The oracle's path of nc [1, Tt, Ts]; asserts that 20 relative
    perturbations of 1e-3 (and of 1e-4 .. 1e-6) leave it unchanged."""
    v = G.np32(nc)
    _, Tt, Ts = v.shape
    tt, ts = np.array([Tt]), np.array([Ts])
    path = mas_oracle.maximum_path_lengths(v, tt, ts)
    rng = np.random.default_rng(0)
    for eps in (1e-6, 1e-5, 1e-4, 1e-3):
        changed = 0
        for _ in range(20):
            p = (v * (1 + eps * rng.standard_normal(v.shape))).astype(np.float32)
            changed += int((mas_oracle.maximum_path_lengths(p, tt, ts) != path).any())
        print(f"{what}: {Tt} frames x {Ts} tokens, eps {eps:g}: {changed} of 20 paths changed")
        assert changed == 0, (what, eps, changed)
    return path[0]


def main():
    torch.set_num_threads(8)
    models, _ = G._ref()
    cfg = G.base_cfg()
    m = models.SynthesizerTrn(cfg["data"]["text_channels"], cfg["data"]["filter_length"] // 2 + 1,
                              cfg["train"]["segment_size"] // cfg["data"]["hop_length"],
                              n_speakers=cfg["data"]["n_speakers"], **cfg["model"]).eval()
    G.deterministic_fill_(m)
    d = cfg["data"]
    assert (d["filter_length"], d["hop_length"], d["win_length"]) == (
        VC.STFT["n_fft"], VC.STFT["hop"], VC.STFT["win"])
    # two more input sets, checked for stability only
    for seed, t_x, frames in ((2025, 12, 40), (11, 33, 97)):
        stable_path(compose(m, cfg, seed, frames * 192 + 57, t_x, A.GOLDEN_SID)[-1],
                    f"seed {seed}")
    wav, x, emo, sid, z_p, m_p, logs_p, nc = compose(m, cfg, A.GOLDEN_SEED, A.GOLDEN_L,
                                                     A.GOLDEN_TX, A.GOLDEN_SID)
    assert z_p.shape[2] == A.GOLDEN_FRAMES
    path = stable_path(nc, "fixture")
    durations = path.sum(0).astype(np.int32)
    tokens = A.path_tokens(path)
    scores = A.token_scores(G.np32(nc)[0], tokens, A.GOLDEN_TX)
    print("durations", durations.tolist())
    np.savez_compressed(os.path.join(HERE, "base_align.npz"), wav=G.np32(wav), x=G.np32(x),
                        emo=G.np32(emo), sid=sid.numpy(), z_p=G.np32(z_p), m_p=G.np32(m_p),
                        logs_p=G.np32(logs_p), neg_cent=G.np32(nc), durations=durations,
                        scores=scores)


if __name__ == "__main__":
    main()

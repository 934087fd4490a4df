"""Generate tests/golden/base_edit.npz FROM THE REFERENCE ITSELF: one speech
edit (SynthesizerTrn.edit) of a short recording, composed from
the reference's own modules on the CPU.

Runs only in the build container, like make_golden_vc.py (whose pattern it
follows): it imports the read-only reference.  Weights: configs/base.json with
vits_amd.utils.deterministic_fill_.  Only inputs and outputs are written.

Composition (the reference has no edit method of its own):
  spec     = spectrogram_torch(wav)              as make_golden_vc.py
  z_p_rec  = flow.forward(enc_q.infer(spec, noise_q), ones, g)
  m_p, s_p = infer_p1(x_new, emo, sid)           models.py:558-566
  z_p      = z_p_rec[:, :f0] | m_p[x(t)] + noise[t] * s_p[x(t)] | z_p_rec[:, f1:]
             (the expansion is attn @ m_p, attn @ s_p with a one-hot path over
             the new span's hand durations, as make_golden_durations.py builds it)
  z_hat    = flow.infer(z_p, g, reverse=True)    models.py:228-235
  o        = dec(z_hat, g)                       models.py:306-318

Contents: 60 frames + 57 samples, 12 -> 13 tokens (span 4, 7, 8), the old
durations and the new span's by hand (a token of 0 frames among them); arrays
wav, x_old, x_new, emo, sid, span, dur_old, dur_new, noise, noise_q, spec,
z_p_rec, z_p, z_hat, o.

Usage: python tests/golden/make_golden_edit.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (puts the repository root on sys.path)
import edit_common as EC  # noqa: E402
import vc_common as VC  # noqa: E402


def main():
    torch.set_num_threads(8)
    models, _ = G._ref()
    cfg = G.base_cfg()
    m = models.SynthesizerTrn(cfg["data"]["text_channels"], cfg["data"]["filter_length"] // 2 + 1,
                              cfg["train"]["segment_size"] // cfg["data"]["hop_length"],
                              n_speakers=cfg["data"]["n_speakers"], **cfg["model"]).eval()
    G.deterministic_fill_(m)
    C = cfg["model"]["inter_channels"]
    a, b_old, b_new = EC.GOLDEN_SPAN
    dur_old = np.asarray(EC.GOLDEN_DUR_OLD, np.int64)
    t_old, t_new = len(dur_old), len(dur_old) - (b_old - a) + (b_new - a)
    dur_new = np.concatenate([dur_old[:a], EC.GOLDEN_DUR_SPAN, dur_old[b_old:]]).astype(np.int64)
    assert (t_old, t_new) == (12, 13) and len(dur_new) == t_new and 0 in EC.GOLDEN_DUR_SPAN
    g = torch.Generator().manual_seed(2026)
    wav = (torch.randn(1, EC.GOLDEN_L, generator=g) * 0.3).clamp(-1, 1)
    x_old = torch.randn(1, t_old, 256, generator=g)
    x_new = torch.cat([x_old[:, :a], torch.randn(1, b_new - a, 256, generator=g),
                       x_old[:, b_old:]], 1)
    emo = torch.randn(1, 1024, generator=g)
    sid = torch.tensor([EC.GOLDEN_SID])
    with torch.no_grad():
        spec = VC.spectrogram(wav)
        ty = spec.shape[2]
        assert ty == 60 == int(dur_old.sum())
        f0, f1 = int(dur_old[:a].sum()), int(dur_old[:b_old].sum())
        n_new = int(dur_new[a:b_new].sum())
        y_new = f0 + n_new + ty - f1
        noise_q = torch.randn(1, C, ty, generator=g) * 0.3
        noise = torch.randn(1, C, y_new, generator=g) * 0.667
        gg = m.emb_g(sid)
        z = m.enc_q.infer(spec, noise_q)
        z_p_rec = m.flow(z, torch.ones(1, 1, ty), g=gg)
        m_p, s_p, _, gg1 = m.infer_p1(x_new, emo, sid)
        assert torch.equal(gg1, gg)
        # the one-hot path of the new span alone: frame f0 + i <- its token
        tok = np.repeat(np.arange(t_new), dur_new)[f0:f0 + n_new]
        attn = np.zeros((1, n_new, t_new), np.float32)
        attn[0, np.arange(n_new), tok] = 1.0
        attn = torch.from_numpy(attn)
        m_e = torch.matmul(attn, m_p.transpose(1, 2)).transpose(1, 2)
        s_e = torch.matmul(attn, s_p.transpose(1, 2)).transpose(1, 2)
        z_p = torch.cat([z_p_rec[:, :, :f0], m_e + noise[:, :, f0:f0 + n_new] * s_e,
                         z_p_rec[:, :, f1:]], 2)
        assert z_p.shape[2] == y_new == 61
        z_hat = m.flow.infer(z_p, g=gg, reverse=True)
        o = m.dec(z_hat, g=gg)
    assert o.shape[-1] == y_new * 192 and torch.isfinite(o).all()
    np.savez_compressed(
        os.path.join(HERE, "base_edit.npz"), wav=G.np32(wav), x_old=G.np32(x_old),
        x_new=G.np32(x_new), emo=G.np32(emo), sid=sid.numpy(),
        span=np.asarray(EC.GOLDEN_SPAN, np.int32), dur_old=dur_old.astype(np.int32),
        dur_new=dur_new.astype(np.int32), noise=G.np32(noise), noise_q=G.np32(noise_q),
        spec=G.np32(spec), z_p_rec=G.np32(z_p_rec), z_p=G.np32(z_p), z_hat=G.np32(z_hat),
        o=G.np32(o))
    print("base_edit.npz: %d -> %d tokens, %d -> %d frames, |o| max %.4f" %
          (t_old, t_new, ty, y_new, o.abs().max().item()))


if __name__ == "__main__":
    main()

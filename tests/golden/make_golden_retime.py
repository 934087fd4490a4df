"""Generate tests/golden/base_retime.npz FROM THE REFERENCE ITSELF: one
retiming (SynthesizerTrn.retime) of a short recording, composed
from the reference's own modules on the CPU.

Runs only in the build container, like make_golden_edit.py (whose pattern,
seed and weights recipe it follows): it imports the read-only reference.
Weights: configs/base.json with vits_amd.utils.deterministic_fill_.  Only
inputs and outputs are written.

Composition (the reference has no retime method of its own):
  spec    = spectrogram_torch(wav)              as make_golden_vc.py
  z_p     = flow.forward(enc_q.infer(spec, noise_q), ones, g_src)
  dur_new = the plan (tests/retime_common.plan) of the hand durations under
            one pin, one scaled token and a target
  z_warp  = the numpy warp (tests/retime_common.warp) of z_p
  z_hat   = flow.infer(z_warp, g_tgt, reverse=True)   models.py:228-235
  o       = dec(z_hat, g_tgt)                          models.py:306-318

Contents: 60 frames + 57 samples, 12 tokens with hand durations (a token of 0
frames among them), 71 new frames; arrays wav, sid_src, sid_tgt, dur_old,
given, tok_scale, target, dur_new, noise_q, spec, z_p, z_warp, z_hat, o.

Usage: python tests/golden/make_golden_retime.py
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
import retime_common as RC  # noqa: E402
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
    dur_old = np.asarray(RC.GOLDEN_DUR_OLD, np.int64)
    given = np.asarray(RC.GOLDEN_GIVEN, np.int64)
    tok_scale = np.asarray(RC.GOLDEN_TOK_SCALE, np.float32)
    t_x = len(dur_old)
    assert t_x == 12 and 0 in dur_old and (given >= 0).sum() == 1 and (tok_scale != 1).sum() == 1
    g = torch.Generator().manual_seed(2026)
    wav = (torch.randn(1, RC.GOLDEN_L, generator=g) * 0.3).clamp(-1, 1)
    sid_src, sid_tgt = torch.tensor([RC.GOLDEN_SID_SRC]), torch.tensor([RC.GOLDEN_SID_TGT])
    with torch.no_grad():
        spec = VC.spectrogram(wav)
        ty = spec.shape[2]
        assert ty == 60 == int(dur_old.sum())
        dur_new, total, status = RC.plan(dur_old[None], [t_x], [ty], given[None], tok_scale[None],
                                         None, [RC.GOLDEN_TARGET])
        assert status[0] == 0 and total[0] == RC.GOLDEN_TARGET == 71
        noise_q = torch.randn(1, C, ty, generator=g) * 0.3
        z = m.enc_q.infer(spec, noise_q)
        z_p = m.flow(z, torch.ones(1, 1, ty), g=m.emb_g(sid_src))
        zw, lens, meta = RC.warp(z_p.numpy(), dur_old[None], dur_new, [t_x], [ty], 71)
        assert meta[:, 0].tolist() == [71, 0] and lens[0, 0] == 71
        z_warp = torch.from_numpy(zw)
        gt = m.emb_g(sid_tgt)
        z_hat = m.flow.infer(z_warp, g=gt, reverse=True)
        o = m.dec(z_hat, g=gt)
    assert o.shape[-1] == 71 * 192 and torch.isfinite(o).all()
    np.savez_compressed(
        os.path.join(HERE, "base_retime.npz"), wav=G.np32(wav), sid_src=sid_src.numpy(),
        sid_tgt=sid_tgt.numpy(), dur_old=dur_old.astype(np.int32), given=given.astype(np.int32),
        tok_scale=tok_scale, target=np.asarray([RC.GOLDEN_TARGET], np.int32),
        dur_new=dur_new[0].astype(np.int32), noise_q=G.np32(noise_q), spec=G.np32(spec),
        z_p=G.np32(z_p), z_warp=G.np32(z_warp), z_hat=G.np32(z_hat), o=G.np32(o))
    print("base_retime.npz: %d tokens, %d -> %d frames, dur_new %s, |o| max %.4f" %
          (t_x, ty, 71, dur_new[0].tolist(), o.abs().max().item()))


if __name__ == "__main__":
    main()

"""Test-side oracle of forced alignment: the composition the golden fixture
base_align.npz pins (tests/golden/make_golden_align.py writes it from the
reference's own modules), restated on oracle/vits_oracle.py, the forward flow
of tests/vc_common.py and the MAS oracle, plus the numpy reductions of a path
that the kernel's epilogue is held to.

  m_p, logs_p = enc_p(x, [Tx], emo, g)          models.py:167-178
  z           = enc_q.infer(spec, 0)            models.py:273-279 (posterior mean)
  z_p         = flow(z, ones, g)                models.py:219-222
  neg_cent    = the four terms                  models.py:484-490
  path        = maximum_path(neg_cent, mask)    models.py:498 (no alignment noise)
"""
import numpy as np
import torch

import vc_common as VC
from oracle import mas as mas_oracle
from oracle import vits_oracle as V

from common import BASE_MODEL

# the fixture's shape: 61 frames and a ragged tail, 20 tokens, speaker 7
GOLDEN_SEED = 7
GOLDEN_FRAMES = 61
GOLDEN_L = GOLDEN_FRAMES * 192 + 57
GOLDEN_TX = 20
GOLDEN_SID = 7


def golden_inputs(seed, n_samples, t_x, text_channels):
    """The seeded inputs of a fixture row: (wav [1, n], x [1, t_x, c], emo [1, 1024])."""
    g = torch.Generator().manual_seed(seed)
    wav = (torch.randn(1, n_samples, generator=g) * 0.3).clamp(-1, 1)
    x = torch.randn(1, t_x, text_channels, generator=g)
    emo = torch.randn(1, 1024, generator=g)
    return wav, x, emo


def path_tokens(path):
    """[Tt, Ts] 0/1 path -> the token of every frame."""
    return np.argmax(path, axis=1).astype(np.int32)


def token_scores(neg_cent, tokens, t_s):
    """Per-token sums of neg_cent [Tt, Ts] along the path, float32 adds in
    increasing frame order from 0.0f: what the kernel computes, exactly."""
    out = np.zeros(t_s, dtype=np.float32)
    nc = np.asarray(neg_cent, dtype=np.float32)
    for y, x in enumerate(tokens):
        out[x] = np.float32(out[x] + nc[y, x])
    return out


def mas_reduce(neg_cent, t_t, t_s):
    """Oracle path of one row neg_cent [Tt, Ts] at lengths (t_t, t_s), reduced:
    (durations int32 [Ts], scores fp32 [Ts], frame_token int32 [Tt]); a row
    without an alignment gives 0 / 0 / -1."""
    Tt, Ts = neg_cent.shape
    dur = np.zeros(Ts, dtype=np.int32)
    sc = np.zeros(Ts, dtype=np.float32)
    ft = np.full(Tt, -1, dtype=np.int32)
    if t_t == 0 or t_s == 0 or t_t < t_s:
        return dur, sc, ft
    live = np.ascontiguousarray(neg_cent[:t_t, :t_s], dtype=np.float32)
    path = mas_oracle.maximum_path_lengths(live[None], np.array([t_t]), np.array([t_s]))[0]
    dur[:t_s] = path.sum(0)
    ft[:t_t] = path_tokens(path)
    sc[:t_s] = token_scores(live, ft[:t_t], t_s)
    return dur, sc, ft


def align_oracle(sd, spec, x, emo, sid, cfg=BASE_MODEL):
    """The fixture's composition on a state dict, B = 1, exact lengths:
    (z_p, m_p, logs_p, neg_cent, durations int32 [Tx], scores fp32 [Tx])."""
    H = cfg["hidden_channels"]
    g = sd["emb_g.weight"][torch.as_tensor(sid).long()]
    t_x = x.shape[1]
    _, m_p, logs_p, _ = V.text_encoder(sd, x, emo, g, cfg["n_layers"], cfg["n_heads"],
                                       cfg["inter_channels"], x_lengths=torch.tensor([t_x]))
    z = V.posterior_infer(sd, spec, 0.0, cfg["n_layers_q"], H)
    z_p = VC.flow_forward(sd, z, g, cfg.get("n_flows", 4), 4, H)
    nc = V.neg_cent(z_p, m_p, logs_p)
    dur, sc, _ = mas_reduce(nc[0].numpy(), z_p.shape[2], t_x)
    return z_p, m_p, logs_p, nc, dur, sc

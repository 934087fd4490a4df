"""Test-side oracle of forced alignment with a text in segments, on the pieces
of tests/align_common.py: the text encoder runs per segment, each with its own
emotion vector, m_p / logs_p are concatenated along the tokens, then the audio
side, neg_cent and the MAS oracle of the whole recording, reduced in numpy.
With one segment this is align_common.align_oracle."""
import numpy as np
import torch

import align_common as A
import vc_common as VC
from oracle import mas as mas_oracle
from oracle import vits_oracle as V

from common import BASE_MODEL

# the recording and text of the GPU comparison (tests/test_align_long_gpu.py):
# 600 frames and a ragged tail, three segments.  SEED is chosen so that the
# oracle's own path is unchanged by relative perturbations of its neg_cent of
# 1e-6 .. 1e-3 (tests/test_align_long.py asserts it on the CPU)
LONG_SEED = 6
LONG_FRAMES = 600
LONG_L = LONG_FRAMES * 192 + 57
LONG_TOKENS = (40, 25, 50)
LONG_SID = 7
LONG_SID_T = torch.tensor([LONG_SID])


def long_inputs(seed, n_samples, tokens, text_channels):
    """The seeded inputs: (wav [1, n], xs [[1, t, c]], emos [[1, 1024]]), one
    x and emo per entry of ``tokens``; with one entry, align_common.golden_inputs."""
    g = torch.Generator().manual_seed(seed)
    wav = (torch.randn(1, n_samples, generator=g) * 0.3).clamp(-1, 1)
    xs, emos = [], []
    for t in tokens:
        xs.append(torch.randn(1, t, text_channels, generator=g))
        emos.append(torch.randn(1, 1024, generator=g))
    return wav, xs, emos


def segment_oracle(sd, spec, xs, emos, sid, cfg=BASE_MODEL):
    """B = 1, exact lengths: (z_p, m_p, logs_p, neg_cent, durations int32
    [Tx_total], scores fp32 [Tx_total], segment token offsets)."""
    H = cfg["hidden_channels"]
    g = sd["emb_g.weight"][torch.as_tensor(sid).long().reshape(1)]
    ms, ls, offs = [], [], [0]
    for x, emo in zip(xs, emos):
        t_x = x.shape[1]
        _, m, lg, _ = V.text_encoder(sd, x, emo, g, cfg["n_layers"], cfg["n_heads"],
                                     cfg["inter_channels"], x_lengths=torch.tensor([t_x]))
        ms.append(m)
        ls.append(lg)
        offs.append(offs[-1] + t_x)
    m_p, logs_p = torch.cat(ms, dim=2), torch.cat(ls, dim=2)
    z = V.posterior_infer(sd, spec, 0.0, cfg["n_layers_q"], H)
    z_p = VC.flow_forward(sd, z, g, cfg.get("n_flows", 4), 4, H)
    nc = V.neg_cent(z_p, m_p, logs_p)
    dur, sc, _ = A.mas_reduce(nc[0].numpy(), z_p.shape[2], offs[-1])
    return z_p, m_p, logs_p, nc, dur, sc, offs


def path_is_stable(nc, trials=20, seed=0):
    """make_golden_align.stable_path without the assertion: {eps: paths
    changed of ``trials``} for relative perturbations nc * (1 + eps * N(0, 1))
    of the oracle's neg_cent [1, Tt, Ts]."""
    v = np.ascontiguousarray(np.asarray(nc, dtype=np.float32))
    _, Tt, Ts = v.shape
    tt, ts = np.array([Tt]), np.array([Ts])
    path = mas_oracle.maximum_path_lengths(v, tt, ts)
    rng = np.random.default_rng(seed)
    out = {}
    for eps in (1e-6, 1e-5, 1e-4, 1e-3):
        changed = 0
        for _ in range(trials):
            p = (v * (1 + eps * rng.standard_normal(v.shape))).astype(np.float32)
            changed += int((mas_oracle.maximum_path_lengths(p, tt, ts) != path).any())
        out[eps] = changed
    return out

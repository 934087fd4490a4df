"""Test-side oracle of voice conversion: the forward coupling and flow
restated on the helpers of oracle/vits_oracle.py (which holds the reverse
direction only), the linear spectrogram restated from mel_processing.py:58-77,
and the composition the golden fixture base_vc.npz pins
(tests/golden/make_golden_vc.py writes it from the reference's own modules).

Forward direction = ResidualCouplingBlock.forward(x, mask, g, reverse=False)
(models.py:219-222): coupling i (modules.py:341-356, mean-only: x1 <- m(x0; g)
+ x1 * mask), then Flip.  The reference's ``flow.infer(z, g, reverse=False)``
is NOT this: ResidualCouplingLayer.infer ignores ``reverse`` and subtracts."""
import torch
import torch.nn.functional as F

from oracle import vits_oracle as V

from common import BASE_MODEL

# data section of configs/base.json that voice conversion needs
STFT = dict(n_fft=1024, hop=192, win=768)
PAD = (STFT["n_fft"] - STFT["hop"]) // 2
# the fixture's shape: L = 24 frames and a ragged tail, speaker 7 -> 1500
GOLDEN_L = 24 * 192 + 57
GOLDEN_SIDS = (7, 1500)


def coupling_forward(sd, pre, x, x_mask, g, n_layers, H):
    """ResidualCouplingLayer.forward, reverse=False (modules.py:341-356), mean-only."""
    half = x.shape[1] // 2
    x0, x1 = x[:, :half], x[:, half:]
    h = V.conv1d(sd, pre + ".pre", x0) * x_mask
    h = V.wn(sd, pre + ".enc", h, x_mask, g, n_layers, H, masked=True)
    m = V.conv1d(sd, pre + ".post", h) * x_mask
    x1 = m + x1 * torch.exp(torch.zeros_like(m)) * x_mask
    return torch.cat([x0, x1], 1)


def flow_forward(sd, z, g, n_flows=4, n_layers=4, H=256, x_mask=None):
    """ResidualCouplingBlock.forward, reverse=False (models.py:219-222)."""
    if x_mask is None:
        x_mask = torch.ones(z.shape[0], 1, z.shape[2], dtype=z.dtype)
    x = z
    for i in range(n_flows):
        x = coupling_forward(sd, f"flow.flows.{2 * i}", x, x_mask, g, n_layers, H)
        x = torch.flip(x, [1])  # Flip (modules.py:278-289)
    return x


def spectrogram(y, n_fft=STFT["n_fft"], hop=STFT["hop"], win=STFT["win"], eps=1e-6):
    """mel_processing.spectrogram_torch (mel_processing.py:58-77): y [B, L] in
    its own precision (float64 for a reference of the kernels)."""
    pad = int((n_fft - hop) / 2)
    window = torch.hann_window(win).to(y.dtype)
    yp = F.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=window, center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    return torch.sqrt(spec.real ** 2 + spec.imag ** 2 + eps)


def stft_mag_ref(x, n_fft, hop, win, pad, eps):
    """float64 magnitude STFT of one fp32 row x [L] with reflect padding
    ``pad`` (the reference of tests/test_stft_edges_gpu.py): [n_fft/2+1, frames]."""
    xd = x.double().view(1, 1, -1)
    xp = F.pad(xd, (pad, pad), mode="reflect").view(1, -1) if pad else xd.view(1, -1)
    spec = torch.stft(xp, n_fft, hop, win, torch.hann_window(win).double(), center=False,
                      return_complex=True)
    return torch.sqrt(spec.real ** 2 + spec.imag ** 2 + eps)[0]


def vc_oracle(sd, spec, noise, sid_src, sid_tgt, cfg=BASE_MODEL):
    """posterior_infer -> flow_forward(g_src) -> flow_reverse(g_tgt) ->
    generator(g_tgt) on a state dict: (z, z_p, z_hat, o)."""
    H = cfg["hidden_channels"]
    g_src = sd["emb_g.weight"][torch.as_tensor(sid_src).long()]
    g_tgt = sd["emb_g.weight"][torch.as_tensor(sid_tgt).long()]
    z = V.posterior_infer(sd, spec, noise, cfg["n_layers_q"], H)
    z_p = flow_forward(sd, z, g_src, cfg.get("n_flows", 4), 4, H)
    z_hat = V.flow_reverse(sd, z_p, g_tgt, cfg.get("n_flows", 4), 4, H)
    o = V.generator(sd, z_hat, g_tgt, cfg)
    return z, z_p, z_hat, o

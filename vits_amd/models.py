"""VITS synthesizer (reference ``models.py``), MI355X-native inference path.

Constructor signatures, attribute names and state_dict keys match the
reference (``models.py:20-575``), so checkpoints, ``train*.py``-style drivers,
``export.load_model`` and ``EmoVITS`` consume this module unchanged.

Execution:
* ``infer`` / ``infer_p1`` / ``infer_p2`` / ``inference`` and any no-grad
  ``Generator`` call run on libvits_amd kernels (``vits_amd.engine``); they
  require a ROCm GPU and raise otherwise (no CPU fallback).
* ``forward`` (training) runs PyTorch-ROCm ops under autograd; its
  monotonic-alignment search is the HIP ``maximum_path`` kernel
  (models.py:498 call contract).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn
from torch.nn import Conv1d, ConvTranspose1d
from torch.nn import functional as F
from torch.nn.utils import remove_weight_norm, weight_norm

from . import attentions, commons, engine, modules, train_ops
from .commons import gen_sin_table, get_padding, init_weights
from .monotonic_align import maximum_path
from .ops import neg_cent as neg_cent_scores


def _needs_grad(module: nn.Module, *tensors) -> bool:
    if not torch.is_grad_enabled():
        return False
    if any(t is not None and t.requires_grad for t in tensors):
        return True
    return any(p.requires_grad for p in module.parameters())


class DurationPredictor(nn.Module):
    """L1-log duration predictor with speaker conditioning (models.py:20-67)."""

    def __init__(self, in_channels, filter_channels, kernel_size=5, p_dropout=0.25, act_func="ReLU",
                 act_func_params={}, gin_channels=0):
        super().__init__()
        self.in_channels = in_channels
        self.filter_channels = filter_channels
        self.kernel_size = kernel_size
        self.p_dropout = p_dropout
        self.gin_channels = gin_channels
        self.drop = nn.Dropout(p_dropout)
        self.pre = nn.Conv1d(in_channels, filter_channels, 1)
        self.conv_1 = nn.Conv1d(filter_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm_1 = modules.LayerNorm(filter_channels)
        self.conv_2 = nn.Conv1d(filter_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm_2 = modules.LayerNorm(filter_channels)
        self.proj = nn.Conv1d(filter_channels, 1, 1)
        self.cond1 = nn.Linear(gin_channels, filter_channels)
        self.cond2 = nn.Linear(gin_channels, filter_channels)
        if act_func.lower() == "swish":
            raise NotImplementedError("act_func_d='swish' is not selected by configs/base.json")
        self.act_1 = getattr(nn, act_func)(**act_func_params)
        self.act_2 = getattr(nn, act_func)(**act_func_params)

    def forward(self, x, x_mask, g):
        x, g = torch.detach(x), torch.detach(g)
        conv = train_ops.conv1d  # HIP under autocast on the GPU, torch otherwise
        x = conv(self.pre, x) + self.cond1(g).unsqueeze(-1)
        x = conv(self.conv_1, x * x_mask)
        x = self.drop(self.norm_1(self.act_1(x)))
        x = x + self.cond2(g).unsqueeze(-1)
        x = conv(self.conv_2, x * x_mask)
        x = self.drop(self.norm_2(self.act_2(x)))
        x = conv(self.proj, x * x_mask)
        return x * x_mask

    @torch.no_grad()
    def infer(self, x, g):
        engine._check_gpu(x, "DurationPredictor.infer")
        plan = engine.get_plan(self, engine.DurationPlan)
        return plan.run(engine._f32(x), g).to(x.dtype)


class TextEncoder(nn.Module):
    """Linear+LN text-vector embedding, emotion projection, scaled sinusoid
    positions, post-LN transformer, 1x1 projection (models.py:103-189)."""

    def __init__(self, in_channels, out_channels, hidden_channels, filter_channels, n_heads, n_layers,
                 kernel_size, p_dropout, ffn="FFN2", gin_channels=0):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.hidden_channels = hidden_channels
        self.filter_channels = filter_channels
        self.n_heads = n_heads
        self.n_layers = n_layers
        self.kernel_size = kernel_size
        self.p_dropout = p_dropout
        self.emb = nn.Sequential(nn.Linear(in_channels, hidden_channels), nn.LayerNorm(hidden_channels))
        self.emo_proj = nn.Linear(1024, hidden_channels)
        self.register_buffer("sin_table", gen_sin_table(256 + 128, hidden_channels), persistent=False)
        self.xscale = math.sqrt(hidden_channels)
        self.alpha = nn.Parameter(torch.tensor(1.0))
        self.encoder = attentions.Encoder(hidden_channels, filter_channels, n_heads, n_layers,
                                          kernel_size, p_dropout, ffn=ffn, gin_channels=gin_channels)
        self.proj = nn.Conv1d(hidden_channels, out_channels * 2, 1)
        nn.init.xavier_uniform_(self.emo_proj.weight)
        nn.init.xavier_uniform_(self.proj.weight)

    def positional_encoding(self, x, alpha):
        T, max_len = x.size(1), self.sin_table.size(1)
        assert not self.training or T < max_len, f"The input T={T} > max_len{max_len}, pls resolve it!"
        pe = self.sin_table[:, :T] if T <= max_len else gen_sin_table(T, x.size(2)).to(x.device)
        return x * self.xscale + pe * alpha

    def forward(self, x, x_lengths, emo, g):
        x = self.emb(x) + self.emo_proj(emo).unsqueeze(1)
        x = self.positional_encoding(x, self.alpha).transpose(1, -1)
        x_mask = torch.unsqueeze(commons.sequence_mask(x_lengths, x.size(2)), 1).to(x.dtype)
        x = self.encoder(x * x_mask, x_mask, g=g)
        stats = train_ops.conv1d(self.proj, x) * x_mask
        m, logs = torch.split(stats, self.out_channels, dim=1)
        return x, m, logs, x_mask

    @torch.no_grad()
    def infer(self, x, emo, g):
        engine._check_gpu(x, "TextEncoder.infer")
        plan = engine.get_plan(self, engine.TextEncoderPlan)
        h, m, logs = plan.run(x, emo, g)
        return h.to(x.dtype), m.to(x.dtype), logs.to(x.dtype)

    @torch.no_grad()
    def forward_masked_hip(self, x, x_lengths, emo, g, exp_logs=False, pad_exact=False):
        """Masked TextEncoder.forward on the HIP path (used by ``inference``);
        pad_exact: TextEncoder.infer of each unpadded utterance instead
        (engine.TextEncoderPlan.run)."""
        plan = engine.get_plan(self, engine.TextEncoderPlan)
        lengths = x_lengths.to(device=x.device, dtype=torch.int32).contiguous()
        return plan.run(x, emo, g, lengths=lengths, exp_logs=exp_logs, pad_exact=pad_exact)


class ResidualCouplingBlock(nn.Module):
    """4 mean-only couplings with channel flips (models.py:192-235)."""

    def __init__(self, channels, hidden_channels, kernel_size, dilation_rate, n_layers, n_flows=4,
                 gin_channels=0):
        super().__init__()
        assert len(dilation_rate) == n_flows
        self.channels = channels
        self.hidden_channels = hidden_channels
        self.kernel_size = kernel_size
        self.dilation_rate = dilation_rate
        self.n_layers = n_layers
        self.n_flows = n_flows
        self.gin_channels = gin_channels
        self.flows = nn.ModuleList()
        for i in range(n_flows):
            self.flows.append(modules.ResidualCouplingLayer(
                channels, hidden_channels, kernel_size, dilation_rate[i], n_layers,
                gin_channels=gin_channels, mean_only=True))
            self.flows.append(modules.Flip())

    @property
    def flows_reversed(self):
        return list(self.flows)[::-1]

    def forward(self, x, x_mask, g=None, reverse=False):
        flows = list(self.flows) if not reverse else list(self.flows)[::-1]
        i = 0
        while i < len(flows):
            f = flows[i]
            # a coupling followed by a Flip: the flip folded into the coupling
            flip = (isinstance(f, modules.ResidualCouplingLayer) and i + 1 < len(flows)
                    and isinstance(flows[i + 1], modules.Flip))
            kw = dict(flip=True) if flip else {}
            if not reverse:
                x, _ = f(x, x_mask, g=g, reverse=reverse, **kw)
            else:
                x = f(x, x_mask, g=g, reverse=reverse, **kw)
            i += 2 if flip else 1
        return x

    @torch.no_grad()
    def infer(self, x, g, reverse=True):
        """The flow without a mask on the HIP plan.  reverse=True: generation
        (models.py:228-235).  reverse=False: the forward flow as training
        runs it, ``forward(x, ones, g, reverse=False)``: each mean-only
        coupling adds its mean, x1 <- x1 + m(x0; g), then Flip - the exact
        inverse of reverse=True.  This is NOT what the reference's
        ``flow.infer(z, g, reverse=False)`` computes: its
        ResidualCouplingLayer.infer (modules.py:362-375) ignores ``reverse``
        and always subtracts, so that call is no forward flow (a round trip
        through it is off by 47 % at the base config)."""
        return engine.flow_infer(self, x, g, reverse=bool(reverse))


class PosteriorEncoder(nn.Module):
    """Linear-spectrogram encoder q(z|x) (models.py:238-279)."""

    def __init__(self, in_channels, out_channels, hidden_channels, kernel_size, dilation_rate,
                 n_layers, gin_channels=0):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.hidden_channels = hidden_channels
        self.kernel_size = kernel_size
        self.dilation_rate = dilation_rate
        self.n_layers = n_layers
        self.gin_channels = gin_channels
        self.pre = nn.Sequential(nn.Conv1d(in_channels, hidden_channels, 1),
                                 modules.LayerNorm(hidden_channels))
        self.enc = modules.WN(hidden_channels, kernel_size, dilation_rate, n_layers,
                              gin_channels=gin_channels)
        self.proj = nn.Conv1d(hidden_channels, out_channels * 2, 1)

    def forward(self, x, x_lengths, g=None, noise=None):
        x_mask = torch.unsqueeze(commons.sequence_mask(x_lengths, x.size(2)), 1).to(x.dtype)
        x = self.pre[1](train_ops.conv1d(self.pre[0], x)) * x_mask
        x = self.enc(x, x_mask, g=g)
        stats = train_ops.conv1d(self.proj, x) * x_mask
        m, logs = torch.split(stats, self.out_channels, dim=1)
        if noise is None:
            noise = torch.randn_like(m)
        z = (m + noise * torch.exp(logs)) * x_mask
        return z, m, logs, x_mask

    @torch.no_grad()
    def infer(self, x, n, g=None):
        engine._check_gpu(x, "PosteriorEncoder.infer")
        plan = engine.get_plan(self, engine.PosteriorPlan)
        return plan.run(x, n, g).to(x.dtype)


class Generator(nn.Module):
    """HiFi-GAN-style decoder with gated, speaker-conditioned ResBlock2
    (models.py:282-318).  Without autograd it runs the fused HIP plan (ROCm
    only); with autograd it runs PyTorch-ROCm ops (training)."""

    def __init__(self, initial_channel, resblock, resblock_kernel_sizes, resblock_dilation_sizes,
                 upsample_rates, upsample_initial_channel, upsample_kernel_sizes, gin_channels=0):
        super().__init__()
        if str(resblock) != "2":
            raise NotImplementedError("only resblock='2' (configs/base.json) is on the hot path")
        self.num_kernels = len(resblock_kernel_sizes)
        self.num_upsamples = len(upsample_rates)
        self.conv_pre = Conv1d(initial_channel, upsample_initial_channel, 7, 1, padding=3)
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            self.ups.append(weight_norm(ConvTranspose1d(
                upsample_initial_channel // (2 ** i), upsample_initial_channel // (2 ** (i + 1)),
                k, u, padding=(k - u) // 2)))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            ch = upsample_initial_channel // (2 ** (i + 1))
            for k, d in zip(resblock_kernel_sizes, resblock_dilation_sizes):
                self.resblocks.append(modules.ResBlock2(ch, k, d, gin_channels))
        self.conv_post = Conv1d(ch, 1, 7, 1, padding=3, bias=False)
        self.ups.apply(init_weights)

    def forward(self, x, g):
        if not _needs_grad(self, x, g):
            # inference: HIP plan only (raises off-GPU; there is no CPU path)
            return engine.generator_forward(self, x, g)
        x = train_ops.conv1d(self.conv_pre, x)
        conds, y16, y32 = self._resblock_conds(g)
        col0 = 0
        for i in range(self.num_upsamples):
            # polyphase on the HIP training conv under autocast (torch otherwise)
            x = train_ops.conv_transpose1d(self.ups[i], x, in_slope=modules.LRELU_SLOPE)
            rbs = self.resblocks[i * self.num_kernels:(i + 1) * self.num_kernels]
            # the stage's branches as grouped launches (fp16 autocast on the GPU)
            xs = train_ops.resblock_stage(x, rbs, y16, y32, col0)
            if xs is None:
                xs = 0
                for j in range(self.num_kernels):
                    rb = i * self.num_kernels + j
                    xs = xs + self.resblocks[rb](x, g=g, conds=None if conds is None else conds[rb])
                xs = xs / self.num_kernels
            x = xs
            col0 += sum(cs.out_features for rb in rbs for cs in rb.conds)
        x = train_ops.conv1d(self.conv_post, x, in_slope=0.01)  # F.leaky_relu default slope
        return torch.tanh(x)

    def _resblock_conds(self, g):
        """Every ResBlock2 conditioning Linear (modules.py:250-255: one per
        dilation pair, 36 at the base config, all applied to the same g) as
        ONE GEMM over the concatenated weights, split back per resblock:
        the same products, one launch instead of 36 (each with its own
        autocast casts and backward GEMMs).  Returns (per-resblock conds,
        the GEMM's output y, its fp32 copy y32 or None), or (None, None,
        None) without a speaker vector."""
        if g is None or not g.is_cuda:
            return None, None, None
        mods = [cs for rb in self.resblocks for cs in rb.conds]
        if not all(isinstance(m, nn.Linear) and m.bias is not None for m in mods):
            return None, None, None
        ws = [train_ops.module_weight(m) for m in mods]
        y = F.linear(g, torch.cat(ws, 0), torch.cat([m.bias for m in mods]))
        sizes = [w.shape[0] for w in ws]
        parts = torch.split(y, sizes, dim=1)
        y32 = train_ops.cond_f32(y)  # one cast for every pair's fused gate
        if y32 is not None:
            parts = list(zip(parts, torch.split(y32, sizes, dim=1)))
        k = len(self.resblocks[0].conds)
        return [parts[i * k:(i + 1) * k] for i in range(len(self.resblocks))], y, y32

    def infer(self, x, g):
        return self.forward(x, g)

    def context_frames(self):
        """Input frames on each side of frame f that its hop output samples
        can depend on, from the modules' own kernels, dilations, strides and
        paddings, exactly and in integers: the interval of samples [0, hop)
        is taken backwards through conv_post, every stage's longest ResBlock2
        branch (per pair c1, dilated, and c2), every transposed conv (output
        t reads the inputs i with 0 <= t + p - i * u < k) and conv_pre."""
        def reach(conv):
            return (conv.kernel_size[0] - 1) // 2 * conv.dilation[0]

        hop = 1
        for up in self.ups:
            hop *= up.stride[0]
        lo, hi = -reach(self.conv_post), hop - 1 + reach(self.conv_post)
        for i in reversed(range(self.num_upsamples)):
            rbs = self.resblocks[i * self.num_kernels:(i + 1) * self.num_kernels]
            r = max(sum(reach(c1) + reach(c2) for c1, c2 in zip(rb.convs1, rb.convs2))
                    for rb in rbs)
            up = self.ups[i]
            k, u, p = up.kernel_size[0], up.stride[0], up.padding[0]
            lo, hi = -((k - 1 - p - (lo - r)) // u), (hi + r + p) // u  # (ceil, floor)
        lo, hi = lo - reach(self.conv_pre), hi + reach(self.conv_pre)
        return max(-lo, hi, 0)


def _control_buffers(static, batch, t_x, dev):
    """The static control buffers of a captured infer_bucketed(control=...),
    neutral (every token free, scale 1, no target); returns the control dict
    of views the capture hands to infer_bucketed."""
    static["given"] = torch.full((batch, t_x), -1, device=dev, dtype=torch.int32)
    static["tok_scale"] = torch.ones(batch, t_x, device=dev, dtype=torch.float32)
    static["target"] = torch.zeros(batch, device=dev, dtype=torch.int32)
    static["ctl_neutral"] = True
    return {k: static[k] for k in ("given", "tok_scale", "target")}


def _control_fill(static, rows, batch, t_x):
    """Write one replay's controls into the static buffers with one upload
    each: ``rows`` = per row None or dict(given=, tok_scale=, target=) whose
    entries may be None; tokens past a row's values and rows past ``rows``
    stay neutral (-1 / 1.0 / 0).  A device tensor as ``given`` is copied
    device to device (no host visit)."""
    if not any(v is not None for row in rows for v in (row or {}).values()):
        # no control in this replay: nothing is uploaded; buffers that still
        # hold an earlier replay's controls are reset on the device
        if not static["ctl_neutral"]:
            static["given"].fill_(-1)
            static["tok_scale"].fill_(1.0)
            static["target"].zero_()
            static["ctl_neutral"] = True
        return
    static["ctl_neutral"] = False
    given = torch.full((batch, t_x), -1, dtype=torch.int32)
    scale = torch.ones(batch, t_x, dtype=torch.float32)
    target = torch.zeros(batch, dtype=torch.int32)
    late = []
    for i, row in enumerate(rows):
        row = row or {}
        unknown = set(row) - {"given", "tok_scale", "target"}
        if unknown:
            raise ValueError(f"replay: unknown control(s) {sorted(unknown)}")
        g, sc, tg = row.get("given"), row.get("tok_scale"), row.get("target")
        for name, v in (("given", g), ("tok_scale", sc)):
            if v is not None and len(v) > t_x:
                raise ValueError(f"replay: {len(v)} values of {name} do not fit {t_x} tokens")
        if isinstance(g, torch.Tensor) and g.is_cuda:
            late.append((i, g))
        elif g is not None:
            given[i, :len(g)] = torch.as_tensor(g, dtype=torch.int32)
        if sc is not None:
            scale[i, :len(sc)] = torch.as_tensor(sc, dtype=torch.float32).cpu()
        if tg is not None:
            target[i] = int(tg)
    static["given"].copy_(given)
    static["tok_scale"].copy_(scale)
    static["target"].copy_(target)
    for i, g in late:
        static["given"][i, :g.numel()].copy_(g.reshape(-1).to(torch.int32))


def _fill_rows(buf, src, n, w=None):
    """One replay input: zero the static buffer, then copy ``src`` (n rows)
    into its first n rows (``w``: into their first w columns)."""
    buf.zero_()
    (buf[:n] if w is None else buf[:n, :w]).copy_(src)


class SynthesizerTrn(nn.Module):
    """Synthesizer for training and inference (models.py:411-575)."""

    def __init__(self, text_channels, spec_channels, segment_size, inter_channels, hidden_channels,
                 filter_channels, n_heads, n_layers, kernel_size, p_dropout,
                 resblock_kernel_sizes=None, resblock_dilation_sizes=None, upsample_rates=None,
                 upsample_initial_channel=None, upsample_kernel_sizes=None, resblock="2",
                 ffn="FFN2", kernel_size_q=5, n_layers_q=16, hidden_size_d=256, kernel_size_d=5,
                 p_dropout_d=0.5, act_func_d="ReLU", act_func_params_d={}, dilation_rate=[1, 1, 1, 1],
                 n_flows=4, n_speakers=0, gin_channels=0, align_noise=0.01, align_noise_decay=1e-6,
                 align_noise_min=0, **kwargs):
        super().__init__()
        assert len(dilation_rate) == n_flows
        assert n_speakers > 1
        self.segment_size = segment_size
        self.text_channels = text_channels
        self.inter_channels = inter_channels
        self.align_noise = align_noise
        self.align_noise_decay = align_noise_decay
        self.align_noise_min = align_noise_min
        self.dec = Generator(inter_channels, resblock, resblock_kernel_sizes, resblock_dilation_sizes,
                             upsample_rates, upsample_initial_channel, upsample_kernel_sizes,
                             gin_channels=gin_channels)
        self.enc_p = TextEncoder(text_channels, inter_channels, hidden_channels, filter_channels,
                                 n_heads, n_layers, kernel_size, p_dropout, ffn=ffn,
                                 gin_channels=gin_channels)
        self.enc_q = PosteriorEncoder(spec_channels, inter_channels, hidden_channels, kernel_size_q,
                                      1, n_layers_q, gin_channels=0)
        self.flow = ResidualCouplingBlock(inter_channels, hidden_channels, 5,
                                          dilation_rate=dilation_rate, n_layers=4, n_flows=n_flows,
                                          gin_channels=gin_channels)
        self.dp = DurationPredictor(hidden_channels, hidden_size_d, kernel_size_d,
                                    p_dropout=p_dropout_d, act_func=act_func_d,
                                    act_func_params=act_func_params_d, gin_channels=gin_channels)
        self.emb_g = nn.Embedding(n_speakers, gin_channels)
        self.hop_total = 1
        for u in upsample_rates:
            self.hop_total *= u
        self._graphs = {}

    # ------------------------------------------------------------------ utils
    def remove_weight_norm(self):
        """Fold weight norm into plain weights (models.py:467-474)."""
        def _remove(m):
            try:
                remove_weight_norm(m)
            except ValueError:
                return
        self.apply(_remove)
        engine.drop_plans(self)
        self._graphs.clear()

    def _apply(self, fn, *args, **kwargs):
        self._graphs = {}
        out = super()._apply(fn, *args, **kwargs)
        engine.drop_plans(self)
        return out

    # --------------------------------------------------------------- training
    def forward(self, x, x_lengths, y, y_lengths, emo, sid=None, noise_q=None, noise_align=None,
                noise_flow=None):
        """Training forward (models.py:476-515).  The optional noise tensors
        replace the three in-graph randn draws (posterior sample, alignment
        noise, reverse-flow sample) for reproducible parity runs."""
        g = self.emb_g(sid)
        x, m_p, logs_p, x_mask = self.enc_p(x, x_lengths, emo, g=g)
        z, m_q, logs_q, y_mask = self.enc_q(y, y_lengths, g=None, noise=noise_q)
        z_p = self.flow(z, y_mask, g=g)

        with torch.no_grad():
            # one fp32 MFMA kernel for the exp / 2 matmuls / 2 sums of
            # models.py:484-489 (vits_neg_cent)
            neg_cent = neg_cent_scores(z_p, m_p, logs_p)
            if self.align_noise > 0:
                eps = noise_align if noise_align is not None else torch.randn_like(neg_cent)
                an = self.__dict__.get("_align_noise_t")
                if an is not None:
                    # graph-captured step: the decaying scale lives on the device
                    # and decays inside the graph (one step per replay)
                    neg_cent = neg_cent + torch.std(neg_cent) * eps * an
                    an.sub_(self.align_noise_decay).clamp_(min=self.align_noise_min)
                else:
                    neg_cent = neg_cent + torch.std(neg_cent) * eps * self.align_noise
                self.align_noise -= self.align_noise_decay
                self.align_noise = max(self.align_noise, self.align_noise_min)
            attn_mask = torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1)
            attn = maximum_path(neg_cent, attn_mask.squeeze(1)).detach()

        w = attn.sum(1, keepdim=True)
        logw_ = torch.log(w + 1e-6) * x_mask
        logw = self.dp(x, x_mask, g=g)
        l_length = torch.sum(torch.abs(logw - logw_), [1, 2]) / torch.sum(x_mask)

        m_p = torch.matmul(attn, m_p.transpose(1, 2)).transpose(1, 2)
        logs_p = torch.matmul(attn, logs_p.transpose(1, 2)).transpose(1, 2)

        z_slice, ids_slice = commons.rand_slice_segments(
            z, y_lengths, self.segment_size,
            device_rng=self.__dict__.get("_device_slice_rng", False))
        o = self.dec(z_slice, g=g)

        if noise_flow is None:
            noise_flow = torch.randn_like(m_p)
        z_q = self.flow(m_p + noise_flow * torch.exp(logs_p), y_mask, g=g, reverse=True)
        return (o, l_length, attn, ids_slice, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q),
                z_q, (x, logw_.detach(), logw))

    # -------------------------------------------------------------- inference
    @torch.no_grad()
    def inference(self, x, x_lengths, emo, sid=None, noise_scale=1, length_scale=1, max_len=None,
                  noise=None):
        """Batched, masked inference (models.py:517-535) on the HIP path.
        ``noise`` (optional, [B, C, T_y] ~ N(0,1)) replaces randn_like(m_p)."""
        engine._check_gpu(x, "SynthesizerTrn.inference")
        g = self.emb_g(sid)
        h, m_p, logs_p = self.enc_p.forward_masked_hip(x, x_lengths, emo, g)
        lengths = x_lengths.to(device=x.device, dtype=torch.int32).contiguous()
        logw = engine.get_plan(self.dp, engine.DurationPlan).run(h, g, lengths=lengths)
        x_mask = torch.unsqueeze(commons.sequence_mask(x_lengths, h.size(2)), 1).to(torch.float32)
        # duration -> path: host-visible lengths (the reference syncs here too)
        w = torch.exp(logw) * x_mask * length_scale
        w_ceil = torch.ceil(w)
        y_lengths = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
        y_mask = torch.unsqueeze(commons.sequence_mask(y_lengths, None), 1).to(x_mask.dtype)
        attn_mask = torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1)
        attn = commons.generate_path(w_ceil, attn_mask.squeeze(1))
        if noise is None:
            noise = torch.randn(m_p.shape[0], m_p.shape[1], attn.shape[1], device=x.device)
        z_p = engine.ops.expand_prior(attn, m_p, logs_p, noise, exp_s=True,
                                      noise_scale=float(noise_scale))
        ylen32 = y_lengths.to(torch.int32).contiguous()
        z = engine.flow_reverse_masked(self.flow, z_p, ylen32, g)
        zm = z * y_mask
        o = self.dec(zm[:, :, :max_len].contiguous(), g=g)
        # returned expansions follow the reference: attn @ m_p / attn @ logs_p
        m_e = torch.matmul(attn, m_p.transpose(1, 2)).transpose(1, 2)
        logs_e = torch.matmul(attn, logs_p.transpose(1, 2)).transpose(1, 2)
        return o.to(x.dtype), attn, y_mask, (z, z_p, m_e, logs_e)

    @torch.no_grad()
    def infer(self, x, emo, sid, noise_scale=0.707, length_scale=1.0, noise=None):
        """Single-utterance inference (models.py:537-556)."""
        assert x.size(0) == 1
        m_p, s_p, logw, g = self.infer_p1(x, emo, sid)
        w = torch.exp(logw) * length_scale
        w_ceil = torch.ceil(w)
        y_len = int(torch.clamp_min(torch.sum(w_ceil), 1).item())
        attn = commons.infer_path(w_ceil, x.size(1), y_len, dtype=torch.float32)
        if noise is None:
            noise = torch.randn(1, m_p.shape[1], y_len, device=x.device)
        # reference: z_p = m + randn * exp(logs) * noise_scale with exp taken after
        # the (one-hot) expansion; infer_p1 already returns s = exp(logs)
        return self.infer_p2(attn, m_p, s_p, g, noise * noise_scale)

    @torch.no_grad()
    def infer_durations(self, x, emo, sid, durations, noise):
        """``infer`` with the durations given instead of predicted: infer_p1,
        commons.infer_path(durations), infer_p2, the way the reference's
        infer_p2(attn, ...) is driven with a hand-made path.  B = 1, exact
        lengths, eager.  ``durations``: [t_x] (or [1, 1, t_x]) frames per
        token, integers >= 0 (a token of 0 frames gets none); ``noise`` [1, C,
        y_len], y_len = max(sum(durations), 1), pre-scaled like infer_p2's.
        This is the definition infer_bucketed(control=...) is held to, bit for
        bit."""
        assert x.size(0) == 1
        m_p, s_p, _, g = self.infer_p1(x, emo, sid)
        d = torch.as_tensor(durations, device=x.device).reshape(1, 1, -1).to(torch.float32)
        if d.shape[-1] != x.size(1) or bool((d < 0).any()):
            raise ValueError(f"infer_durations: need {x.size(1)} durations >= 0, got "
                             f"{tuple(d.shape)}")
        y_len = max(int(d.sum().item()), 1)
        attn = commons.infer_path(d, x.size(1), y_len, dtype=torch.float32)
        return self.infer_p2(attn, m_p, s_p, g, noise)

    @torch.no_grad()
    def infer_p1(self, x, emo, sid):
        """Text side (models.py:558-566): returns m_p, s_p = exp(logs_p), logw, g."""
        assert x.size(0) == 1
        engine._check_gpu(x, "SynthesizerTrn.infer_p1")
        g = self.emb_g(sid)
        plan = engine.get_plan(self.enc_p, engine.TextEncoderPlan)
        h, m_p, s_p = plan.run(x, emo, g, exp_logs=True)
        logw = engine.get_plan(self.dp, engine.DurationPlan).run(h, g)
        dt = x.dtype
        return m_p.to(dt), s_p.to(dt), logw.to(dt), g

    @torch.no_grad()
    def infer_p2(self, attn, m_p, s_p, g, noise):
        """Acoustic side (models.py:568-575): prior expansion + noise, reverse
        flow, decoder — all libvits_amd kernels."""
        z = self.infer_p2_front(attn, m_p, s_p, g, noise)
        gplan = engine.get_plan(self.dec, engine.GeneratorPlan)
        o = gplan.run(z, engine._f32(g))
        return o.to(m_p.dtype)

    @torch.no_grad()
    def infer_p2_front(self, attn, m_p, s_p, g, noise):
        """infer_p2 up to and including the reverse flow: z fp32 [B, C, t_y],
        the decoder's input."""
        engine._check_gpu(m_p, "SynthesizerTrn.infer_p2")
        z = engine.ops.expand_prior(attn, m_p, s_p, noise)
        engine.get_plan(self.flow, engine.CouplingFlowPlan).run_(z, engine._f32(g))
        return z

    # stage multipliers of the lengths the bucketed infer hands to the flow,
    # conv_pre and the upsample stages (frames -> samples after each ups)
    def _stage_mult(self):
        mult, u = [1, 1], 1
        for up in self.dec.ups:
            u *= up.stride[0]
            mult.append(u)
        return tuple(mult)

    @torch.no_grad()
    def infer_bucketed(self, x, emo, sid, noise, t_y, *, x_lengths=None, length_scale=1.0,
                       noise_start=None, n_rows=None, control=None):
        """infer (models.py:537-556) / EmoVITS.infer (infer.py:160-182) with
        NO host synchronisation, over a static bucket of t_y frames - the
        whole utterance can be captured into one hipGraph
        (capture_infer_bucketed).  The durations, y_len and the path are
        computed on the device (ops.expand_durations: the exp / ceil / sum /
        .item() / infer_path / expansion of models.py:544-553); the reverse
        flow and the decoder run masked at y_len (every conv output is zero
        past it, i.e. the zero padding the reference's decoder sees at the
        utterance end) and tiles past y_len + 64 are skipped
        (ops.length_skip), so the work follows y_len, not t_y.

        ``noise``: pre-scaled like infer_p2's (z = m + noise * s): [B, C,
        t_y], or a flat buffer sliced as EmoVITS slices it at
        np.random.randint(numel - C * y_len), drawn on the device from
        ``noise_start`` = int32 [B, ops.ED_DRAWS] raw MT19937 words
        (ops.numpy_draw_pool); the returned y_len is then int32 [2, B]:
        (y_len, generator words consumed; -1 when the slice does not
        fit, -2 when every word of the pool was rejected: the caller
        advances numpy's generator past the pool and runs again).  ``x_lengths`` (int32 [B]): padded text, encoded
        as TextEncoder.infer of each unpadded utterance (every layer masked,
        engine.TextEncoderPlan pad_exact); None: the exact-length infer_p1
        path (B = 1).  Returns (wav [B, 1, t_y * hop], y_len int32 [B]);
        samples past y_len * hop are not meaningful (crop on the host).

        Shared-pool form (a batch that must draw as B consecutive EmoVITS
        calls would): ``noise_start`` = int32 [P] raw words and ``n_rows``
        (int or int32 [1] device tensor: rows at or past it are the padding
        of a batch bucket and draw nothing).  ops.draw_starts draws every
        row's start in row order from the one pool, the expansion reads them
        (vits_expand_durations mode 2).  Returns (wav, y_len [B], status
        [B], used_total [1]) as ops.draw_starts defines them.

        ``length_scale``: a number, or a contiguous fp32 [B] device tensor
        of per-row speeds read on the device (ops.expand_durations'
        ``rate``): row b is then what the call with float(length_scale[b])
        computes, and a captured graph serves every mix of speeds.

        ``control`` = dict(given=, tok_scale=, target=) of device tensors
        (int32 [B, t_x], fp32 [B, t_x], int32 [B]; each may be None or left
        out): the durations come from ops.duration_plan (pinned tokens,
        per-token scales, a total to fit; ``length_scale`` is its rate) and the
        start draw and the expansion read them (their ``durations=`` forms).
        The call then additionally returns (dur int32 [B, t_x], plan_meta
        int32 [2, B] = total | status) as its last two values; each row is bit
        for bit infer_durations of its returned durations.  None: nothing
        changes and no further kernel is launched."""
        z, g, dt, lens, draw, plan = self._front(
            "infer_bucketed", x, emo, sid, noise, t_y, x_lengths, length_scale, noise_start,
            n_rows, control)
        with engine.ops.length_skip(64):
            o = engine.get_plan(self.dec, engine.GeneratorPlan).run(z, engine._f32(g),
                                                                    lengths=lens[1:])
        return (o.to(dt),) + draw + plan

    @torch.no_grad()
    def infer_front_bucketed(self, x, emo, sid, noise, t_y, *, x_lengths=None, length_scale=1.0,
                             noise_start=None, n_rows=None, control=None):
        """infer_bucketed up to and including the reverse flow (the text
        side of a streamed utterance): the same arguments, the
        same kernels in the same order, no decoder.  Returns (z fp32 [B, C,
        t_y], the decoder's input, masked at y_len; g [B, gin] in the model's
        dtype) followed by what infer_bucketed returns after its waveform:
        y_len (int32 [B], or [2, B] with the draw status under
        ``noise_start``; y_len, status, used_total in the shared-pool form)
        and, with ``control``, (dur, plan_meta).  decode_window_bucketed
        over windows of z gives the samples infer_bucketed gives."""
        z, g, _, _, draw, plan = self._front(
            "infer_front_bucketed", x, emo, sid, noise, t_y, x_lengths, length_scale, noise_start,
            n_rows, control)
        return (z, g) + draw + plan

    def _front(self, what, x, emo, sid, noise, t_y, x_lengths, length_scale, noise_start, n_rows,
               control):
        """The text side of infer_bucketed (documented there): text encoder,
        durations, draw, prior expansion, reverse flow.  Returns (z, g, the
        model's dtype, stage lengths int32 [n, B], the length / draw results
        as a tuple, the duration plan's as a tuple)."""
        engine._check_gpu(x, "SynthesizerTrn." + what)
        rate = length_scale if isinstance(length_scale, torch.Tensor) else float(length_scale)
        dt = x.dtype
        shared_pool = noise_start is not None and noise_start.dim() == 1
        if shared_pool and n_rows is None:
            n_rows = x.shape[0]
        if x_lengths is None:
            m_p, s_p, logw, g = self.infer_p1(x, emo, sid)
            xl = None
        else:
            g = self.emb_g(sid)
            xl = x_lengths.to(device=x.device, dtype=torch.int32).contiguous()
            h, m_p, s_p = self.enc_p.forward_masked_hip(x, xl, emo, g, exp_logs=True,
                                                        pad_exact=True)
            logw = engine.get_plan(self.dp, engine.DurationPlan).run(h, g, lengths=xl)
            m_p, s_p, logw = m_p.to(dt), s_p.to(dt), logw.to(dt)
        starts = None
        # how the durations reach the draw and the expansion: the predictor's
        # logw with the speed, or the plan's integers
        src = dict(rate=rate, half_round=dt == torch.float16)
        plan = ()
        if control is not None:
            unknown = set(control) - {"given", "tok_scale", "target"}
            if unknown:
                raise ValueError(f"infer_bucketed: unknown control(s) {sorted(unknown)}")
            plan_meta = torch.empty(2, x.shape[0], device=x.device, dtype=torch.int32)
            dur = engine.ops.duration_plan(
                logw, rate=rate, x_len=xl, half_round=dt == torch.float16,
                given=control.get("given"), tok_scale=control.get("tok_scale"),
                target=control.get("target"), meta=plan_meta)[0]
            src = dict(durations=dur)
            plan = (dur, plan_meta)
        if shared_pool:
            starts, y_len, status, used_total = engine.ops.draw_starts(
                logw, m_p.shape[1], noise.numel(), noise_start, x_len=xl, n_rows=n_rows, **src)
            noise_start = None
        z, lens = engine.ops.expand_durations(
            logw, m_p, s_p, noise, int(t_y), x_len=xl, noise_start=noise_start,
            stage_mult=self._stage_mult(), starts=starts, **src)
        with engine.ops.length_skip(64):
            engine.get_plan(self.flow, engine.CouplingFlowPlan).run_(z, engine._f32(g),
                                                                     lengths=lens[0])
        if shared_pool:
            draw = (y_len, status, used_total)
        elif noise_start is not None:
            draw = (lens[0::len(lens) - 1],)
        else:
            draw = (lens[0],)
        return z, g, m_p.dtype, lens, draw, plan

    @torch.no_grad()
    def decode_window_bucketed(self, z_win, win_len, g):
        """The decoder over one window of a streamed utterance: z_win fp32
        [B, C, W] holds frames [a, a + win_len) of infer_front_bucketed's z,
        zero past win_len (int32 [B] on the device); g as the front returns
        it.  GeneratorPlan.run masked at win_len under ops.length_skip(64),
        as infer_bucketed runs it at y_len: a window that ends at y_len sees
        the utterance's own end, one that starts at frame 0 its own start,
        and a sample Generator.context_frames() frames from any other edge is
        the whole utterance's.  No host sync.  Returns [B, 1, W * hop] in
        g's dtype (the model's, as infer_bucketed's waveform); samples at or
        past win_len * hop are not meaningful."""
        engine._check_gpu(z_win, "SynthesizerTrn.decode_window_bucketed")
        mult = self.__dict__.get("_win_mult")
        if mult is None or mult.device != z_win.device:
            mult = self.__dict__["_win_mult"] = torch.tensor(
                self._stage_mult()[1:], device=z_win.device, dtype=torch.int32).view(-1, 1)
        lens = mult * win_len.view(1, -1)
        with engine.ops.length_skip(64):
            o = engine.get_plan(self.dec, engine.GeneratorPlan).run(z_win, engine._f32(g),
                                                                    lengths=lens)
        return o.to(g.dtype)

    @torch.no_grad()
    def capture_decode_window(self, W, warmup=2):
        """One hipGraph for decode_window_bucketed over a window bucket of W
        frames.  It depends on no text: one graph per W serves every
        utterance.  Returns run(win_len) -> wav [1, 1, W * hop] (a view of a
        static buffer) for a caller that has written ``run.static["z"]`` [1,
        C, W] (ops.copy_windows straight from the front's z, zero-filled to
        W) and ``run.static["g"]`` [1, gin] itself; win_len is a host int."""
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        W = int(W)
        static = dict(z=torch.zeros(1, self.inter_channels, W, device=dev),
                      g=torch.zeros(1, self.emb_g.embedding_dim, device=dev, dtype=dt),
                      n=torch.full((1,), W, device=dev, dtype=torch.int32))
        self.decode_window_bucketed(static["z"], static["n"], static["g"])  # (builds the plan)

        def body():
            return self.decode_window_bucketed(static["z"], static["n"], static["g"])

        graph, out = self._capture_body(body, warmup, dev)

        def run(win_len):
            if not 1 <= int(win_len) <= W:
                raise ValueError(f"decode replay: {win_len} frames do not fit a window of {W}")
            static["n"].fill_(int(win_len))
            graph.replay()
            return out

        return self._graph_run(run, graph, static, t_y=W)

    # ------------------------------------------------------------ hipGraphs
    # Every capture_* below is the same three steps: static input buffers, a
    # ``body`` over them captured by _capture_body, and a ``run`` closure that
    # fills the buffers, replays and returns the captured outputs.
    @staticmethod
    def _capture_body(body, warmup, dev):
        """Warm ``body`` up on a side stream, then capture it on the current
        one (torch.cuda.CUDAGraph is HIP graphs on ROCm): (graph, its outputs)."""
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                body()
        torch.cuda.current_stream(dev).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = body()
        return graph, out

    @staticmethod
    def _graph_run(run, graph, static, **attrs):
        """``run`` with its graph, its static buffers and ``attrs`` (t_x, t_y,
        batch, pool_len, output: what the capture has) attached."""
        run.graph, run.static = graph, static
        for k, v in attrs.items():
            setattr(run, k, v)
        return run

    @torch.no_grad()
    def capture_infer_bucketed(self, t_x, t_y, *, noise_len=None, padded_text=False,
                               length_scale=1.0, warmup=2, batch=1, pool_len=None,
                               control=False, _front=False):
        """One hipGraph for a whole utterance (infer_bucketed) of t_x tokens
        (padded_text: up to t_x, x_lengths given at replay) into a t_y-frame
        bucket.  noise_len: replay reads a flat noise buffer of that many
        elements at a per-call start offset (EmoVITS); else noise [1, C,
        t_y].  Returns run(x, emo, sid, noise, noise_start=None,
        x_length=None) -> (wav, y_len) views of static buffers; with
        noise_len, noise_start is the [ops.ED_DRAWS] raw-word pool of
        ops.numpy_draw_pool and y_len is [2, 1] (y_len, words consumed).

        batch > 1 (needs padded_text and noise_len): one graph for up to
        ``batch`` utterances, infer_bucketed's shared-pool form over a pool of
        ``pool_len`` words (default ops.ED_DRAWS * batch).  Returns run(x [n,
        t <= t_x, c], emo [n, 1024], sid [n], x_lengths (n ints), pool int32
        [pool_len], n_rows=n) -> (wav [batch, 1, t_y * hop], y_len [batch],
        status [batch], used_total [1]), views of static buffers.  Text rows
        are zeroed past their length; rows at or past n are padding: zero
        text, length 0 (y_len 1), no draw.

        ``length_scale`` as an fp32 [batch] tensor (its values: the initial
        speeds) captures a rate-free graph: the speeds live in the static
        buffer ``rates`` and replay takes them per call, batch > 1 as
        run(..., rates=[n floats]) (padding rows get 1.0), batch 1 as
        run(..., rate=float); without them the buffer keeps what it holds.

        ``control=True`` captures infer_bucketed(control=...) over the static
        buffers ``given`` (int32 [batch, t_x]), ``tok_scale`` (fp32 [batch,
        t_x]) and ``target`` (int32 [batch]); the graph is always rate-free
        (a number as ``length_scale`` is the initial speed of every row).
        Replay takes them per call as run(..., control=dict(given=,
        tok_scale=, target=)): batch 1 one row each (sequences of up to t_x
        values, an int), batch > 1 lists with one entry per row; a missing or
        None entry, the tokens past a row's values and padding rows get -1 /
        1.0 / 0 (free, unscaled, no target), so does a replay without
        ``control``.  The outputs gain (dur, plan_meta) as their last two."""
        if control and not isinstance(length_scale, torch.Tensor):
            length_scale = torch.full((int(batch),), float(length_scale))
        if batch > 1:
            return self._capture_infer_batch(t_x, t_y, int(batch), noise_len, padded_text,
                                             length_scale, warmup, pool_len, control, _front)
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        C = self.inter_channels
        static = dict(x=torch.zeros(1, t_x, self.text_channels, device=dev, dtype=dt),
                      emo=torch.zeros(1, 1024, device=dev, dtype=dt),
                      sid=torch.zeros(1, device=dev, dtype=torch.long),
                      start=torch.zeros(1, engine.ops.ED_DRAWS, device=dev, dtype=torch.int32),
                      xl=torch.full((1,), t_x, device=dev, dtype=torch.int32),
                      noise=torch.zeros(noise_len if noise_len else C * t_y, device=dev))
        if isinstance(length_scale, torch.Tensor):
            static["rates"] = length_scale.to(device=dev, dtype=torch.float32).reshape(1).clone()
        ctl = _control_buffers(static, 1, t_x, dev) if control else None

        infer = self.infer_front_bucketed if _front else self.infer_bucketed

        def body():
            noise = static["noise"] if noise_len else static["noise"].view(1, C, t_y)
            return infer(static["x"], static["emo"], static["sid"], noise, t_y,
                         x_lengths=static["xl"] if padded_text else None,
                         length_scale=static.get("rates", length_scale),
                         noise_start=static["start"] if noise_len else None, control=ctl)

        graph, out = self._capture_body(body, warmup, dev)

        def run(x, emo, sid, noise=None, noise_start=None, x_length=None, rate=None,
                control=None):
            if ctl is not None:
                _control_fill(static, [control], 1, t_x)
            elif control is not None:
                raise ValueError("replay: this graph was captured without control")
            if rate is not None:
                if "rates" not in static:
                    raise ValueError("replay: this graph was captured at a fixed length_scale")
                static["rates"].fill_(float(rate))
            if padded_text:
                n = x.shape[1] if x_length is None else int(x_length)
                static["x"].zero_()
                static["x"][:, :x.shape[1]].copy_(x)
                static["xl"].fill_(n)
            else:
                static["x"].copy_(x)
            static["emo"].copy_(emo)
            static["sid"].copy_(sid)
            if noise is not None:
                static["noise"].copy_(noise.reshape(-1))
            if noise_start is not None:
                static["start"].copy_(torch.as_tensor(noise_start, dtype=torch.int32).view(1, -1))
            graph.replay()
            return out

        return self._graph_run(run, graph, static, t_y=t_y)

    @torch.no_grad()
    def capture_infer_front_bucketed(self, t_x, t_y, *, noise_len=None, padded_text=False,
                                     length_scale=1.0, warmup=2, batch=1, pool_len=None,
                                     control=False):
        """capture_infer_bucketed for infer_front_bucketed: the same static
        buffers and the same ``run``, whose result starts with (z [batch, C,
        t_y], g [batch, gin]) in place of the waveform."""
        return self.capture_infer_bucketed(
            t_x, t_y, noise_len=noise_len, padded_text=padded_text, length_scale=length_scale,
            warmup=warmup, batch=batch, pool_len=pool_len, control=control, _front=True)

    def _capture_infer_batch(self, t_x, t_y, batch, noise_len, padded_text, length_scale, warmup,
                             pool_len, control=False, front=False):
        """capture_infer_bucketed for batch > 1 (see there)."""
        if not padded_text or not noise_len:
            raise ValueError("capture_infer_bucketed: batch > 1 needs padded_text=True and noise_len")
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        P = int(pool_len) if pool_len else engine.ops.ED_DRAWS * batch
        static = dict(x=torch.zeros(batch, t_x, self.text_channels, device=dev, dtype=dt),
                      emo=torch.zeros(batch, 1024, device=dev, dtype=dt),
                      sid=torch.zeros(batch, device=dev, dtype=torch.long),
                      xl=torch.zeros(batch, device=dev, dtype=torch.int32),
                      pool=torch.zeros(P, device=dev, dtype=torch.int32),
                      n_rows=torch.zeros(1, device=dev, dtype=torch.int32),
                      noise=torch.zeros(noise_len, device=dev))
        if isinstance(length_scale, torch.Tensor):
            static["rates"] = length_scale.to(device=dev, dtype=torch.float32).reshape(
                batch).clone()
        cols = torch.arange(t_x, device=dev).view(1, t_x, 1)
        ctl = _control_buffers(static, batch, t_x, dev) if control else None

        infer = self.infer_front_bucketed if front else self.infer_bucketed

        def body():
            return infer(static["x"], static["emo"], static["sid"], static["noise"], t_y,
                         x_lengths=static["xl"], length_scale=static.get("rates", length_scale),
                         noise_start=static["pool"], n_rows=static["n_rows"], control=ctl)

        graph, out = self._capture_body(body, warmup, dev)

        def run(x, emo, sid, x_lengths, pool, n_rows=None, rates=None, control=None):
            n = x.shape[0] if n_rows is None else int(n_rows)
            if ctl is not None:
                for k, v in (control or {}).items():
                    if v is not None and len(v) != n:
                        raise ValueError(f"batched replay: {n} rows need {n} entries of "
                                         f"control {k!r}, got {len(v)}")
                rows = [{k: (v[i] if v is not None else None) for k, v in (control or {}).items()}
                        for i in range(n)]
                _control_fill(static, rows, batch, t_x)
            elif control is not None:
                raise ValueError("batched replay: this graph was captured without control")
            if rates is not None:
                if "rates" not in static:
                    raise ValueError("batched replay: this graph was captured at a fixed "
                                     "length_scale")
                rates = [float(v) for v in rates][:n]
                if len(rates) != n:
                    raise ValueError(f"batched replay: {n} rows need {n} rates, got {len(rates)}")
                static["rates"].copy_(torch.tensor(rates + [1.0] * (batch - n),
                                                   dtype=torch.float32))
            lengths = [int(v) for v in x_lengths][:n]
            if not 1 <= n <= batch or len(lengths) != n or x.shape[1] > t_x or max(lengths) > x.shape[1]:
                raise ValueError(f"batched replay: {n} rows of lengths {lengths} in x "
                                 f"{tuple(x.shape)} do not fit [{batch}, {t_x}]")
            static["xl"].copy_(torch.tensor(lengths + [0] * (batch - n), dtype=torch.int32))
            _fill_rows(static["x"], x[:n], n, x.shape[1])
            static["x"].masked_fill_(cols >= static["xl"].view(batch, 1, 1), 0)
            _fill_rows(static["emo"], emo[:n], n)
            _fill_rows(static["sid"], torch.as_tensor(sid)[:n], n)
            pool = torch.as_tensor(pool, dtype=torch.int32).view(-1)
            if pool.numel() != P:
                raise ValueError(f"batched replay: the pool must have {P} words, got {pool.numel()}")
            static["pool"].copy_(pool)
            static["n_rows"].fill_(n)
            graph.replay()
            return out

        return self._graph_run(run, graph, static, t_y=t_y, batch=batch, pool_len=P)

    # ----------------------------------- the audio side of VC and alignment
    def _audio_latents(self, spec, noise, lens, g, keep=False):
        """spec [B, F, T] fp32 -> z = enc_q(spec) (noise None: the posterior
        mean) -> z_p = flow(z; g), the forward flow, every layer masked at
        lens (int32 [B], device); kernels only, no host sync.  Returns (z,
        z_p, stage lengths int32 [n, B]); z_p is z updated in place unless
        ``keep``."""
        z, sl = engine.get_plan(self.enc_q, engine.PosteriorPlan).run_bucketed(
            spec, noise, lens, stage_mult=self._stage_mult())
        z_p = z.clone() if keep else z
        engine.get_plan(self.flow, engine.CouplingFlowPlan).run_(z_p, g, lengths=sl[0],
                                                                 forward=True)
        return z, z_p, sl

    def _spec_rows(self, what, wav, n_samples, t_y, stft):
        """The linear spectrogram of a ragged waveform batch over a bucket of
        t_y frames (convert_bucketed documents it): (spec [B, F, t_y], y_len
        int32 [B])."""
        n_fft, hop, win = (int(v) for v in stft)
        if hop != self.hop_total or n_fft // 2 + 1 != self.enc_q.in_channels:
            raise ValueError(f"{what}: stft {tuple(stft)} does not fit a model of "
                             f"{self.enc_q.in_channels} bins and hop {self.hop_total}")
        if wav.dim() != 2 or wav.dtype != torch.float32 or wav.shape[1] < t_y * hop:
            raise ValueError(f"{what}: wav must be fp32 [B, >= {t_y * hop}], got "
                             f"{wav.dtype} {tuple(wav.shape)}")
        return engine.ops.stft_mag_rows(wav, n_samples, self._vc_window(win, wav.device), n_fft,
                                        hop, win, t_y, pad=(n_fft - hop) // 2, eps=1e-6)

    # ------------------------------------------------------- voice conversion
    def _vc_core(self, spec, noise, lens, sid_src, sid_tgt, keep=False):
        """spec [B, F, T] fp32 -> enc_q -> flow(g_src) -> flow^-1(g_tgt) ->
        dec(g_tgt), every layer masked at lens (int32 [B], device); kernels
        and the two embedding lookups only, no host sync.  Returns (o fp32
        [B, 1, T * hop], (z, z_p, z_hat) when ``keep`` else None)."""
        g_tgt = engine._f32(self.emb_g(sid_tgt))
        z, z_p, sl = self._audio_latents(spec, noise, lens, engine._f32(self.emb_g(sid_src)), keep)
        z_hat = z_p.clone() if keep else z_p
        engine.get_plan(self.flow, engine.CouplingFlowPlan).run_(z_hat, g_tgt, lengths=sl[0])
        o = engine.get_plan(self.dec, engine.GeneratorPlan).run(z_hat, g_tgt, lengths=sl[1:])
        # the decoder's last conv runs unmasked over the whole buffer (its halo
        # spills 3 samples past a row's end, and skipped tiles hold nothing
        # meaningful): cut every row at lens * hop, zero behind
        out = torch.empty_like(o)
        engine.ops.resample_poly(o[:, 0], 1, 1, lengths=sl[0], length_scale=self.hop_total,
                                 out=out[:, 0])
        return out, ((z, z_p, z_hat) if keep else None)

    @torch.no_grad()
    def voice_conversion(self, y, y_lengths, sid_src, sid_tgt, noise=None):
        """Upstream VITS' ``voice_conversion``: the linear spectrogram y [B,
        F, T] of speaker sid_src rendered in the voice of sid_tgt: z =
        enc_q(y) (speaker-free), z_p = flow(z; g_src) (the forward flow,
        see ResidualCouplingBlock.infer), z_hat = flow^-1(z_p; g_tgt), o_hat =
        dec(z_hat; g_tgt).  ``noise`` [B, C, T], already scaled, is the
        posterior draw (z = m + noise * exp(logs)); None gives the posterior
        mean.  Rows are masked at y_lengths (latents zero past them, o_hat
        zero past y_lengths * hop).  Exact-length and eager: this is the
        definition convert_bucketed is held to, bit for bit.  Returns (o_hat
        [B, 1, T * hop], y_mask [B, 1, T], (z, z_p, z_hat))."""
        engine._check_gpu(y, "SynthesizerTrn.voice_conversion")
        lens = y_lengths.to(device=y.device, dtype=torch.int32).contiguous()
        o, zs = self._vc_core(engine._f32(y), noise, lens, sid_src, sid_tgt, keep=True)
        y_mask = torch.unsqueeze(commons.sequence_mask(y_lengths.to(y.device), y.size(2)), 1).to(
            y.dtype)
        return o.to(y.dtype), y_mask, tuple(t.to(y.dtype) for t in zs)

    def vc_context_frames(self, stft):
        """Frames on each side of a frame that can influence its converted
        samples (``stft`` as convert_bucketed takes it): a window of a long
        recording with this many real frames between an artificial edge and
        its core reproduces the whole recording's samples on that core.  The
        audio side is local in time, so the parts add up:
          - the STFT: frames at a row's ends whose support [j * hop - pad,
            j * hop - pad + n_fft) leaves the row and sees reflected samples;
          - enc_q: its WN stack, sum_i (k - 1) / 2 * dilation_rate ** i (the
            1x1 convs and the channel LayerNorm add nothing);
          - the flow, forward and reverse: every coupling's WN stack, twice;
          - the decoder: Generator.context_frames."""
        n_fft, hop, _ = (int(v) for v in stft)
        if hop != self.hop_total:
            raise ValueError(f"vc_context_frames: hop {hop} is not the decoder's {self.hop_total}")
        pad = (n_fft - hop) // 2

        def wn(m):
            k = m.kernel_size[0]
            return sum((k - 1) // 2 * m.dilation_rate ** i for i in range(m.n_layers))

        edge = max(-(-pad // hop), -(-(n_fft - pad) // hop) - 1)
        flow = sum(wn(f.enc) for f in self.flow.flows
                   if isinstance(f, modules.ResidualCouplingLayer))
        return edge + wn(self.enc_q.enc) + 2 * flow + self.dec.context_frames()

    def _vc_window(self, win, dev):
        w = self.__dict__.get("_vc_win")
        if w is None or w.numel() != win or w.device != dev:
            w = self.__dict__["_vc_win"] = torch.hann_window(win, device=dev, dtype=torch.float32)
        return w

    @torch.no_grad()
    def convert_bucketed(self, wav, n_samples, sid_src, sid_tgt, noise, t_y, *, stft):
        """voice_conversion from the waveform with NO host synchronisation,
        over a static bucket of t_y frames (capture_convert_bucketed makes it
        one hipGraph).  wav [B, t_y * hop + hop - 1] fp32, n_samples int32
        [B] on the device; noise [B, C, t_y] (pre-scaled) or None.

        ``stft`` = (filter_length, hop_length, win_length) of the model's
        data config, given to the call (spec_channels alone fixes neither
        hop nor window; hop must equal the decoder's total upsampling).  The
        spectrogram is mel_processing.spectrogram_torch's (reflect padding
        (n_fft - hop) / 2 at each row's own end, eps 1e-6), computed per row
        at its own length (ops.stft_mag_rows), so y_len = n_samples // hop
        frames (0 for a row of at most (n_fft - hop) / 2 samples).  Every
        layer runs masked at y_len under ops.length_skip(64).

        Returns (wav_out fp32 [B, 1, t_y * hop], y_len int32 [B]): the first
        y_len * hop samples of row b are bit for bit voice_conversion of that
        row alone on its own exact-length spectrogram; the rest is zero."""
        engine._check_gpu(wav, "SynthesizerTrn.convert_bucketed")
        spec, y_len = self._spec_rows("convert_bucketed", wav, n_samples, int(t_y), stft)
        with engine.ops.length_skip(64):
            o, _ = self._vc_core(spec, noise, y_len, sid_src, sid_tgt)
        return o, y_len

    @torch.no_grad()
    def capture_convert_bucketed(self, t_y, batch=1, warmup=2, *, stft):
        """One hipGraph for convert_bucketed over [batch, t_y] (``stft`` as
        there).  Returns run(wav, n_samples, sid_src, sid_tgt, noise=None) ->
        (wav_out [batch, 1, t_y * hop], y_len [batch]), views of static
        buffers: wav [n, <= t_y * hop + hop - 1] fp32 rows, n_samples /
        sid_src / sid_tgt n host ints (or tensors), noise [n, C, t_y] or None
        (the static noise is then zeroed: the posterior mean).  Rows at or
        past n get length 0.

        ``run.replay(n, n_samples, sid_src, sid_tgt)`` is the same replay for
        a caller that has written the rows of ``run.static["wav"]`` [batch,
        t_y * hop + hop - 1] and ``run.static["noise"]`` [batch, C, t_y]
        itself (ops.copy_windows of a long recording: no staging tensor and
        no second copy); it touches neither buffer."""
        dev = next(self.parameters()).device
        n_fft, hop, win = (int(v) for v in stft)
        t_y, batch = int(t_y), int(batch)
        C = self.inter_channels
        cap = t_y * hop + hop - 1
        static = dict(wav=torch.zeros(batch, cap, device=dev),
                      n=torch.zeros(batch, device=dev, dtype=torch.int32),
                      src=torch.zeros(batch, device=dev, dtype=torch.long),
                      tgt=torch.zeros(batch, device=dev, dtype=torch.long),
                      noise=torch.zeros(batch, C, t_y, device=dev))
        self._vc_window(win, dev)  # (built outside the capture)

        def body():
            return self.convert_bucketed(static["wav"], static["n"], static["src"], static["tgt"],
                                         static["noise"], t_y, stft=(n_fft, hop, win))

        graph, out = self._capture_body(body, warmup, dev)
        _ints = self._row_ints

        def replay(n, n_samples, sid_src, sid_tgt):
            if not 1 <= n <= batch:
                raise ValueError(f"convert replay: {n} rows do not fit a batch of {batch}")
            _fill_rows(static["n"], _ints(n_samples, n, torch.int32), n)
            _fill_rows(static["src"], _ints(sid_src, n, torch.long), n)
            _fill_rows(static["tgt"], _ints(sid_tgt, n, torch.long), n)
            graph.replay()
            return out

        def run(wav, n_samples, sid_src, sid_tgt, noise=None):
            n = wav.shape[0]
            if not 1 <= n <= batch or wav.shape[1] > cap:
                raise ValueError(f"convert replay: wav {tuple(wav.shape)} does not fit "
                                 f"[{batch}, {cap}]")
            static["wav"][:n, :wav.shape[1]].copy_(wav)
            if noise is None:
                static["noise"].zero_()
            else:
                static["noise"][:n].copy_(noise)
            return replay(n, n_samples, sid_src, sid_tgt)

        return self._graph_run(run, graph, static, t_y=t_y, batch=batch, replay=replay)

    @staticmethod
    def _row_ints(v, n, dtype):
        t = torch.as_tensor(v, dtype=dtype).reshape(-1)[:n]
        if t.numel() != n:
            raise ValueError(f"replay: {n} rows need {n} values, got {t.numel()}")
        return t

    # ------------------------------------------------------ forced alignment
    def _align_core(self, spec, noise, y_len, x, x_len, emo, sid):
        """Both sides of the model scored against each other and the best
        monotonic path reduced to durations: (durations int32 [B, Tx], scores
        fp32 [B, Tx], (z_p, m_p, logs_p, neg_cent) in fp32).  The text side is
        TextEncoder.infer of each row's own tokens (pad_exact), the audio side
        voice conversion's (_audio_latents) with the row's speaker; kernels
        and one embedding lookup only, no host sync."""
        g = self.emb_g(sid)
        _, m_p, logs_p = self.enc_p.forward_masked_hip(x, x_len, emo, g, pad_exact=True)
        _, z_p, _ = self._audio_latents(spec, noise, y_len, engine._f32(g))
        nc = engine.ops.neg_cent(z_p, m_p, logs_p)
        dur, scores, _ = engine.ops.maximum_path_durations(nc, y_len, x_len)
        return dur, scores, (z_p, m_p, logs_p, nc)

    @torch.no_grad()
    def align(self, x, x_lengths, y, y_lengths, emo, sid, noise=None):
        """Forced alignment of the linear spectrogram y [B, F, Ty] (y_lengths
        frames) with the text x [B, Tx, c] (x_lengths tokens) of speaker sid:
        the monotonic path that the training forward searches (models.py:
        483-498), without alignment noise, autograd or decoder.  m_p, logs_p
        = enc_p(x), z = enc_q(y) (``noise`` [B, C, Ty], already scaled, is the
        posterior draw; None, the default, takes the posterior mean), z_p =
        flow(z; g), neg_cent = the four terms of models.py:484-489, then MAS.
        Exact-length and eager: this is the definition align_bucketed is held
        to.  Returns (durations int32 [B, Tx]: frames per token, 0 past
        x_lengths; scores fp32 [B, Tx]: the sum of neg_cent over each token's
        frames, a log-likelihood (higher = better match), 0 past x_lengths;
        (z_p, m_p, logs_p, neg_cent) in fp32).  A row with no frames, no
        tokens or fewer frames than tokens has no alignment: durations and
        scores are 0."""
        engine._check_gpu(x, "SynthesizerTrn.align")
        dev = x.device
        y_len = y_lengths.to(device=dev, dtype=torch.int32).contiguous()
        x_len = x_lengths.to(device=dev, dtype=torch.int32).contiguous()
        return self._align_core(engine._f32(y).contiguous(), noise, y_len, x, x_len, emo, sid)

    def align_context_frames(self, stft):
        """Frames on each side of a frame that can influence its z_p (``stft``
        as convert_bucketed takes it): the context a window of a long
        recording needs so that z_p on its core is the whole recording's.  The
        parts of vc_context_frames with the flow counted once (forward only)
        and no decoder: the STFT's edge frames, enc_q's WN stack and every
        coupling's WN stack."""
        n_fft, hop, _ = (int(v) for v in stft)
        if hop != self.hop_total:
            raise ValueError(f"align_context_frames: hop {hop} is not the decoder's "
                             f"{self.hop_total}")
        pad = (n_fft - hop) // 2

        def wn(m):
            k = m.kernel_size[0]
            return sum((k - 1) // 2 * m.dilation_rate ** i for i in range(m.n_layers))

        edge = max(-(-pad // hop), -(-(n_fft - pad) // hop) - 1)
        flow = sum(wn(f.enc) for f in self.flow.flows
                   if isinstance(f, modules.ResidualCouplingLayer))
        return edge + wn(self.enc_q.enc) + flow

    @torch.no_grad()
    def align_segments(self, xs, emos, y, y_length, sid, noise=None):
        """Forced alignment of ONE recording with a text in segments: the
        linear spectrogram y [1, F, Ty] (y_length frames) of speaker sid
        against the segments xs (a list of [Tx_i, c]), each encoded on its own
        with its own emotion vector (emos: a list of [1024]), as ``speaking``
        feeds the model; m_p / logs_p of the segments are concatenated along
        the tokens and searched as one text.  Exact-length and eager: the
        definition EmoVITS.align_long is held to.  Up to 2048 tokens in all
        the search is ``align``'s (ops.neg_cent and maximum_path_durations);
        above, ops.maximum_path_durations_long, which equals it bit for bit
        wherever both run.  Returns (durations int32 [Tx_total], scores fp32
        [Tx_total], segment token offsets (a list of n + 1 ints, cumulative),
        (z_p [1, C, Ty], m_p, logs_p [1, C, Tx_total]) in fp32)."""
        engine._check_gpu(y, "SynthesizerTrn.align_segments")
        if len(xs) == 0 or len(xs) != len(emos):
            raise ValueError(f"align_segments: {len(xs)} segments and {len(emos)} emotion vectors")
        dev = y.device
        y = y if y.dim() == 3 else y[None]
        sid = torch.as_tensor(sid, device=dev, dtype=torch.long).reshape(1)
        g = self.emb_g(sid)
        ms, ls, offs = [], [], [0]
        for x, emo in zip(xs, emos):
            x = x.reshape(1, -1, self.text_channels)
            n = x.shape[1]
            if n == 0:
                raise ValueError("align_segments: an empty segment")
            x_len = torch.full((1,), n, device=dev, dtype=torch.int32)
            _, m, lg = self.enc_p.forward_masked_hip(x, x_len, emo.reshape(1, -1), g,
                                                     pad_exact=True)
            ms.append(engine._f32(m))
            ls.append(engine._f32(lg))
            offs.append(offs[-1] + n)
        m_p, logs_p = torch.cat(ms, dim=2), torch.cat(ls, dim=2)
        y_len = torch.as_tensor(y_length, dtype=torch.int32).reshape(1).to(dev)
        _, z_p, _ = self._audio_latents(engine._f32(y).contiguous(), noise, y_len, engine._f32(g))
        t_s = torch.full((1,), offs[-1], device=dev, dtype=torch.int32)
        if offs[-1] <= 2048:
            dur, scores, _ = engine.ops.maximum_path_durations(
                engine.ops.neg_cent(z_p, m_p, logs_p), y_len, t_s)
        else:
            dur, scores, _ = engine.ops.maximum_path_durations_long(z_p, m_p, logs_p, y_len, t_s)
        return dur[0], scores[0], offs, (z_p, m_p, logs_p)

    @torch.no_grad()
    def latents_bucketed(self, wav, n_samples, sid, noise, t_y, *, stft):
        """The audio side of align_bucketed alone, with NO host
        synchronisation, over a static bucket of t_y frames: wav, n_samples,
        noise and ``stft`` as convert_bucketed takes them, sid [B] the rows'
        speakers.  Returns (z_p fp32 [B, C, t_y], y_len int32 [B]): the first
        y_len[b] frames of row b are z_p of that row alone at its exact
        length, the rest is zero."""
        engine._check_gpu(wav, "SynthesizerTrn.latents_bucketed")
        spec, y_len = self._spec_rows("latents_bucketed", wav, n_samples, int(t_y), stft)
        with engine.ops.length_skip(64):
            _, z_p, _ = self._audio_latents(spec, noise, y_len, engine._f32(self.emb_g(sid)))
        return z_p, y_len

    @torch.no_grad()
    def capture_latents_bucketed(self, t_y, batch=1, warmup=2, *, stft):
        """One hipGraph for latents_bucketed over [batch, t_y] (``stft`` as
        there).  Returns run with ``run.static`` (wav [batch, t_y * hop + hop
        - 1], noise [batch, C, t_y], which the caller fills: ops.copy_windows
        of a long recording) and ``run.replay(n, n_samples, sid)`` -> (z_p
        [batch, C, t_y], y_len [batch]), views of static buffers; rows at or
        past n get length 0."""
        dev = next(self.parameters()).device
        n_fft, hop, win = (int(v) for v in stft)
        t_y, batch = int(t_y), int(batch)
        static = dict(wav=torch.zeros(batch, t_y * hop + hop - 1, device=dev),
                      n=torch.zeros(batch, device=dev, dtype=torch.int32),
                      sid=torch.zeros(batch, device=dev, dtype=torch.long),
                      noise=torch.zeros(batch, self.inter_channels, t_y, device=dev))
        self._vc_window(win, dev)  # (built outside the capture)

        def body():
            return self.latents_bucketed(static["wav"], static["n"], static["sid"],
                                         static["noise"], t_y, stft=(n_fft, hop, win))

        graph, out = self._capture_body(body, warmup, dev)
        _ints = self._row_ints

        def replay(n, n_samples, sid):
            if not 1 <= n <= batch:
                raise ValueError(f"latents replay: {n} rows do not fit a batch of {batch}")
            _fill_rows(static["n"], _ints(n_samples, n, torch.int32), n)
            _fill_rows(static["sid"], _ints(sid, n, torch.long), n)
            graph.replay()
            return out

        return self._graph_run(replay, graph, static, t_y=t_y, batch=batch, replay=replay)

    @torch.no_grad()
    def align_bucketed(self, wav, n_samples, x, x_lengths, emo, sid, noise, t_x, t_y, *, stft):
        """align from the waveform with NO host synchronisation, over a
        static bucket of t_x tokens and t_y frames (capture_align_bucketed
        makes it one hipGraph).  wav [B, >= t_y * hop] fp32 and n_samples
        int32 [B] as convert_bucketed takes them (``stft`` too; the
        spectrogram is computed per row at its own length, y_len = n_samples
        // hop); x [B, t_x, c] with x_lengths int32 [B] on the device; noise
        [B, C, t_y] (pre-scaled) or None.  The audio side runs masked at
        y_len under ops.length_skip(64), the text side masked at x_lengths.

        Returns (durations int32 [B, t_x], scores fp32 [B, t_x], y_len int32
        [B]): the first x_lengths[b] entries of row b are bit for bit
        ``align`` of that row alone at its exact lengths; the rest is zero."""
        engine._check_gpu(wav, "SynthesizerTrn.align_bucketed")
        t_x, t_y = int(t_x), int(t_y)
        if x.dim() != 3 or x.shape[0] != wav.shape[0] or x.shape[1] != t_x:
            raise ValueError(f"align_bucketed: x must be [{wav.shape[0]}, {t_x}, c], got "
                             f"{tuple(x.shape)}")
        spec, y_len = self._spec_rows("align_bucketed", wav, n_samples, t_y, stft)
        x_len = x_lengths.to(device=x.device, dtype=torch.int32).contiguous()
        with engine.ops.length_skip(64):
            dur, scores, _ = self._align_core(spec, noise, y_len, x, x_len, emo, sid)
        return dur, scores, y_len

    @torch.no_grad()
    def capture_align_bucketed(self, t_x, t_y, batch=1, warmup=2, *, stft):
        """One hipGraph for align_bucketed over [batch, t_x tokens, t_y
        frames] (``stft`` as there).  Returns run(wav, n_samples, x,
        x_lengths, emo, sid, noise=None) -> (durations [batch, t_x], scores
        [batch, t_x], y_len [batch]), views of static buffers: wav [n, <= t_y
        * hop + hop - 1] fp32 rows, x [n, <= t_x, c], emo [n, 1024], n_samples
        / x_lengths / sid n host ints (or tensors), noise [n, C, t_y] or None
        (the static noise is then zeroed: the posterior mean).  Rows at or
        past n get zero text and length 0 on both sides: they come back as
        "no alignment"."""
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        n_fft, hop, win = (int(v) for v in stft)
        t_x, t_y, batch = int(t_x), int(t_y), int(batch)
        cap = t_y * hop + hop - 1
        static = dict(wav=torch.zeros(batch, cap, device=dev),
                      n=torch.zeros(batch, device=dev, dtype=torch.int32),
                      x=torch.zeros(batch, t_x, self.text_channels, device=dev, dtype=dt),
                      xl=torch.zeros(batch, device=dev, dtype=torch.int32),
                      emo=torch.zeros(batch, 1024, device=dev, dtype=dt),
                      sid=torch.zeros(batch, device=dev, dtype=torch.long),
                      noise=torch.zeros(batch, self.inter_channels, t_y, device=dev))
        self._vc_window(win, dev)  # (built outside the capture)

        def body():
            return self.align_bucketed(static["wav"], static["n"], static["x"], static["xl"],
                                       static["emo"], static["sid"], static["noise"], t_x, t_y,
                                       stft=(n_fft, hop, win))

        graph, out = self._capture_body(body, warmup, dev)
        _ints = self._row_ints

        def run(wav, n_samples, x, x_lengths, emo, sid, noise=None):
            n = wav.shape[0]
            if not 1 <= n <= batch or wav.shape[1] > cap:
                raise ValueError(f"align replay: wav {tuple(wav.shape)} does not fit "
                                 f"[{batch}, {cap}]")
            if x.shape[0] != n or x.shape[1] > t_x:
                raise ValueError(f"align replay: x {tuple(x.shape)} does not fit [{n}, {t_x}, c]")
            static["wav"][:n, :wav.shape[1]].copy_(wav)
            _fill_rows(static["n"], _ints(n_samples, n, torch.int32), n)
            _fill_rows(static["x"], x, n, x.shape[1])
            _fill_rows(static["xl"], _ints(x_lengths, n, torch.int32), n)
            _fill_rows(static["emo"], emo, n)
            _fill_rows(static["sid"], _ints(sid, n, torch.long), n)
            if noise is None:
                static["noise"].zero_()
            else:
                static["noise"][:n].copy_(noise)
            graph.replay()
            return out

        return self._graph_run(run, graph, static, t_x=t_x, t_y=t_y, batch=batch)

    # ---------------------------------------------------------- speech editing
    def edit_context_frames(self):
        """Frames on each side of an edited span whose samples the edit can
        change: further from the span than this, ``edit`` returns the plain
        reconstruction of the recording.  Between the spliced z_p and the
        samples lie the reverse flow (every coupling's WN stack, once) and the
        decoder (Generator.context_frames); enc_q and the forward flow ran on
        the untouched recording."""
        def wn(m):
            k = m.kernel_size[0]
            return sum((k - 1) // 2 * m.dilation_rate ** i for i in range(m.n_layers))

        flow = sum(wn(f.enc) for f in self.flow.flows
                   if isinstance(f, modules.ResidualCouplingLayer))
        return flow + self.dec.context_frames()

    def _edit_tail(self, dur_new, spans, y_len, x_len_new, m_p, s_p, g, noise, z_p_rec, keep=False):
        """The acoustic side of an edit: splice, reverse flow, decoder, cut at
        y_new * hop; kernels only, no host sync.  Returns (o fp32 [B, 1, t_y *
        hop], lens, splice meta, (z_p, z_hat) when ``keep`` else None)."""
        z, lens, smeta = engine.ops.edit_splice(dur_new, spans, y_len, m_p, s_p, noise, z_p_rec,
                                                x_len=x_len_new, stage_mult=self._stage_mult())
        z_p = z.clone() if keep else None
        gf = engine._f32(g)
        engine.get_plan(self.flow, engine.CouplingFlowPlan).run_(z, gf, lengths=lens[0])
        o = engine.get_plan(self.dec, engine.GeneratorPlan).run(z, gf, lengths=lens[1:])
        out = torch.empty_like(o)  # (the cut of _vc_core)
        engine.ops.resample_poly(o[:, 0], 1, 1, lengths=lens[0], length_scale=self.hop_total,
                                 out=out[:, 0])
        return out, lens, smeta, ((z_p, z) if keep else None)

    @staticmethod
    def _span_target(span_frames, dev):
        """span_frames (None, an int > 0 or "keep") as vits_edit_pins' span_target."""
        if span_frames is None:
            return None
        if isinstance(span_frames, str) and span_frames == "keep":
            v = -1
        elif hasattr(span_frames, "__index__") and not isinstance(span_frames, bool) \
                and int(span_frames) > 0:
            v = int(span_frames)
        else:
            raise ValueError(f"edit: span_frames must be None, an int > 0 or 'keep', got "
                             f"{span_frames!r}")
        return torch.full((1,), v, device=dev, dtype=torch.int32)

    @torch.no_grad()
    def edit(self, y, y_lengths, x_old, x_new, emo, sid, span, *, durations_old=None, given=None,
             tok_scale=None, span_frames=None, length_scale=1.0, noise=None, noise_q=None,
             emo_new=None):
        """Re-speak a span of a recording with new text, in latent space.  y
        [1, F, Ty] is the linear spectrogram of speaker sid saying x_old [1,
        Tx_old, c]; ``span`` = (a, b_old, b_new): tokens [a, b_old) of x_old
        are replaced by tokens [a, b_new) of x_new [1, Tx_new, c] (the texts
        agree on the first a tokens and on the last Tx_old - b_old == Tx_new -
        b_new; b_old == a inserts, b_new == a deletes).  Eager, B = 1, exact
        lengths: the definition edit_bucketed is held to.

        dur_old = ``durations_old`` (Tx_old ints) or align(x_old, ..., y,
        ...)[0]; f0 = sum(dur_old[:a]), f1 = sum(dur_old[:b_old]).  m_p, s_p,
        logw, g come from the text side of x_new (``emo_new`` or ``emo``).
        The new text's durations are ops.duration_plan's under the pins
        dur_old outside the span and ``given`` inside it (Tx_new ints, or
        b_new - a ints for the span alone; default -1 = free), ``tok_scale``,
        ``length_scale`` as its rate and the row target ``span_frames``: None,
        an int (the new span lasts exactly that many frames) or "keep" (the
        span keeps its old length).  z_p_rec = flow(enc_q(y); g) is
        _audio_latents' (``noise_q`` [1, C, Ty] pre-scaled, None: the
        posterior mean).  With n_new = sum(dur_new[a:b_new]) and y_new = f0 +
        n_new + Ty - f1, the spliced z_p is z_p_rec[:, :f0], then m_p[:, x(t)]
        + noise[:, t] * s_p[:, x(t)] on the new span (``noise`` [1, C, y_new]
        pre-scaled, indexed by output frame; None: zeros), then z_p_rec[:,
        f1:Ty] (ops.edit_splice); o = dec(flow^-1(z_p; g); g) masked at y_new.

        Returns (o [1, 1, y_new * hop] in y's dtype, as voice_conversion
        returns it, dur_new int32 [Tx_new], (f0, n_new, f1), scores fp32
        [Tx_old] or None with durations_old, (z_p, z_hat)).
        Samples further than edit_context_frames() frames from the new span
        are bit for bit voice_conversion(y, ., sid, sid)."""
        engine._check_gpu(y, "SynthesizerTrn.edit")
        if y.size(0) != 1 or x_old.size(0) != 1 or x_new.size(0) != 1:
            raise ValueError("edit: one recording per call (edit_bucketed takes batches)")
        dev, dt = y.device, x_new.dtype
        i32 = torch.int32
        Ty, Tx_old, Tx_new = int(y_lengths.reshape(-1)[0]), x_old.size(1), x_new.size(1)
        a, b_old, b_new = (int(v) for v in span)
        if not (0 <= a <= b_old <= Tx_old and a <= b_new <= Tx_new
                and Tx_old - b_old == Tx_new - b_new):
            raise ValueError(f"edit: span {(a, b_old, b_new)} does not fit texts of {Tx_old} and "
                             f"{Tx_new} tokens")
        y_len = torch.full((1,), Ty, device=dev, dtype=i32)
        xl_old = torch.full((1,), Tx_old, device=dev, dtype=i32)
        xl_new = torch.full((1,), Tx_new, device=dev, dtype=i32)
        spans = torch.tensor([[a, b_old, b_new]], dtype=i32).to(dev)
        spec = engine._f32(y)[:, :, :Ty].contiguous()
        g = self.emb_g(sid)
        scores = None
        if durations_old is None:
            dur_old, scores, (z_p_rec, _, _, _) = self._align_core(spec, noise_q, y_len, x_old,
                                                                   xl_old, emo, sid)
        else:
            dur_old = torch.as_tensor(durations_old).reshape(1, -1).to(device=dev, dtype=i32)
            if dur_old.shape[1] != Tx_old:
                raise ValueError(f"edit: {Tx_old} old tokens need {Tx_old} durations_old, got "
                                 f"{dur_old.shape[1]}")
            _, z_p_rec, _ = self._audio_latents(spec, noise_q, y_len, engine._f32(g))
        span_given = None
        if given is not None:
            gv = torch.as_tensor(given).reshape(-1).to(i32)
            span_given = torch.full((1, Tx_new), -1, dtype=i32)
            if gv.numel() == Tx_new:
                span_given[0] = gv
            elif gv.numel() == b_new - a:
                span_given[0, a:b_new] = gv
            else:
                raise ValueError(f"edit: given needs {Tx_new} values (or {b_new - a} for the "
                                 f"span), got {gv.numel()}")
            span_given = span_given.to(dev)
        if tok_scale is not None:
            tok_scale = torch.as_tensor(tok_scale, dtype=torch.float32).reshape(1, Tx_new).to(
                dev).contiguous()
        pins, target, pmeta = engine.ops.edit_pins(
            dur_old.contiguous(), xl_old, xl_new, Tx_new, spans, y_len, span_given=span_given,
            span_target=self._span_target(span_frames, dev))
        m_p, s_p, logw, _ = self.infer_p1(x_new, emo if emo_new is None else emo_new, sid)
        dur_new, total, pstat = engine.ops.duration_plan(
            logw, rate=float(length_scale), half_round=dt == torch.float16, given=pins,
            tok_scale=tok_scale, target=target)
        # exact lengths: the one host visit of the eager definition
        pm, y_new, ps = pmeta.cpu(), int(total.item()), int(pstat.item())
        if int(pm[2, 0]) != 0:
            raise ValueError("edit: the old durations do not describe the recording (no "
                             f"alignment, or their sum is not its {Ty} frames)")
        if ps != 0:
            raise ValueError(f"edit: span_frames={span_frames!r} cannot be met by the new span")
        C = self.inter_channels
        if noise is None:
            noise = torch.zeros(1, C, max(y_new, 1), device=dev)
        noise = engine._f32(noise).contiguous()
        if tuple(noise.shape) != (1, C, max(y_new, 1)):
            raise ValueError(f"edit: the edited recording has {y_new} frames: noise must be "
                             f"[1, {C}, {max(y_new, 1)}], got {tuple(noise.shape)}")
        o, _, smeta, zs = self._edit_tail(dur_new, spans, y_len, xl_new, m_p, s_p, g, noise,
                                          z_p_rec.contiguous(), keep=True)
        f0, n_new, f1, st = (int(v) for v in smeta.cpu()[:, 0])
        if st != 0:
            raise ValueError(f"edit: the splice refused the row (status {st})")
        return (o[:, :, :y_new * self.hop_total].to(y.dtype), dur_new[0], (f0, n_new, f1),
                None if scores is None else scores[0], tuple(t.to(y.dtype) for t in zs))

    @torch.no_grad()
    def edit_bucketed(self, wav, n_samples, x_old, x_old_len, x_new, x_new_len, emo, emo_new, sid,
                      spans, controls, noise, t_rec, t_y, *, stft, durations_old=None):
        """``edit`` from the waveform with NO host synchronisation, over
        static buckets of t_rec recording frames and t_y output frames
        (capture_edit_bucketed makes it one hipGraph).  wav [B, >= t_rec *
        hop] fp32 and n_samples int32 [B] as convert_bucketed takes them
        (``stft`` too); x_old [B, t_x_old, c] / x_new [B, t_x_new, c] with
        x_old_len / x_new_len int32 [B] on the device; emo / emo_new [B, 1024]
        (emo_new None: emo); spans int32 [B, 3]; ``controls`` = None or
        dict(given= int32 [B, t_x_new], tok_scale= fp32 [B, t_x_new],
        span_target= int32 [B] (> 0 exact frames of the new span, 0 none, < 0
        keep), rate= a number or fp32 [B]); ``noise`` = the prior noise [B, C,
        t_y] (pre-scaled, indexed by output frame) or a pair (noise, noise_q
        [B, C, t_rec]); ``durations_old`` int32 [B, t_x_old]: the alignment is
        skipped (x_old and emo are then not read).

        The chain: ragged STFT -> _audio_latents -> old text -> neg_cent ->
        MAS durations -> edit_pins -> new text + duration predictor ->
        duration_plan -> edit_splice -> reverse flow -> decoder -> cut, under
        ops.length_skip(64).  Returns (o fp32 [B, 1, t_y * hop], y_new int32
        [B], dur_new int32 [B, t_x_new], meta int32 [6, B] = f0 | n_new | f1 |
        splice status | pins status | plan status, scores fp32 [B, t_x_old] or
        None): where all three statuses are 0, the first y_new * hop samples
        of row b are bit for bit ``edit`` of that row alone; a row whose
        splice status is not 0 is zero with y_new 0."""
        engine._check_gpu(wav, "SynthesizerTrn.edit_bucketed")
        t_rec, t_y = int(t_rec), int(t_y)
        dev, dt = wav.device, x_new.dtype
        B = wav.shape[0]
        noise, noise_q = noise if isinstance(noise, (tuple, list)) else (noise, None)
        controls = dict(controls or {})
        unknown = set(controls) - {"given", "tok_scale", "span_target", "rate"}
        if unknown:
            raise ValueError(f"edit_bucketed: unknown control(s) {sorted(unknown)}")
        if x_new.dim() != 3 or x_new.shape[0] != B or tuple(noise.shape) != (
                B, self.inter_channels, t_y):
            raise ValueError(f"edit_bucketed: x_new must be [{B}, t_x_new, c] and noise [{B}, "
                             f"{self.inter_channels}, {t_y}]")
        spec, y_len = self._spec_rows("edit_bucketed", wav, n_samples, t_rec, stft)
        xl_old = x_old_len.to(device=dev, dtype=torch.int32).contiguous()
        xl_new = x_new_len.to(device=dev, dtype=torch.int32).contiguous()
        g = self.emb_g(sid)
        scores = None
        with engine.ops.length_skip(64):
            if durations_old is None:
                dur_old, scores, (z_p_rec, _, _, _) = self._align_core(spec, noise_q, y_len, x_old,
                                                                       xl_old, emo, sid)
            else:
                dur_old = durations_old
                _, z_p_rec, _ = self._audio_latents(spec, noise_q, y_len, engine._f32(g))
            pins, target, pmeta = engine.ops.edit_pins(
                dur_old, xl_old, xl_new, x_new.shape[1], spans, y_len,
                span_given=controls.get("given"), span_target=controls.get("span_target"))
            h, m_p, s_p = self.enc_p.forward_masked_hip(
                x_new, xl_new, emo if emo_new is None else emo_new, g, exp_logs=True,
                pad_exact=True)
            logw = engine.get_plan(self.dp, engine.DurationPlan).run(h, g, lengths=xl_new)
            m_p, s_p, logw = m_p.to(dt), s_p.to(dt), logw.to(dt)
            dur_new, _, pstat = engine.ops.duration_plan(
                logw, rate=controls.get("rate", 1.0), x_len=xl_new,
                half_round=dt == torch.float16, given=pins, tok_scale=controls.get("tok_scale"),
                target=target)
            o, lens, smeta, _ = self._edit_tail(dur_new, spans, y_len, xl_new, m_p, s_p, g, noise,
                                                z_p_rec)
        meta = torch.cat([smeta, pmeta[2:3], pstat.reshape(1, B)], dim=0)
        return o, lens[0], dur_new, meta, scores

    @torch.no_grad()
    def capture_edit_bucketed(self, t_x_old, t_x_new, t_rec, t_y, batch=1, warmup=2, *, stft,
                              given_durations=False):
        """One hipGraph for edit_bucketed over [batch, t_x_old / t_x_new
        tokens, t_rec recording frames, t_y output frames] (``stft`` as
        there; ``given_durations``: the graph reads durations_old from a
        static buffer and holds no alignment).  Returns run(wav, n_samples,
        x_old, x_old_len, x_new, x_new_len, emo, emo_new, sid, spans,
        controls=None, noise=None, noise_q=None, durations_old=None) ->
        edit_bucketed's outputs as views of static buffers.  wav [n, <= t_rec
        * hop + hop - 1] fp32 rows, x_old [n, <= t_x_old, c] (None with
        given_durations), x_new [n, <= t_x_new, c], emo / emo_new [n, 1024]
        (emo_new None: emo), the lengths, sid and spans host ints (or
        tensors), ``controls`` a list of n dicts(given=, tok_scale=,
        span_target=, rate=) or None, noise [n, C, t_y] / noise_q [n, C,
        t_rec] (None: the static buffer is zeroed), durations_old [n, <=
        t_x_old] ints.  Rows at or past n get zero text and length 0: they
        come back with pins status 1.  ``run.replay()`` replays for a caller
        who has filled ``run.static`` itself."""
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        n_fft, hop, win = (int(v) for v in stft)
        t_x_old, t_x_new, t_rec, t_y, batch = (int(v) for v in (t_x_old, t_x_new, t_rec, t_y,
                                                                 batch))
        C = self.inter_channels
        cap = t_rec * hop + hop - 1
        i32 = torch.int32
        static = dict(wav=torch.zeros(batch, cap, device=dev),
                      n=torch.zeros(batch, device=dev, dtype=i32),
                      x_old=torch.zeros(batch, t_x_old, self.text_channels, device=dev, dtype=dt),
                      xl_old=torch.zeros(batch, device=dev, dtype=i32),
                      x_new=torch.zeros(batch, t_x_new, self.text_channels, device=dev, dtype=dt),
                      xl_new=torch.zeros(batch, device=dev, dtype=i32),
                      emo=torch.zeros(batch, 1024, device=dev, dtype=dt),
                      emo_new=torch.zeros(batch, 1024, device=dev, dtype=dt),
                      sid=torch.zeros(batch, device=dev, dtype=torch.long),
                      spans=torch.zeros(batch, 3, device=dev, dtype=i32),
                      given=torch.full((batch, t_x_new), -1, device=dev, dtype=i32),
                      tok_scale=torch.ones(batch, t_x_new, device=dev),
                      span_target=torch.zeros(batch, device=dev, dtype=i32),
                      rate=torch.ones(batch, device=dev),
                      noise=torch.zeros(batch, C, t_y, device=dev),
                      noise_q=torch.zeros(batch, C, t_rec, device=dev))
        if given_durations:
            static["dur_old"] = torch.zeros(batch, t_x_old, device=dev, dtype=i32)
        self._vc_window(win, dev)  # (built outside the capture)
        ctl = {k: static[k] for k in ("given", "tok_scale", "span_target", "rate")}

        def body():
            return self.edit_bucketed(
                static["wav"], static["n"], static["x_old"], static["xl_old"], static["x_new"],
                static["xl_new"], static["emo"], static["emo_new"], static["sid"], static["spans"],
                ctl, (static["noise"], static["noise_q"]), t_rec, t_y, stft=(n_fft, hop, win),
                durations_old=static.get("dur_old"))

        graph, out = self._capture_body(body, warmup, dev)
        _ints = self._row_ints

        def replay():
            graph.replay()
            return out

        def run(wav, n_samples, x_old, x_old_len, x_new, x_new_len, emo, emo_new, sid, spans,
                controls=None, noise=None, noise_q=None, durations_old=None):
            n = wav.shape[0]
            if not 1 <= n <= batch or wav.shape[1] > cap:
                raise ValueError(f"edit replay: wav {tuple(wav.shape)} does not fit "
                                 f"[{batch}, {cap}]")
            if x_new.shape[0] != n or x_new.shape[1] > t_x_new or (
                    x_old is not None and (x_old.shape[0] != n or x_old.shape[1] > t_x_old)):
                raise ValueError(f"edit replay: the texts do not fit [{n}, {t_x_old} / {t_x_new}, c]")
            if given_durations != (durations_old is not None):
                raise ValueError("edit replay: durations_old go with a graph captured with "
                                 "given_durations, and only with it")
            static["wav"].zero_()
            static["wav"][:n, :wav.shape[1]].copy_(wav)
            _fill_rows(static["n"], _ints(n_samples, n, i32), n)
            if x_old is not None:
                _fill_rows(static["x_old"], x_old, n, x_old.shape[1])
            _fill_rows(static["xl_old"], _ints(x_old_len, n, i32), n)
            _fill_rows(static["x_new"], x_new, n, x_new.shape[1])
            _fill_rows(static["xl_new"], _ints(x_new_len, n, i32), n)
            _fill_rows(static["emo"], emo, n)
            _fill_rows(static["emo_new"], emo if emo_new is None else emo_new, n)
            _fill_rows(static["sid"], _ints(sid, n, torch.long), n)
            _fill_rows(static["spans"], torch.as_tensor(spans, dtype=i32).reshape(n, 3), n)
            given = torch.full((batch, t_x_new), -1, dtype=i32)
            scale = torch.ones(batch, t_x_new)
            target = torch.zeros(batch, dtype=i32)
            rate = torch.ones(batch)
            for i, row in enumerate(controls or ()):
                row = row or {}
                unknown = set(row) - set(ctl)
                if unknown or i >= n:
                    raise ValueError(f"edit replay: controls {sorted(unknown)} of row {i}")
                for buf, v in ((given, row.get("given")), (scale, row.get("tok_scale"))):
                    if v is not None:
                        v = torch.as_tensor(v, dtype=buf.dtype).reshape(-1)
                        buf[i, :v.numel()] = v
                if row.get("span_target") is not None:
                    target[i] = int(row["span_target"])
                if row.get("rate") is not None:
                    rate[i] = float(row["rate"])
            for k, v in (("given", given), ("tok_scale", scale), ("span_target", target),
                         ("rate", rate)):
                static[k].copy_(v)
            for k, v in (("noise", noise), ("noise_q", noise_q)):
                static[k].zero_()
                if v is not None:
                    static[k][:n].copy_(v)
            if given_durations:
                d = torch.as_tensor(durations_old, dtype=i32).reshape(n, -1)
                _fill_rows(static["dur_old"], d, n, d.shape[1])
            return replay()

        return self._graph_run(run, graph, static, t_x_old=t_x_old, t_x_new=t_x_new, t_rec=t_rec,
                               t_y=t_y, batch=batch, replay=replay)

    # ---------------------------------------------------- retiming a recording
    def _retime_tail(self, z, lens, g_tgt):
        """Reverse flow (in place on z), decoder and the cut at y_new * hop."""
        engine.get_plan(self.flow, engine.CouplingFlowPlan).run_(z, g_tgt, lengths=lens[0])
        o = engine.get_plan(self.dec, engine.GeneratorPlan).run(z, g_tgt, lengths=lens[1:])
        out = torch.empty_like(o)  # (the cut of _vc_core)
        engine.ops.resample_poly(o[:, 0], 1, 1, lengths=lens[0], length_scale=self.hop_total,
                                 out=out[:, 0])
        return out

    @staticmethod
    def _retime_sources(dur_old, dur_new, ty):
        """The warp rule of vits_retime_warp on the host, in int64 tensors:
        (j0, j1 int64 [y_new], w fp32 [y_new], plain bool [y_new]); ``plain``
        frames copy z[j0]."""
        do = dur_old.to(torch.int64).clamp(0, 1 << 18)
        dn = dur_new.to(torch.int64).clamp(0, 1 << 18)
        c_old = torch.cumsum(do, 0) - do
        c_new = torch.cumsum(dn, 0) - dn
        i = torch.repeat_interleave(torch.arange(do.numel()), dn)  # each frame's owner
        k = torch.arange(i.numel(), dtype=torch.int64) - c_new[i]
        num = (2 * k + 1) * do[i] - dn[i]
        den = 2 * dn[i]
        qf = torch.div(num, den, rounding_mode="floor")
        r = num - qf * den
        j0 = (c_old[i] + qf).clamp(0, ty - 1)
        j1 = (c_old[i] + qf + 1).clamp(0, ty - 1)
        w = r.to(torch.float32) / den.to(torch.float32)  # (IEEE division on the host)
        return j0, j1, w, (r == 0) | (j0 == j1)

    @torch.no_grad()
    def retime(self, y, y_lengths, sid_src, sid_tgt, dur_old, dur_new, noise=None):
        """Retime a recording in latent space.  y [1, F, Ty] is the linear
        spectrogram of speaker sid_src; ``dur_old`` (Tx ints summing to Ty)
        says how many frames each token (any unit of the take: one for the
        whole of it) lasts, ``dur_new`` how many it shall last.  Eager, B = 1,
        exact lengths: the definition retime_bucketed is held to.

        z_p = flow(enc_q(y); g_src) is _audio_latents' (``noise`` [1, C, Ty]
        pre-scaled, None: the posterior mean).  With c_old / c_new the
        exclusive prefix sums of the durations, frame t of the result, the
        k-th of token i, reads the recording at c_old[i] + (k + 1/2) *
        dur_old[i] / dur_new[i] - 1/2, between its two nearest frames (clamped
        to the recording), linearly: vits_retime_warp's rule (include/
        vits_amd.h), here with torch indexing and the same separately rounded
        fp32 subtraction, product and sum.  Then z_hat = flow^-1(z_warp;
        g_tgt), o = dec(z_hat; g_tgt), masked at y_new = sum(dur_new).

        Returns (o [1, 1, y_new * hop] in y's dtype, (z_p, z_warp, z_hat)).
        With dur_new == dur_old the warp copies and o is bit for bit
        voice_conversion(y, ., sid_src, sid_tgt); samples further than
        edit_context_frames() frames from every retimed token are that too,
        shifted by the change of length before them."""
        engine._check_gpu(y, "SynthesizerTrn.retime")
        if y.size(0) != 1:
            raise ValueError("retime: one recording per call (retime_bucketed takes batches)")
        dev = y.device
        i32 = torch.int32
        Ty = int(y_lengths.reshape(-1)[0])
        do = torch.as_tensor(dur_old).reshape(-1).cpu().to(torch.int64)
        dn = torch.as_tensor(dur_new).reshape(-1).cpu().to(torch.int64)
        if do.numel() != dn.numel() or do.numel() == 0:
            raise ValueError(f"retime: {do.numel()} old durations against {dn.numel()} new ones")
        if int(do.min()) < 0 or int(dn.min()) < 0 or int(do.sum()) != Ty or Ty < 1:
            raise ValueError(f"retime: dur_old must be >= 0 and sum to the recording's {Ty} frames")
        y_new = int(dn.sum())
        if y_new < 1:
            raise ValueError("retime: the new durations leave no frame")
        y_len = torch.full((1,), Ty, device=dev, dtype=i32)
        spec = engine._f32(y)[:, :, :Ty].contiguous()
        g_tgt = engine._f32(self.emb_g(sid_tgt))
        _, z_p, _ = self._audio_latents(spec, noise, y_len, engine._f32(self.emb_g(sid_src)))
        j0, j1, w, plain = (t.to(dev) for t in self._retime_sources(do, dn, Ty))
        a = z_p[:, :, j0]
        d = z_p[:, :, j1] - a
        p = w * d
        z_warp = torch.where(plain, a, a + p).contiguous()
        lens = torch.tensor([[y_new * m] for m in self._stage_mult()], dtype=i32).to(dev)
        z_hat = z_warp.clone()
        o = self._retime_tail(z_hat, lens, g_tgt)
        return (o[:, :, :y_new * self.hop_total].to(y.dtype),
                tuple(t.to(y.dtype) for t in (z_p, z_warp, z_hat)))

    @torch.no_grad()
    def retime_bucketed(self, wav, n_samples, sid_src, sid_tgt, noise, t_rec, t_y, *, stft, x=None,
                        x_lengths=None, emo=None, durations_old=None, controls=None):
        """``retime`` from the waveform with NO host synchronisation, over
        static buckets of t_rec recording frames and t_y output frames
        (capture_retime_bucketed makes it one hipGraph).  wav [B, >= t_rec *
        hop] fp32 and n_samples int32 [B] as convert_bucketed takes them
        (``stft`` too); noise [B, C, t_rec] (pre-scaled posterior draw) or
        None.  The durations to warp from:
          - ``x`` [B, t_x, c] with ``x_lengths`` int32 [B] and ``emo``: the
            recording is aligned with its text (text encoder, neg_cent, MAS);
          - ``durations_old`` int32 [B, t_x] with ``x_lengths``: those three
            steps are skipped (x and emo are not read);
          - neither: the row is one token of y_len frames; no text encoder
            and no MAS run.
        ``controls`` = None or dict(given= int32 [B, t_x], tok_scale= fp32 [B,
        t_x], rate= fp32 [B], target= int32 [B]), ops.retime_plan's.

        The chain: ragged STFT -> _audio_latents -> dur_old -> retime_plan ->
        retime_warp -> reverse flow -> decoder -> cut, under
        ops.length_skip(64).  Returns (o fp32 [B, 1, t_y * hop], y_new int32
        [B], dur_old int32 [B, t_x], dur_new int32 [B, t_x], meta int32 [3, B]
        = the plan's total | warp status | plan status, scores fp32 [B, t_x]
        or None): where both statuses are 0, the first y_new * hop samples of
        row b are bit for bit ``retime`` of that row alone under these
        durations; a row whose warp status is -1 is zero with y_new 0."""
        engine._check_gpu(wav, "SynthesizerTrn.retime_bucketed")
        t_rec, t_y = int(t_rec), int(t_y)
        dev = wav.device
        B = wav.shape[0]
        controls = dict(controls or {})
        unknown = set(controls) - {"given", "tok_scale", "rate", "target"}
        if unknown:
            raise ValueError(f"retime_bucketed: unknown control(s) {sorted(unknown)}")
        if durations_old is not None and x_lengths is None:
            raise ValueError("retime_bucketed: durations_old need x_lengths")
        if durations_old is None and x is not None and (x_lengths is None or emo is None):
            raise ValueError("retime_bucketed: a text needs x_lengths and emo")
        spec, y_len = self._spec_rows("retime_bucketed", wav, n_samples, t_rec, stft)
        scores = x_len = None
        if x_lengths is not None:
            x_len = x_lengths.to(device=dev, dtype=torch.int32).contiguous()
        with engine.ops.length_skip(64):
            if durations_old is None and x is not None:
                dur_old, scores, (z_p, _, _, _) = self._align_core(spec, noise, y_len, x, x_len,
                                                                   emo, sid_src)
            else:
                dur_old = y_len.view(B, 1) if durations_old is None else durations_old
                if durations_old is None:
                    x_len = None
                _, z_p, _ = self._audio_latents(spec, noise, y_len,
                                                engine._f32(self.emb_g(sid_src)))
            dur_new, total, pstat = engine.ops.retime_plan(
                dur_old, y_len, x_len=x_len, given=controls.get("given"),
                tok_scale=controls.get("tok_scale"), rate=controls.get("rate"),
                target=controls.get("target"))
            z, lens, wmeta = engine.ops.retime_warp(z_p.contiguous(), dur_old, dur_new, y_len, t_y,
                                                    x_len=x_len, stage_mult=self._stage_mult())
            o = self._retime_tail(z, lens, engine._f32(self.emb_g(sid_tgt)))
        meta = torch.cat([wmeta, pstat.reshape(1, B)], dim=0)
        return o, lens[0], dur_old, dur_new, meta, scores

    @torch.no_grad()
    def capture_retime_bucketed(self, t_x, t_rec, t_y, batch=1, warmup=2, *, stft,
                                given_durations=False):
        """One hipGraph for retime_bucketed over [batch, t_x tokens, t_rec
        recording frames, t_y output frames] (``stft`` as there).  t_x == 0
        captures the text-free chain (one token per row); ``given_durations``:
        the graph reads durations_old from a static buffer and holds no
        alignment.  Returns run(wav, n_samples, sid_src, sid_tgt, x=None,
        x_lengths=None, emo=None, controls=None, noise=None,
        durations_old=None) -> retime_bucketed's outputs as views of static
        buffers.  wav [n, <= t_rec * hop + hop - 1] fp32 rows, the lengths
        and speakers host ints (or tensors), x [n, <= t_x, c], emo [n, 1024],
        ``controls`` a list of n dicts(given=, tok_scale=, rate=, target=) or
        None: the static given / tok_scale / rate / target are then reset to
        neutral on the device (nothing is uploaded), noise [n, C, t_rec] or
        None (the static noise is zeroed), durations_old [n, <= t_x] ints.
        Rows at or past n have no samples: warp status -1."""
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        n_fft, hop, win = (int(v) for v in stft)
        t_x, t_rec, t_y, batch = (int(v) for v in (t_x, t_rec, t_y, batch))
        if given_durations and t_x < 1:
            raise ValueError("capture_retime_bucketed: given durations need t_x >= 1")
        text = t_x > 0 and not given_durations
        tw = max(t_x, 1)  # (a text-free row is one token)
        cap = t_rec * hop + hop - 1
        i32 = torch.int32
        static = dict(wav=torch.zeros(batch, cap, device=dev),
                      n=torch.zeros(batch, device=dev, dtype=i32),
                      src=torch.zeros(batch, device=dev, dtype=torch.long),
                      tgt=torch.zeros(batch, device=dev, dtype=torch.long),
                      given=torch.full((batch, tw), -1, device=dev, dtype=i32),
                      tok_scale=torch.ones(batch, tw, device=dev),
                      rate=torch.ones(batch, device=dev),
                      target=torch.zeros(batch, device=dev, dtype=i32),
                      noise=torch.zeros(batch, self.inter_channels, t_rec, device=dev))
        if t_x > 0:
            static["xl"] = torch.zeros(batch, device=dev, dtype=i32)
        if text:
            static["x"] = torch.zeros(batch, t_x, self.text_channels, device=dev, dtype=dt)
            static["emo"] = torch.zeros(batch, 1024, device=dev, dtype=dt)
        if given_durations:
            static["dur_old"] = torch.zeros(batch, t_x, device=dev, dtype=i32)
        self._vc_window(win, dev)  # (built outside the capture)
        ctl = {k: static[k] for k in ("given", "tok_scale", "rate", "target")}
        state = dict(neutral=True)

        def body():
            return self.retime_bucketed(
                static["wav"], static["n"], static["src"], static["tgt"], static["noise"], t_rec,
                t_y, stft=(n_fft, hop, win), x=static.get("x"), x_lengths=static.get("xl"),
                emo=static.get("emo"), durations_old=static.get("dur_old"), controls=ctl)

        graph, out = self._capture_body(body, warmup, dev)
        _ints = self._row_ints

        def replay():
            graph.replay()
            return out

        def fill_controls(controls, n):
            if not any(v is not None for row in controls or () for v in (row or {}).values()):
                if not state["neutral"]:  # reset on the device, nothing uploaded
                    static["given"].fill_(-1)
                    static["tok_scale"].fill_(1.0)
                    static["rate"].fill_(1.0)
                    static["target"].zero_()
                    state["neutral"] = True
                return
            state["neutral"] = False
            given = torch.full((batch, tw), -1, dtype=i32)
            scale = torch.ones(batch, tw)
            rate = torch.ones(batch)
            target = torch.zeros(batch, dtype=i32)
            for i, row in enumerate(controls):
                row = row or {}
                unknown = set(row) - set(ctl)
                if unknown or i >= n:
                    raise ValueError(f"retime replay: controls {sorted(unknown)} of row {i}")
                for name, buf in (("given", given), ("tok_scale", scale)):
                    if row.get(name) is not None:
                        v = torch.as_tensor(row[name], dtype=buf.dtype).reshape(-1).cpu()
                        if v.numel() > tw:
                            raise ValueError(f"retime replay: {v.numel()} values of {name} do "
                                             f"not fit {tw} tokens")
                        buf[i, :v.numel()] = v
                if row.get("rate") is not None:
                    rate[i] = float(row["rate"])
                if row.get("target") is not None:
                    target[i] = int(row["target"])
            for k, v in (("given", given), ("tok_scale", scale), ("rate", rate),
                         ("target", target)):
                static[k].copy_(v)

        def run(wav, n_samples, sid_src, sid_tgt, x=None, x_lengths=None, emo=None, controls=None,
                noise=None, durations_old=None):
            n = wav.shape[0]
            if not 1 <= n <= batch or wav.shape[1] > cap:
                raise ValueError(f"retime replay: wav {tuple(wav.shape)} does not fit "
                                 f"[{batch}, {cap}]")
            if text != (x is not None) or given_durations != (durations_old is not None):
                raise ValueError("retime replay: a text goes with a graph captured with t_x > 0, "
                                 "durations_old with one captured with given_durations, and "
                                 "only with it")
            if text and (x.shape[0] != n or x.shape[1] > t_x):
                raise ValueError(f"retime replay: x {tuple(x.shape)} does not fit [{n}, {t_x}, c]")
            fill_controls(controls, n)
            static["wav"].zero_()
            static["wav"][:n, :wav.shape[1]].copy_(wav)
            _fill_rows(static["n"], _ints(n_samples, n, i32), n)
            _fill_rows(static["src"], _ints(sid_src, n, torch.long), n)
            _fill_rows(static["tgt"], _ints(sid_tgt, n, torch.long), n)
            if t_x > 0:
                _fill_rows(static["xl"], _ints(x_lengths, n, i32), n)
            if text:
                _fill_rows(static["x"], x, n, x.shape[1])
                _fill_rows(static["emo"], emo, n)
            if given_durations:
                d = torch.as_tensor(durations_old, dtype=i32).reshape(n, -1)
                if d.shape[1] > t_x:
                    raise ValueError(f"retime replay: {d.shape[1]} durations_old do not fit "
                                     f"{t_x} tokens")
                _fill_rows(static["dur_old"], d, n, d.shape[1])
            static["noise"].zero_()
            if noise is not None:
                static["noise"][:n].copy_(noise)
            return replay()

        return self._graph_run(run, graph, static, t_x=t_x, t_rec=t_rec, t_y=t_y, batch=batch,
                               replay=replay)

    # --------------------------------------- the two halves, captured apart
    @torch.no_grad()
    def capture_infer_p1(self, t_x, warmup=2):
        """Capture infer_p1 for one utterance of t_x tokens into a hipGraph
        (the text side is ~55 small launches whose host-side descriptor
        building dominates its B=1 latency).  Returns a callable(x, emo, sid)
        -> (m_p, s_p, logw, g) reading / returning static buffers."""
        dev = next(self.parameters()).device
        dt = next(self.parameters()).dtype
        static = dict(x=torch.zeros(1, t_x, self.text_channels, device=dev, dtype=dt),
                      emo=torch.zeros(1, 1024, device=dev, dtype=dt),
                      sid=torch.zeros(1, device=dev, dtype=torch.long))

        def body():
            return self.infer_p1(static["x"], static["emo"], static["sid"])

        graph, out = self._capture_body(body, warmup, dev)

        def run(x, emo, sid):
            static["x"].copy_(x)
            static["emo"].copy_(emo)
            static["sid"].copy_(sid)
            graph.replay()
            return out

        return self._graph_run(run, graph, static)

    @torch.no_grad()
    def capture_infer_p2(self, batch, t_x, t_y, warmup=2):
        """Capture infer_p2 for a static shape into a hipGraph (torch.cuda.CUDAGraph
        is HIP graphs on ROCm).  Returns a callable(attn, m_p, s_p, g, noise) -> wav
        that copies inputs into static buffers and replays the graph."""
        dev = next(self.parameters()).device
        C = self.inter_channels
        gin = self.emb_g.embedding_dim
        static = dict(
            attn=torch.zeros(batch, t_y, t_x, device=dev), m=torch.zeros(batch, C, t_x, device=dev),
            s=torch.ones(batch, C, t_x, device=dev), g=torch.zeros(batch, gin, device=dev),
            n=torch.zeros(batch, C, t_y, device=dev))
        fplan = engine.get_plan(self.flow, engine.CouplingFlowPlan)
        gplan = engine.get_plan(self.dec, engine.GeneratorPlan)

        def body():
            z = engine.ops.expand_prior(static["attn"], static["m"], static["s"], static["n"])
            fplan.run_(z, static["g"])
            return gplan.run(z, static["g"])

        graph, out = self._capture_body(body, warmup, dev)

        def run(attn, m_p, s_p, g, noise):
            static["attn"].copy_(attn)
            static["m"].copy_(m_p)
            static["s"].copy_(s_p)
            static["g"].copy_(g)
            static["n"].copy_(noise)
            graph.replay()
            return out

        return self._graph_run(run, graph, static, output=out)


# train.py's discriminator lives beside the generator in the reference's
# models.py (models.py:321-408); the implementation is in discriminators.py
from .discriminators import DiscriminatorP, DiscriminatorS, MultiPeriodDiscriminator  # noqa: E402,F401

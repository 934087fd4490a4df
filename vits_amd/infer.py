"""EmoVITS inference wrapper (reference ``infer.py``), on the HIP engine.

Same constructor and ``infer`` contract as ``infer.py:12-184``: speaker-id
mapping files ``*.map``, per-speaker emotion banks ``{spk}.emo`` next to the
checkpoint, an fp16 model (``.half()`` like the reference: its convs run on
the fp16-MFMA kernel variant with fp32 accumulation), a fixed noise
buffer sliced at a random offset per call.  Differences: the noise buffer
lives on the device (no host->device copy per call) and the CLI writes WAVs
with scipy instead of soundfile.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import durations as dur_host
from . import ops, utils
from .commons import infer_path
from .export import load_model


@dataclass
class PcmRequest:
    """One request of EmoVITS.infer_pcm_requests: ``items`` = [(spkid, text
    [N, c], emo), ...] and the controls of infer_pcm_batch, its own."""
    items: Sequence
    duration_rate: float = 1.0
    pitch: float = 1.0
    sampling_rate: Optional[int] = None
    volume: float = 1.0
    tail_silence: float = 0.0
    # duration controls, one entry per item (None: no control for that item)
    durations: Optional[Sequence] = None
    token_scale: Optional[Sequence] = None
    target_frames: Optional[Sequence] = None


class _Output(NamedTuple):
    """The output controls of one call or row, resolved (EmoVITS._output)."""
    pitch: float
    sampling_rate: int  # (the model's when the caller gave None)
    volume: float
    tail_silence: float
    tail: int  # tail silence in samples at sampling_rate
    passes: list  # (up, down) resampling passes (EmoVITS._post_passes)


class _Window(NamedTuple):
    """One window of a long recording (EmoVITS._long_plan)."""
    core_lo: int  # it owns the frames [core_lo, core_hi) of the recording
    core_hi: int
    a: int  # its row spans the frames [a, b)
    b: int
    s0: int  # and the samples [s0, s1)
    s1: int
    core_off: int  # samples into the row at which the core starts


class _Chunk(NamedTuple):
    """One chunk of a streamed utterance (EmoVITS._stream_plan)."""
    core_lo: int  # it owns the frames [core_lo, core_hi) of the utterance
    core_hi: int
    a: int  # its decoder window spans the frames [a, b)
    b: int
    out_lo: int  # and it yields the output samples [out_lo, out_hi) (the last: tail included)
    out_hi: int
    # per pass of the output stage: (in_lo, in_hi, out_lo, out_hi), the span of
    # the pass's output the chunk computes and the exact range of its input
    # that needs (ops.resample_span_input); with no pass, the one copy pass
    passes: tuple


class PcmStream(object):
    """What EmoVITS.infer_pcm_stream returns: an iterator over the int16
    chunks of one utterance.  Known before the first chunk exists:
    ``n_samples`` (all chunks together, tail silence included), ``n_model``
    (samples at the model's rate), ``durations`` (int32 [Tx] frames per
    token; None for a call without duration controls or return_durations)
    and ``emo``.  ``close()`` drops the chunks not yet taken; the engine
    stays usable and numpy's generator is where a complete call leaves it."""

    def __init__(self, chunks, n_samples, n_model, durations, emo):
        self._chunks = chunks
        self.n_samples, self.n_model, self.durations, self.emo = n_samples, n_model, durations, emo

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._chunks)

    def close(self):
        self._chunks.close()


class EmoVITS(object):
    def __init__(self, checkpoint_path=None, device=None, *, loglv=0, hps=None, model=None,
                 graph_cache=0, graph=True, max_graphs=16, half=True):
        """graph: synthesise each utterance as ONE hipGraph replay
        (SynthesizerTrn.capture_infer_bucketed: the durations, the output
        length and the path computed on the device, no host sync before the
        waveform copy), graphs cached per (text bucket, frame bucket), at
        most ``max_graphs`` (the batched graphs of infer_batch /
        infer_pcm_batch and the rate-free ones of infer_pcm_requests
        included); graph=False: the reference's eager
        sequence (infer_p1 -> host durations -> infer_p2).  half=False keeps
        the model, its inputs and the noise buffer fp32 (the reference serves
        fp16; the fp32 engine is the one whose bucketed and exact-length runs
        agree bit for bit at every length)."""
        self.loglv = loglv
        self.dtype = torch.float16 if half else torch.float32
        self.graph_cache = int(graph_cache)
        self._p1_graphs = {}
        self.graph = bool(graph)
        self.max_graphs = int(max_graphs)
        self._graphs = {}
        self._ty_bucket = {}
        self._pinned = {}
        self._vc_gen = None  # device generator of convert's posterior draws (made on first use)
        if checkpoint_path is None and model is None:
            checkpoint_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "checkpoint",
                                           "checkpoint.pth")
        self.res_root_path = os.path.dirname(checkpoint_path) if checkpoint_path else "."
        if hps is None:
            hps = utils.get_hparams_from_file(os.path.join(self.res_root_path, "config.json"))
        self.hps = hps
        self.sampling_rate = hps.data["sampling_rate"]
        self.hop_size = hps.data["hop_length"]
        self.text_channels = hps.data["text_channels"]
        self.inter_channels = hps.model["inter_channels"]
        self.num_speaker = hps.data["n_speakers"]
        self.noise_scale = hps.data["noise_scale"]

        self.spkid_mapping, self.spkid_mapping_mtime = {}, {}
        for map_path in utils.find_files(self.res_root_path, "*.map"):
            self._load_spkid_mapping(map_path)
        self.spk_emo_embed, self.spk_emo_embed_mtime = {}, {}
        for emo_path in utils.find_files(self.res_root_path, "*.emo"):
            self._load_spk_emo_embed(int(os.path.splitext(os.path.basename(emo_path))[0]))

        if isinstance(device, str):
            device = torch.device(device)
        self.device = device if device is not None else torch.device("cuda")
        if model is None:
            model = load_model(checkpoint_path, hps)
        model.remove_weight_norm()
        self.model = model.to(self.dtype).eval().to(self.device)
        self.noise = (torch.randn(1 * self.inter_channels * 4096) * self.noise_scale).to(
            self.dtype).to(self.device)
        self.inference = self.infer
        if self.device.type != "cuda":
            self.graph = False

    # -- speaker / emotion banks (infer.py:77-133) ----------------------------
    def _load_spkid_mapping(self, mapfn):
        if not os.path.exists(mapfn):
            return
        with open(mapfn, "rt") as f:
            for line in f:
                line = line.strip()
                if not line or line[0] == "#":
                    continue
                arr = line.split()
                if len(arr) != 2 or not (arr[0].isdigit() and arr[1].isdigit()):
                    continue
                self.spkid_mapping[int(arr[0])] = int(arr[1])
        self.spkid_mapping_mtime[mapfn] = int(os.stat(mapfn).st_mtime)

    def _load_spk_emo_embed(self, spkid: int):
        emo_path = os.path.join(self.res_root_path, f"{spkid}.emo")
        if os.path.exists(emo_path):
            emb = torch.from_numpy(np.fromfile(emo_path, dtype=np.float32).reshape(-1, 1024)).half()
            self.spk_emo_embed[spkid] = emb
            self.spk_emo_embed_mtime[emo_path] = int(os.stat(emo_path).st_mtime)
            return emb
        return None

    def _get_spk_emo_embed(self, emo: tuple):
        if isinstance(emo[0], (int, np.integer)):
            emb = self.spk_emo_embed.get(int(emo[0]))
            if emb is None:
                emb = self._load_spk_emo_embed(int(emo[0]))
            assert emb is not None, f"no emotion bank for speaker {emo[0]}"
        elif isinstance(emo[0], np.ndarray):
            emb = torch.from_numpy(emo[0].reshape(-1, 1024).astype(np.float32)).half()
        else:
            raise ValueError("emo[0] must be int or ndarray")
        eid = -1 if len(emo) == 1 else int(emo[1])
        if eid < 0 or eid > emb.size(0):
            eid = np.random.randint(0, emb.size(0))
        return emb[eid]

    def update(self):
        for map_path in list(self.spkid_mapping_mtime.keys()):
            if not os.path.exists(map_path):
                self.spkid_mapping_mtime.pop(map_path)
                continue
            if int(os.stat(map_path).st_mtime) != self.spkid_mapping_mtime[map_path]:
                self._load_spkid_mapping(map_path)
        for emo_path in list(self.spk_emo_embed_mtime.keys()):
            if not os.path.exists(emo_path):
                self.spk_emo_embed_mtime.pop(emo_path)
                continue
            if int(os.stat(emo_path).st_mtime) != self.spk_emo_embed_mtime[emo_path]:
                self._load_spk_emo_embed(int(os.path.splitext(os.path.basename(emo_path))[0]))

    # -- synthesis (infer.py:135-184) ------------------------------------------
    @torch.no_grad()
    def _infer_p1(self, text_t, emo, sid):
        """infer_p1, optionally replayed from a per-length hipGraph (captured
        on first use of a token count, at most `graph_cache` lengths kept).
        Off by default: on MI355X the B=1 text side is GPU-bound (3.3 ms
        eager vs 3.3 ms replayed at Tx=100), so capture only adds latency."""
        t_x = text_t.shape[1]
        if self.graph_cache <= 0:
            return self.model.infer_p1(text_t, emo, sid)
        run = self._cached_graph(t_x, lambda: self.model.capture_infer_p1(t_x), p1=True)
        return tuple(t.clone() for t in run(text_t, emo, sid))

    def _cached_graph(self, key, capture, p1=False):
        """The graph cached under ``key`` in self._graphs (at most
        ``max_graphs``; p1: in self._p1_graphs, at most ``graph_cache``),
        most recently used last.  A miss evicts the least recently used
        entries while the cache is full, then keeps what ``capture()``
        returns."""
        cache, limit = ((self._p1_graphs, self.graph_cache) if p1
                        else (self._graphs, self.max_graphs))
        run = cache.pop(key, None)
        if run is None:
            while len(cache) >= limit:
                cache.pop(next(iter(cache)))
            run = capture()
        cache[key] = run  # most recently used last
        return run

    def _capture_synthesis(self, xb, tyb, front=False, **kw):
        """A whole-utterance graph (capture_infer_bucketed over padded text;
        ``front``: capture_infer_front_bucketed, the text side alone) that
        reads this object's noise buffer."""
        capture = (self.model.capture_infer_front_bucketed if front
                   else self.model.capture_infer_bucketed)
        run = capture(xb, tyb, noise_len=self.noise.numel(), padded_text=True, **kw)
        run.static["noise"].copy_(self.noise.float())
        return run

    def _resolve(self, spkid, emo):
        """Speaker mapping and emotion lookup of infer (infer.py:135-158):
        (mapped spkid, emo fp16 [1, 1024] on the device).  A lookup without
        an emotion id draws it from numpy's generator."""
        spkid = self.spkid_mapping.get(spkid, spkid)
        assert spkid < self.num_speaker, f"spkid={spkid} must be less than {self.num_speaker}"
        if isinstance(emo, torch.Tensor):
            emo = emo.to(self.dtype)
        else:
            if emo is None:
                emo = (spkid, -1)
            if isinstance(emo[0], (int, np.integer)):
                emo = tuple([self.spkid_mapping.get(emo[0], emo[0]) if emo[0] != 0 else spkid,
                             -1 if len(emo) == 1 else emo[1]])
            emo = self._get_spk_emo_embed(emo).unsqueeze(0)
        return spkid, emo.to(device=self.device, dtype=self.dtype)

    def _inputs(self, spkid, text, emo):
        spkid, emo = self._resolve(spkid, emo)
        x_length, text_t, sid = self._one_tensors(spkid, np.ascontiguousarray(text))
        return x_length, text_t, emo, sid

    @staticmethod
    def _controls(x_length, durations, token_scale, target_frames, want=False):
        """The duration controls of one utterance, checked on the host before
        anything is uploaded (durations.check_controls raises ValueError):
        None when there is none, else (given int32 [Tx] or None, scale fp32
        [Tx] or None, target, known total or None).  ``want`` (the caller
        asked for the durations back): the neutral controls instead of None,
        so that the utterance takes the path that reports them."""
        if durations is None and token_scale is None and target_frames is None and not want:
            return None
        return dur_host.check_controls(x_length, durations, token_scale, target_frames)

    def infer(self, spkid, text, emo, *, duration_rate=1.0, durations=None, token_scale=None,
              target_frames=None, return_durations=False):
        """``durations`` (frames per token; < 0: left to the predictor),
        ``token_scale`` (a factor >= 0 per token on the predicted durations)
        and ``target_frames`` (the utterance lasts exactly that many frames;
        ``duration_rate`` is then not applied) control the timing: the
        durations come from ops.duration_plan inside the utterance graph
        (graph mode) or from its host restatement (durations.plan_durations).
        ``return_durations``: the frames per token as a third result.  The
        plain graphs do not report durations, so in graph mode a call with
        ``return_durations`` and no control replays the controlled graph with
        neutral controls (one more cached graph per bucket pair; the same
        samples, except that an fp16 model's plain call rounds a total above
        2048 frames to fp16 and this one does not)."""
        ctl = self._controls(text.shape[0], durations, token_scale, target_frames,
                             return_durations)  # (refuses before anything is uploaded)
        x_length, text_t, emo, sid = self._inputs(spkid, text, emo)
        got = [] if return_durations else None
        wav = self._infer_one(x_length, text_t, emo, sid, duration_rate, ctl, got)
        return (wav, emo, got[0]) if return_durations else (wav, emo)

    def _infer_one(self, x_length, text_t, emo, sid, duration_rate, ctl=None, got=None):
        if self.graph and x_length <= 4096:
            return self._infer_graph(text_t, emo, sid, duration_rate, ctl=ctl, got=got)
        wav = self._infer_eager(x_length, text_t, emo, sid, duration_rate, ctl, got)
        return wav.float().view(-1).cpu().numpy()

    def _host_durations(self, logw, duration_rate, ctl):
        """w_ceil [1, 1, Tx] of the eager path: ceil(exp(logw) * rate) in the
        model's dtype (the reference sums it in that dtype), or under controls
        the duration plan's rule on the host, fp32 integers, in the arithmetic
        of the device plan (the model's dtype for exp, the rate and the scale;
        the target drops the rate)."""
        if ctl is None:
            return torch.ceil(torch.exp(logw) * duration_rate)
        given, scale, target, _ = ctl
        if isinstance(given, torch.Tensor):
            given = given.cpu().numpy()
        w = torch.exp(logw)
        if not target:
            w = w * duration_rate
        if scale is not None:
            w = (w.float() * torch.from_numpy(scale).to(w.device).view(1, 1, -1)).to(logw.dtype)
        d, _ = dur_host.plan_durations(w.float().view(-1).cpu().numpy(), given, target)
        return torch.from_numpy(d.astype(np.float32)).to(logw.device).view(1, 1, -1)

    def _infer_eager(self, x_length, text_t, emo, sid, duration_rate, ctl=None, got=None,
                     front=False):
        """The reference's sequence: infer_p1 -> host durations -> infer_p2;
        the waveform stays on the device.  ``front``: infer_p2 stops behind
        the flow (infer_p2_front) and (z [1, C, y_length], g) is returned."""
        m_p, s_p, logw, g = self._infer_p1(text_t, emo, sid)
        w_ceil = self._host_durations(logw, duration_rate, ctl)
        if got is not None:
            got.append(w_ceil.view(-1).cpu().numpy().astype(np.int32))
        y_length = int(torch.clamp_min(torch.sum(w_ceil), 1).item())
        if ctl is not None and y_length > dur_host.MAX_FRAMES:
            raise ValueError(f"utterance of {y_length} frames is over the limit of "
                             f"{dur_host.MAX_FRAMES}")
        nl = self.inter_channels * y_length
        start = np.random.randint(max(1, self.noise.size(0) - nl))
        noise = self.noise[start:start + nl].view(1, self.inter_channels, y_length)
        attn = infer_path(w_ceil.float(), x_length, y_length).to(self.dtype)
        if front:
            return self.model.infer_p2_front(attn, m_p, s_p, g, noise), g
        return self.model.infer_p2(attn, m_p, s_p, g, noise)

    def _post_passes(self, pitch, sampling_rate):
        """The (up, down) resampling passes of VITSWrap.speaking, in its
        order: pitch (int(sr / pitch) -> sr), then the rate change (sr ->
        sampling_rate); a step that leaves the rate as it is is dropped."""
        sr = self.sampling_rate
        steps = []
        if pitch != 1.0:
            steps.append((int(sr / pitch), sr))
        if sampling_rate != sr:
            steps.append((sr, sampling_rate))
        passes = [ops.resample_ratio(o, t) for o, t in steps if o != t]
        return [(u, d) for u, d in passes if u != d]

    def _output(self, pitch, sampling_rate, volume, tail_silence):
        """A call's output controls, resolved: the sampling rate (None: the
        model's), the tail silence in samples and the resampling passes."""
        sampling_rate = self.sampling_rate if sampling_rate is None else int(sampling_rate)
        tail = int(tail_silence * sampling_rate) if tail_silence > 0 else 0
        return _Output(pitch, sampling_rate, volume, tail_silence, tail,
                       self._post_passes(pitch, sampling_rate))

    @staticmethod
    def _n_out(n, passes):
        """Samples that n model samples come to after ``passes``."""
        for up, down in passes:
            n = ops.resample_out_len(n, up, down)
        return n

    def _post(self, wav, out, *, lengths, length_scale=1):
        """wav [B, cap] -> int16 [B, >= n_out + tail] on the current stream
        under the controls ``out`` (_output): every pass but the last writes
        an fp32 intermediate and its length, the last one (or pcm16 alone)
        the PCM, zero past its end."""
        passes, volume, tail = out.passes, out.volume, out.tail
        B = wav.shape[0]
        cap = wav.shape[1] if isinstance(lengths, torch.Tensor) else int(lengths)
        x = wav
        for i, (up, down) in enumerate(passes):
            cap = ops.resample_out_len(cap, up, down)
            if i == len(passes) - 1:
                break
            mid = torch.empty(B, max(1, cap), device=wav.device, dtype=torch.float32)
            if isinstance(lengths, torch.Tensor):
                nxt = torch.empty(B, device=wav.device, dtype=torch.int32)
                ops.resample_poly(x, up, down, lengths=lengths, length_scale=length_scale,
                                  out=mid, out_lengths=nxt)
                lengths, length_scale = nxt, 1
            else:
                ops.resample_poly(x, up, down, lengths=lengths, out=mid)
                lengths = cap
            x = mid
        pcm = torch.empty(B, max(1, cap + tail), device=wav.device, dtype=torch.int16)
        if passes:
            up, down = passes[-1]
            return ops.resample_pcm16(x, up, down, volume, lengths=lengths,
                                      length_scale=length_scale, out=pcm)
        return ops.pcm16(x, volume, lengths=lengths, length_scale=length_scale, out=pcm)

    def infer_pcm(self, spkid, text, emo, *, duration_rate=1.0, pitch=1.0, sampling_rate=None,
                  volume=1.0, tail_silence=0.0, durations=None, token_scale=None,
                  target_frames=None, return_durations=False):
        """infer plus the output stage of VITSWrap.speaking (vits_wrap.py:
        186-197) on the device: pitch / sampling-rate resampling
        (ops.resample_poly), volume, clip and int16 conversion, tail silence.
        Only the int16 PCM is copied to the host.  In graph mode the post
        kernels are plain launches right behind the utterance graph, over the
        whole bucket, with the length read from the graph's y_len on the
        device; the one host sync stays the y_len read.  Draws from numpy's
        generator exactly as infer does.  On a CPU device: infer and the host
        chain.  ``durations`` / ``token_scale`` / ``target_frames`` /
        ``return_durations`` as in infer (the durations are then a fourth
        result).  Returns (pcm int16 [n], emo, n_model_samples)."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        ctl = self._controls(text.shape[0], durations, token_scale, target_frames,
                             return_durations)  # (refuses before anything is uploaded)
        x_length, text_t, emo, sid = self._inputs(spkid, text, emo)
        got = [] if return_durations else None
        pcm, n = self._infer_pcm_one(x_length, text_t, emo, sid, duration_rate, out, ctl, got)
        return (pcm, emo, n, got[0]) if return_durations else (pcm, emo, n)

    def infer_pcm_like(self, wav, spkid_src, spkid, text, emo, *, sampling_rate_in=None,
                       pitch=1.0, sampling_rate=None, volume=1.0, tail_silence=0.0,
                       return_durations=False):
        """``text`` spoken by ``spkid`` with the timing of the recording
        ``wav`` of speaker ``spkid_src`` saying it: an alignment graph replay
        (align's) whose durations are copied device to device into the
        controlled synthesis graph's ``given`` buffer, then that replay and
        infer_pcm's output stage.  The durations do not visit the host on
        the way; what comes back is what ``align`` followed by
        ``infer_pcm(durations=...)`` returns, sample for sample, with numpy's
        generator left in the same state.  The frame bucket comes from the
        recording's frame count, which the host knows.  Needs a ROCm GPU."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        text = np.ascontiguousarray(text)
        (dur, frames), = self._align_rows([wav], [spkid_src], [text], [emo], sampling_rate_in,
                                          0.0, device=True)
        x_length, text_t, emo, sid = self._inputs(spkid, text, emo)
        got = [] if return_durations else None
        pcm, n = self._infer_pcm_one(x_length, text_t, emo, sid, 1.0, out,
                                     (dur, None, 0, int(frames)), got)
        return (pcm, emo, n, got[0]) if return_durations else (pcm, emo, n)

    def _infer_pcm_one(self, x_length, text_t, emo, sid, duration_rate, out, ctl=None, got=None):
        """One utterance under the output controls ``out`` (_output): (pcm
        int16 [n] on the host, model samples)."""
        if self.device.type != "cuda":
            from . import vits_wrap

            wav = self._infer_one(x_length, text_t, emo, sid, duration_rate, ctl, got)
            pcm = vits_wrap.host_pcm(wav, self.sampling_rate, out.pitch, out.sampling_rate,
                                     out.volume, out.tail_silence)
            return pcm, len(wav)
        if self.graph and x_length <= 4096:
            pcm, n = self._infer_graph(
                text_t, emo, sid, duration_rate,
                post=lambda wav, y_len: self._post(wav, out, lengths=y_len,
                                                   length_scale=self.hop_size),
                ctl=ctl, got=got)
            n *= self.hop_size
        else:
            wav = self._infer_eager(x_length, text_t, emo, sid, duration_rate, ctl, got)
            n = wav.shape[-1]
            pcm = self._post(wav.reshape(1, -1), out, lengths=n)
        return pcm[0, :self._n_out(n, out.passes) + out.tail].cpu().numpy(), n

    # -- streaming: the front once, the decoder and the output stage per chunk (4w) --
    # the window buckets whose cores are the default first and later chunk
    # sizes (measured: profiles/stream_latency.txt)
    STREAM_FIRST_WINDOW, STREAM_WINDOW = 256, 2048
    STREAM_MIN_WINDOW = 64

    def _stream_sizes(self, first_chunk_frames, chunk_frames, ctx):
        """The core sizes of a streamed call: the given ones, or windows of
        STREAM_FIRST_WINDOW and STREAM_WINDOW frames less 2 * ctx of context.
        ValueError for a size below one frame."""
        first = (max(1, self.STREAM_FIRST_WINDOW - 2 * ctx) if first_chunk_frames is None
                 else int(first_chunk_frames))
        chunk = (max(first, self.STREAM_WINDOW - 2 * ctx) if chunk_frames is None
                 else int(chunk_frames))
        if first < 1 or chunk < 1:
            raise ValueError(f"streaming needs chunks of at least one frame, got first_chunk_frames"
                             f"={first}, chunk_frames={chunk}")
        return first, chunk

    @classmethod
    def _stream_bucket(cls, frames):
        """The window bucket of a decoder window: a power of two, at least
        STREAM_MIN_WINDOW."""
        return max(cls.STREAM_MIN_WINDOW, 1 << max(0, int(frames) - 1).bit_length())

    def _stream_plan(self, y_len, out, first_chunk_frames, chunk_frames, context):
        """The chunks of an utterance of ``y_len`` frames under the output
        controls ``out`` (_output), for decoder windows with ``context`` frames
        between an artificial edge and what must be exact
        (Generator.context_frames).  Chunk k owns the core frames [s_k, e_k):
        ``first_chunk_frames`` of them, then twice the last size up to
        ``chunk_frames``; the cores partition [0, y_len).  Its output span is
        the core's samples [s_k * hop, e_k * hop) taken forwards through the
        passes (n -> ceil(n * up / down), so the spans partition [0, n_out));
        the last chunk also owns the tail.  From the last pass back to the
        first, ops.resample_span_input gives the exact range of each pass's
        input that span needs; the frames that hold the first pass's range
        join the core, and the window is that with ``context`` frames on each
        side, cut at 0 and y_len: the utterance's own edges, where the
        whole-utterance decoder is cut too.  Host arithmetic only; ValueError
        for y_len, a chunk size below 1 or a negative context."""
        hop = self.hop_size
        y_len, first, chunk, ctx = (int(y_len), int(first_chunk_frames), int(chunk_frames),
                                    int(context))
        if y_len < 1 or first < 1 or chunk < 1 or ctx < 0:
            raise ValueError(f"no stream plan for {y_len} frames in chunks of {first} / {chunk} "
                             f"frames with {ctx} frames of context")
        passes = out.passes or [(1, 1)]
        lens = [y_len * hop]
        for up, down in passes:
            lens.append(ops.resample_out_len(lens[-1], up, down))
        plan, s, size = [], 0, first
        while s < y_len:
            e = min(y_len, s + size)
            lo, hi = s * hop, e * hop
            for up, down in passes:
                lo, hi = ops.resample_out_len(lo, up, down), ops.resample_out_len(hi, up, down)
            if e == y_len:
                hi += out.tail
            spans, need = [], (lo, hi)
            for i in reversed(range(len(passes))):
                src = ops.resample_span_input(need[0], need[1], lens[i], *passes[i])
                spans.append(src + need)
                need = src
            f_lo, f_hi = s, e
            if need[0] < need[1]:  # the frames under the first pass's input join the core
                f_lo, f_hi = min(s, need[0] // hop), max(e, -(-need[1] // hop))
            plan.append(_Chunk(s, e, max(0, f_lo - ctx), min(y_len, f_hi + ctx), lo, hi,
                               tuple(reversed(spans))))
            s, size = e, min(2 * size, chunk)
        return plan

    def infer_pcm_stream(self, spkid, text, emo, *, first_chunk_frames=None, chunk_frames=None,
                         duration_rate=1.0, pitch=1.0, sampling_rate=None, volume=1.0,
                         tail_silence=0.0, durations=None, token_scale=None, target_frames=None,
                         return_durations=False):
        """infer_pcm, streamed: a PcmStream whose int16 chunks, end to end,
        are the array infer_pcm returns for the same call, sample for sample
        (an fp16 model at the base config: to its decoder's rounding,
        DESIGN.md 4w), with numpy's generator left where infer_pcm leaves it.
        The text side runs ONCE, as a replay of the front graph (text
        encoder, durations, draw, prior expansion, reverse flow: cached under
        ("front", ...) beside the utterance graphs, same buckets and re-run);
        the host then reads y_len, the call's one extra sync, so the stream's
        ``n_samples``, ``n_model`` and ``durations`` are set when this call
        returns, before any audio exists.  Then, per chunk of _stream_plan:
        ops.copy_windows moves the window of z into the static input of the
        decode graph cached under ("dec", window bucket), the graph replays,
        the span passes of the output stage (ops.resample_poly_span /
        resample_pcm16_span) run behind it and one device-to-host copy brings
        the chunk's int16.  Chunk k + 1 is enqueued before chunk k's copy is
        waited for (two PCM buffers, an event per chunk; the stream is never
        synchronised).

        ``first_chunk_frames`` / ``chunk_frames``: the first core and the
        largest; the cores double in between.  Default: the cores of 256- and
        2048-frame windows.  ValueError below one frame.  graph=False or text
        past 4096 tokens: the same plan through the eager functions.  A CPU
        device: infer_pcm, sliced on the plan's boundaries.  The other
        arguments as in infer_pcm."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        ctx = self.model.dec.context_frames()
        first, chunk = self._stream_sizes(first_chunk_frames, chunk_frames, ctx)
        ctl = self._controls(text.shape[0], durations, token_scale, target_frames,
                             return_durations)  # (refuses before anything is uploaded)
        x_length, text_t, emo, sid = self._inputs(spkid, text, emo)
        return self._stream_one(x_length, text_t, emo, sid, duration_rate, out, ctl, first, chunk,
                                ctx)

    def infer_pcm_streams(self, items, *, first_chunk_frames=None, chunk_frames=None,
                          duration_rate=1.0, pitch=1.0, sampling_rate=None, volume=1.0,
                          tail_silence=0.0, batch=True):
        """infer_pcm_stream for items = [(spkid, text, emo), ...] that share
        their controls (the segments of a request): one PcmStream per item,
        whose chunks are what infer_pcm_batch returns for it.  EVERY front
        runs before this returns, so all lengths are known before any audio
        exists; ``batch``: groups of up to MAX_BATCH items as ONE replay of a
        batched front graph (the rows and draws of infer_pcm_batch), else one
        front replay per item.  The chunks of each stream are then decoded as
        it is iterated, in any order.  Emotion lookups and numpy's generator
        as infer_pcm_batch."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        ctx = self.model.dec.context_frames()
        first, chunk = self._stream_sizes(first_chunk_frames, chunk_frames, ctx)
        texts, spkids, emos = self._resolve_items(items)
        streams = []
        for lo, hi in self._groups(len(texts)):
            if not batch or hi - lo == 1 or not self._batchable(texts[lo:hi]):
                for i in range(lo, hi):
                    x_length, text_t, sid = self._one_tensors(spkids[i], texts[i])
                    streams.append(self._stream_one(x_length, text_t, emos[i], sid, duration_rate,
                                                    out, None, first, chunk, ctx))
                continue
            (z, g), y = self._infer_graph_batch(texts[lo:hi], emos[lo:hi], spkids[lo:hi],
                                                duration_rate, front=True)
            for i, n in enumerate(y):
                chunks = self._stream_latents(z[i:i + 1], g[i:i + 1], n, out, first, chunk, ctx)
                streams.append(PcmStream(
                    chunks, self._n_out(n * self.hop_size, out.passes) + out.tail,
                    n * self.hop_size, None, emos[lo + i]))
        return streams

    def _stream_one(self, x_length, text_t, emo, sid, duration_rate, out, ctl, first, chunk, ctx):
        """The front of one utterance, now, and the PcmStream of its chunks."""
        got = [] if ctl is not None else None
        hop = self.hop_size
        if self.device.type != "cuda":
            pcm, n = self._infer_pcm_one(x_length, text_t, emo, sid, duration_rate, out, ctl, got)
            y_len = n // hop
            plan = self._stream_plan(y_len, out, first, chunk, ctx)
            chunks = (pcm[c.out_lo:c.out_hi] for c in plan if c.out_hi > c.out_lo)
        else:
            if self.graph and x_length <= 4096:
                (z, g), y_len = self._infer_graph(text_t, emo, sid, duration_rate, ctl=ctl,
                                                  got=got, front=True)
            else:
                z, g = self._infer_eager(x_length, text_t, emo, sid, duration_rate, ctl, got,
                                         front=True)
                y_len = z.shape[2]
            chunks = self._stream_latents(z, g, y_len, out, first, chunk, ctx)
        return PcmStream(chunks, self._n_out(y_len * hop, out.passes) + out.tail, y_len * hop,
                         got[0] if got else None, emo)

    def _stream_latents(self, z, g, y_len, out, first, chunk, ctx):
        """The chunk generator over row 0 of a front's (z [., C, >= y_len], g):
        both are copied out of the graph's static buffers, so that another
        call on this engine between two chunks changes nothing."""
        z = z[:1, :, :y_len].float().clone(memory_format=torch.contiguous_format)
        return self._stream_chunks(z, g[:1].clone(), y_len,
                                   self._stream_plan(y_len, out, first, chunk, ctx), out)

    def _stream_chunks(self, z, g, y_len, plan, out):
        """The chunks of ``plan`` over z [1, C, y_len] (infer_pcm_stream
        documents the order of work)."""
        passes = out.passes or [(1, 1)]
        lens = [y_len * self.hop_size]
        for up, down in passes:
            lens.append(ops.resample_out_len(lens[-1], up, down))
        plan = [c for c in plan if c.out_hi > c.out_lo]
        cap = max([1] + [c.out_hi - c.out_lo for c in plan])
        dev = [torch.empty(cap, device=self.device, dtype=torch.int16) for _ in range(2)]
        host = [torch.empty(cap, dtype=torch.int16, pin_memory=True) for _ in range(2)]
        done = [torch.cuda.Event() for _ in range(2)]
        pending = None
        for k, c in enumerate(plan):
            slot, n = k % 2, c.out_hi - c.out_lo
            with torch.no_grad():
                self._stream_enqueue(z, g, c, passes, lens, out.volume, dev[slot])
                host[slot][:n].copy_(dev[slot][:n], non_blocking=True)
            done[slot].record(torch.cuda.current_stream(self.device))
            if pending is not None:
                done[pending[0]].synchronize()
                yield host[pending[0]][:pending[1]].numpy().copy()
            pending = (slot, n)
        if pending is not None:
            done[pending[0]].synchronize()
            yield host[pending[0]][:pending[1]].numpy().copy()

    def _stream_enqueue(self, z, g, c, passes, lens, volume, pcm):
        """Chunk c on the current stream: window copy, decoder, span passes;
        its int16 samples land in pcm[:c.out_hi - c.out_lo].  No sync."""
        hop, C = self.hop_size, self.inter_channels
        w = c.b - c.a
        W = self._stream_bucket(w)
        if self.graph:
            dec = self._cached_graph(("dec", W), lambda: self.model.capture_decode_window(W))
            z_win = dec.static["z"]
            dec.static["g"].copy_(g)
        else:
            z_win = torch.empty(1, C, W, device=self.device)
        ops.copy_windows(z, z_win, [(c.a, 0, w, W)], channels=C, src_rstride=z.shape[2],
                         dst_rstride=W)
        if self.graph:
            wav = dec(w)
        else:
            wav = self.model.decode_window_bucketed(
                z_win, torch.tensor([w], dtype=torch.int32, device=self.device), g)
        x, x_lo = wav.reshape(-1)[:w * hop], c.a * hop
        for i, (up, down) in enumerate(passes):
            o_lo, o_hi = c.passes[i][2:]
            if i == len(passes) - 1:
                ops.resample_pcm16_span(x, x_lo, lens[i], up, down, o_lo, o_hi - o_lo, volume,
                                        out=pcm)
            else:
                x = ops.resample_poly_span(x, x_lo, lens[i], up, down, o_lo, o_hi - o_lo)
                x_lo = o_lo

    # -- batched serving: all segments of a request in one utterance graph --------
    MAX_BATCH = 16
    BATCH_BUCKETS = (2, 4, 8, 16)

    @classmethod
    def _batch_bucket(cls, n):
        """The smallest batch bucket that holds n rows."""
        for b in cls.BATCH_BUCKETS:
            if n <= b:
                return b
        raise ValueError(f"{n} rows exceed the largest batch bucket {cls.BATCH_BUCKETS[-1]}")

    @classmethod
    def _groups(cls, n):
        """[(lo, hi)] consecutive groups of at most MAX_BATCH items, in order."""
        step = max(1, min(int(cls.MAX_BATCH), cls.BATCH_BUCKETS[-1]))
        return [(lo, min(lo + step, n)) for lo in range(0, n, step)]

    def _resolve_items(self, items):
        """All emotion lookups (their numpy draws) first, in item order; the
        noise draws follow in item order.  That is the order of a
        VITSWrap.speaking request, whose first segment looks the emotion up
        and whose later segments reuse the returned tensor."""
        items = list(items)
        resolved = [self._resolve(spkid, emo) for spkid, _, emo in items]
        texts = [np.ascontiguousarray(text) for _, text, _ in items]
        return texts, [s for s, _ in resolved], [e for _, e in resolved]

    def _batchable(self, texts):
        return self.graph and self.device.type == "cuda" and max(t.shape[0] for t in texts) <= 4096

    def _one_tensors(self, spkid, text):
        sid = torch.tensor([spkid], dtype=torch.long, device=self.device)
        return text.shape[0], torch.from_numpy(text).to(self.dtype).to(self.device).unsqueeze(0), sid

    def _item_controls(self, items, durations, token_scale, target_frames, want=False):
        """_controls of every item of a batch call (per-item lists or None),
        checked before any item is looked up or uploaded."""
        n = len(items)
        cols = []
        for name, v in (("durations", durations), ("token_scale", token_scale),
                        ("target_frames", target_frames)):
            v = [None] * n if v is None else list(v)
            if len(v) != n:
                raise ValueError(f"{name}: need one entry per item ({n}), got {len(v)}")
            cols.append(v)
        return [self._controls(np.shape(items[i][1])[0], cols[0][i], cols[1][i], cols[2][i], want)
                for i in range(n)]

    def _one_by_one(self, spkids, texts, emos, rates, ctls, outs, want):
        """The rows of a group that is not batched (a single row, a CPU
        device, graph=False), one after another on infer's path, or on
        infer_pcm's under ``outs`` (one _output per row; None: waveforms).
        Returns the lists (samples, model samples or None, durations or None
        without ``want``), one entry per row."""
        res = []
        for i, (spkid, text) in enumerate(zip(spkids, texts)):
            x_length, text_t, sid = self._one_tensors(spkid, text)
            got = [] if want else None
            if outs is None:
                pcm, n = self._infer_one(x_length, text_t, emos[i], sid, rates[i], ctls[i],
                                         got), None
            else:
                pcm, n = self._infer_pcm_one(x_length, text_t, emos[i], sid, rates[i], outs[i],
                                             ctls[i], got)
            res.append((pcm, n, got[0] if want else None))
        return [list(col) for col in zip(*res)]

    # The packed buffer of a group: ONE int16 tensor that one device-to-host
    # copy brings over.  In front of the samples stand the int32 words
    #   [offsets (B + 1) | y_len (B) | status (B) | used_total (1) | extra]
    # (extra: the durations [B, text bucket] of a controlled group, else
    # nothing), rounded up to 16 bytes: _header int16 elements.  Behind them,
    # row after row at a stride of (numel - header) / B, the rows' PCM, of
    # which samples [header, header + offsets[n]) are the n rows back to back
    # (ops.pack_pcm / pack_pcm_rows write the offsets and move the samples).
    # _pack writes the words, _unpack copies and reads them; no other code
    # knows the layout.
    @staticmethod
    def _header(B, extra=0):
        """int16 elements in front of a packed group's samples."""
        return -(-2 * (3 * B + 2 + extra) // 8) * 8

    @classmethod
    def _pack(cls, B, pack, words, extra=None):
        """The packed buffer of a group: ``pack(header)`` -> the int16 buffer
        with its offsets and samples in place (a pack kernel), then ``words``
        = (y_len [B], status [B], used_total [1]) and ``extra`` (int32, or
        None) behind the offsets."""
        n_extra = 0 if extra is None else extra.numel()
        out = pack(cls._header(B, n_extra))
        torch.cat(words, out=out[2 * (B + 1):2 * (3 * B + 2)].view(torch.int32))
        if n_extra:
            out[2 * (3 * B + 2):2 * (3 * B + 2 + n_extra)].view(torch.int32).copy_(
                extra.reshape(-1))
        return out

    def _unpack(self, packed, bb, n, n_extra=0):
        """The first n rows of a packed buffer of batch bucket bb on the host,
        after its ONE copy (_to_host; the padding rows hold nothing and stay
        behind): (samples int16 [offsets[n]], offsets int32 [n + 1], y_len
        list [n], status list [n], used_total, extra int32 [n_extra] or
        None)."""
        header = self._header(bb, n_extra)
        row_cap = (packed.numel() - header) // bb
        buf = self._to_host(packed[:header + n * row_cap])
        w = buf[:2 * (3 * bb + 2 + n_extra)].view(np.int32)
        offs = w[:n + 1]
        y, status = w[bb + 1:bb + 1 + n].tolist(), w[2 * bb + 1:2 * bb + 1 + n].tolist()
        return (buf[header:header + int(offs[n])], offs, y, status, int(w[3 * bb + 1]),
                w[3 * bb + 2:] if n_extra else None)

    def infer_batch(self, items, *, duration_rate=1.0, durations=None, token_scale=None,
                    target_frames=None, return_durations=False):
        """infer for items = [(spkid, text [N, c], emo), ...]: [(wav float32
        [n], emo), ...], bit for bit what a loop over infer returns for emo
        tensors (see _resolve_items for the order of numpy draws otherwise),
        with numpy's generator left where the loop leaves it.  Groups of up
        to MAX_BATCH items run as ONE replay of a batched utterance graph
        (batch buckets 2, 4, 8, 16); a single item, a CPU device or
        graph=False run infer's path per item.  ``durations`` /
        ``token_scale`` / ``target_frames``: per-item lists (None entries:
        no control) as in infer; a control on any row of a group routes the
        group to a graph cached under ("ctl", batch bucket, text bucket,
        frame bucket).  ``return_durations``: (wav, emo, durations) tuples."""
        items = list(items)
        ctls = self._item_controls(items, durations, token_scale, target_frames, return_durations)
        texts, spkids, emos = self._resolve_items(items)
        if not texts:
            return []
        out = []
        for lo, hi in self._groups(len(texts)):
            if hi - lo == 1 or not self._batchable(texts[lo:hi]):
                wavs, _, durs = self._one_by_one(
                    spkids[lo:hi], texts[lo:hi], emos[lo:hi], [duration_rate] * (hi - lo),
                    ctls[lo:hi], None, return_durations)
            else:
                durs = []
                wav, y = self._infer_graph_batch(texts[lo:hi], emos[lo:hi], spkids[lo:hi],
                                                 duration_rate, ctls=ctls[lo:hi], got=durs)
                hop = self.hop_size
                host = wav[:hi - lo, 0, :max(y) * hop].cpu()  # one copy for the group
                wavs = [host[i, :n * hop].float().numpy() for i, n in enumerate(y)]
            out += [(w, emos[lo + i]) + ((durs[i],) if return_durations else ())
                    for i, w in enumerate(wavs)]
        return out

    def infer_pcm_batch(self, items, *, duration_rate=1.0, pitch=1.0, sampling_rate=None,
                        volume=1.0, tail_silence=0.0, durations=None, token_scale=None,
                        target_frames=None, return_durations=False):
        """infer_pcm for items = [(spkid, text, emo), ...] that share one
        rate, pitch, sampling rate, volume and tail: (pcm int16 [total],
        offsets int64 [len + 1], emos, n_model list).  Item i's PCM, its tail
        silence included, is pcm[offsets[i]:offsets[i + 1]], sample for
        sample what infer_pcm returns; numpy's generator ends where the loop
        over infer_pcm leaves it.  A group of up to MAX_BATCH items is one
        graph replay, the post passes over all its rows, the ragged pack
        (ops.pack_pcm) and ONE device-to-host copy with the one host sync:
        offsets, lengths and draw status arrive in front of the samples.
        ``durations`` / ``token_scale`` / ``target_frames``: per-item lists
        as in infer_batch; a controlled group's final durations ride in the
        same copy, behind the header words, and come back as a fifth result
        (a list of int32 arrays) with ``return_durations``."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        items = list(items)
        ctls = self._item_controls(items, durations, token_scale, target_frames, return_durations)
        texts, spkids, emos = self._resolve_items(items)
        chunks, offsets, n_model, durs = [], [0], [], []
        for lo, hi in self._groups(len(texts)):
            if hi - lo == 1 or not self._batchable(texts[lo:hi]):
                pcms, ns, ds = self._one_by_one(
                    spkids[lo:hi], texts[lo:hi], emos[lo:hi], [duration_rate] * (hi - lo),
                    ctls[lo:hi], [out] * (hi - lo), return_durations)
                chunks += pcms
                offsets += (offsets[-1] + np.cumsum([len(p) for p in pcms])).tolist()
                n_model += ns
                durs += ds
                continue
            (pcm, offs), y = self._infer_graph_batch(
                texts[lo:hi], emos[lo:hi], spkids[lo:hi], duration_rate,
                post=lambda wav, y_len, n_rows, words, extra: self._post_pack(
                    wav, y_len, n_rows, words, out, extra),
                ctls=ctls[lo:hi], got=durs)
            chunks.append(pcm)
            offsets += [offsets[-1] + int(o) for o in offs[1:]]
            n_model += [n * self.hop_size for n in y]
        pcm = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int16)
        res = (pcm, np.asarray(offsets, dtype=np.int64), emos, n_model)
        return res + (durs,) if return_durations else res

    def _post_pack(self, wav, y_len, n_rows, words, out, extra=None):
        """The post passes (_post under ``out``) over every row of the
        bucket, then the ragged pack into the packed buffer (_pack)."""
        rows = self._post(wav, out, lengths=y_len, length_scale=self.hop_size)
        return self._pack(
            wav.shape[0],
            lambda header: ops.pack_pcm(rows, y_len, self.hop_size, out.passes, out.tail,
                                        n_rows=n_rows, header=header)[0],
            words, extra)

    # -- mixed requests: rows with their own speed, pitch, rate, volume, tail ------
    def infer_pcm_requests(self, requests, *, return_durations=False):
        """infer_pcm_batch for several requests at once, each a PcmRequest
        with its own controls: one (pcm, offsets, emos, n_model) per request,
        what ``infer_pcm_batch(r.items, **controls)`` returns for it when the
        calls are made in order, with numpy's generator left in the same
        state.  Order of numpy draws: every request's emotion lookups first,
        in request and item order, then the noise draws in row order
        (_resolve_items' rule over the whole call; the in-order loop's
        exactly when the emotions are tensors or explicit ids).

        The rows of all requests are flattened in order and cut into groups
        of at most MAX_BATCH.  A group is ONE replay of a rate-free batched
        graph (the speeds are a device input, so one graph per (batch, text,
        frame) bucket serves every speed and pitch), then as many per-row
        post launches as the row with the most passes needs
        (ops.resample_rows: a row with fewer passes copies in the slot it
        does not use), the per-row pack (ops.pack_pcm_rows) and ONE
        device-to-host copy.  A group of one row, a CPU device or graph=False
        run infer_pcm's path per row.  A request's ``durations`` /
        ``token_scale`` / ``target_frames`` (per-item lists) control its
        rows as in infer_pcm_batch; controlled and plain rows share a group.
        ``return_durations``: a fifth entry per request, its rows' durations."""
        requests = list(requests)
        row_ctl = []
        for r in requests:  # every check before any lookup or upload
            row_ctl += self._item_controls(list(r.items), r.durations, r.token_scale,
                                           r.target_frames, return_durations)
        rows, spans = [], []  # per row: (text, spkid, emo, request); per request: (lo, hi, emos)
        for r in requests:
            texts, spkids, emos = self._resolve_items(r.items)
            spans.append((len(rows), len(rows) + len(texts), emos))
            rows += [(t, s, e, r) for t, s, e in zip(texts, spkids, emos)]
        pcms, n_model, durs = [], [], []
        for lo, hi in self._groups(len(rows)):
            texts, spkids, emos, reqs = (list(col) for col in zip(*rows[lo:hi]))
            rates = [r.duration_rate for r in reqs]
            outs = [self._output(r.pitch, r.sampling_rate, r.volume, r.tail_silence)
                    for r in reqs]
            if hi - lo == 1 or not self._batchable(texts):
                got = self._one_by_one(spkids, texts, emos, rates, row_ctl[lo:hi], outs,
                                       return_durations)
                pcms += got[0]
                n_model += got[1]
                durs += got[2]
                continue
            (pcm, offs), y = self._infer_graph_batch(
                texts, emos, spkids, None, rates=rates,
                post=lambda wav, y_len, n_rows, words, extra: self._post_pack_rows(
                    wav, y_len, n_rows, words, outs, extra),
                ctls=row_ctl[lo:hi], got=durs)
            pcms += [pcm[int(offs[i]):int(offs[i + 1])] for i in range(hi - lo)]
            n_model += [n * self.hop_size for n in y]
        out = []
        for lo, hi, emos in spans:
            offsets = np.cumsum([0] + [len(p) for p in pcms[lo:hi]]).astype(np.int64)
            pcm = np.concatenate(pcms[lo:hi]) if hi > lo else np.zeros(0, dtype=np.int16)
            out.append((pcm, offsets, emos, n_model[lo:hi])
                       + ((durs[lo:hi],) if return_durations else ()))
        return out

    def _post_pack_rows(self, wav, y_len, n_rows, words, outs, extra=None):
        """_post_pack with per-row controls: ``outs``, the _output of each of
        the group's rows (the padding rows of the bucket copy at volume 1
        with no tail).  max(1, most passes of a row) launches of
        ops.resample_rows: the last one writes the PCM, the ones before it
        fp32 and the lengths; a row's passes fill the first slots, (1, 1)
        the rest, which leaves its samples as they are."""
        B = wav.shape[0]
        pad = B - len(outs)
        passes = [o.passes for o in outs] + [[]] * pad
        volumes = [o.volume for o in outs] + [1.0] * pad
        tails = [o.tail for o in outs] + [0] * pad
        n_launch = max(1, max(len(p) for p in passes))
        x, lengths, scale = wav, y_len, self.hop_size
        caps = [wav.shape[1]] * B
        for i in range(n_launch):
            ratios = [p[i] if i < len(p) else (1, 1) for p in passes]
            caps = [ops.resample_out_len(c, u, d) for c, (u, d) in zip(caps, ratios)]
            if i == n_launch - 1:
                break
            mid = torch.empty(B, max(1, max(caps)), device=wav.device, dtype=torch.float32)
            nxt = torch.empty(B, device=wav.device, dtype=torch.int32)
            ops.resample_rows(x, ratios, lengths=lengths, length_scale=scale, out=mid,
                              out_lengths=nxt)
            x, lengths, scale = mid, nxt, 1
        pcm = torch.empty(B, max(1, max(caps) + max(tails)), device=wav.device, dtype=torch.int16)
        ops.resample_rows(x, ratios, lengths=lengths, length_scale=scale, volumes=volumes,
                          pcm=True, out=pcm)
        return self._pack(
            B, lambda header: ops.pack_pcm_rows(pcm, y_len, self.hop_size, passes, tails,
                                                n_rows=n_rows, header=header)[0],
            words, extra)

    def _to_host(self, t):
        """One device-to-host copy of t through a reused pinned buffer, and
        the host sync that completes it."""
        n = t.numel()
        buf = self._pinned.get(t.dtype)
        if buf is None or buf.numel() < n:
            buf = self._pinned[t.dtype] = torch.empty(max(n, 1 << 16), dtype=t.dtype,
                                                      pin_memory=True)
        buf[:n].copy_(t.reshape(-1), non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return buf[:n].numpy().copy()

    def _infer_graph_batch(self, texts, emos, spkids, duration_rate, post=None, rates=None,
                           ctls=None, got=None, front=False):
        """2..16 utterances as one replay of a batched utterance graph, cached
        with the B = 1 graphs per (batch bucket, text bucket, frame bucket,
        rate); with ``rates`` (one speed per row; ``duration_rate`` unused)
        a rate-free graph whose speeds are a device input, cached per
        ("rows", batch bucket, text bucket, frame bucket) for every speed.
        The noise starts are drawn on the device in row order from ONE pool
        of raw words of numpy's generator (ops.draw_starts), so they and the
        generator's final state are those of consecutive infer calls.
        Returns (wav [B, 1, frames * hop] on the device, y_len list), or with
        ``post(wav [B, frames * hop], y_len, n_rows, (y_len, status,
        used_total), extra)`` -> the packed buffer (_pack): ((pcm, offsets),
        y_len list) on the host after its single copy.  A row longer than the
        frame bucket re-runs the group at a larger bucket (same draws), an
        exhausted pool re-runs it with a pool twice as long.

        ``ctls`` (per row: the result of _controls, or None) with a control
        on any row: the group replays a controlled, rate-free graph cached
        under ("ctl", batch bucket, text bucket, frame bucket); rows without
        a control get the neutral one.  The frame bucket is at least what the
        rows whose total the host knows need.  The final durations [B, text
        bucket] ride behind the header words of the packed buffer (``post``
        gets them as ``extra``, None for a plain group), or with the words when
        there is no post, and row i's int32 [t_x_i] is appended to ``got``.

        ``front`` (no post): the group replays the batched front graph
        (capture_infer_front_bucketed, cached under ("front",) + the key above)
        and ((z [B, C, frames], g [B, gin]), y_len list) is returned, views of
        the graph's static buffers."""
        n = len(texts)
        controlled = ctls is not None and any(c is not None for c in ctls)
        if controlled and rates is None:
            rates = [duration_rate] * n
        bb = self._batch_bucket(n)
        lengths = [t.shape[0] for t in texts]
        xb = self._text_bucket(max(lengths))
        x = self._text_rows(texts, lengths)
        emo = torch.cat(emos)
        sid = torch.tensor(spkids, dtype=torch.long)
        pool_mult = 1
        memo = (bb, xb, duration_rate) if rates is None else ("rows", bb, xb)
        control, known = None, 0
        if controlled:
            memo = ("ctl", bb, xb)
            rows = [c if c is not None else (None, None, 0, None) for c in ctls]
            control = dict(given=[c[0] for c in rows], tok_scale=[c[1] for c in rows],
                           target=[c[2] for c in rows])
            known = max([c[3] or 0 for c in rows])
        n_extra = bb * xb if controlled else 0
        while True:
            tyb = self._ty_bucket.get(memo, 256)
            if known > tyb:
                tyb = self._frame_bucket(known)
            key = (bb, xb, tyb, float(duration_rate)) if rates is None else ("rows", bb, xb, tyb)
            if controlled:
                key = ("ctl", bb, xb, tyb)
            if front:
                key = ("front",) + key
            run = self._cached_graph(key, lambda: self._capture_synthesis(
                xb, tyb, front=front, batch=bb, control=controlled,
                length_scale=duration_rate if rates is None else torch.ones(bb)))
            pool, state = ops.numpy_draw_pool(run.pool_len * pool_mult)
            if pool_mult == 1:
                res = run(x, emo, sid, lengths, pool, n, rates=rates, control=control)
            else:
                # the graph's pool is static: the (p < 2^-32 per row) longer
                # pool runs the same kernels eagerly on the graph's inputs
                st = run.static
                infer = self.model.infer_front_bucketed if front else self.model.infer_bucketed
                res = infer(
                    st["x"], st["emo"], st["sid"], st["noise"], tyb, x_lengths=st["xl"],
                    length_scale=duration_rate if rates is None else st["rates"],
                    noise_start=torch.from_numpy(pool).to(self.device), n_rows=st["n_rows"],
                    control={k: st[k] for k in ("given", "tok_scale", "target")}
                    if controlled else None)
            if front:
                head, res = res[:2], res[1:]
            wav, words, dur = res[0], res[1:4], res[4] if controlled else None
            if post is None:
                host = torch.cat(words + ((dur.reshape(-1),) if controlled else ())).tolist()
                y, st_rows, used, d = host[:n], host[bb:bb + n], host[2 * bb], host[2 * bb + 1:]
            else:
                packed = post(wav[:, 0], words[0], run.static["n_rows"], words, dur)
                pcm, offs, y, st_rows, used, d = self._unpack(packed, bb, n, n_extra)
            if max(y) > tyb:
                self._grow_bucket(memo, state, tyb, max(y))  # same draws
                continue
            if -2 in st_rows:
                np.random.set_state(state)
                pool_mult *= 2
                continue
            if -1 in st_rows:
                raise self._misfit(state, y[st_rows.index(-1)])
            ops.numpy_draw_commit(state, used)
            if controlled and got is not None:
                d = np.asarray(d, np.int32).reshape(bb, xb)
                got += [d[i, :lengths[i]].copy() for i in range(n)]
            if front:
                return head, y
            return (wav, y) if post is None else ((pcm, offs), y)

    # -- voice conversion: waveform in, waveform out --------------------------------
    # frame buckets of the conversion graphs: powers of two, 256 .. 4096
    VC_MIN_FRAMES, VC_MAX_FRAMES = 256, 4096

    def _vc_stft(self):
        """(filter_length, hop_length, win_length) of the data config."""
        d = self.hps.data
        missing = [k for k in ("filter_length", "hop_length", "win_length") if k not in d]
        if missing:
            raise ValueError(f"voice conversion needs data.{', data.'.join(missing)} in the config")
        return int(d["filter_length"]), int(d["hop_length"]), int(d["win_length"])

    def _map_spkid(self, spkid):
        spkid = self.spkid_mapping.get(spkid, spkid)  # (the mapping of _resolve)
        assert spkid < self.num_speaker, f"spkid={spkid} must be less than {self.num_speaker}"
        return int(spkid)

    @classmethod
    def _vc_bucket(cls, frames):
        """The smallest frame bucket (a power of two, 256 .. 4096) holding ``frames``."""
        if frames > cls.VC_MAX_FRAMES:
            raise ValueError(f"recording of {frames} frames exceeds the largest conversion bucket "
                             f"of {cls.VC_MAX_FRAMES} frames (chunk it)")
        return cls._frame_bucket(frames)

    def _vc_plan(self, n_in, sampling_rate_in=None):
        """Host arithmetic of one recording of n_in samples at sampling_rate_in
        (None: the model's rate): ((up, down) of the input resampling or None,
        samples at the model rate, frames, frame bucket).  Raises ValueError
        for a recording of at most pad = (n_fft - hop) / 2 samples (the
        reflect padding needs more) or of more than 4096 frames."""
        ratio, n, frames = self._vc_lengths(n_in, sampling_rate_in)
        return ratio, n, frames, self._vc_bucket(frames)

    def _vc_lengths(self, n_in, sampling_rate_in=None):
        """_vc_plan without the bucket, so without the cap of 4096 frames."""
        n_fft, hop, _ = self._vc_stft()
        ratio, n = None, int(n_in)
        if sampling_rate_in is not None and int(sampling_rate_in) != self.sampling_rate:
            ratio = ops.resample_ratio(int(sampling_rate_in), self.sampling_rate)
            n = ops.resample_out_len(n, *ratio)
        pad = (n_fft - hop) // 2
        if n <= pad:
            raise ValueError(f"recording of {n} samples at {self.sampling_rate} Hz is too short: "
                             f"voice conversion needs more than {pad}")
        return ratio, n, n // hop

    def _vc_input(self, wav, sampling_rate_in, capped=True):
        """One recording on the device at the model rate: (fp32 [n], frames,
        bucket).  int16 is scaled by 1 / 32768 (data_utils), floats are taken
        as they are; another rate takes one ops.resample_poly pass (the host
        knows every length: no sync).  ``capped=False`` (convert_long): any
        number of frames, and None for the bucket."""
        wav = np.asarray(wav).reshape(-1)
        ratio, n, frames = self._vc_lengths(wav.shape[0], sampling_rate_in)
        bucket = self._vc_bucket(frames) if capped else None
        if wav.dtype == np.int16:
            x = torch.from_numpy(wav.astype(np.float32) / 32768.0)
        elif np.issubdtype(wav.dtype, np.floating):
            x = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
        else:
            raise ValueError(f"wav must be int16 or float, got {wav.dtype}")
        x = x.to(self.device)
        if ratio is not None:
            x = ops.resample_poly(x, *ratio)
            assert x.numel() >= n
            x = x[:n]
        return x, frames, bucket

    def _vc_begin(self, what):
        """The recording paths (``what``: convert, align) need a ROCm GPU and
        the STFT parameters of the data config, which this returns."""
        if self.device.type != "cuda":
            raise ops._lib.VitsAmdError(f"EmoVITS.{what}: the vits_amd inference path runs on a "
                                        f"ROCm GPU only (got {self.device})")
        return self._vc_stft()

    def _vc_upload(self, wavs, sampling_rate_in, noise_scale):
        """1 .. MAX_BATCH recordings on the device (_vc_input each): (fp32
        [n, longest] rows, zero past their ends; samples per row; frames per
        row; the frame bucket of the longest; the batch bucket, 1 for one
        row; the posterior noise [n, C, frame bucket] drawn from the device
        generator this object owns and scaled, or None at noise_scale 0)."""
        rows = [self._vc_input(w, sampling_rate_in) for w in wavs]
        frames = [f for _, f, _ in rows]
        tyb = max(b for _, _, b in rows)
        n = len(rows)
        bb = 1 if n == 1 else self._batch_bucket(n)
        lens = [x.numel() for x, _, _ in rows]
        x = torch.zeros(n, max(lens), device=self.device)
        for i, (r, _, _) in enumerate(rows):
            x[i, :lens[i]] = r
        noise = None
        if noise_scale > 0:
            if self._vc_gen is None:
                self._vc_gen = torch.Generator(device=self.device)
            noise = torch.randn(n, self.inter_channels, tyb, device=self.device,
                                generator=self._vc_gen) * float(noise_scale)
        return x, lens, frames, tyb, bb, noise

    def _pad_rows(self, v, bb, width=None, dtype=None):
        """An input of the eager (graph=False) bucketed calls, zero-padded to
        the batch bucket by hand: a tensor [n, w, ...] -> [bb, width or w,
        ...]; with ``dtype`` a list of n ints -> a [bb] device tensor; None
        stays None."""
        if v is None:
            return None
        if dtype is not None:
            return torch.tensor(list(v) + [0] * (bb - len(v)), dtype=dtype).to(self.device)
        out = torch.zeros((bb, width or v.shape[1]) + tuple(v.shape[2:]), device=self.device,
                          dtype=v.dtype)
        out[:v.shape[0], :v.shape[1]] = v
        return out

    def _convert_rows(self, wavs, srcs, tgts, sampling_rate_in, noise_scale, post=None):
        """1 .. MAX_BATCH recordings through one conversion graph, cached in
        self._graphs under ("vc", batch bucket, frame bucket) (graph=False:
        the same convert_bucketed call, eagerly).  Returns (wav_out [B, 1,
        bucket * hop] fp32 on the device, frames list), or with ``post(wav
        [B, bucket * hop], y_len int32 [B])`` its result in place of the
        waveform.  No host sync: the host knows every length."""
        stft = self._vc_begin("convert")
        x, lens, frames, tyb, bb, noise = self._vc_upload(wavs, sampling_rate_in, noise_scale)
        src = [self._map_spkid(s) for s in srcs]
        tgt = [self._map_spkid(s) for s in tgts]
        if self.graph:
            run = self._cached_graph(("vc", bb, tyb), lambda: self.model.capture_convert_bucketed(
                tyb, batch=bb, stft=stft))
            out, y_len = run(x, lens, src, tgt, noise)
        else:
            pad = self._pad_rows
            out, y_len = self.model.convert_bucketed(
                pad(x, bb, tyb * stft[1] + stft[1] - 1), pad(lens, bb, dtype=torch.int32),
                pad(src, bb, dtype=torch.long), pad(tgt, bb, dtype=torch.long), pad(noise, bb),
                tyb, stft=stft)
        if post is not None:
            return post(out[:, 0], y_len), frames
        return out, frames

    def convert(self, wav, spkid_src, spkid_tgt, *, sampling_rate_in=None, noise_scale=0.0):
        """Voice conversion: the recording ``wav`` (int16, scaled by 1 /
        32768, or float in [-1, 1]; at ``sampling_rate_in``, default the
        model's rate) of speaker spkid_src in the voice of spkid_tgt, as a
        float32 waveform of (n // hop) * hop samples at the model's rate (n:
        the samples at that rate).  One replay of a cached graph per call;
        noise_scale > 0 samples the posterior (torch.randn on the device from
        the generator this object owns), 0 takes its mean.  Raises
        ValueError for a recording of more than 4096 frames or of at most
        (n_fft - hop) / 2 samples, VitsAmdError on a CPU device."""
        out, frames = self._convert_rows([wav], [spkid_src], [spkid_tgt], sampling_rate_in,
                                         noise_scale)
        return out[0, 0, :frames[0] * self.hop_size].cpu().numpy()

    def convert_pcm(self, wav, spkid_src, spkid_tgt, *, sampling_rate_in=None, noise_scale=0.0,
                    pitch=1.0, sampling_rate=None, volume=1.0, tail_silence=0.0):
        """convert plus infer_pcm's output stage on the device (pitch /
        sampling-rate resampling, volume, clip, int16, tail silence), the
        length read from the graph's y_len; one device-to-host copy, of the
        int16 PCM.  Returns (pcm int16 [n], n_model_samples)."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        pcm, frames = self._convert_rows(
            [wav], [spkid_src], [spkid_tgt], sampling_rate_in, noise_scale,
            post=lambda w, y_len: self._post(w, out, lengths=y_len, length_scale=self.hop_size))
        n = frames[0] * self.hop_size
        return pcm[0, :self._n_out(n, out.passes) + out.tail].cpu().numpy(), n

    def convert_pcm_batch(self, items, *, sampling_rate_in=None, noise_scale=0.0, pitch=1.0,
                          sampling_rate=None, volume=1.0, tail_silence=0.0):
        """convert_pcm for items = [(wav, spkid_src, spkid_tgt), ...] that
        share the controls: (pcm int16 [total], offsets int64 [len + 1],
        n_model list); item i's PCM, tail included, is
        pcm[offsets[i]:offsets[i + 1]], byte for byte what convert_pcm returns
        (at noise_scale 0; a draw's shape follows the batch).  A group of up
        to MAX_BATCH items (batch buckets 2, 4, 8, 16) is one graph replay,
        the post passes over its rows, the ragged pack and ONE device-to-host
        copy."""
        items = list(items)
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        chunks, offsets, n_model = [], [0], []
        for lo, hi in self._groups(len(items)):
            if hi - lo == 1:
                pcm, n = self.convert_pcm(*items[lo], sampling_rate_in=sampling_rate_in,
                                          noise_scale=noise_scale, pitch=pitch,
                                          sampling_rate=out.sampling_rate, volume=volume,
                                          tail_silence=tail_silence)
                chunks.append(pcm)
                offsets.append(offsets[-1] + len(pcm))
                n_model.append(n)
                continue
            n = hi - lo
            bb = self._batch_bucket(n)

            def post(w, y_len):
                zeros = torch.zeros(bb + 1, device=w.device, dtype=torch.int32)
                return self._post_pack(w, y_len, n, (y_len, zeros[:bb], zeros[bb:]), out)

            packed, frames = self._convert_rows(
                [w for w, _, _ in items[lo:hi]], [s for _, s, _ in items[lo:hi]],
                [t for _, _, t in items[lo:hi]], sampling_rate_in, noise_scale, post=post)
            pcm, offs = self._unpack(packed, bb, n)[:2]
            chunks.append(pcm)
            offsets += [offsets[-1] + int(o) for o in offs[1:]]
            n_model += [f * self.hop_size for f in frames]
        pcm = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int16)
        return pcm, np.asarray(offsets, dtype=np.int64), n_model

    # -- long recordings: overlapping windows, seamless cores --------
    # the frame bucket of a window (measured: profiles/vc_long_latency.txt)
    LONG_WINDOW_FRAMES = 4096
    # the resampler and the output stage carry every length as a C int
    LONG_MAX_SAMPLES = 2 ** 31 - 1

    def _long_plan(self, n, window_frames, context):
        """The windows of a recording of n samples at the model rate, F = n //
        hop frames, for rows of ``window_frames`` frames with ``context``
        frames between an artificial edge and the core: Cf = window_frames -
        2 * context core frames per window (ValueError when Cf < 1).  Window
        w owns the core frames [w * Cf, min((w + 1) * Cf, F)) and its row
        spans the frames [a, b) = [max(0, w * Cf - context), min(F, (w + 1) *
        Cf + context)), the samples [a * hop, b * hop); a row that reaches
        the last frame (b == F: the last window, and every earlier one whose
        right context does) runs to sample n, so the remainder and the
        reflection at the true end are the whole recording's, as those at
        the true start are the rows' with a == 0.  (A row with b == F cut at
        F * hop would fold its reflection n % hop samples early: an
        artificial edge with no context behind it.)  W = ceil(F / Cf)
        windows, none empty.  Host arithmetic only."""
        hop = self.hop_size
        n, wf, ctx = int(n), int(window_frames), int(context)
        cf = wf - 2 * ctx
        if ctx < 0 or cf < 1:
            raise ValueError(f"windows of {wf} frames leave no core beside 2 x {ctx} frames of "
                             "context")
        F = n // hop
        plan = []
        for w in range(-(-F // cf)):
            lo, hi = w * cf, min((w + 1) * cf, F)
            a, b = max(0, lo - ctx), min(F, (w + 1) * cf + ctx)
            plan.append(_Window(lo, hi, a, b, a * hop, n if b == F else b * hop, (lo - a) * hop))
        return plan

    def _long_check(self, n_in, sampling_rate_in, out=None):
        """The host arithmetic of a long recording, before anything is
        uploaded: its frames at the model rate.  ValueError for what
        _vc_lengths refuses, and for a recording whose samples, at the input
        rate, at the model rate or after any pass of the output stage
        ``out`` (tail included), exceed LONG_MAX_SAMPLES."""
        n_in = int(n_in)
        worst, frames = n_in, 0
        if n_in <= self.LONG_MAX_SAMPLES:
            _, n, frames = self._vc_lengths(n_in, sampling_rate_in)
            worst = max(worst, n)
            if out is not None:
                m = frames * self.hop_size
                for up, down in out.passes:
                    m = ops.resample_out_len(m, up, down)
                    worst = max(worst, m)
                worst = max(worst, m + out.tail)
        if worst > self.LONG_MAX_SAMPLES:
            raise ValueError(f"recording of {n_in} samples comes to {worst} at some stage: the "
                             f"resampler and the output stage take at most "
                             f"{self.LONG_MAX_SAMPLES} per row")
        return frames

    def _convert_windows(self, wav, spkid_src, spkid_tgt, sampling_rate_in, noise_scale,
                         window_frames, context):
        """A recording of any length, uploaded once (_vc_input without the
        cap), through the windows of _long_plan (_run_windows): (the stitched
        waveform fp32 [1, max(1, F * hop)] on the device, F).  A recording of
        at most window_frames frames is ONE window, the whole of it, with no
        artificial edge.  noise_scale > 0: ONE [C, F] posterior draw for the
        whole recording from the generator this object owns."""
        stft = self._vc_begin("convert_long")
        wf = self.LONG_WINDOW_FRAMES if window_frames is None else int(window_frames)
        if not self.VC_MIN_FRAMES <= wf <= self.VC_MAX_FRAMES or self._frame_bucket(wf) != wf:
            raise ValueError(f"window_frames must be a conversion bucket (a power of two, "
                             f"{self.VC_MIN_FRAMES} .. {self.VC_MAX_FRAMES}), got {wf}")
        x, F, _ = self._vc_input(wav, sampling_rate_in, capped=False)
        if 0 < F <= wf:
            plan = [_Window(0, F, 0, F, 0, x.numel(), 0)]
        else:
            ctx = self.model.vc_context_frames(stft) if context is None else int(context)
            plan = self._long_plan(x.numel(), wf, ctx)
        noise = None
        if noise_scale > 0:
            if self._vc_gen is None:
                self._vc_gen = torch.Generator(device=self.device)
            noise = torch.randn(self.inter_channels, max(1, F), device=self.device,
                                generator=self._vc_gen) * float(noise_scale)
        out = self._run_windows(x, plan, wf, self._map_spkid(spkid_src),
                                self._map_spkid(spkid_tgt), noise)
        return out, F

    def _run_windows(self, x, plan, wf, src, tgt, noise=None):
        """The windows ``plan`` of the recording x (fp32 [n] on the device) as
        rows of ``wf`` frames, stitched: fp32 [1, max(1, F * hop)].  Per group
        of up to MAX_BATCH windows one ops.copy_windows gathers the rows into
        the static wav of the conversion graph cached under ("vc", batch
        bucket, wf), zero past each row's length; one more gathers the rows'
        slices of ``noise`` (fp32 [C, F], scaled; None: the posterior mean)
        into its static noise, so overlapping rows see the same noise; the
        graph replays; a third launch scatters the cores into their places.
        graph=False: the same gathers into fresh tensors and convert_bucketed
        eagerly.  No host sync: the host knows every length."""
        stft = self._vc_stft()
        hop = stft[1]
        F = x.numel() // hop
        C, cap = self.inter_channels, wf * hop + hop - 1
        out = torch.empty(1, max(1, F * hop), device=self.device)
        for lo, hi in self._groups(len(plan)):
            rows = plan[lo:hi]
            m = len(rows)
            bb = 1 if m == 1 else self._batch_bucket(m)
            lens = [w.s1 - w.s0 for w in rows]
            if self.graph:
                run = self._cached_graph(("vc", bb, wf), lambda: self.model.capture_convert_bucketed(
                    wf, batch=bb, stft=stft))
                wav_rows, noise_rows = run.static["wav"], run.static["noise"]
                if noise is None:
                    noise_rows.zero_()
            else:
                wav_rows = torch.zeros(bb, cap, device=self.device)
                noise_rows = None if noise is None else torch.zeros(bb, C, wf, device=self.device)
            ops.copy_windows(x, wav_rows, [(w.s0, i * cap, lens[i], cap)
                                           for i, w in enumerate(rows)])
            if noise is not None:
                ops.copy_windows(noise, noise_rows, [(w.a, i * C * wf, w.b - w.a, wf)
                                                     for i, w in enumerate(rows)],
                                 channels=C, src_rstride=noise.shape[1], dst_rstride=wf)
            if self.graph:
                o, _ = run.replay(m, lens, [src] * m, [tgt] * m)
            else:
                pad = self._pad_rows
                o, _ = self.model.convert_bucketed(
                    wav_rows, pad(lens, bb, dtype=torch.int32), pad([src] * m, bb, dtype=torch.long),
                    pad([tgt] * m, bb, dtype=torch.long), noise_rows, wf, stft=stft)
            ops.copy_windows(o, out, [(i * wf * hop + w.core_off, w.core_lo * hop,
                                       (w.core_hi - w.core_lo) * hop,
                                       (w.core_hi - w.core_lo) * hop)
                                      for i, w in enumerate(rows)])
        return out

    def convert_long(self, wav, spkid_src, spkid_tgt, *, sampling_rate_in=None, noise_scale=0.0,
                     window_frames=None, _context=None):
        """``convert`` for a recording of any length: float32 [(n // hop) *
        hop], with no seam.  The recording runs as overlapping windows of
        ``window_frames`` frames (a conversion bucket; default
        LONG_WINDOW_FRAMES) through the conversion graphs ``convert`` uses,
        up to MAX_BATCH windows per replay; every window carries
        SynthesizerTrn.vc_context_frames real frames between an artificial
        edge and its core, so the cores, stitched on the device, are bit for
        bit the conversion of the whole recording (an fp16 model at the base
        config: to fp16 rounding, its decoder depends on a row's start;
        DESIGN.md 4t).  A recording that fits one window is that window,
        with the bytes ``convert`` returns at noise_scale 0; noise_scale > 0
        draws once for the whole recording.  Raises ValueError for a
        recording of at most (n_fft - hop) / 2 samples or of more than
        LONG_MAX_SAMPLES, VitsAmdError on a CPU device."""
        self._vc_begin("convert_long")
        self._long_check(np.asarray(wav).reshape(-1).shape[0], sampling_rate_in)
        out, frames = self._convert_windows(wav, spkid_src, spkid_tgt, sampling_rate_in,
                                            noise_scale, window_frames, _context)
        return self._to_host(out[0, :frames * self.hop_size])

    def convert_pcm_long(self, wav, spkid_src, spkid_tgt, *, sampling_rate_in=None,
                         noise_scale=0.0, window_frames=None, pitch=1.0, sampling_rate=None,
                         volume=1.0, tail_silence=0.0):
        """convert_long plus the output stage of convert_pcm over the
        stitched waveform as ONE row of (n // hop) * hop samples; one
        device-to-host copy, of the int16 PCM.  The output stage carries its
        lengths as C ints: a recording that exceeds LONG_MAX_SAMPLES samples
        at the input rate, at the model rate or after a resampling pass
        (tail included) is refused with ValueError before anything is
        uploaded.  Returns (pcm int16 [n], n_model_samples)."""
        self._vc_begin("convert_pcm_long")
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        self._long_check(np.asarray(wav).reshape(-1).shape[0], sampling_rate_in, out)
        w, frames = self._convert_windows(wav, spkid_src, spkid_tgt, sampling_rate_in,
                                          noise_scale, window_frames, None)
        n = frames * self.hop_size
        pcm = self._post(w, out, lengths=n)
        return self._to_host(pcm[0, :self._n_out(n, out.passes) + out.tail]), n

    # -- forced alignment: recording and text in, durations out ---------------------
    # the widest text the alignment kernel takes (vits_maximum_path_durations)
    ALIGN_MAX_TOKENS = 2048

    def _align_rows(self, wavs, spkids, texts, emos, sampling_rate_in, noise_scale, device=False):
        """1 .. MAX_BATCH (recording, text) pairs through one alignment graph,
        cached in self._graphs under ("align", batch bucket, text bucket,
        frame bucket) (graph=False: the same align_bucketed call, eagerly).
        Returns [(durations int32 [Tx], scores fp32 [Tx], frames)] on the host
        after ONE device-to-host copy.  The host knows every length: a
        recording with fewer frames than tokens is refused here.  ``device``:
        [(durations int32 [Tx] on the device, frames)] with no copy at all."""
        stft = self._vc_begin("align")
        n = len(wavs)
        tokens = [int(np.shape(t)[0]) for t in texts]
        for w, t in zip(wavs, tokens):
            frames = self._vc_plan(np.asarray(w).reshape(-1).shape[0], sampling_rate_in)[2]
            if t < 1 or frames < t:
                raise ValueError(f"recording of {frames} frames cannot be aligned with {t} "
                                 "tokens: every token takes at least one frame")
        xb = self._text_bucket(max(tokens))
        if xb > self.ALIGN_MAX_TOKENS:
            raise ValueError(f"text of {max(tokens)} tokens exceeds the alignment kernel's "
                             f"{self.ALIGN_MAX_TOKENS}")
        wav, lens, frames, tyb, bb, noise = self._vc_upload(wavs, sampling_rate_in, noise_scale)
        resolved = [self._resolve(s, e) for s, e in zip(spkids, emos)]
        sids = [int(s) for s, _ in resolved]
        emo = torch.cat([e for _, e in resolved])
        x = self._text_rows(texts, tokens)
        if self.graph:
            run = self._cached_graph(
                ("align", bb, xb, tyb),
                lambda: self.model.capture_align_bucketed(xb, tyb, batch=bb, stft=stft))
            dur, scores, _ = run(wav, lens, x, tokens, emo, sids, noise)
        else:
            pad = self._pad_rows
            dur, scores, _ = self.model.align_bucketed(
                pad(wav, bb, tyb * stft[1] + stft[1] - 1), pad(lens, bb, dtype=torch.int32),
                pad(x, bb, xb), pad(tokens, bb, dtype=torch.int32), pad(emo, bb),
                pad(sids, bb, dtype=torch.long), pad(noise, bb), xb, tyb, stft=stft)
        if device:  # (infer_pcm_like: the durations stay on the device, nothing is copied)
            return [(dur[i, :tokens[i]], frames[i]) for i in range(n)]
        host = self._to_host(torch.cat([dur[:n], scores[:n].view(torch.int32)], 1)).reshape(n, -1)
        return [(host[i, :tokens[i]].copy(), host[i, xb:xb + tokens[i]].view(np.float32).copy(),
                 frames[i]) for i in range(n)]

    def align(self, wav, spkid, text, emo, *, sampling_rate_in=None, noise_scale=0.0):
        """Forced alignment of the recording ``wav`` (as ``convert`` takes
        it: int16 or float, at ``sampling_rate_in``, default the model's
        rate) with its text [Tx, c] spoken by spkid with emotion ``emo`` (as
        ``infer`` takes them): (durations int32 [Tx], frames per token, each
        at least 1, summing to ``frames``; scores float32 [Tx], the model's
        log-likelihood of each token's frames (compare score / duration
        between tokens: a low one marks text that does not match its audio);
        frames = samples at the model's rate // hop).  One replay of a cached
        graph and one device-to-host copy per call; noise_scale > 0 samples
        the posterior, 0 (the default) takes its mean.  Raises ValueError for
        a recording of more than 4096 frames, of at most (n_fft - hop) / 2
        samples or of fewer frames than tokens, and for more than 2048
        tokens; VitsAmdError on a CPU device."""
        return self._align_rows([wav], [spkid], [text], [emo], sampling_rate_in, noise_scale)[0]

    def align_batch(self, items, *, sampling_rate_in=None, noise_scale=0.0):
        """align for items = [(wav, spkid, text, emo), ...]: the list of
        align's results, equal to the loop over align (at noise_scale 0; a
        draw's shape follows the batch).  A group of up to MAX_BATCH items
        (batch buckets 2, 4, 8, 16) is one graph replay and one
        device-to-host copy."""
        items = list(items)
        out = []
        for lo, hi in self._groups(len(items)):
            group = items[lo:hi]
            out += self._align_rows([w for w, _, _, _ in group], [s for _, s, _, _ in group],
                                    [t for _, _, t, _ in group], [e for _, _, _, e in group],
                                    sampling_rate_in, noise_scale)
        return out

    # -- speech editing: a span of a recording re-spoken with new text
    @staticmethod
    def edit_span(text_old, text_new):
        """The span (a, b_old, b_new) that turns text_old [N, c] into
        text_new [M, c]: a = the longest common prefix of token rows, then the
        longest common suffix of what remains, so that tokens [a, b_old) of
        the old text are replaced by tokens [a, b_new) of the new one
        (identical texts: (N, N, N), an empty edit at the end)."""
        old, new = np.asarray(text_old), np.asarray(text_new)
        n, m = old.shape[0], new.shape[0]
        a = 0
        while a < min(n, m) and np.array_equal(old[a], new[a]):
            a += 1
        k = 0
        while k < min(n, m) - a and np.array_equal(old[n - 1 - k], new[m - 1 - k]):
            k += 1
        return a, n - k, m - k

    def _edit_check(self, n_in, sampling_rate_in, text_old, text_new, span, durations,
                    token_scale, span_frames, durations_old):
        """Everything about an edit the host can refuse before anything is
        uploaded (ValueError): returns (span, frames, given int32 [Tx_new] or
        None, scale fp32 [Tx_new] or None, span_target, durations_old int32
        [Tx_old] or None)."""
        n_old, n_new = int(text_old.shape[0]), int(text_new.shape[0])
        span = self.edit_span(text_old, text_new) if span is None else tuple(int(v) for v in span)
        a, b_old, b_new = span if len(span) == 3 else (-1, -1, -1)
        if not (0 <= a <= b_old <= n_old and a <= b_new <= n_new and n_old - b_old == n_new - b_new
                and np.array_equal(text_old[:a], text_new[:a])
                and np.array_equal(text_old[b_old:], text_new[b_new:])):
            raise ValueError(f"span {span} does not turn the old text ({n_old} tokens) into the "
                             f"new one ({n_new} tokens)")
        frames = self._vc_plan(n_in, sampling_rate_in)[2]  # (over VC_MAX_FRAMES: ValueError)
        if n_old < 1 or frames < n_old:
            raise ValueError(f"recording of {frames} frames cannot be aligned with {n_old} "
                             "tokens: every token takes at least one frame")
        if max(n_old, n_new) > self.ALIGN_MAX_TOKENS:
            raise ValueError(f"text of {max(n_old, n_new)} tokens exceeds the alignment kernel's "
                             f"{self.ALIGN_MAX_TOKENS}")
        target = 0
        if span_frames is not None:
            if b_new == a:
                raise ValueError("span_frames needs a new span: this edit only deletes")
            if isinstance(span_frames, str) and span_frames == "keep":
                target = -1
            elif isinstance(span_frames, (int, np.integer)) and span_frames > 0:
                target = int(span_frames)
            else:
                raise ValueError(f"span_frames must be None, an int > 0 or 'keep', got "
                                 f"{span_frames!r}")
        given = None
        if durations is not None:
            d = np.asarray(durations).reshape(-1)
            given = np.full(n_new, -1, np.int32)
            if d.shape[0] == n_new:
                given[a:b_new] = d[a:b_new]
            elif d.shape[0] == b_new - a:
                given[a:b_new] = d
            else:
                raise ValueError(f"durations need {n_new} values (or {b_new - a} for the span), "
                                 f"got {d.shape[0]}")
        scale = None
        if token_scale is not None:
            scale = np.asarray(token_scale, np.float32).reshape(-1)
            if scale.shape[0] != n_new or not bool(np.all(scale >= 0)):
                raise ValueError(f"token_scale needs {n_new} factors >= 0")
        if durations_old is not None:
            durations_old = np.asarray(durations_old).reshape(-1).astype(np.int32)
            if (durations_old.shape[0] != n_old or bool((durations_old < 0).any())
                    or int(durations_old.sum()) != frames):
                raise ValueError(f"durations_old must be {n_old} frame counts >= 0 that sum to "
                                 f"the recording's {frames} frames")
        return span, frames, given, scale, target, durations_old

    def _edit_rows(self, wav, spkid, text_old, text_new, emo, span, sampling_rate_in, durations,
                   token_scale, span_frames, duration_rate, noise_scale, durations_old, emo_new,
                   patch, margin_frames, fade, post=None):
        """One edit through one graph, cached in self._graphs under ("edit",
        old text bucket, new text bucket, recording frame bucket, output frame
        bucket, durations_old given) (graph=False: the same edit_bucketed
        call, eagerly, on the same padded inputs).  Returns (wav_out [1, n]
        fp32 on the device, or ``post(wav_out, lengths, length_scale)``'s
        result; y_new; dur_new; (f0, n_new, f1); scores) after ONE small
        device-to-host copy (meta, durations and scores)."""
        stft = self._vc_begin("edit")
        hop = self.hop_size
        text_old = np.ascontiguousarray(text_old)
        text_new = np.ascontiguousarray(text_new)
        n_in = np.asarray(wav).reshape(-1).shape[0]
        span, frames, given, scale, target, durations_old = self._edit_check(
            n_in, sampling_rate_in, text_old, text_new, span, durations, token_scale, span_frames,
            durations_old)
        n_old, n_new = text_old.shape[0], text_new.shape[0]
        margin = self.model.edit_context_frames() if margin_frames is None else int(margin_frames)
        fade = hop if fade is None else int(fade)
        if margin < 0 or fade < 0:
            raise ValueError("margin_frames and fade must be >= 0")
        x, lens, _, trb, _, _ = self._vc_upload([wav], sampling_rate_in, 0.0)
        spk, e_old = self._resolve(spkid, emo)
        e_new = e_old if emo_new is None else self._resolve(spkid, emo_new)[1]
        xb_old, xb_new = self._text_bucket(n_old), self._text_bucket(n_new)
        dev, dt, i32 = self.device, self.dtype, torch.int32
        C = self.inter_channels
        g_row = np.full(xb_new, -1, np.int32)
        if given is not None:
            g_row[:n_new] = given
        s_row = np.ones(xb_new, np.float32)
        if scale is not None:
            s_row[:n_new] = scale
        pad = self._pad_rows
        inputs = dict(
            wav=pad(x, 1, trb * hop + hop - 1), n=pad(lens, 1, dtype=i32),
            x_old=pad(self._text_rows([text_old], [n_old]), 1, xb_old),
            xl_old=pad([n_old], 1, dtype=i32),
            x_new=pad(self._text_rows([text_new], [n_new]), 1, xb_new),
            xl_new=pad([n_new], 1, dtype=i32), emo=e_old, emo_new=e_new,
            sid=pad([int(spk)], 1, dtype=torch.long),
            spans=torch.tensor([list(span)], dtype=i32).to(dev),
            given=torch.from_numpy(g_row).view(1, -1).to(dev),
            tok_scale=torch.from_numpy(s_row).view(1, -1).to(dev),
            span_target=pad([target], 1, dtype=i32),
            rate=torch.full((1,), float(duration_rate), device=dev),
            noise_q=torch.zeros(1, C, trb, device=dev))
        if durations_old is not None:
            d_row = np.zeros(xb_old, np.int32)
            d_row[:n_old] = durations_old
            inputs["dur_old"] = torch.from_numpy(d_row).view(1, -1).to(dev)
        y_len_old = pad([frames], 1, dtype=i32)
        if self._vc_gen is None:
            self._vc_gen = torch.Generator(device=dev)
        gen_state = self._vc_gen.get_state()
        memo = ("edit", xb_old, xb_new, trb)
        while True:
            tyb = trb if target < 0 else max(trb, self._ty_bucket.get(memo, trb))
            # the prior noise of the whole output bucket, from the device
            # generator of the conversion paths (a re-run draws from the same state)
            self._vc_gen.set_state(gen_state)
            if noise_scale > 0:
                inputs["noise"] = torch.randn(1, C, tyb, device=dev,
                                              generator=self._vc_gen) * float(noise_scale)
            else:
                inputs["noise"] = torch.zeros(1, C, tyb, device=dev)
            if self.graph:
                run = self._cached_graph(
                    ("edit", 1, xb_old, xb_new, trb, tyb, durations_old is not None),
                    lambda: self.model.capture_edit_bucketed(
                        xb_old, xb_new, trb, tyb, stft=stft,
                        given_durations=durations_old is not None))
                for k, v in inputs.items():
                    run.static[k].copy_(v)
                o, lengths, dur_new, meta, scores = run.replay()
            else:
                i = inputs
                o, lengths, dur_new, meta, scores = self.model.edit_bucketed(
                    i["wav"], i["n"], i["x_old"], i["xl_old"], i["x_new"], i["xl_new"], i["emo"],
                    i["emo_new"], i["sid"], i["spans"],
                    {k: i[k] for k in ("given", "tok_scale", "span_target", "rate")},
                    (i["noise"], i["noise_q"]), trb, tyb, stft=stft,
                    durations_old=i.get("dur_old"))
            w, scale_l = o[:, 0], hop  # (lengths: y_new in frames)
            if patch:
                w, lengths = ops.edit_patch(inputs["wav"], o[:, 0], y_len_old, meta[:4], hop,
                                            margin=margin, fade=fade)
                scale_l = 1
            posted = None if post is None else post(w, lengths, scale_l)
            parts = [meta[:, 0], dur_new[0, :n_new]]
            if scores is not None:
                parts.append(scores[0, :n_old].view(i32))
            host = self._to_host(torch.cat(parts))  # the one copy back (synchronises)
            f0, n_span, f1, s_st, p_st, d_st = (int(v) for v in host[:6])
            if p_st:
                raise ValueError("the old durations do not describe the recording (no alignment, "
                                 f"or their sum is not its {frames} frames)")
            if d_st:
                raise ValueError(f"span_frames={span_frames!r} cannot be met: the span's pins "
                                 "leave no room for it")
            if s_st == 1:
                raise ValueError(f"span {span} cannot be spliced into this recording")
            y_new = f0 + n_span + frames - f1
            if s_st == -1:
                if y_new > self.VC_MAX_FRAMES:
                    raise ValueError(f"edited recording of {y_new} frames exceeds the largest "
                                     f"bucket of {self.VC_MAX_FRAMES} frames")
                # re-run at the next output bucket, which this memo keeps.  (The
                # patch and the post stage of this attempt ran over a zero row: the
                # status is known only after the copy.  _grow_bucket puts numpy's
                # generator back for the synthesis paths; this one never draws from
                # it, so it is handed the state as it is.)
                self._grow_bucket(memo, np.random.get_state(), tyb, y_new)
                continue
            dur = host[6:6 + n_new].copy()
            sc = host[6 + n_new:].view(np.float32).copy() if scores is not None else None
            return (w if post is None else posted), y_new, dur, (f0, n_span, f1), sc

    def edit(self, wav, spkid, text_old, text_new, emo, *, span=None, sampling_rate_in=None,
             durations=None, token_scale=None, span_frames=None, duration_rate=1.0,
             noise_scale=0.667, durations_old=None, emo_new=None, patch=False, margin_frames=None,
             fade=None):
        """Re-speak part of a recording: ``wav`` (as ``convert`` takes it) is
        speaker spkid saying text_old [N, c]; the result says text_new [M, c].
        ``span`` = (a, b_old, b_new) (default: edit_span of the two texts):
        tokens [a, b_old) of the old text become tokens [a, b_new) of the new
        one.  The recording is aligned with its text (or ``durations_old``
        taken as its alignment), the new text is encoded as a whole, the new
        span gets durations from the duration plan (``durations``: frames for
        the span's tokens, < 0 free; ``token_scale``; ``duration_rate``;
        ``span_frames``: an int, the new span lasts exactly that many frames,
        or "keep", it lasts what the old one did) and its prior (noise from
        this object's device generator times ``noise_scale``) is spliced
        between the recording's own latents, which the reverse flow and the
        decoder then render as one utterance: SynthesizerTrn.edit, through one
        cached graph and one small device-to-host copy.  ``patch``: outside
        the edited frames widened by ``margin_frames`` (default
        edit_context_frames()) the samples are the recording's own, with a
        cross-fade of ``fade`` samples (default one hop) at each seam
        (ops.edit_patch); else the whole result is the model's rendering.

        Returns (wav float32 [y_new * hop] at the model's rate, dur_new int32
        [M], (f0, n_new, f1) the edited frames [f0, f1) of the recording and
        [f0, f0 + n_new) of the result, scores float32 [N] of the alignment or
        None with durations_old).  Raises ValueError, before anything is
        uploaded, for a span that does not match the texts, a recording of
        more than 4096 frames or of fewer frames than tokens, span_frames with
        an empty new span; after the copy for durations that do not describe
        the recording or a span_frames that cannot be met."""
        w, y_new, dur, pos, scores = self._edit_rows(
            wav, spkid, text_old, text_new, emo, span, sampling_rate_in, durations, token_scale,
            span_frames, duration_rate, noise_scale, durations_old, emo_new, patch, margin_frames,
            fade)
        return w[0, :y_new * self.hop_size].cpu().numpy(), dur, pos, scores

    def edit_pcm(self, wav, spkid, text_old, text_new, emo, *, span=None, sampling_rate_in=None,
                 durations=None, token_scale=None, span_frames=None, duration_rate=1.0,
                 noise_scale=0.667, durations_old=None, emo_new=None, patch=True,
                 margin_frames=None, fade=None, pitch=1.0, sampling_rate=None, volume=1.0,
                 tail_silence=0.0):
        """edit plus convert_pcm's output stage on the device (pitch /
        sampling-rate resampling, volume, clip, int16, tail silence), the
        length read on the device; ``patch`` defaults to True.  Returns (pcm
        int16 [n], n_model_samples, dur_new, (f0, n_new, f1), scores)."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        pcm, y_new, dur, pos, scores = self._edit_rows(
            wav, spkid, text_old, text_new, emo, span, sampling_rate_in, durations, token_scale,
            span_frames, duration_rate, noise_scale, durations_old, emo_new, patch, margin_frames,
            fade, post=lambda w, lengths, scale: self._post(w, out, lengths=lengths,
                                                            length_scale=scale))
        n = y_new * self.hop_size
        return pcm[0, :self._n_out(n, out.passes) + out.tail].cpu().numpy(), n, dur, pos, scores

    # -- retiming a recording: speed, fitted length, per-token timing
    RETIME_MIN_SCALE, RETIME_MAX_SCALE = 1.0 / 16, 16.0

    def _retime_check(self, n_in, sampling_rate_in, speed, pitch, target_frames, text, durations,
                      token_scale, durations_old):
        """Everything about a retiming the host can refuse before anything is
        uploaded (ValueError): returns (frames, tokens (0: text-free), given
        int32 [tokens] or None, scale fp32 [tokens] or None, target,
        durations_old int32 [tokens] or None, the durations' rate = speed /
        pitch, the host bound on y_new)."""
        lo, hi = self.RETIME_MIN_SCALE, self.RETIME_MAX_SCALE
        frames = self._vc_plan(n_in, sampling_rate_in)[2]  # (over VC_MAX_FRAMES: ValueError)

        def in_range(name, v):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(v) or not lo <= float(v) <= hi:
                raise ValueError(f"{name} must be a finite number in [1/16, 16], got {v!r}")
            return float(v)

        rate = in_range("speed / pitch", in_range("speed", speed) / float(pitch))
        if text is None and (durations is not None or token_scale is not None):
            raise ValueError("durations and token_scale are per token: they need text")
        n_tok = 0 if text is None else int(text.shape[0])
        if durations_old is not None:
            durations_old = np.asarray(durations_old).reshape(-1).astype(np.int32)
            if text is None:
                n_tok = int(durations_old.shape[0])
            if (durations_old.shape[0] != n_tok or n_tok < 1 or bool((durations_old < 0).any())
                    or int(durations_old.sum()) != frames):
                raise ValueError(f"durations_old must be {n_tok} frame counts >= 0 that sum to "
                                 f"the recording's {frames} frames")
        if text is not None and (n_tok < 1 or frames < n_tok):
            raise ValueError(f"recording of {frames} frames cannot be aligned with {n_tok} "
                             "tokens: every token takes at least one frame")
        if n_tok > self.ALIGN_MAX_TOKENS:
            raise ValueError(f"text of {n_tok} tokens exceeds the alignment kernel's "
                             f"{self.ALIGN_MAX_TOKENS}")
        target = 0
        if target_frames is not None:
            if isinstance(target_frames, bool) or not isinstance(target_frames, (int, np.integer)) \
                    or not 0 < target_frames <= self.VC_MAX_FRAMES:
                raise ValueError(f"target_frames must be an int in 1 .. {self.VC_MAX_FRAMES}, got "
                                 f"{target_frames!r}")
            target = int(target_frames)
        given = None
        if durations is not None:
            d = np.asarray(durations).reshape(-1)
            if d.shape[0] != n_tok:
                raise ValueError(f"durations need {n_tok} values (< 0: free), got {d.shape[0]}")
            given = np.where(d < 0, -1, np.minimum(d, 1 << 18)).astype(np.int32)
        scale = None
        if token_scale is not None:
            scale = np.asarray(token_scale, np.float32).reshape(-1)
            if scale.shape[0] != n_tok or not bool(np.all(np.isfinite(scale))) or not bool(
                    np.all((scale >= lo) & (scale <= hi))):
                raise ValueError(f"token_scale needs {n_tok} finite factors in [1/16, 16]")
        if target:
            bound = target
        else:
            pins = 0 if given is None else int(given[given >= 0].sum())
            top = 1.0 if scale is None else float(scale.max())
            bound = int(np.ceil(frames * float(rate) * top)) + max(n_tok, 1) + pins
        if bound > self.VC_MAX_FRAMES:
            raise ValueError(f"the retimed recording may take {bound} frames: more than the "
                             f"largest bucket of {self.VC_MAX_FRAMES} frames")
        return frames, n_tok, given, scale, target, durations_old, rate, bound

    def _retime_rows(self, wav, spkid_src, spkid_tgt, speed, pitch, target_frames, text, emo,
                     durations, token_scale, durations_old, sampling_rate_in, noise_scale,
                     post=None):
        """One retiming through one graph, cached in self._graphs under
        ("retime", 1, text bucket or 0, recording frame bucket, output frame
        bucket, durations_old given) (graph=False: the same retime_bucketed
        call, eagerly, on the same padded inputs).  The output bucket holds a
        host bound on y_new, so no re-run is ever needed.  Returns (wav_out
        [1, n] fp32 on the device, or ``post(wav_out, lengths,
        length_scale)``'s result; y_new; dur_old; dur_new; scores) after ONE
        small device-to-host copy (meta, both duration rows and the scores)."""
        stft = self._vc_begin("retime")
        hop = self.hop_size
        text = None if text is None else np.ascontiguousarray(text)
        n_in = np.asarray(wav).reshape(-1).shape[0]
        frames, n_tok, given, scale, target, durations_old, rate, bound = self._retime_check(
            n_in, sampling_rate_in, speed, pitch, target_frames, text, durations, token_scale,
            durations_old)
        src, tgt = self._map_spkid(spkid_src), self._map_spkid(spkid_tgt)
        x, lens, _, trb, _, noise = self._vc_upload([wav], sampling_rate_in, noise_scale)
        aligned = text is not None and durations_old is None
        xt = e = None
        if aligned:
            e = self._resolve(spkid_src, emo)[1]
            xt = self._text_rows([text], [n_tok])
        xb = self._text_bucket(n_tok) if n_tok else 0
        tw, nt = max(xb, 1), max(n_tok, 1)
        tyb = self._frame_bucket(bound)
        dev, i32 = self.device, torch.int32
        g_row = np.full(tw, -1, np.int32)
        if given is not None:
            g_row[:n_tok] = given
        s_row = np.ones(tw, np.float32)
        if scale is not None:
            s_row[:n_tok] = scale
        d_row = None
        if durations_old is not None:
            d_row = np.zeros(xb, np.int32)
            d_row[:n_tok] = durations_old
        if self.graph:
            run = self._cached_graph(
                ("retime", 1, xb, trb, tyb, durations_old is not None),
                lambda: self.model.capture_retime_bucketed(
                    xb, trb, tyb, stft=stft, given_durations=durations_old is not None))
            neutral = given is None and scale is None and target == 0 and float(rate) == 1.0
            ctl = None if neutral else [dict(given=g_row, tok_scale=s_row, rate=float(rate),
                                             target=target)]
            o, y_len, dur_old, dur_new, meta, scores = run(
                x, lens, [src], [tgt], x=xt, x_lengths=[n_tok] if xb else None, emo=e,
                controls=ctl, noise=noise, durations_old=d_row)
        else:
            pad = self._pad_rows
            ctl = dict(given=torch.from_numpy(g_row).view(1, -1).to(dev),
                       tok_scale=torch.from_numpy(s_row).view(1, -1).to(dev),
                       rate=torch.full((1,), float(rate), device=dev),
                       target=pad([target], 1, dtype=i32))
            o, y_len, dur_old, dur_new, meta, scores = self.model.retime_bucketed(
                pad(x, 1, trb * hop + hop - 1), pad(lens, 1, dtype=i32),
                pad([src], 1, dtype=torch.long), pad([tgt], 1, dtype=torch.long), noise, trb, tyb,
                stft=stft, x=None if xt is None else pad(xt, 1, xb),
                x_lengths=pad([n_tok], 1, dtype=i32) if xb else None, emo=e,
                durations_old=None if d_row is None else torch.from_numpy(d_row).view(1, -1).to(dev),
                controls=ctl)
        posted = None if post is None else post(o[:, 0], y_len, hop)
        parts = [meta[:, 0], dur_old[0, :nt], dur_new[0, :nt]]
        if scores is not None:
            parts.append(scores[0, :nt].view(i32))
        host = self._to_host(torch.cat(parts))  # the one copy back (synchronises)
        y_new, w_st, p_st = (int(v) for v in host[:3])
        if p_st:
            raise ValueError(
                f"target_frames={target_frames!r} cannot be met (the pins leave no room for it), "
                f"or the old durations do not sum to the recording's {frames} frames")
        if w_st:
            raise ValueError(f"the retimed recording of {y_new} frames does not fit its bucket "
                             f"of {tyb} frames")
        d_old, d_new = host[3:3 + nt].copy(), host[3 + nt:3 + 2 * nt].copy()
        sc = host[3 + 2 * nt:].view(np.float32).copy() if scores is not None else None
        return (o[:, 0] if post is None else posted), y_new, d_old, d_new, sc

    def retime(self, wav, spkid_src, spkid_tgt, *, speed=1.0, target_frames=None, text=None,
               emo=None, durations=None, token_scale=None, durations_old=None,
               sampling_rate_in=None, noise_scale=0.0, graph=True, return_durations=False):
        """Retime a recording and keep its performance and voice: ``wav`` (as
        ``convert`` takes it) of speaker spkid_src comes back in the voice of
        spkid_tgt (the same id: its own) with its timing changed in latent
        space (SynthesizerTrn.retime).  ``speed`` multiplies
        every duration, as duration_rate does in ``infer`` (1.1: ten per cent
        slower); ``target_frames``: the result lasts exactly that many model
        frames (speed is then not applied).  With ``text`` [N, c] (and ``emo``
        as ``align`` takes it) the recording is aligned with it, or
        ``durations_old`` (N frame counts summing to the recording's frames)
        taken as its alignment, and each token can be timed on its own:
        ``durations`` (N frame counts, < 0: free) pins tokens, ``token_scale``
        (N factors) multiplies the free ones.  Without text the take is one
        token.  noise_scale as in ``convert``.  ``graph=False`` runs the same
        chain eagerly and gives the same bytes.

        Returns wav float32 [y_new * hop] at the model's rate; with
        ``return_durations`` (wav, dur_old int32 [N], dur_new int32 [N],
        scores float32 [N] of the alignment or None).  Raises ValueError,
        before anything is uploaded, for a recording of more than 4096 frames
        or of fewer frames than tokens, a speed or token_scale outside [1/16,
        16] or not finite, durations or token_scale without text, lengths
        that do not match the text, durations_old that do not sum to the
        frames, a result that may exceed 4096 frames; after the copy for a
        target the pins leave no room for."""
        keep, self.graph = self.graph, bool(graph) and self.graph
        try:
            w, y_new, d_old, d_new, sc = self._retime_rows(
                wav, spkid_src, spkid_tgt, speed, 1.0, target_frames, text, emo, durations,
                token_scale, durations_old, sampling_rate_in, noise_scale)
        finally:
            self.graph = keep
        out = w[0, :y_new * self.hop_size].cpu().numpy()
        return (out, d_old, d_new, sc) if return_durations else out

    def retime_pcm(self, wav, spkid_src, spkid_tgt, *, speed=1.0, target_frames=None, text=None,
                   emo=None, durations=None, token_scale=None, durations_old=None,
                   sampling_rate_in=None, noise_scale=0.0, graph=True, return_durations=False,
                   pitch=1.0, sampling_rate=None, volume=1.0, tail_silence=0.0):
        """retime plus convert_pcm's output stage on the device, the length
        read on the device.  The durations' rate is speed / pitch, so the
        change of length of the pitch resampler cancels, as in ``speaking``:
        pitch changes and the length stays.  ``target_frames`` counts model
        frames before the output stage.  Returns (pcm int16 [n],
        n_model_samples), with ``return_durations`` followed by (dur_old,
        dur_new, scores)."""
        out = self._output(pitch, sampling_rate, volume, tail_silence)
        keep, self.graph = self.graph, bool(graph) and self.graph
        try:
            pcm, y_new, d_old, d_new, sc = self._retime_rows(
                wav, spkid_src, spkid_tgt, speed, pitch, target_frames, text, emo,
                durations, token_scale, durations_old, sampling_rate_in, noise_scale,
                post=lambda w, lengths, scale: self._post(w, out, lengths=lengths,
                                                          length_scale=scale))
        finally:
            self.graph = keep
        n = y_new * self.hop_size
        res = (pcm[0, :self._n_out(n, out.passes) + out.tail].cpu().numpy(), n)
        return res + (d_old, d_new, sc) if return_durations else res

    # -- forced alignment of long recordings: many segments, any length
    # the caps of align_long: the total tokens of a text (a 40-minute reading
    # at 1 token per 6 frames), and the bytes of the search's workspace plus
    # one panel of scores (at the token cap: a recording of 78 minutes)
    ALIGN_LONG_MAX_TOKENS = 32768
    ALIGN_LONG_MAX_BYTES = 2 ** 31
    ALIGN_LONG_PANEL_FRAMES = 4096
    ALIGN_LONG_STRIP_TOKENS = 2048

    def _align_long_bytes(self, frames, tokens, strip, panel):
        """Device bytes of the long search at [frames, tokens]: the workspace
        of vits_mas_long_* (the decision words, frames * tokens / 8, and a few
        vectors) plus one panel of scores; (bytes, strip, panel as run)."""
        strip, panel = ops.mas_long_plan(frames, tokens, strip, panel)
        ws = int(ops._lib.load().vits_mas_long_workspace(1, frames, tokens, strip, panel))
        if ws <= 0:
            raise ValueError(f"no long alignment plan for {frames} frames x {tokens} tokens at "
                             f"strips of {strip} and panels of {panel}")
        return ws + 4 * panel * tokens, strip, panel

    def _align_long_check(self, n_in, sampling_rate_in, tokens, window_frames, panel_frames,
                          strip_tokens):
        """Everything align_long refuses, from host arithmetic alone, before
        anything is uploaded: (frames, window frames, strip, panel)."""
        if len(tokens) == 0:
            raise ValueError("align_long: no text segment")
        for i, t in enumerate(tokens):
            if t < 1:
                raise ValueError(f"align_long: segment {i} is empty")
        total = sum(tokens)
        frames = self._long_check(n_in, sampling_rate_in)
        if frames < total:
            raise ValueError(f"recording of {frames} frames cannot be aligned with {total} "
                             "tokens: every token takes at least one frame")
        if total > self.ALIGN_LONG_MAX_TOKENS:
            raise ValueError(f"text of {total} tokens exceeds align_long's "
                             f"{self.ALIGN_LONG_MAX_TOKENS}")
        wf = self.LONG_WINDOW_FRAMES if window_frames is None else int(window_frames)
        if not self.VC_MIN_FRAMES <= wf <= self.VC_MAX_FRAMES or self._frame_bucket(wf) != wf:
            raise ValueError(f"window_frames must be a conversion bucket (a power of two, "
                             f"{self.VC_MIN_FRAMES} .. {self.VC_MAX_FRAMES}), got {wf}")
        strip = self.ALIGN_LONG_STRIP_TOKENS if strip_tokens is None else int(strip_tokens)
        panel = self.ALIGN_LONG_PANEL_FRAMES if panel_frames is None else int(panel_frames)
        if strip not in ops.MAS_LONG_STRIPS:
            raise ValueError(f"strip_tokens must be one of {ops.MAS_LONG_STRIPS}, got {strip}")
        if panel < 32 or panel % 32:
            raise ValueError(f"panel_frames must be a positive multiple of 32, got {panel}")
        need, strip, panel = self._align_long_bytes(frames, total, strip, panel)
        if need > self.ALIGN_LONG_MAX_BYTES:
            raise ValueError(f"aligning {frames} frames with {total} tokens takes {need} bytes of "
                             f"workspace, above align_long's {self.ALIGN_LONG_MAX_BYTES}")
        return frames, wf, strip, panel

    def _latent_windows(self, x, plan, wf, sid, noise=None):
        """z_p fp32 [1, C, F] of the recording x (fp32 [n] on the device)
        through the windows ``plan`` as rows of ``wf`` frames: _run_windows'
        gathers (waveform, and the rows' slices of ``noise`` fp32 [C, F]) into
        the static buffers of the graph cached under ("latents", batch
        bucket, wf), a replay, and one ops.copy_windows that scatters the
        cores' columns into their places (R = channels).  graph=False: the
        same gathers into fresh tensors and latents_bucketed eagerly.  No
        host sync."""
        stft = self._vc_stft()
        hop = stft[1]
        F = x.numel() // hop
        C, cap = self.inter_channels, wf * hop + hop - 1
        out = torch.empty(1, C, F, device=self.device)
        for lo, hi in self._groups(len(plan)):
            rows = plan[lo:hi]
            m = len(rows)
            bb = 1 if m == 1 else self._batch_bucket(m)
            lens = [w.s1 - w.s0 for w in rows]
            if self.graph:
                run = self._cached_graph(
                    ("latents", bb, wf),
                    lambda: self.model.capture_latents_bucketed(wf, batch=bb, stft=stft))
                wav_rows, noise_rows = run.static["wav"], run.static["noise"]
                if noise is None:
                    noise_rows.zero_()
            else:
                wav_rows = torch.zeros(bb, cap, device=self.device)
                noise_rows = None if noise is None else torch.zeros(bb, C, wf, device=self.device)
            ops.copy_windows(x, wav_rows, [(w.s0, i * cap, lens[i], cap)
                                           for i, w in enumerate(rows)])
            if noise is not None:
                ops.copy_windows(noise, noise_rows, [(w.a, i * C * wf, w.b - w.a, wf)
                                                     for i, w in enumerate(rows)],
                                 channels=C, src_rstride=noise.shape[1], dst_rstride=wf)
            if self.graph:
                z, _ = run.replay(m, lens, [sid] * m)
            else:
                pad = self._pad_rows
                z, _ = self.model.latents_bucketed(
                    wav_rows, pad(lens, bb, dtype=torch.int32), pad([sid] * m, bb, dtype=torch.long),
                    noise_rows, wf, stft=stft)
            ops.copy_windows(z, out, [(i * C * wf + w.core_lo - w.a, w.core_lo,
                                       w.core_hi - w.core_lo, w.core_hi - w.core_lo)
                                      for i, w in enumerate(rows)],
                             channels=C, src_rstride=wf, dst_rstride=F)
        return out

    @torch.no_grad()
    def _segment_priors(self, texts, tokens, sids, emos):
        """m_p, logs_p fp32 [1, C, sum(tokens)] of the segments, each encoded
        on its own (pad_exact) with its own emotion vector, in groups of up
        to MAX_BATCH at the text buckets; each row's exact-length columns are
        gathered into their place with ops.copy_windows.  No host sync."""
        C, total = self.inter_channels, sum(tokens)
        m_all = torch.empty(1, C, total, device=self.device)
        l_all = torch.empty(1, C, total, device=self.device)
        offs = np.concatenate([[0], np.cumsum(tokens)])
        pad = self._pad_rows
        for lo, hi in self._groups(len(texts)):
            m = hi - lo
            bb = 1 if m == 1 else self._batch_bucket(m)
            tk = tokens[lo:hi]
            xb = self._text_bucket(max(tk))
            x = pad(self._text_rows(texts[lo:hi], tk), bb, xb)
            emo = pad(torch.cat(emos[lo:hi]), bb)
            g = self.model.emb_g(pad(sids[lo:hi], bb, dtype=torch.long))
            _, m_p, logs_p = self.model.enc_p.forward_masked_hip(
                x, pad(tk, bb, dtype=torch.int32), emo, g, pad_exact=True)
            jobs = [(i * C * xb, int(offs[lo + i]), tk[i], tk[i]) for i in range(m)]
            for src, dst in ((m_p, m_all), (logs_p, l_all)):
                ops.copy_windows(src.float().contiguous(), dst, jobs, channels=C, src_rstride=xb,
                                 dst_rstride=total)
        return m_all, l_all

    def align_long(self, wav, spkid, texts, emos, *, sampling_rate_in=None, noise_scale=0.0,
                   window_frames=None, panel_frames=None, strip_tokens=None, _context=None,
                   _keep=None):
        """``align`` for a recording of any length against a text in any
        number of segments: ``texts`` a list of [Tx_i, c], ``emos`` one
        emotion per segment (as ``infer`` takes them), each segment encoded on
        its own as ``infer_batch`` feeds the model, the concatenated text
        aligned with the whole recording by one exact global search
        (SynthesizerTrn.align_segments is the definition).  Returns
        (durations: a list of int32 arrays, one per segment; scores:
        likewise, float32; segment_frames int64 [n_seg + 1]: the frame at
        which each segment starts, cumulative, ending at ``frames``; frames).

        z_p of the recording comes from overlapping windows of
        ``window_frames`` frames (a conversion bucket; default
        LONG_WINDOW_FRAMES) with SynthesizerTrn.align_context_frames of
        context, up to MAX_BATCH per replay of a graph cached under
        ("latents", batch bucket, window_frames); the search
        (ops.maximum_path_durations_long) takes it in panels of
        ``panel_frames`` frames (default 4096) and strips of ``strip_tokens``
        tokens (default 2048) and never holds the score matrix.  One
        device-to-host copy at the end, no sync before it.  noise_scale > 0
        draws once for the whole recording.  Raises ValueError, before
        anything is uploaded, for an empty segment, fewer frames than total
        tokens, more than ALIGN_LONG_MAX_TOKENS tokens, a workspace above
        ALIGN_LONG_MAX_BYTES and what convert_long refuses; VitsAmdError on a
        CPU device."""
        stft = self._vc_begin("align_long")
        texts = [np.ascontiguousarray(t) for t in texts]
        emos = list(emos)
        if len(emos) != len(texts):
            raise ValueError(f"align_long: {len(texts)} segments need {len(texts)} emotions, got "
                             f"{len(emos)}")
        tokens = [int(t.shape[0]) for t in texts]
        F, wf, strip, panel = self._align_long_check(
            np.asarray(wav).reshape(-1).shape[0], sampling_rate_in, tokens, window_frames,
            panel_frames, strip_tokens)
        resolved = [self._resolve(spkid, e) for e in emos]
        sids = [int(s) for s, _ in resolved]
        x, F2, _ = self._vc_input(wav, sampling_rate_in, capped=False)
        assert F2 == F
        if F <= wf:
            plan = [_Window(0, F, 0, F, 0, x.numel(), 0)]
        else:
            ctx = self.model.align_context_frames(stft) if _context is None else int(_context)
            plan = self._long_plan(x.numel(), wf, ctx)
        noise = None
        if noise_scale > 0:
            if self._vc_gen is None:
                self._vc_gen = torch.Generator(device=self.device)
            noise = torch.randn(self.inter_channels, F, device=self.device,
                                generator=self._vc_gen) * float(noise_scale)
        z_p = self._latent_windows(x, plan, wf, sids[0], noise)
        m_p, logs_p = self._segment_priors(texts, tokens, sids, [e for _, e in resolved])
        total = sum(tokens)
        lens = torch.tensor([F, total], dtype=torch.int32).to(self.device)
        dur, scores, _ = ops.maximum_path_durations_long(z_p, m_p, logs_p, lens[:1], lens[1:],
                                                         strip=strip, panel=panel)
        if _keep is not None:  # (tests: the latents on the device)
            _keep.update(z_p=z_p, m_p=m_p, logs_p=logs_p)
        host = self._to_host(torch.cat([dur[0], scores[0].view(torch.int32)]))
        d, s = host[:total], host[total:].view(np.float32)
        offs = np.concatenate([[0], np.cumsum(tokens)])
        seg_frames = np.concatenate([[0], np.cumsum(d, dtype=np.int64)[offs[1:] - 1]])
        return ([d[offs[i]:offs[i + 1]].copy() for i in range(len(tokens))],
                [s[offs[i]:offs[i + 1]].copy() for i in range(len(tokens))],
                seg_frames.astype(np.int64), F)

    # text tokens are padded to a multiple of TX_BUCKET (masked encoder);
    # frame buckets are powers of two from 256 up to the noise buffer's 4096
    TX_BUCKET = 32

    @classmethod
    def _text_bucket(cls, t):
        """The smallest multiple of TX_BUCKET that holds t tokens."""
        return -(-t // cls.TX_BUCKET) * cls.TX_BUCKET

    @classmethod
    def _frame_bucket(cls, n, cap=None):
        """The smallest frame bucket that holds n frames: a power of two, at
        least 256; with ``cap`` at most that (the 4096 frames of the noise
        buffer, where a bucket grows towards it)."""
        b = max(cls.VC_MIN_FRAMES, 1 << max(0, int(n) - 1).bit_length())
        return b if cap is None else min(cap, b)

    def _text_rows(self, texts, lengths):
        """Texts of ``lengths`` tokens as one [n, longest, c] tensor on the
        device in the model's dtype, zero past each row's end."""
        x = np.zeros((len(texts), max(lengths), np.shape(texts[0])[1]), dtype=np.float32)
        for i, t in enumerate(texts):
            x[i, :lengths[i]] = t
        return torch.from_numpy(x).to(self.dtype).to(self.device)

    def _grow_bucket(self, memo, state, tyb, n):
        """An utterance of n frames did not fit its frame bucket ``tyb``:
        restore numpy's generator (the re-run makes the same draws) and keep
        a bucket that holds n under ``memo``, or raise RuntimeError when the
        bucket already is the noise buffer's 4096 frames."""
        np.random.set_state(state)
        if tyb >= 4096:
            raise RuntimeError(f"utterance of {n} frames exceeds the 4096-frame noise buffer")
        self._ty_bucket[memo] = self._frame_bucket(n, cap=4096)

    def _misfit(self, state, n):
        """The ValueError of an utterance of n frames that is longer than the
        noise buffer, with numpy's generator put back."""
        np.random.set_state(state)
        return ValueError(f"utterance of {n} frames does not fit the "
                          f"{self.noise.numel()}-sample noise buffer")

    def _infer_graph(self, text_t, emo, sid, duration_rate, post=None, ctl=None, got=None,
                     front=False):
        """One replay of the whole-utterance graph; the one host sync is the
        waveform copy (y_len read with it).  A bucket that turns out too
        small (y_len > frames) is re-run once at a large enough bucket,
        which this text bucket keeps from then on.  ``post(wav [1, frames *
        hop], y_len int32 [1])`` is launched behind every replay, before the
        sync; its result is then returned with the frame count, in place of
        the waveform.

        ``ctl`` (the result of _controls): the utterance runs through a
        controlled, rate-free graph cached under ("ctl", 1, text bucket, frame
        bucket) in the same most-recently-used cache; the speed and the
        controls are replay inputs, so one graph serves every control.  When
        the host knows the total (a target, or every token pinned) the frame
        bucket is chosen from it; else the bucket is remembered per text
        bucket and grown by the re-run below.  ``got`` (a list): the final
        durations (int32 [t_x]) are appended to it.

        ``front``: the replay is the front graph of a streamed utterance
        (capture_infer_front_bucketed, cached under ("front",) + the key the
        whole-utterance graph has): the same buckets, re-run and draw commit;
        returns ((z [1, C, bucket], g), frames), views of static buffers."""
        t_x = text_t.shape[1]
        xb = self._text_bucket(t_x)
        memo = (xb, duration_rate) if ctl is None else ("ctl", xb)
        while True:
            tyb = self._ty_bucket.get(memo, 256)
            if ctl is not None and ctl[3] is not None:
                tyb = self._frame_bucket(ctl[3])
            key = (xb, tyb, float(duration_rate)) if ctl is None else ("ctl", 1, xb, tyb)
            if front:
                key = ("front",) + key
            run = self._cached_graph(key, lambda: self._capture_synthesis(
                xb, tyb, front=front, length_scale=duration_rate, control=ctl is not None))
            # infer.py:173's np.random.randint(len - nl), drawn on the device
            # from raw words of numpy's own generator: the same start as the
            # reference, and the generator ends where the reference's does
            pool, state = ops.numpy_draw_pool()
            if ctl is None:
                res = run(text_t, emo, sid, noise_start=pool, x_length=t_x)
            else:
                res = run(text_t, emo, sid, noise_start=pool, x_length=t_x, rate=duration_rate,
                          control=dict(given=ctl[0], tok_scale=ctl[1], target=ctl[2]))
            head, res = (res[:2], res[2:]) if front else (res[:1], res[1:])
            wav, y_len = head[0], res[0]
            dur = res[1] if ctl is not None else None
            posted = None if post is None else post(wav[0], y_len[0])
            if ctl is None:
                n, used = (int(v) for v in y_len[:, 0].tolist())  # (synchronises)
            else:  # the durations ride in the y_len read: still one small copy
                host = torch.cat([y_len[:, 0], dur[0, :t_x]]).tolist()
                n, used = host[:2]
                if got is not None and n <= tyb:
                    del got[:]
                    got.append(np.asarray(host[2:], np.int32))
            if n <= tyb and used == -2:
                # every word of the pool was rejected (p < 2^-32): numpy's
                # randint would go on drawing - advance past the pool and
                # replay with the next words of the same stream
                ops.numpy_draw_commit(state, ops.ED_DRAWS)
                continue
            if n <= tyb:
                if used < 0:
                    raise self._misfit(state, n)
                ops.numpy_draw_commit(state, used)
                if front:
                    return head, n
                if post is not None:
                    return posted, n
                return wav[0, 0, :n * self.hop_size].float().cpu().numpy()
            self._grow_bucket(memo, state, tyb, n)  # re-run at a larger bucket: same draw


def main(argv=None):
    import argparse
    import time

    from scipy.io import wavfile

    ap = argparse.ArgumentParser(description="Decode text vectors with vits_amd (EmoVITS).")
    ap.add_argument("--scpfn", "--scp", required=True)
    ap.add_argument("--spkid", "--sid", default=None, type=int)
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--checkpoint", "--ckpt", default=None)
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    os.makedirs(args.outdir, exist_ok=True)
    model = EmoVITS(args.checkpoint, args.device, loglv=1)
    total_rtf, n = 0.0, 0
    with open(args.scpfn) as fid:
        for line in fid:
            line = line.strip()
            if not line or line[0] == "#":
                continue
            parts = line.split("|")
            utt_id = os.path.splitext(os.path.basename(parts[0]))[0]
            spkid = int(args.spkid) if args.spkid is not None else (int(parts[-1]) if len(parts) > 1 else 1)
            start = time.time()
            text = np.fromfile(parts[0], dtype=np.float32).reshape(-1, model.text_channels)
            wav, _ = model.infer(spkid, text, None)
            wavfile.write(os.path.join(args.outdir, f"{utt_id}.wav"), model.sampling_rate,
                          np.clip(wav * 32767, -32768, 32767).astype(np.int16))
            total_rtf += (time.time() - start) / (len(wav) / model.sampling_rate)
            n += 1
    sys.stderr.write(f"Finished generation of {n} utterances (RTF = {total_rtf / max(1, n):.03f}).\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

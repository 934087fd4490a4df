"""VITSWrap text-to-speech wrapper (reference ``vits_wrap.py``).

``speaking(dict) -> dict`` keeps the reference contract (vits_wrap.py:168-218):
chunked text -> front-end -> ``EmoVITS.infer`` -> pitch / sampling-rate
resampling -> int16 PCM with a RIFF header, plus segment info, front/back-end
times (ms) and RTF.  The reference's text front-end (``textparser``) is a
private package absent from the reference tree, so it is *pluggable*: pass
any object with ``__call__(utt_id, text) -> (utt_id, segtext, vec[N, c])``,
``max_utt_length`` and ``update()``.  librosa is replaced by
``scipy.signal.resample_poly`` for the resampling steps.
"""
from __future__ import annotations

import struct
import time

import numpy as np
import torch

from . import ops
from .infer import EmoVITS, PcmRequest


def _gen_wav_header(sample_num, sample_rate=8000, bit_num=16):
    """44-byte PCM RIFF header (vits_wrap.py:16-26)."""
    h = b"RIFF" + struct.pack("i", sample_num * 2 + 44 - 8)
    h += b"WAVEfmt \x10\x00\x00\x00\x01\x00\x01\x00"
    h += struct.pack("i", sample_rate) + struct.pack("i", sample_rate * bit_num // 8)
    h += struct.pack("H", bit_num // 8) + struct.pack("H", bit_num)
    h += b"data" + struct.pack("i", sample_num * 2)
    return h


def _resample(wav, orig_sr, target_sr):
    from scipy.signal import resample_poly

    if orig_sr == target_sr:
        return wav
    up, down = ops.resample_ratio(orig_sr, target_sr)
    return resample_poly(wav, up, down).astype(np.float32)


def host_pcm(wav, model_sr, pitch, sampling_rate, volume, tail_silence):
    """The host output stage of ``speaking`` (vits_wrap.py:186-197): pitch
    and sampling-rate resampling, volume, clip, int16, tail silence."""
    if pitch != 1.0:
        wav = _resample(wav, int(model_sr / pitch), model_sr)
    if sampling_rate != model_sr:
        wav = _resample(wav, model_sr, sampling_rate)
    wav = np.clip(wav * volume * 32767, -32768, 32767).astype(np.int16)
    if tail_silence > 0:
        wav = np.pad(wav, [0, int(tail_silence * sampling_rate)])
    return wav


class VITSWrap(object):
    default_spkid = 1
    default_volume = 1.0
    default_speed = 1.0
    default_pitch = 1.0
    default_tail_silece = 0.0

    # batch_segments batches a request of at least this many segments; fewer
    # run one after another (measured crossover: profiles/serve_batch_ab.txt)
    BATCH_MIN_SEGMENTS = 2
    # speaking_many batches a call of at least this many segments in all;
    # fewer run through speaking (measured crossover: profiles/serve_mixed_ab.txt)
    MANY_MIN_ROWS = 2

    def __init__(self, ckpt_path: str = None, device: torch.device = None, loglv: int = 0, *,
                 textparser=None, speecher: EmoVITS = None, device_post: bool = False,
                 batch_segments: bool = False):
        """device_post: run the output stage (resampling, volume, int16, tail
        silence) on the GPU behind the synthesis (EmoVITS.infer_pcm) and copy
        only the int16 PCM to the host; off: the host chain (scipy / numpy).
        batch_segments (CUDA only; implies device_post): the front end runs
        over all segments of a request first, then ONE
        EmoVITS.infer_pcm_batch call synthesises them (one graph replay per
        16 segments, one device-to-host copy); same result, same dict."""
        if textparser is None:
            raise ValueError("VITSWrap needs a text front-end (the reference's private `textparser` "
                             "is not available): pass textparser=...")
        self.loglv = loglv
        self.textparser = textparser
        self.speecher = speecher if speecher is not None else EmoVITS(ckpt_path, device=device)
        self.batch_segments = bool(batch_segments) and self.speecher.device.type == "cuda"
        self.device_post = ((bool(device_post) or self.batch_segments)
                            and self.speecher.device.type == "cuda")
        self.asv = None  # optional bandwidth extension (fbandext) is not part of the reference tree
        self.default_sampling_rate = self.speecher.sampling_rate
        self.max_utt_length = getattr(self.textparser, "max_utt_length", 256)

    def update(self):
        if hasattr(self.textparser, "update"):
            self.textparser.update()
        self.speecher.update()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    def _parse_input(self, inputs):
        volume = max(0.0, min(1.0, float(inputs.get("volume", self.default_volume))))
        speed = max(0.5, min(2.0, float(inputs.get("speed", self.default_speed))))
        pitch = max(0.5, min(2.0, float(inputs.get("pitch", self.default_pitch))))
        sampling_rate = min(48000, max(8000, int(inputs.get("sampling_rate", self.default_sampling_rate))))
        tail_silence = float(inputs.get("tail_silence", self.default_tail_silece))
        speed /= pitch
        utt_id = inputs.get("id", str(time.time()).replace(".", "_"))
        return (inputs, utt_id, inputs.get("text", "。"), int(inputs.get("spkid", self.default_spkid)),
                volume, speed, pitch, sampling_rate, tail_silence, inputs.get("emotion"))

    def _split_utt_text(self, utt_id, utt_text):
        """Split long input at sentence punctuation into chunks of at most
        max_utt_length characters (vits_wrap.py:101-166, simplified: the
        reference's punctuation ranking is front-end specific)."""
        puncs = "。！？；!?;，,、 "
        out_id, out_txt, i = [], [], 0
        while utt_text:
            if len(utt_text) <= self.max_utt_length:
                out_id.append(f"{utt_id}-{i}")
                out_txt.append(utt_text)
                break
            cut = max(utt_text.rfind(p, 0, self.max_utt_length) for p in puncs)
            cut = self.max_utt_length if cut <= 0 else cut + 1
            out_id.append(f"{utt_id}-{i}")
            out_txt.append(utt_text[:cut])
            utt_text = utt_text[cut:]
            i += 1
        return out_id, out_txt

    def _duration_controls(self, inputs, n_segments, what):
        """The duration controls of a request: None, or the keyword arguments
        of EmoVITS.infer / infer_pcm.  ``durations`` (frames per token of the
        front end's vector sequence, < 0: predicted), ``token_scale`` (a
        factor per token), ``duration_s`` (the utterance lasts round(s * rate
        / hop) frames of the model, before the output stage).  They address
        the tokens of ONE segment: text that _split_utt_text cuts is refused,
        as in ``aligning``."""
        d, s, sec = inputs.get("durations"), inputs.get("token_scale"), inputs.get("duration_s")
        if d is None and s is None and sec is None:
            return None
        if n_segments != 1:
            raise ValueError(f"{what}: the text splits into {n_segments} segments of at most "
                             f"{self.max_utt_length} characters; duration controls address the "
                             "tokens of one segment")
        target = None
        if sec is not None:
            sec = float(sec)
            sp = self.speecher
            if not np.isfinite(sec) or sec <= 0:
                raise ValueError(f"{what}: duration_s must be a positive number, got {sec}")
            target = int(round(sec * sp.sampling_rate / sp.hop_size))
            if target < 1:
                raise ValueError(f"{what}: duration_s = {sec} is less than one frame")
        return dict(durations=d, token_scale=s, target_frames=target, return_durations=True)

    def _with_durations(self, out, durations):
        sp = self.speecher
        out["durations"] = durations
        out["boundaries_s"] = (np.concatenate([[0], np.cumsum(durations, dtype=np.int64)])
                               * (sp.hop_size / sp.sampling_rate))
        return out

    @torch.no_grad()
    def speaking(self, inputs: dict) -> dict:
        """One synthesis request (vits_wrap.py:168-218).  ``durations`` /
        ``token_scale`` / ``duration_s`` in the request (see
        _duration_controls) control the timing of a one-segment text;
        the result then also holds ``durations`` (int32 [Tx], the frames per
        token that were spoken) and ``boundaries_s`` (float64 [Tx + 1], at the
        model's rate, before pitch and rate changes)."""
        inputs, utt_id, utt_text, spkid, volume, speed, pitch, sampling_rate, tail_silence, emotion = \
            self._parse_input(inputs)
        ids, texts = self._split_utt_text(utt_id, utt_text)
        ctl = self._duration_controls(inputs, len(texts), "speaking")
        if ctl is not None:
            t0 = time.time()
            _, segtext, vec = self.textparser(ids[0], texts[0])
            t1 = time.time()
            if self.device_post:
                wav, emotion, n_model, dur = self.speecher.infer_pcm(
                    spkid, vec, emotion, duration_rate=speed, pitch=pitch,
                    sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence, **ctl)
            else:
                wav, emotion, dur = self.speecher.infer(spkid, vec, emotion, duration_rate=speed,
                                                        **ctl)
                n_model = len(wav)
                wav = host_pcm(wav, self.default_sampling_rate, pitch, sampling_rate, volume,
                               tail_silence)
            out = self._finish(inputs, texts, [segtext], [len(wav)], [wav], n_model,
                               sampling_rate, t1 - t0, time.time() - t1)
            return self._with_durations(out, dur)
        batch_wav, batch_wavlen = [], 0
        segtexts, seg_samples = [], []  # per segment: front-end text, PCM samples (tail included)
        t_front, t_back = 0.0, 0.0
        if self.batch_segments and len(texts) >= self.BATCH_MIN_SEGMENTS:
            t0 = time.time()
            parsed = [self.textparser(uid, text) for uid, text in zip(ids, texts)]
            t1 = time.time()
            t_front = t1 - t0
            # the first segment looks the emotion up (its draw comes before
            # every noise draw, as in the loop below); the others reuse it
            _, emotion = self.speecher._resolve(spkid, emotion)
            pcm, offsets, _, n_model = self.speecher.infer_pcm_batch(
                [(spkid, vec, emotion) for _, _, vec in parsed], duration_rate=speed, pitch=pitch,
                sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence)
            batch_wav.append(pcm)
            batch_wavlen = sum(n_model)
            segtexts = [segtext for _, segtext, _ in parsed]
            seg_samples = [int(n) for n in np.diff(offsets)]
            t_back = time.time() - t1
        else:
            for uid, text in zip(ids, texts):
                t0 = time.time()
                uid, segtext, vec = self.textparser(uid, text)
                t1 = time.time()
                t_front += t1 - t0
                if self.device_post:
                    wav, emotion, n_model = self.speecher.infer_pcm(
                        spkid, vec, emotion, duration_rate=speed, pitch=pitch,
                        sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence)
                    batch_wavlen += n_model
                else:
                    wav, emotion = self.speecher.infer(spkid, vec, emotion, duration_rate=speed)
                    batch_wavlen += len(wav)
                    wav = host_pcm(wav, self.default_sampling_rate, pitch, sampling_rate, volume,
                                   tail_silence)
                batch_wav.append(wav)
                segtexts.append(segtext)
                seg_samples.append(len(wav))
                t_back += time.time() - t1
        return self._finish(inputs, texts, segtexts, seg_samples, batch_wav, batch_wavlen,
                            sampling_rate, t_front, t_back)

    def speaking_stream(self, inputs: dict):
        """``speaking``, streamed: an iterator of bytes whose first item is
        the 44-byte RIFF header with the exact final length and whose items,
        joined, are ``speaking(inputs)["wav"]``, byte for byte, with numpy's
        generator left where ``speaking`` leaves it.  The front end and the
        text side of EVERY segment run before this returns (one batched
        front replay with batch_segments=True, else one per segment), so the
        header is exact before any audio exists; the segments' chunks then
        follow in order as they are decoded (EmoVITS.infer_pcm_stream), each
        segment's tail silence in its last chunk.  ``first_chunk_frames`` /
        ``chunk_frames`` in the request set the chunk sizes; ``durations`` /
        ``token_scale`` / ``duration_s`` control a one-segment text as in
        ``speaking``.  Needs device_post=True on a ROCm GPU."""
        if not self.device_post:
            raise ValueError("VITSWrap.speaking_stream needs device_post=True on a ROCm GPU")
        inputs, utt_id, utt_text, spkid, volume, speed, pitch, sampling_rate, tail_silence, emotion = \
            self._parse_input(inputs)
        ids, texts = self._split_utt_text(utt_id, utt_text)
        ctl = self._duration_controls(inputs, len(texts), "speaking_stream")
        parsed = [self.textparser(uid, text) for uid, text in zip(ids, texts)]
        sp = self.speecher
        kw = dict(first_chunk_frames=inputs.get("first_chunk_frames"),
                  chunk_frames=inputs.get("chunk_frames"), duration_rate=speed, pitch=pitch,
                  sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence)
        with torch.no_grad():
            if ctl is not None:
                ctl = {k: v for k, v in ctl.items() if k != "return_durations"}
                streams = [sp.infer_pcm_stream(spkid, parsed[0][2], emotion, **kw, **ctl)]
            else:
                # one emotion lookup for the request, before every noise draw (speaking's order)
                _, emotion = sp._resolve(spkid, emotion)
                streams = sp.infer_pcm_streams(
                    [(spkid, vec, emotion) for _, _, vec in parsed],
                    batch=self.batch_segments and len(texts) >= self.BATCH_MIN_SEGMENTS, **kw)

        def items():
            yield _gen_wav_header(sum(s.n_samples for s in streams), sampling_rate, 16)
            for s in streams:
                for chunk in s:
                    yield chunk.tobytes()

        return items()

    def _finish(self, inputs, texts, segtexts, seg_samples, batch_wav, batch_wavlen, sampling_rate,
                t_front, t_back):
        """The result dict of ``speaking`` (vits_wrap.py:199-218)."""
        segment_info, start_ms, end_ms = [], 0.0, 0.0
        for text, segtext, n in zip(texts, segtexts, seg_samples):
            end_ms += n / sampling_rate * 1000
            segment_info.append({"start_ms": start_ms, "end_ms": end_ms, "input_text": text,
                                 "segtext": segtext.printer() if hasattr(segtext, "printer") else str(segtext)})
            start_ms = end_ms
        rtf = (t_front + t_back) / max(1e-9, batch_wavlen / self.default_sampling_rate)
        pcm = b"".join(w.tobytes() for w in batch_wav)
        out = inputs
        out["wav"] = _gen_wav_header(len(pcm) // 2, sampling_rate, 16) + pcm
        out["sr"] = sampling_rate
        out["segment_info"] = segment_info
        out["time_used_frontend"] = t_front * 1000
        out["time_used_backend"] = t_back * 1000
        out["rtf"] = rtf
        return out

    @torch.no_grad()
    def converting(self, inputs: dict) -> dict:
        """Voice conversion request: {"wav" (int16 or float samples),
        "sampling_rate_in", "spkid_src", "spkid_tgt", "pitch",
        "sampling_rate", "volume", "tail_silence", "id"} -> the dict of
        ``speaking`` without its text fields: "wav" (RIFF bytes), "sr",
        "segment_info" (one entry, start_ms / end_ms), the times and rtf.
        Clamps as in ``speaking``.  Needs device_post=True: the recording is
        converted and post-processed on the GPU (EmoVITS.convert_pcm; a
        recording of more than 4096 frames: convert_pcm_long, seamless
        windows) and only the int16 PCM comes back."""
        if not self.device_post:
            raise ValueError("VITSWrap.converting needs device_post=True on a ROCm GPU")
        volume = max(0.0, min(1.0, float(inputs.get("volume", self.default_volume))))
        pitch = max(0.5, min(2.0, float(inputs.get("pitch", self.default_pitch))))
        sampling_rate = min(48000, max(8000, int(inputs.get("sampling_rate",
                                                            self.default_sampling_rate))))
        tail_silence = float(inputs.get("tail_silence", self.default_tail_silece))
        inputs.setdefault("id", str(time.time()).replace(".", "_"))
        spkid_tgt = int(inputs.get("spkid_tgt", self.default_spkid))
        t0 = time.time()
        # a recording past the largest conversion bucket runs as seamless windows
        ev = self.speecher
        frames = ev._vc_lengths(np.asarray(inputs["wav"]).reshape(-1).shape[0],
                                inputs.get("sampling_rate_in"))[2]
        convert = ev.convert_pcm_long if frames > ev.VC_MAX_FRAMES else ev.convert_pcm
        pcm, n_model = convert(
            inputs["wav"], int(inputs["spkid_src"]), spkid_tgt,
            sampling_rate_in=inputs.get("sampling_rate_in"), pitch=pitch,
            sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence)
        t_back = time.time() - t0
        out = inputs
        out["wav"] = _gen_wav_header(len(pcm), sampling_rate, 16) + pcm.tobytes()
        out["sr"] = sampling_rate
        out["segment_info"] = [{"start_ms": 0.0, "end_ms": len(pcm) / sampling_rate * 1000}]
        out["time_used_frontend"] = 0.0
        out["time_used_backend"] = t_back * 1000
        out["rtf"] = t_back / max(1e-9, n_model / self.default_sampling_rate)
        return out

    @torch.no_grad()
    def retiming(self, inputs: dict) -> dict:
        """Retiming request: the fields of ``converting`` ("spkid_tgt"
        defaults to "spkid_src": the take keeps its voice) plus "speed" (1.1:
        ten per cent slower; clamped to 0.5 .. 2 as in ``speaking``),
        "duration_s" (the result lasts round(s * rate / hop) model frames;
        speed is then not applied), and optionally "text" (what the recording
        says, one segment) with "emotion", and with it "durations" (frames
        per token of the front end's vector sequence, < 0: free) and
        "token_scale" (a factor per token).  Pitch changes and the length
        stays: the durations' rate is speed / pitch.  -> the dict of
        ``converting`` plus "length_s" (the result's seconds at the model's
        rate, before pitch and rate changes) and, with text, "durations_old"
        (int32 [Tx], the recording's alignment), "durations" (int32 [Tx], the
        frames per token of the result) and "boundaries_s" (of the result).
        Needs device_post=True on a ROCm GPU (EmoVITS.retime_pcm); recordings
        of at most 4096 frames."""
        if not self.device_post:
            raise ValueError("VITSWrap.retiming needs device_post=True on a ROCm GPU")
        if "wav" not in inputs or "spkid_src" not in inputs:
            raise ValueError("retiming needs the recording (wav) and its speaker (spkid_src)")
        volume = max(0.0, min(1.0, float(inputs.get("volume", self.default_volume))))
        speed = max(0.5, min(2.0, float(inputs.get("speed", self.default_speed))))
        pitch = max(0.5, min(2.0, float(inputs.get("pitch", self.default_pitch))))
        sampling_rate = min(48000, max(8000, int(inputs.get("sampling_rate",
                                                            self.default_sampling_rate))))
        tail_silence = float(inputs.get("tail_silence", self.default_tail_silece))
        utt_id = inputs.setdefault("id", str(time.time()).replace(".", "_"))
        sp = self.speecher
        text = inputs.get("text")
        if text is None and (inputs.get("durations") is not None
                             or inputs.get("token_scale") is not None):
            raise ValueError("retiming: durations and token_scale are per token: they need text")
        target = None
        if inputs.get("duration_s") is not None:
            sec = float(inputs["duration_s"])
            if not np.isfinite(sec) or sec <= 0:
                raise ValueError(f"retiming: duration_s must be a positive number, got {sec}")
            target = int(round(sec * sp.sampling_rate / sp.hop_size))
            if target < 1:
                raise ValueError(f"retiming: duration_s = {sec} is less than one frame")
        vec = None
        t0 = time.time()
        if text is not None:
            ids, texts = self._split_utt_text(utt_id, text)
            if len(texts) != 1:
                raise ValueError(f"retiming: the text splits into {len(texts)} segments of at "
                                 f"most {self.max_utt_length} characters; one segment per "
                                 "recording")
            _, _, vec = self.textparser(ids[0], texts[0])
        t1 = time.time()
        spkid_src = int(inputs["spkid_src"])
        pcm, n_model, d_old, d_new, _ = sp.retime_pcm(
            inputs["wav"], spkid_src, int(inputs.get("spkid_tgt", spkid_src)), speed=speed,
            target_frames=target, text=vec, emo=inputs.get("emotion"),
            durations=inputs.get("durations"), token_scale=inputs.get("token_scale"),
            sampling_rate_in=inputs.get("sampling_rate_in"), pitch=pitch,
            sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence,
            return_durations=True)
        t_back = time.time() - t1
        out = inputs
        out["wav"] = _gen_wav_header(len(pcm), sampling_rate, 16) + pcm.tobytes()
        out["sr"] = sampling_rate
        out["segment_info"] = [{"start_ms": 0.0, "end_ms": len(pcm) / sampling_rate * 1000}]
        out["time_used_frontend"] = (t1 - t0) * 1000
        out["time_used_backend"] = t_back * 1000
        out["rtf"] = t_back / max(1e-9, n_model / self.default_sampling_rate)
        out["length_s"] = n_model / sp.sampling_rate
        if text is not None:
            out["durations_old"] = d_old
            self._with_durations(out, d_new)
        return out

    @torch.no_grad()
    def speaking_like(self, inputs: dict) -> dict:
        """``text`` in the voice of ``spkid`` with the timing of a recording:
        {"wav", "sampling_rate_in", "spkid_src", "text"} as ``aligning`` takes
        them (spkid_src: the recording's speaker) plus the fields of
        ``speaking`` for the target voice.  One alignment graph replay whose
        durations go device to device into the controlled synthesis graph,
        then that replay (EmoVITS.infer_pcm_like): the result of ``aligning``
        followed by ``speaking`` with its durations, byte for byte, without
        the durations visiting the host in between.  One-segment text only;
        needs device_post=True on a ROCm GPU."""
        if not self.device_post:
            raise ValueError("VITSWrap.speaking_like needs device_post=True on a ROCm GPU")
        inputs, utt_id, utt_text, spkid, volume, speed, pitch, sampling_rate, tail_silence, emotion = \
            self._parse_input(inputs)
        ids, texts = self._split_utt_text(utt_id, utt_text)
        if len(texts) != 1:
            raise ValueError(f"speaking_like: the text splits into {len(texts)} segments of at "
                             f"most {self.max_utt_length} characters; one segment per recording")
        if "spkid_src" not in inputs or "wav" not in inputs:
            raise ValueError("speaking_like needs the recording (wav) and its speaker (spkid_src)")
        rec = inputs.pop("wav")
        t0 = time.time()
        _, segtext, vec = self.textparser(ids[0], texts[0])
        t1 = time.time()
        wav, emotion, n_model, dur = self.speecher.infer_pcm_like(
            rec, int(inputs["spkid_src"]), spkid, vec, emotion,
            sampling_rate_in=inputs.get("sampling_rate_in"), pitch=pitch,
            sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence,
            return_durations=True)
        out = self._finish(inputs, texts, [segtext], [len(wav)], [wav], n_model, sampling_rate,
                           t1 - t0, time.time() - t1)
        return self._with_durations(out, dur)

    @torch.no_grad()
    def editing(self, inputs: dict) -> dict:
        """Speech-editing request: {"wav" (the recording, int16 or float
        samples), "sampling_rate_in", "spkid", "text" (what the recording
        says), "text_new" (what it should say), "emotion", "duration_s" (the
        re-spoken span lasts round(s * rate / hop) frames) or "keep_length"
        (it lasts what the replaced span did), "patch" (default True: the
        recording's own samples outside the edit), and the output fields of
        ``converting``} -> the dict of ``converting`` plus "durations" (int32
        [Tx_new], the frames per token of the result), "boundaries_s",
        "scores" (float32 [Tx_old], the alignment's) and "span_s": {"old":
        (start, end), "new": (start, end)}, the edited region in seconds of
        the recording and of the result at the model's rate.  The span is the
        one EmoVITS.edit_span finds between the two vector sequences.  Both
        texts must be one segment each; needs device_post=True on a ROCm GPU
        (EmoVITS.edit_pcm)."""
        if not self.device_post:
            raise ValueError("VITSWrap.editing needs device_post=True on a ROCm GPU")
        inputs, utt_id, utt_text, spkid, volume, _, pitch, sampling_rate, tail_silence, emotion = \
            self._parse_input(inputs)
        if "wav" not in inputs or "text_new" not in inputs:
            raise ValueError("editing needs the recording (wav), its text and text_new")
        parsed = []
        for what, text in (("text", utt_text), ("text_new", inputs["text_new"])):
            ids, texts = self._split_utt_text(utt_id, text)
            if len(texts) != 1:
                raise ValueError(f"editing: {what} splits into {len(texts)} segments of at most "
                                 f"{self.max_utt_length} characters; one segment per recording")
            parsed.append((ids[0], texts[0]))
        sp = self.speecher
        span_frames = None
        if inputs.get("duration_s") is not None and inputs.get("keep_length"):
            raise ValueError("editing: give duration_s or keep_length, not both")
        if inputs.get("keep_length"):
            span_frames = "keep"
        elif inputs.get("duration_s") is not None:
            sec = float(inputs["duration_s"])
            if not np.isfinite(sec) or sec <= 0:
                raise ValueError(f"editing: duration_s must be a positive number, got {sec}")
            span_frames = int(round(sec * sp.sampling_rate / sp.hop_size))
            if span_frames < 1:
                raise ValueError(f"editing: duration_s = {sec} is less than one frame")
        rec = inputs.pop("wav")
        t0 = time.time()
        (_, segtext, vec_old), (_, segtext_new, vec_new) = [self.textparser(i, t) for i, t in parsed]
        t1 = time.time()
        pcm, n_model, dur, (f0, n_new, f1), scores = sp.edit_pcm(
            rec, spkid, vec_old, vec_new, emotion, sampling_rate_in=inputs.get("sampling_rate_in"),
            span_frames=span_frames, patch=bool(inputs.get("patch", True)), pitch=pitch,
            sampling_rate=sampling_rate, volume=volume, tail_silence=tail_silence)
        out = self._finish(inputs, [parsed[1][1]], [segtext_new], [len(pcm)], [pcm], n_model,
                           sampling_rate, t1 - t0, time.time() - t1)
        sec = sp.hop_size / sp.sampling_rate
        out["scores"] = scores
        out["span_s"] = {"old": (f0 * sec, f1 * sec), "new": (f0 * sec, (f0 + n_new) * sec)}
        return self._with_durations(out, dur)

    @torch.no_grad()
    def aligning(self, inputs: dict) -> dict:
        """Forced-alignment request: {"wav" (int16 or float samples), "text",
        "spkid", "emotion", "sampling_rate_in", "id"} -> the same dict plus
        "durations" (int32 [Tx], frames per token of the front end's vector
        sequence), "boundaries_s" (float64 [Tx + 1]: token i spans
        boundaries_s[i] .. boundaries_s[i + 1] seconds of the recording at the
        model's rate), "scores" (float32 [Tx]), "frames", "segtext", and the
        timing fields of ``speaking`` (time_used_frontend / _backend in ms,
        rtf against the recording's duration).  The text must be one segment:
        text that _split_utt_text would cut is refused (ValueError), because
        the recording cannot be cut to match before it is aligned.  Unlike
        ``converting`` this needs no device_post: there is no output stage,
        only durations come back; it needs a ROCm GPU (EmoVITS.align)."""
        utt_id = inputs.setdefault("id", str(time.time()).replace(".", "_"))
        spkid = int(inputs.get("spkid", self.default_spkid))
        ids, texts = self._split_utt_text(utt_id, inputs.get("text", "。"))
        if len(texts) != 1:
            raise ValueError(f"aligning: the text splits into {len(texts)} segments of at most "
                             f"{self.max_utt_length} characters; align one segment per recording")
        t0 = time.time()
        _, segtext, vec = self.textparser(ids[0], texts[0])
        t1 = time.time()
        durations, scores, frames = self.speecher.align(
            inputs["wav"], spkid, vec, inputs.get("emotion"),
            sampling_rate_in=inputs.get("sampling_rate_in"))
        t_back = time.time() - t1
        sp = self.speecher
        out = inputs
        out["durations"] = durations
        out["boundaries_s"] = (np.concatenate([[0], np.cumsum(durations, dtype=np.int64)])
                               * (sp.hop_size / sp.sampling_rate))
        out["scores"] = scores
        out["frames"] = frames
        out["segtext"] = segtext.printer() if hasattr(segtext, "printer") else str(segtext)
        out["time_used_frontend"] = (t1 - t0) * 1000
        out["time_used_backend"] = t_back * 1000
        out["rtf"] = (t1 - t0 + t_back) / max(1e-9, frames * sp.hop_size / sp.sampling_rate)
        return out

    @torch.no_grad()
    def aligning_long(self, inputs: dict) -> dict:
        """``aligning`` for a recording of any length whose text may split
        into any number of segments: the request dict of ``aligning`` -> the
        same dict plus flat "durations" (int32, the tokens of all segments in
        order), "boundaries_s" (float64, one more entry than tokens),
        "scores" (float32) and "frames" as there, "segtext" (a list, one per
        segment) and "segments": a list of {"text", "start_s", "end_s",
        "durations", "scores"}, one per segment, with the seconds of the
        recording (at the model's rate) at which the segment starts and ends:
        the points at which to cut it.  The segments share one emotion lookup,
        as in ``speaking``.  Timing fields as in ``aligning``.  Needs a ROCm
        GPU (EmoVITS.align_long)."""
        utt_id = inputs.setdefault("id", str(time.time()).replace(".", "_"))
        spkid = int(inputs.get("spkid", self.default_spkid))
        ids, texts = self._split_utt_text(utt_id, inputs.get("text", "。"))
        t0 = time.time()
        parsed = [self.textparser(uid, text) for uid, text in zip(ids, texts)]
        t1 = time.time()
        sp = self.speecher
        _, emotion = sp._resolve(spkid, inputs.get("emotion"))
        durations, scores, seg_frames, frames = sp.align_long(
            inputs["wav"], spkid, [vec for _, _, vec in parsed], [emotion] * len(parsed),
            sampling_rate_in=inputs.get("sampling_rate_in"))
        t_back = time.time() - t1
        sec = sp.hop_size / sp.sampling_rate
        out = inputs
        out["durations"] = np.concatenate(durations)
        out["boundaries_s"] = (np.concatenate([[0], np.cumsum(out["durations"], dtype=np.int64)])
                               * sec)
        out["scores"] = np.concatenate(scores)
        out["frames"] = frames
        out["segtext"] = [s.printer() if hasattr(s, "printer") else str(s) for _, s, _ in parsed]
        out["segments"] = [
            {"text": texts[i], "start_s": float(seg_frames[i] * sec),
             "end_s": float(seg_frames[i + 1] * sec), "durations": durations[i],
             "scores": scores[i]} for i in range(len(parsed))]
        out["time_used_frontend"] = (t1 - t0) * 1000
        out["time_used_backend"] = t_back * 1000
        out["rtf"] = (t1 - t0 + t_back) / max(1e-9, frames * sec)
        return out

    @torch.no_grad()
    def speaking_many(self, list_of_inputs) -> list:
        """``speaking`` for several requests at once: one dict per input, the
        same ``wav``, ``sr`` and ``segment_info`` as ``[speaking(i) for i in
        list_of_inputs]``.  With batch_segments=True and at least
        MANY_MIN_ROWS segments in all, the front end runs over all segments
        of all requests, then ONE EmoVITS.infer_pcm_requests call synthesises
        them: requests with different speed, pitch, sampling rate, volume and
        tail share graph replays of up to 16 rows, whatever their controls.
        Every dict then reports the front-end and back-end times of the whole
        call (the requests are not timed apart) and the call's rtf.  A request
        without an explicit emotion id draws it before any noise draw of the
        call (see infer_pcm_requests); with explicit emotions numpy's
        generator ends where the loop leaves it.  Otherwise: the loop."""
        list_of_inputs = list(list_of_inputs)
        if any(i.get(k) is not None for i in list_of_inputs
               for k in ("durations", "token_scale", "duration_s")):
            # a request with duration controls: the loop (speaking serves it)
            return [self.speaking(inputs) for inputs in list_of_inputs]
        parsed = [self._parse_input(inputs) for inputs in list_of_inputs] \
            if self.batch_segments else []
        split = [self._split_utt_text(p[1], p[2]) for p in parsed]
        if not self.batch_segments or sum(len(t) for _, t in split) < self.MANY_MIN_ROWS:
            return [self.speaking(inputs) for inputs in list_of_inputs]
        t0 = time.time()
        front = [[self.textparser(uid, text) for uid, text in zip(ids, texts)]
                 for ids, texts in split]
        t1 = time.time()
        requests = []
        for p, segs in zip(parsed, front):
            _, _, _, spkid, volume, speed, pitch, sampling_rate, tail_silence, emotion = p
            _, emotion = self.speecher._resolve(spkid, emotion)
            requests.append(PcmRequest([(spkid, vec, emotion) for _, _, vec in segs],
                                       duration_rate=speed, pitch=pitch,
                                       sampling_rate=sampling_rate, volume=volume,
                                       tail_silence=tail_silence))
        results = self.speecher.infer_pcm_requests(requests)
        t_front, t_back = t1 - t0, time.time() - t1
        total = sum(sum(n_model) for _, _, _, n_model in results)
        outs = []
        for p, (_, texts), segs, (pcm, offsets, _, _) in zip(parsed, split, front, results):
            outs.append(self._finish(p[0], texts, [segtext for _, segtext, _ in segs],
                                     [int(n) for n in np.diff(offsets)], [pcm], total, p[7],
                                     t_front, t_back))
        return outs

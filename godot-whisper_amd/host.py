"""Host-side mirror of the GDExtension node that owns the boundary
(`SpeechToText`, src/speech_to_text.cpp:106-573) and of the two GDScript call patterns
(`AudioStreamToText.get_text`, addon/audio_stream_to_text.gd:31-62;
`CaptureStreamToText.transcribe_thread`, addon/capture_stream_to_text.gd:65-120).

Godot / godot-cpp / SCons are not in this image, so the node is restated in Python over the
same C ABI calls, in the same order, with the same parameter set.  It works over ANY library
that exports whisper.h (`abi.WHISPER_API`): the product `libwhisper_mi355.so`, or —
in tests only — the compiled reference, which is how the parity tests drive both sides
through one code path.
"""
from __future__ import annotations

import ctypes as C
import math
import re

import numpy as np

from . import abi

# ProjectSettings defaults, src/register_types.cpp:64-69 (spelling is the reference's)
SETTINGS = {
    "audio/input/transcribe/entropy_treshold": 2.8,
    "audio/input/transcribe/freq_treshold": 200.0,
    "audio/input/transcribe/max_tokens": 16,
    "audio/input/transcribe/vad_treshold": 2.0,
    "audio/input/transcribe/use_gpu": True,
    "audio/input/transcribe/speed_up_2x": False,
}


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class SpeechToText:
    """One `whisper_context` per node (src/speech_to_text.h:135); not re-entrant."""

    def __init__(self, lib: C.CDLL, settings: dict | None = None, no_speech: int = 0, token_dtw=False, grammar=None,
                 grammar_penalty: float = 100.0, grammar_device: bool = False, speaker_labels=False, speaker_ratio: float = 1.1,
                 wav_adpcm: bool = False):
        """grammar: rules in the format of abi.make_grammar (a list of rules, each a list of (type, value) without the closing END; rule 0
        is the start rule) — every full_params() then carries them with grammar_penalty; None: no grammar.
        grammar_device (product library only, include/wmi_device.h wmi_set_grammar_device): True — the grammar's reject masks and the
        penalised sampling run on the device; False — the reference's host path.
        token_dtw (product library only, include/wmi_device.h wmi_set_token_dtw): True — DTW token times over the default alignment
        heads — or a list of (layer, head) pairs; every token dictionary then gains "t_dtw" (10 ms units, -1 for a token that is no text).
        "t0" / "t1" stay the reference's.
        no_speech (product library only, include/wmi_device.h wmi_set_no_speech): 0 off — the reference's behaviour —, 1 report the
        windows' no-speech probability, 2 drop (OpenAI's rule), 3 gate.  The windows of a call are in last_windows after collect().
        speaker_labels (product library only, include/wmi_device.h wmi_set_speaker): True — the stereo clips of transcribe_wav*, and a
        capture session's steps, leave a dictionary per segment in last_speakers (t0, t1, text, "speaker" 0 / 1 / None, "channel_energy"
        (left, right)); "tokens" — with params.token_timestamps every token dictionary gains "speaker" as well.  speaker_ratio: how much
        louder a channel must be (whisper.cpp --diarize: 1.1).
        wav_adpcm (product library only, include/wmi_device.h wmi_set_wav_adpcm): True — transcribe_wav, transcribe_wav_long,
        transcribe_wav_batch, transcribe_wav_channels and AudioStreamToText.get_text_wav accept format 2 (AudioStreamWAV.FORMAT_IMA_ADPCM):
        the compressed bytes are decoded on the device.  False — format 2 is refused (last_ret -111), as ever."""
        self.lib = lib
        self.ctx = None
        self.no_speech = int(no_speech)
        self.token_dtw = token_dtw
        self.grammar_device = bool(grammar_device)
        self.speaker_labels, self.speaker_ratio = speaker_labels, float(speaker_ratio)
        self.last_speakers = []
        self._speaker_called = False
        self.wav_adpcm = bool(wav_adpcm)
        self._adpcm_called = False
        self.grammar_penalty = float(grammar_penalty)
        self._grammar = None
        self.set_grammar(grammar, grammar_penalty)
        self.last_windows = []
        self.last_draft_status = {}
        self.language = "en"  # Language enum -> code, src/speech_to_text.cpp:117-324
        self.settings = dict(SETTINGS)
        if settings:
            self.settings.update(settings)
        self._keep = []

    # -- set_language_model / _load_model (src/speech_to_text.cpp:326-346)
    def set_language_model(self, model_bytes: bytes | None):
        self.lib.whisper_free(self.ctx)
        self.ctx = None
        if not model_bytes:
            return
        buf = C.create_string_buffer(model_bytes, len(model_bytes))
        cp = abi.whisper_context_params(bool(self.settings["audio/input/transcribe/use_gpu"]))
        self.ctx = self.lib.whisper_init_from_buffer_with_params(C.cast(buf, C.c_void_p), len(model_bytes), cp)
        del buf  # the loader only borrows the buffer during the call (W/whisper.cpp:3231-3240)
        self.set_no_speech(self.no_speech)
        self.set_token_dtw(self.token_dtw)
        self.set_grammar_device(self.grammar_device)
        self.set_speaker_labels(self.speaker_labels, self.speaker_ratio)
        self.set_wav_adpcm(self.wav_adpcm)

    def set_wav_adpcm(self, on: bool) -> int:
        """The context's IMA-ADPCM mode from the next WAV call on; returns the previous mode (0 without a context)."""
        self.wav_adpcm = bool(on)
        if not self.ctx or not (on or self._adpcm_called):                # (a node that never asks for the mode never makes the call)
            return 0
        self._adpcm_called = True
        return self.lib.wmi_set_wav_adpcm(self.ctx, abi.WAV_ADPCM_ON if on else abi.WAV_ADPCM_OFF)

    def set_speaker_labels(self, labels, ratio: float = 1.1) -> int:
        """The context's speaker mode from the next transcription call on (False, True or "tokens"); returns the previous mode (0
        without a context)."""
        self.speaker_labels, self.speaker_ratio = labels, float(ratio)
        if not self.ctx or not (labels or self._speaker_called):          # (a node that never asks for labels never makes the call)
            return 0
        self._speaker_called = True
        mode = abi.SPEAKER_TOKENS if labels == "tokens" else abi.SPEAKER_SEGMENTS if labels else abi.SPEAKER_OFF
        return self.lib.wmi_set_speaker(self.ctx, mode, self.speaker_ratio)

    def speakers(self) -> list:
        """A dictionary per segment the accessors show now: t0, t1, text, "speaker" (0, 1, None for the reference's "?") and
        "channel_energy" (left, right), "samples" (is0, is1).  Empty where the result carries no table (wmi_full_get_segment_speaker -2)."""
        lib, ctx, out = self.lib, self.ctx, []
        if not ctx or not self.speaker_labels:
            return out
        rec = abi.wmi_speaker()
        for i in range(lib.whisper_full_n_segments(ctx)):
            if lib.wmi_full_get_segment_speaker(ctx, i, C.byref(rec)) != 0:
                return []
            out.append({"t0": lib.whisper_full_get_segment_t0(ctx, i), "t1": lib.whisper_full_get_segment_t1(ctx, i),
                        "text": lib.whisper_full_get_segment_text(ctx, i), "speaker": rec.speaker if rec.speaker >= 0 else None,
                        "channel_energy": (rec.e0, rec.e1), "samples": (rec.is0, rec.is1)})
        return out

    def set_grammar(self, rules, penalty: float = 100.0):
        """The grammar of every later full_params() (None: none).  The element arrays stay referenced by this node."""
        self.grammar_penalty = float(penalty)
        self._grammar = abi.make_grammar(rules) if rules else None

    def set_grammar_device(self, on: bool) -> int:
        """The context's grammar route from the next transcription call on; returns the previous mode (0 without a context)."""
        self.grammar_device = bool(on)
        if not self.ctx or not (self.grammar_device or hasattr(self.lib, "wmi_set_grammar_device")):
            return 0
        return self.lib.wmi_set_grammar_device(self.ctx, 1 if self.grammar_device else 0)

    def grammar_status(self) -> dict:
        """wmi_grammar_status of the last call: device steps, host fallback rows, the compiled capacities"""
        st = abi.wmi_grammar_status()
        assert self.lib.wmi_grammar_status(self.ctx, C.byref(st)) == 0
        return {k: getattr(st, k) for k, _ in st._fields_}

    def set_token_dtw(self, token_dtw) -> int:
        """The context's alignment mode from the next transcription call on (False, True or (layer, head) pairs); returns the previous
        mode, -1 for pairs the model does not have (nothing changed), 0 without a context."""
        self.token_dtw = token_dtw
        if not self.ctx or not (token_dtw or hasattr(self.lib, "wmi_set_token_dtw")):
            return 0
        pairs = [] if isinstance(token_dtw, bool) or not token_dtw else [int(v) for lh in token_dtw for v in lh]
        arr = (C.c_int32 * max(1, len(pairs)))(*pairs)
        return self.lib.wmi_set_token_dtw(self.ctx, 1 if token_dtw else 0, arr if pairs else None, len(pairs) // 2)

    def set_no_speech(self, mode: int) -> int:
        """The context's no-speech mode from the next transcription call on; returns the previous one (0 without a context)."""
        self.no_speech = int(mode)
        if not self.ctx or not (self.no_speech or hasattr(self.lib, "wmi_set_no_speech")):
            return 0
        return self.lib.wmi_set_no_speech(self.ctx, self.no_speech)      # (a library without the call cannot serve a mode: AttributeError)

    def close(self):
        self.lib.whisper_free(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- transcribe (src/speech_to_text.cpp:401-450)
    def full_params(self, initial_prompt: str = "", audio_ctx: int = 0) -> abi.whisper_full_params:
        p = self.lib.whisper_full_default_params(abi.WHISPER_SAMPLING_GREEDY)
        lang = self.language.encode()
        prompt = initial_prompt.encode("utf-8")
        self._keep = [lang, prompt]  # the reference lets this dangle (:413); we keep it alive
        p.language = lang
        p.audio_ctx = int(audio_ctx)
        p.speed_up = bool(self.settings["audio/input/transcribe/speed_up_2x"])
        p.split_on_word = True
        p.token_timestamps = True
        p.suppress_non_speech_tokens = True
        p.single_segment = True
        p.max_tokens = int(self.settings["audio/input/transcribe/max_tokens"])
        p.entropy_thold = float(self.settings["audio/input/transcribe/entropy_treshold"])
        p.initial_prompt = prompt
        if self._grammar is not None:
            ptrs, n_rules, _ = self._grammar
            p.grammar_rules = C.cast(ptrs, C.c_void_p); p.n_grammar_rules = n_rules; p.i_start_rule = 0
            p.grammar_penalty = self.grammar_penalty
        if getattr(self, "n_threads", 0):            # tests: the CPU reference behind this mirror (results do not depend on the thread count)
            p.n_threads = int(self.n_threads)
        return p

    def draft_status(self) -> dict:
        """include/wmi_device.h wmi_draft_status: what became of the last transcription call's draft"""
        s = abi.wmi_draft_status()
        if not self.ctx or self.lib.wmi_draft_status(self.ctx, C.byref(s)) != 0:
            return {}
        return {k: int(getattr(s, k)) for k, _ in abi.wmi_draft_status._fields_}

    def transcribe(self, buffer: np.ndarray, initial_prompt: str = "", audio_ctx: int = 0, params=None, draft=None) -> list:
        """draft (product library only, include/wmi_device.h wmi_set_draft): token ids the call verifies in one decoder pass and decodes
        on from where they stop being the greedy decode; the result is the undrafted call's.  last_draft_status says what became of it."""
        if not self.ctx:
            return []  # ERR_PRINT("Context instance is null")
        buffer = np.ascontiguousarray(buffer, dtype=np.float32)
        p = params if params is not None else self.full_params(initial_prompt, audio_ctx)
        if draft is not None:
            d = np.ascontiguousarray(draft, dtype=np.int32)
            if self.lib.wmi_set_draft(self.ctx, d.ctypes.data_as(C.c_void_p) if d.size else None, int(d.size)) != 0:
                raise ValueError("wmi_set_draft refused the draft (an id outside the vocabulary)")
        ret = self.lib.whisper_full(self.ctx, p, _fptr(buffer), int(buffer.size))
        self.last_ret = ret
        if draft is not None or hasattr(self.lib, "wmi_draft_status"):
            self.last_draft_status = self.draft_status()
        if ret != 0:
            return []  # ERR_PRINT("Failed to process audio, returned ...")
        return self.collect()

    # -- not in the reference: candidate texts scored against the audio (include/wmi_device.h: wmi_score_pcm).  The reference's guided mode
    # (examples/command/command.cpp:254-462) sums the probabilities of each command's FIRST token; this scores every token of every text.
    def tokenize(self, text: str) -> list:
        b = text.encode("utf-8")
        buf = (C.c_int32 * (len(b) + 8))()
        n = self.lib.whisper_tokenize(self.ctx, b, buf, len(buf))
        return list(buf[:max(n, 0)])

    def score(self, pcm: np.ndarray, texts: list, prompt=None, length_norm: bool = False, audio_ctx: int = 0) -> list:
        """-> per text {text, tokens, token_logprobs, sum_logprob, avg_logprob, posterior}; every text is tokenized with a leading
        space, as command.cpp:276 insists.  Leaves the list in last_scores and the return code in last_ret; [] on an error."""
        self.last_scores = []
        if not self.ctx:
            return []
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        toks = [self.tokenize(" " + t) for t in texts]
        p = self.lib.wmi_score_default_params()
        p.length_norm = int(bool(length_norm))
        if self.lib.whisper_is_multilingual(self.ctx):
            p.lang_id = max(0, self.lib.whisper_lang_id(self.language.encode()))          # ("auto": English, nothing is detected here)
        pt = np.asarray(self.tokenize(prompt) if prompt else [], np.int32)
        if pt.size:
            p.prompt_tokens = pt.ctypes.data_as(C.POINTER(C.c_int32)); p.prompt_n_tokens = int(pt.size)
        flat = np.asarray([t for y in toks for t in y], np.int32)
        nt = np.asarray([len(y) for y in toks], np.int32)
        out = (abi.wmi_text_score * max(1, len(texts)))()
        lp = np.zeros(int(nt.sum()) + len(texts), np.float32)
        self.last_ret = self.lib.wmi_score_pcm(self.ctx, p, pcm.ctypes.data_as(C.c_void_p), int(pcm.size), 0, int(audio_ctx),
                                               flat.ctypes.data_as(C.c_void_p) if flat.size else None, nt.ctypes.data_as(C.c_void_p), len(texts), out,
                                               lp.ctypes.data_as(C.c_void_p))
        if self.last_ret != 0:
            return []
        self.last_scores = [{"text": t, "tokens": y, "token_logprobs": lp[o.first:o.first + o.n_scored].tolist(), "sum_logprob": o.sum_logprob,
                             "avg_logprob": o.avg_logprob, "posterior": o.posterior} for t, y, o in zip(texts, toks, out)]
        return self.last_scores

    def collect(self) -> list:
        out, full_text = [], b""
        lib, ctx = self.lib, self.ctx
        for i in range(lib.whisper_full_n_segments(ctx)):
            full_text += lib.whisper_full_get_segment_text(ctx, i)
            for j in range(lib.whisper_full_n_tokens(ctx, i)):
                t = lib.whisper_full_get_token_data(ctx, i, j)
                out.append({
                    "text": lib.whisper_full_get_token_text(ctx, i, j), "id": t.id, "p": t.p, "plog": t.plog,
                    "pt": t.pt, "ptsum": t.ptsum, "t0": t.t0, "t1": t.t1, "tid": t.tid, "vlen": t.vlen,
                })
                if self.token_dtw:
                    out[-1]["t_dtw"] = lib.wmi_full_get_token_dtw(ctx, i, j)
                if self.speaker_labels == "tokens":
                    rec = abi.wmi_speaker()
                    if lib.wmi_full_get_token_speaker(ctx, i, j, C.byref(rec)) == 0:
                        out[-1]["speaker"] = rec.speaker if rec.speaker >= 0 else None
        out.insert(0, full_text)
        self.last_windows = self.windows()
        self.last_speakers = self.speakers()
        return out

    def windows(self) -> list:
        """The windows of the last call (or of the chunk selected last): seek in 10 ms frames, no_speech_prob, outcome (abi.WINDOW_*),
        first segment, segment count.  Empty in mode 0 and for a library without the interface."""
        lib, ctx = self.lib, self.ctx
        if not ctx or not hasattr(lib, "wmi_full_n_windows"):
            return []
        out = []
        for i in range(lib.wmi_full_n_windows(ctx)):
            w = abi.wmi_window()
            assert lib.wmi_full_get_window(ctx, i, C.byref(w)) == 0
            out.append({"seek": w.seek, "no_speech_prob": w.no_speech_prob, "outcome": w.outcome, "i_segment": w.i_segment,
                        "n_segments": w.n_segments})
        return out

    # -- several independent buffers at once (product library only: include/wmi_device.h wmi_full_batch).  The
    #    reference host has no such call; the semantics are "transcribe() of each buffer, on a fresh context".
    #    audio_ctxs: an encoder length per buffer (wmi_full_batch_ctx) instead of the common audio_ctx.
    def transcribe_batch(self, buffers: list, initial_prompt: str = "", audio_ctx: int = 0, params=None,
                         device_ptrs: list | None = None, audio_ctxs: list | None = None) -> list:
        if not self.ctx:
            return []
        p = params if params is not None else self.full_params(initial_prompt, audio_ctx)
        n = len(buffers)
        assert audio_ctxs is None or len(audio_ctxs) == n, (n, audio_ctxs)
        if device_ptrs is None:
            bufs = [np.ascontiguousarray(b, dtype=np.float32) for b in buffers]
            ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
            lens = (C.c_int * n)(*[int(b.size) for b in bufs])
            on_dev = 0
        else:
            ptrs = (C.c_void_p * n)(*device_ptrs)
            lens = (C.c_int * n)(*[int(b) for b in buffers])          # sample counts
            on_dev = 1
        if audio_ctxs is None:
            ret = self.lib.wmi_full_batch(self.ctx, p, ptrs, lens, n, on_dev)
        else:
            ret = self.lib.wmi_full_batch_ctx(self.ctx, p, ptrs, lens, (C.c_int * n)(*[int(a) for a in audio_ctxs]), n, on_dev)
        self.last_ret = ret
        if ret != 0:
            return []
        return self.collect_batch(n)

    def collect_batch(self, n: int) -> list:
        """The n results of the last lock-step call (wmi_batch_select), and last_modes / last_langs / last_batch_windows."""
        out = []
        self.last_batch_windows = []
        self.last_modes = []
        self.last_langs = []                                          # per chunk: the language id whisper_full would report (detected with "auto")
        self.last_batch_speakers = []                                 # per chunk: speakers() ([] for a mono clip)
        for c in range(n):
            assert self.lib.wmi_batch_select(self.ctx, c) >= 0
            self.last_modes.append(self.lib.wmi_batch_chunk_mode(self.ctx, c))
            self.last_langs.append(self.lib.wmi_batch_lang_id(self.ctx, c))
            out.append(self.collect())
            self.last_batch_windows.append(self.last_windows)
            self.last_batch_speakers.append(self.last_speakers)
        return out

    # -- a whole recording (product library only: include/wmi_device.h wmi_full_long): cut at its silences on the device, the pieces
    #    decoded in lock-step, one merged result with times relative to the recording.
    def transcribe_long(self, buffer, params=None, long_params=None, device_ptr: int | None = None) -> list:
        """-> the merged result in collect()'s form.  Leaves last_pieces (frame0, frame1, audio_ctx, mode, i_segment, n_segments per
        piece), last_modes (wmi_batch_chunk_mode per piece), last_segments ((t0, t1, text) of the merged segments) and last_windows.
        long_params: an abi.wmi_long_params (None: the library's defaults).  device_ptr: the PCM is on the device, `buffer` its sample count."""
        self.last_pieces, self.last_modes, self.last_segments = [], [], []
        if not self.ctx:
            return []
        p = params if params is not None else self.full_params()
        lp = C.byref(long_params) if long_params is not None else None
        if device_ptr is None:
            buffer = np.ascontiguousarray(buffer, dtype=np.float32)
            ret = self.lib.wmi_full_long(self.ctx, p, buffer.ctypes.data_as(C.c_void_p), int(buffer.size), 0, lp)
        else:
            ret = self.lib.wmi_full_long(self.ctx, p, C.c_void_p(device_ptr), int(buffer), 1, lp)
        self.last_ret = ret
        if ret != 0:
            return []
        for i in range(self.lib.wmi_long_n_pieces(self.ctx)):
            pc = abi.wmi_long_piece()
            assert self.lib.wmi_long_get_piece(self.ctx, i, C.byref(pc)) == 0
            self.last_pieces.append({name: getattr(pc, name) for name, _ in abi.wmi_long_piece._fields_})
            self.last_modes.append(pc.mode)
        out = self.collect()
        self.last_segments = self.segments()
        return out

    # -- an AudioStreamWAV as it is (product library only: include/wmi_device.h wmi_full_wav & co.): `data` are the asset's bytes, 8 or
    #    16 bit (AudioStreamWAV.FORMAT_8_BITS = 0 / FORMAT_16_BITS = 1; abi.WMI_WAV_F32 for f32; FORMAT_IMA_ADPCM = 2 with wav_adpcm),
    #    mono or stereo, at its own mix rate.
    #    The reference node decodes them in a GDScript loop as if they were 16 kHz mono (audio_stream_to_text.gd:40-46).
    @staticmethod
    def _wav(data, format: int, stereo, mix_rate: int):
        """-> (abi.wmi_wav, keepalive) for host bytes; an empty clip still gets a non-NULL pointer."""
        raw = bytes(data)
        buf = C.create_string_buffer(raw, max(len(raw), 1))
        return abi.wmi_wav(C.cast(buf, C.c_void_p), len(raw), int(format), int(stereo), int(mix_rate), 0), buf

    def transcribe_wav(self, data: bytes, format: int, stereo, mix_rate: int, initial_prompt: str = "", audio_ctx: int = 0,
                       interpolator_type: int = 2, params=None) -> list:
        if not self.ctx:
            return []
        wav, _keep = self._wav(data, format, stereo, mix_rate)
        p = params if params is not None else self.full_params(initial_prompt, audio_ctx)
        self.last_ret = self.lib.wmi_full_wav(self.ctx, p, C.byref(wav), int(interpolator_type))
        if self.last_ret != 0:
            return []
        return self.collect()

    def transcribe_wav_long(self, data: bytes, format: int, stereo, mix_rate: int, interpolator_type: int = 2, params=None,
                            long_params=None) -> list:
        """transcribe_long on the asset's bytes; leaves what transcribe_long leaves."""
        self.last_pieces, self.last_modes, self.last_segments = [], [], []
        if not self.ctx:
            return []
        wav, _keep = self._wav(data, format, stereo, mix_rate)
        p = params if params is not None else self.full_params()
        lp = C.byref(long_params) if long_params is not None else None
        self.last_ret = self.lib.wmi_full_long_wav(self.ctx, p, C.byref(wav), int(interpolator_type), lp)
        if self.last_ret != 0:
            return []
        for i in range(self.lib.wmi_long_n_pieces(self.ctx)):
            pc = abi.wmi_long_piece()
            assert self.lib.wmi_long_get_piece(self.ctx, i, C.byref(pc)) == 0
            self.last_pieces.append({name: getattr(pc, name) for name, _ in abi.wmi_long_piece._fields_})
            self.last_modes.append(pc.mode)
        out = self.collect()
        self.last_segments = self.segments()
        return out

    def transcribe_wav_batch(self, clips: list, initial_prompt: str = "", audio_ctx: int = 0, interpolator_type: int = 2, params=None) -> list:
        """clips: (data, format, stereo, mix_rate) each — a folder of voice lines in one lock-step call (wmi_full_batch_wav)."""
        if not self.ctx:
            return []
        made = [self._wav(*c) for c in clips]
        wavs = (abi.wmi_wav * max(len(made), 1))(*[w for w, _ in made])
        p = params if params is not None else self.full_params(initial_prompt, audio_ctx)
        self.last_ret = self.lib.wmi_full_batch_wav(self.ctx, p, wavs, len(made), int(interpolator_type))
        if self.last_ret != 0:
            return []
        return self.collect_batch(len(made))

    def transcribe_wav_channels(self, data: bytes, format: int, mix_rate: int, initial_prompt: str = "", audio_ctx: int = 0,
                                interpolator_type: int = 2, params=None) -> list:
        """A stereo asset with one voice per channel (wmi_full_wav_channels): both channels transcribed apart in one lock-step call.
        -> the dialogue, a dictionary per segment in the order of the merged view: "channel" (0 left, 1 right), "index" (the segment's
        place in that channel's result), t0, t1 (10 ms units), text.  Leaves last_channels (the two per-channel results in collect()'s
        form), last_modes / last_langs / last_batch_windows per channel, and the dialogue view selected."""
        self.last_channels = []
        if not self.ctx:
            return []
        wav, _keep = self._wav(data, format, 1, mix_rate)
        p = params if params is not None else self.full_params(initial_prompt, audio_ctx)
        self.last_ret = self.lib.wmi_full_wav_channels(self.ctx, p, C.byref(wav), int(interpolator_type))
        if self.last_ret != 0:
            return []
        self.last_channels = self.collect_batch(2)
        n = self.lib.wmi_channels_select(self.ctx, -1)
        assert n >= 0
        rec, out = abi.wmi_channel_segment(), []
        for i, (t0, t1, text) in enumerate(self.segments()):
            assert self.lib.wmi_channels_get_segment(self.ctx, i, C.byref(rec)) == 0
            out.append({"channel": rec.channel, "index": rec.index, "t0": t0, "t1": t1, "text": text})
        return out

    def segments(self) -> list:
        """(t0, t1, text) of the segments the accessors show now (10 ms units)."""
        lib, ctx = self.lib, self.ctx
        return [(lib.whisper_full_get_segment_t0(ctx, i), lib.whisper_full_get_segment_t1(ctx, i), lib.whisper_full_get_segment_text(ctx, i))
                for i in range(lib.whisper_full_n_segments(ctx))]

    # -- resample (src/speech_to_text.cpp:353-376): stereo capture frames at the mix rate -> mono 16 kHz.  The reference goes through
    #    libsamplerate on the CPU; here both steps run on the device (wmi_downmix_stereo, wmi_resample).
    SRC_SINC_BEST_QUALITY, SRC_SINC_MEDIUM_QUALITY, SRC_SINC_FASTEST = 0, 1, 2        # src/speech_to_text.h:151-156
    SRC_ZERO_ORDER_HOLD, SRC_LINEAR = 3, 4

    def resample(self, buffer_xy: np.ndarray, interpolator_type: int = 2, mix_rate: int = 44100) -> np.ndarray:
        xy = np.ascontiguousarray(buffer_xy, dtype=np.float32).reshape(-1, 2)
        n = int(xy.shape[0])
        expected = n * abi.WHISPER_SAMPLE_RATE // int(mix_rate)                        # :356
        mono = np.empty(n, np.float32)
        if n and self.lib.wmi_downmix_stereo(self.ctx, xy.ctypes.data_as(C.c_void_p), n, 0, mono.ctypes.data_as(C.c_void_p)) != 0:
            return np.zeros(0, np.float32)
        out = np.empty(max(expected, n if mix_rate == abi.WHISPER_SAMPLE_RATE else 0, 1), np.float32)
        got = self.lib.wmi_resample(self.ctx, mono.ctypes.data_as(C.c_void_p), n, int(mix_rate), abi.WHISPER_SAMPLE_RATE,
                                    int(interpolator_type), 0, out.ctypes.data_as(C.c_void_p), int(out.size))
        if got < 0:
            got = 0
        if got != expected:                                                            # :368-370
            self.last_resample_warning = f"size differ exp: {expected} res: {got}"
        return out[:got].copy()

    # -- voice_activity_detection (src/speech_to_text.cpp:53-104, 378-399)
    def voice_activity_detection(self, buffer: np.ndarray) -> bool:
        n_win = abi.WHISPER_SAMPLE_RATE * 3
        if buffer.size < n_win:
            return False
        if getattr(self, "device_vad", False) and hasattr(self.lib, "wmi_vad") and self.ctx:
            # the product's device kernel (include/wmi_device.h): same decision, no per-sample host loop
            b = np.ascontiguousarray(buffer[-n_win:], dtype=np.float32)
            r = self.lib.wmi_vad(self.ctx, b.ctypes.data_as(C.c_void_p), int(b.size), 0,
                                 float(self.settings["audio/input/transcribe/vad_treshold"]),
                                 float(self.settings["audio/input/transcribe/freq_treshold"]), None)
            assert r >= 0, r
            return bool(r)
        pcm = np.array(buffer[-n_win:], dtype=np.float32)
        return vad_simple(pcm, abi.WHISPER_SAMPLE_RATE, 500,
                          float(self.settings["audio/input/transcribe/vad_treshold"]),
                          float(self.settings["audio/input/transcribe/freq_treshold"]))


def high_pass_filter(data: np.ndarray, cutoff: float, sample_rate: float) -> None:
    """src/speech_to_text.cpp:53-66, operation for operation.  The reference filters IN PLACE and reads data[i - 1] after it
    has been overwritten, so its "previous input" is the previous OUTPUT: y = alpha * ((y + x_i) - y).  (Math_PI is a double:
    rc is computed in double and rounded to float.)"""
    rc = np.float32(1.0 / (2.0 * math.pi * float(np.float32(cutoff))))
    dt = np.float32(1.0) / np.float32(sample_rate)
    alpha = np.float32(dt / np.float32(rc + dt))
    y = np.float32(data[0])
    for i in range(1, data.size):
        y = np.float32(alpha * np.float32(np.float32(y + np.float32(data[i])) - np.float32(data[i - 1])))
        data[i] = y


def vad_simple(pcm: np.ndarray, sample_rate: int, last_ms: int, vad_thold: float, freq_thold: float) -> bool:
    n = pcm.size
    n_last = (sample_rate * last_ms) // 1000
    if n_last >= n:
        return False
    if freq_thold > 0.0:
        high_pass_filter(pcm, freq_thold, sample_rate)
    a = np.abs(pcm.astype(np.float32))
    # running f32 sums in sample order, as the reference's loop (np.cumsum accumulates sequentially; np.add.reduce would pair)
    e_all = np.float32(np.cumsum(a, dtype=np.float32)[-1]) / np.float32(n)
    e_last = np.float32(np.cumsum(a[n - n_last:], dtype=np.float32)[-1]) / np.float32(max(n_last, 1))
    vad_simple.last_energies = (float(e_all), float(e_last))
    vad_thold = np.float32(vad_thold)
    # note the host's extra "not both < 1e-4" clause vs upstream vad_simple
    if not (e_all < 0.0001 and e_last < 0.0001) or e_last > vad_thold * e_all:
        return False
    return True


class CaptureSession:
    """include/wmi_device.h wmi_capture_*: the accumulated capture frames of one node and their 16 kHz PCM, resident on the device."""

    def __init__(self, node: SpeechToText, mix_rate: int, converter: int = 2, frames_hint: int = 0):
        self.lib, self.node = node.lib, node
        self.cap = self.lib.wmi_capture_init(node.ctx, int(mix_rate), int(converter), int(frames_hint))
        if not self.cap:
            raise RuntimeError("wmi_capture_init failed (context cannot compute, or bad mix rate / converter)")

    def close(self):
        if self.cap:
            self.lib.wmi_capture_free(self.cap)
        self.cap = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push(self, frames_xy: np.ndarray) -> int:
        xy = np.ascontiguousarray(frames_xy, dtype=np.float32).reshape(-1, 2)
        r = self.lib.wmi_capture_push(self.cap, xy.ctypes.data_as(C.c_void_p), int(xy.shape[0]), 0)
        assert r >= 0, r
        return r

    def push_device(self, d_ptr, n_frames: int) -> int:
        return self.lib.wmi_capture_push(self.cap, C.c_void_p(d_ptr), int(n_frames), 1)

    def keep_last(self, n_frames: int) -> int:
        return self.lib.wmi_capture_keep_last(self.cap, int(n_frames))

    def resample(self):
        """-> (result_size, expected), src/speech_to_text.cpp:356-370"""
        exp = C.c_int(0)
        return self.lib.wmi_capture_resample(self.cap, C.byref(exp)), exp.value

    def read_pcm(self) -> np.ndarray:
        n, _ = self.resample()
        out = np.empty(max(n, 1), np.float32)
        got = self.lib.wmi_capture_read_pcm(self.cap, out.ctypes.data_as(C.c_void_p), int(out.size))
        assert got == max(n, 0), (got, n)
        return out[:max(got, 0)].copy()

    def vad(self, vad_thold: float, freq_thold: float, energies: np.ndarray | None = None) -> int:
        return self.lib.wmi_capture_vad(self.cap, float(vad_thold), float(freq_thold),
                                        energies.ctypes.data_as(C.c_void_p) if energies is not None else None)

    def full(self, params) -> int:
        return self.lib.wmi_capture_full(self.cap, params)

    def stats(self) -> tuple:
        """(bytes copied host -> device, outputs computed, outputs reused, 1 if everything was recomputed)"""
        out = (C.c_int64 * 4)()
        assert self.lib.wmi_capture_stats(self.cap, out) == 0
        return tuple(int(v) for v in out)

    @staticmethod
    def full_batch(sessions: list, params, audio_ctxs: list | None = None) -> int:
        """wmi_capture_full_batch: the transcribe step of several sessions of one node in lock-step; results through
        node.collect_batch(len(sessions))."""
        n = len(sessions)
        caps = (C.c_void_p * max(n, 1))(*[s.cap for s in sessions])
        ctxs = (C.c_int * n)(*[int(a) for a in audio_ctxs]) if audio_ctxs is not None else None
        lib = sessions[0].lib if n else None
        return lib.wmi_capture_full_batch(caps, n, params, ctxs) if lib else -1


class AudioStreamToText(SpeechToText):
    """addon/audio_stream_to_text.gd: one-shot "transcribe this WAV" node."""

    def get_text(self, pcm: np.ndarray, initial_prompt: str = "", long_form: bool = False) -> str:
        """long_form (product library only): the recording is cut at its silences and the pieces decoded in lock-step (transcribe_long)
        instead of whisper_full's walk window by window."""
        tokens = self.transcribe_long(pcm, self.full_params(initial_prompt, 0)) if long_form else self.transcribe(pcm, initial_prompt, 0)
        if not tokens:
            return ""
        text = tokens.pop(0).decode("utf-8", errors="replace")
        return remove_special_characters(text)

    def get_text_wav(self, data: bytes, format: int, stereo, mix_rate: int, initial_prompt: str = "", interpolator_type: int = 2,
                     long_form: bool = False, speaker_prefix: bool = False, channels: bool = False) -> str:
        """get_text on audio_stream.data / .format / .stereo / .mix_rate themselves: every sample is decoded, a stereo asset is folded
        and another rate resampled on the device — what the node's own loop (audio_stream_to_text.gd:40-46) gets wrong.
        speaker_prefix (a node made with speaker_labels, a stereo asset): "(speaker 0) " / "(speaker 1) " / "(speaker ?) " in front of
        every segment's text, as whisper.cpp's --diarize prints it (examples/main/main.cpp:262-265).
        channels (a stereo asset with one voice per channel): the two channels are transcribed apart (transcribe_wav_channels) and the
        dialogue joined with the same prefix per segment, the channel being the speaker."""
        if channels:
            return "".join("(speaker %d) " % s["channel"] + remove_special_characters(s["text"].decode("utf-8", errors="replace"))
                           for s in self.transcribe_wav_channels(data, format, mix_rate, initial_prompt, 0, interpolator_type))
        if long_form:
            tokens = self.transcribe_wav_long(data, format, stereo, mix_rate, interpolator_type, self.full_params(initial_prompt, 0))
        else:
            tokens = self.transcribe_wav(data, format, stereo, mix_rate, initial_prompt, 0, interpolator_type)
        if not tokens:
            return ""
        if speaker_prefix and self.last_speakers:
            return "".join("(speaker %s) " % ("?" if s["speaker"] is None else s["speaker"]) +
                           remove_special_characters(s["text"].decode("utf-8", errors="replace")) for s in self.last_speakers)
        return remove_special_characters(tokens.pop(0).decode("utf-8", errors="replace"))


def remove_special_characters(message: str) -> str:
    # addon/audio_stream_to_text.gd:64-88 — drop [..] and <..> spans and a ". you." hallucination
    for a, b in (("[", "]"), ("<", ">")):
        while True:
            i = message.find(a)
            j = message.find(b)
            if i == -1 or j == -1 or j < i:
                break
            message = message[:i] + message[j + 1:]
    message = re.sub(r"\. you\.$", ".", message)
    return message


class CaptureStreamToText(SpeechToText):
    """addon/capture_stream_to_text.gd: the streaming loop.  `stream` restates it over a pre-recorded 16 kHz buffer instead of
    AudioEffectCapture: every `interval` seconds of simulated time the whole accumulated buffer is re-transcribed with
    audio_ctx = total_s*50 + 128 (:84).  `stream_capture` is the node's own loop over stereo capture frames at the mix rate —
    append, resample, VAD, transcribe (:69-120) — on a capture session (include/wmi_device.h wmi_capture_*: the frames and their
    16 kHz PCM stay on the device) or, for comparison, over resample() / voice_activity_detection() / transcribe() on host arrays."""

    def __init__(self, lib, settings=None, transcribe_interval: float = 0.3, minimum_sentence_ms: int = 3000,
                 maximum_sentence_ms: int = 15000, punctuation_characters: str = ".!?;。；？！", no_speech_gate: bool = False,
                 draft_reuse: bool = False, speaker_labels=False):
        """no_speech_gate: transcribe in the no-speech mode "gate" (wmi_set_no_speech 3).  A step whose window was gated is treated like
        "no activity": nothing is emitted for it and the loop goes on.
        draft_reuse (stream_capture on a session; wmi_capture_set_draft 1): every step offers the previous step's tokens as a draft —
        the messages are the same, the steps shorter; draft_statuses collects every step's wmi_draft_status.
        speaker_labels (stream_capture on a session; wmi_set_speaker): every step's collect() leaves last_speakers, from the session's
        resident stereo frames."""
        super().__init__(lib, settings, no_speech=abi.NO_SPEECH_GATE if no_speech_gate else 0, speaker_labels=speaker_labels)
        self.no_speech_gate = bool(no_speech_gate)
        self.draft_reuse = bool(draft_reuse)
        self.draft_statuses = []
        self.interval = transcribe_interval
        self.min_ms = minimum_sentence_ms
        self.max_ms = maximum_sentence_ms
        self.punct = punctuation_characters

    def _gated(self, tokens: list) -> bool:
        """The call just collected produced no tokens because its window was gated (no_speech_gate)."""
        return self.no_speech_gate and len(tokens) <= 1 and any(w["outcome"] == abi.WINDOW_GATED for w in self.last_windows)

    def stream(self, pcm16k: np.ndarray, max_calls: int | None = None):
        """Yield (is_final, text, n_samples_used, audio_ctx, token dicts) per transcribe call."""
        sr = abi.WHISPER_SAMPLE_RATE
        step = int(round(self.interval * sr))
        start, pos, calls = 0, 0, 0
        last_tokens = -1
        while pos < pcm16k.size:
            pos = min(pos + step, pcm16k.size)
            acc = pcm16k[start:pos]
            total_s = acc.size / sr
            if total_s < 1.0:
                continue
            no_activity = self.voice_activity_detection(acc)
            audio_ctx = min(int(total_s * 50 + 128), 1500)
            tokens = self.transcribe(acc, "", audio_ctx)
            calls += 1
            if not tokens:
                continue
            if self._gated(tokens):
                if max_calls is not None and calls >= max_calls:
                    return
                continue
            text = remove_special_characters(tokens.pop(0).decode("utf-8", errors="replace"))
            n_tok = len(tokens)
            call_tokens = list(tokens)
            finish = False
            total_ms = total_s * 1000
            if total_ms > self.min_ms:
                ends_punct = len(text) > 0 and text[-1] in self.punct
                if (ends_punct or no_activity) and abs(n_tok - last_tokens) <= 1:
                    finish = True
                if total_ms > self.max_ms:
                    finish = True
            last_tokens = n_tok
            yield finish, text, acc.size, audio_ctx, call_tokens
            if finish:
                start = max(pos - int(0.2 * sr), 0)  # keep only the last 0.2 s (:111)
                last_tokens = -1
            if max_calls is not None and calls >= max_calls:
                return

    def stream_capture(self, frames_xy: np.ndarray, mix_rate: int, interpolator_type: int = 2, max_calls: int | None = None,
                       use_session: bool = True, minimum_sentence_time: float = 3, maximum_sentence_time: float = 15,
                       hallucinating_count: int = 1, temperature_inc: float | None = None):
        """transcribe_thread (addon/capture_stream_to_text.gd:69-120) over pre-recorded stereo capture frames at `mix_rate`: every pass
        appends `interval` seconds of frames, resamples the whole accumulation, runs the VAD and transcribes with the node's
        parameters and audio_ctx = total_time * 1500 / 30 + 128.  Yields, per transcribe call,
        (finish_sentence, text, n_samples_used, audio_ctx, token dicts, no_activity); as in the node, a pass with no_activity neither
        ends the sentence nor updates the token count, and a finished sentence keeps the last 0.2 * mix_rate frames.
        use_session: the capture session (device-resident frames and PCM), else the same loop over resample() /
        voice_activity_detection() / transcribe() on host arrays — the same tuples either way.
        temperature_inc (tests): replaces the node's default in the parameters of every call (0.0 = no temperature fallback)."""
        xy = np.ascontiguousarray(frames_xy, dtype=np.float32).reshape(-1, 2)
        sr = abi.WHISPER_SAMPLE_RATE
        step = max(int(round(self.interval * mix_rate)), 1)
        vad_thold = float(self.settings["audio/input/transcribe/vad_treshold"])
        freq_thold = float(self.settings["audio/input/transcribe/freq_treshold"])
        sess = CaptureSession(self, mix_rate, interpolator_type, frames_hint=int(maximum_sentence_time * mix_rate)) if use_session else None
        if sess and self.draft_reuse:
            self.lib.wmi_capture_set_draft(sess.cap, 1)
        self.draft_statuses = []
        try:
            start, pos, calls, last_token_count = 0, 0, 0, 0
            while pos < xy.shape[0]:
                new = xy[pos:pos + step]
                pos += new.shape[0]
                if sess:
                    sess.push(new)                                                  # _accumulated_frames.append_array(...) (:73)
                    size, _ = sess.resample()
                else:
                    resampled = self.resample(xy[start:pos], interpolator_type, mix_rate)
                    size = int(resampled.size)
                if size <= 0:
                    continue
                if sess:
                    no_activity = bool(sess.vad(vad_thold, freq_thold))
                else:
                    no_activity = self.voice_activity_detection(resampled)
                total_time = size / sr
                audio_ctx = min(int(total_time * 1500 / 30 + 128), 1500)            # :84
                p = self.full_params("", audio_ctx)
                if temperature_inc is not None:
                    p.temperature_inc = float(temperature_inc)
                if sess:
                    self.last_ret = sess.full(p)
                    self.draft_statuses.append(self.draft_status())
                    tokens = self.collect() if self.last_ret == 0 else []
                else:
                    tokens = self.transcribe(resampled, "", audio_ctx, params=p)
                calls += 1
                if not tokens:
                    return                                                          # push_warning("No tokens generated") (:88-90)
                if self._gated(tokens):
                    if max_calls is not None and calls >= max_calls:
                        return
                    continue
                full_text = tokens.pop(0).decode("utf-8", errors="replace")
                finish = total_time > maximum_sentence_time
                text = remove_special_characters("".join(t["text"].decode("utf-8", errors="replace") for t in tokens))
                if any(ch in text for ch in self.punct) or no_activity:
                    finish = True
                if total_time < minimum_sentence_time or abs(len(tokens) - last_token_count) > hallucinating_count:
                    finish = False
                yield finish, full_text, size, audio_ctx, list(tokens), no_activity
                if not no_activity:                                                 # `if no_activity: continue` (:108-109)
                    if finish:                                                      # :110-113
                        keep = int(0.2 * mix_rate)
                        if sess:
                            sess.keep_last(keep)
                        else:
                            start = max(pos - keep, start)
                    last_token_count = len(tokens)
                if max_calls is not None and calls >= max_calls:
                    return
        finally:
            if sess:
                sess.close()

    def stream_capture_many(self, streams: list, mix_rates: list, interpolator_type: int = 2, max_calls: int | None = None,
                            minimum_sentence_time: float = 3, maximum_sentence_time: float = 15, hallucinating_count: int = 1,
                            temperature_inc: float | None = None):
        """stream_capture's loop for several pre-recorded speakers on ONE node, one capture session each: every pass pushes `interval`
        seconds of each speaker's frames, resamples and runs the VAD per session, then transcribes the sessions that hold at least one
        output sample with ONE wmi_capture_full_batch, each at the node's audio_ctx = total_time * 1500 / 30 + 128.  Yields
        (speaker, finish_sentence, text, n_samples_used, audio_ctx, token dicts, no_activity) — per speaker the tuples stream_capture
        yields for that speaker alone; keep_last and the token count are kept per speaker.  A speaker whose frames are used up (or who
        produced no tokens, where stream_capture returns) drops out of later passes; max_calls counts passes with a transcription.
        temperature_inc as in stream_capture.  self.pass_modes collects, per pass, wmi_batch_chunk_mode of its sessions (0 = lock-step row,
        1 = the session asked for the temperature fallback and was run alone)."""
        self.pass_modes = []
        xys = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 2) for f in streams]
        n = len(xys)
        assert len(mix_rates) == n
        sr = abi.WHISPER_SAMPLE_RATE
        steps = [max(int(round(self.interval * r)), 1) for r in mix_rates]
        vad_thold = float(self.settings["audio/input/transcribe/vad_treshold"])
        freq_thold = float(self.settings["audio/input/transcribe/freq_treshold"])
        sessions = [CaptureSession(self, r, interpolator_type, frames_hint=int(maximum_sentence_time * r)) for r in mix_rates]
        try:
            pos, last_token_count, live = [0] * n, [0] * n, [True] * n
            calls = 0
            while any(live[i] and pos[i] < xys[i].shape[0] for i in range(n)):
                ready = []                                                          # (speaker, size, no_activity, audio_ctx)
                for i in range(n):
                    if not live[i] or pos[i] >= xys[i].shape[0]:
                        continue
                    new = xys[i][pos[i]:pos[i] + steps[i]]
                    pos[i] += new.shape[0]
                    sessions[i].push(new)
                    size, _ = sessions[i].resample()
                    if size <= 0:
                        continue
                    no_activity = bool(sessions[i].vad(vad_thold, freq_thold))
                    total_time = size / sr
                    ready.append((i, size, no_activity, min(int(total_time * 1500 / 30 + 128), 1500)))
                if not ready:
                    continue
                # (one parameter block for the pass: the speakers differ in audio_ctx only, which travels per session)
                p = self.full_params("", 0)
                if temperature_inc is not None:
                    p.temperature_inc = float(temperature_inc)
                self.last_ret = CaptureSession.full_batch([sessions[i] for i, _, _, _ in ready], p, [a for _, _, _, a in ready])
                results = self.collect_batch(len(ready)) if self.last_ret == 0 else [[] for _ in ready]
                if self.last_ret == 0:
                    self.pass_modes.append(list(self.last_modes))
                calls += 1
                for (i, size, no_activity, audio_ctx), tokens in zip(ready, results):
                    if not tokens:
                        live[i] = False                                             # push_warning("No tokens generated") (:88-90)
                        continue
                    total_time = size / sr
                    full_text = tokens.pop(0).decode("utf-8", errors="replace")
                    finish = total_time > maximum_sentence_time
                    text = remove_special_characters("".join(t["text"].decode("utf-8", errors="replace") for t in tokens))
                    if any(ch in text for ch in self.punct) or no_activity:
                        finish = True
                    if total_time < minimum_sentence_time or abs(len(tokens) - last_token_count[i]) > hallucinating_count:
                        finish = False
                    yield i, finish, full_text, size, audio_ctx, list(tokens), no_activity
                    if not no_activity:
                        if finish:
                            sessions[i].keep_last(int(0.2 * mix_rates[i]))
                        last_token_count[i] = len(tokens)
                if max_calls is not None and calls >= max_calls:
                    return
        finally:
            for s in sessions:
                s.close()

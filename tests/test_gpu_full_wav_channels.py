"""-m gpu: wmi_full_wav_channels (include/wmi_device.h) — the two channels of a stereo clip transcribed apart in one lock-step call.

Per channel the call must give what wmi_full_batch gives on the judge's two host arrays (tests/channels_ref.py), strictly: segments,
tokens with ids and times, text, language id, wmi_batch_chunk_mode, windows and counters — the converted samples are the judge's bit for
bit (tests/test_gpu_wav_channels.py), and behind them the same code runs on the same build.  The dialogue view is the judge's merge of
the two results."""
import ctypes as C

import numpy as np
import pytest

import channels_ref as cr
import wav_ref as wr
from godot_whisper_amd import abi, host, synth

pytestmark = pytest.mark.gpu

SR = 16000


@pytest.fixture(scope="module")
def model():
    return synth.make_model("micro.en", seed=2024)


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture
def node(product_lib, model):
    n = host.SpeechToText(product_lib); n.set_language_model(model)
    yield n
    n.close()


def _params(node):
    p = node.full_params("", 0); p.temperature_inc = 0.0
    return p


def _counters(lib, ctx):
    t6, n5 = (C.c_int64 * 6)(), (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return np.array(list(n5))


def _stats(lib, ctx):
    s = (C.c_int64 * 5)()
    assert lib.wmi_wav_stats(ctx, s) == 0
    return list(s)


def _clip(fmt, rate, seconds, seed, silent=None):
    """synthetic speech at `rate` (the 16 kHz generator's samples played at that rate), a different voice per channel; `silent`: that
    channel is digital silence"""
    n = int(seconds * rate)
    chans = [np.zeros(n, np.float32) if c == silent else synth.make_pcm(n / SR, seed=seed + c)[:n] for c in range(2)]
    return wr.pack(np.stack(chans, axis=1).reshape(-1), fmt)


def _shown(node):
    """what the accessors show now, per segment: (t0, t1, text, [(id, tid, t0, t1, p, plog, t_dtw) per token])"""
    lib, ctx = node.lib, node.ctx
    out = []
    for i in range(lib.whisper_full_n_segments(ctx)):
        toks = []
        for j in range(lib.whisper_full_n_tokens(ctx, i)):
            t = lib.whisper_full_get_token_data(ctx, i, j)
            toks.append((t.id, t.tid, t.t0, t.t1, t.p, t.plog, lib.wmi_full_get_token_dtw(ctx, i, j)))
        out.append((lib.whisper_full_get_segment_t0(ctx, i), lib.whisper_full_get_segment_t1(ctx, i), lib.whisper_full_get_segment_text(ctx, i), toks))
    return out


def _per_chunk(node, before):
    """after a lock-step call of two chunks: everything a caller can read per chunk, and the counter deltas"""
    lib, ctx = node.lib, node.ctx
    per = []
    for c in range(2):
        assert lib.wmi_batch_select(ctx, c) >= 0
        per.append((_shown(node), lib.whisper_full_lang_id(ctx), lib.wmi_batch_chunk_mode(ctx, c), lib.wmi_batch_lang_id(ctx, c), node.windows()))
    return per, list(_counters(lib, ctx) - before)


def _channels_route(node, data, fmt, rate, conv):
    before = _counters(node.lib, node.ctx)
    dialogue = node.transcribe_wav_channels(data, fmt, rate, interpolator_type=conv, params=_params(node))
    assert node.last_ret == 0, node.last_ret
    listed = list(node.last_channels)
    per, delta = _per_chunk(node, before)
    return dialogue, listed, per, delta


def _batch_route(node, pcms):
    before = _counters(node.lib, node.ctx)
    listed = node.transcribe_batch(list(pcms), params=_params(node))
    assert node.last_ret == 0, node.last_ret
    per, delta = _per_chunk(node, before)
    return listed, per, delta


def _check_dialogue(node, dialogue, per):
    """the dialogue view against the judge's merge of the two per-channel results, through every accessor"""
    lib, ctx = node.lib, node.ctx
    segs = [p[0] for p in per]
    order = cr.merge([s[0] for s in segs[0]], [s[0] for s in segs[1]])
    assert lib.wmi_channels_select(ctx, -1) == len(order) == len(segs[0]) + len(segs[1])
    shown = _shown(node)
    assert shown == [segs[c][i] for c, i in order]                                  # copies: text, tokens, times, DTW times untouched
    rec = abi.wmi_channel_segment()
    for i, (c, ix) in enumerate(order):
        assert lib.wmi_channels_get_segment(ctx, i, C.byref(rec)) == 0 and (rec.channel, rec.index) == (c, ix)
    assert lib.wmi_channels_get_segment(ctx, len(order), C.byref(rec)) == -1 and lib.wmi_channels_get_segment(ctx, -1, C.byref(rec)) == -1
    assert [(d["channel"], d["index"], d["t0"], d["t1"], d["text"]) for d in dialogue] == [(c, i) + segs[c][i][:3] for c, i in order]
    assert lib.whisper_full_lang_id(ctx) == per[0][1]                               # the language id is channel 0's
    assert lib.wmi_full_n_windows(ctx) == 0                                         # no window records, no speaker table
    sp = abi.wmi_speaker()
    assert not order or lib.wmi_full_get_segment_speaker(ctx, 0, C.byref(sp)) == -2
    # the selection round-trips
    for c in (0, 1, -1, 1, 0, -1):
        n = lib.wmi_channels_select(ctx, c)
        assert n == (len(order) if c < 0 else len(segs[c])) and _shown(node) == (shown if c < 0 else segs[c])
        assert lib.wmi_channels_get_segment(ctx, 0, C.byref(rec)) == (0 if c < 0 and order else -1)     # only the dialogue view answers
        assert lib.wmi_full_n_windows(ctx) == (0 if c < 0 else len(per[c][4]))
    assert lib.wmi_channels_select(ctx, 2) == -1 and lib.wmi_channels_select(ctx, -2) == -1
    assert lib.wmi_batch_select(ctx, 1) == len(segs[1]) and lib.wmi_channels_get_segment(ctx, 0, C.byref(rec)) == -1
    assert lib.wmi_channels_select(ctx, -1) == len(order)
    return order


@pytest.mark.parametrize("fmt,rate,conv,seconds", [(wr.S16, 48000, 2, 5.0), (wr.S8, 16000, 2, 4.0), (wr.F32, 22050, 1, 4.0)],
                         ids=["s16-48000-sinc", "s8-16000", "f32-22050-medium"])
def test_channels_equal_full_batch_on_the_judges_samples(product_lib, node, fmt, rate, conv, seconds):
    data = _clip(fmt, rate, seconds, seed=60)
    pcms = cr.convert_channels(data, fmt, rate, conv)
    assert pcms[0].size == pcms[1].size and abs(pcms[0].size - seconds * SR) <= 1 and pcms[0].tobytes() != pcms[1].tobytes()
    dialogue, listed, per, delta = _channels_route(node, data, fmt, rate, conv)
    s = _stats(product_lib, node.ctx)
    n = pcms[0].size
    assert s[:4] == [len(data) + (12 * n if rate == 22050 else 0), int(seconds * rate), 2 * n, 1] and s[4] >= 0
    order = _check_dialogue(node, dialogue, per)
    want_listed, want_per, want_delta = _batch_route(node, pcms)
    assert (listed, per, delta) == (want_listed, want_per, want_delta)
    assert all(len(r) > 1 for r in listed) and len(order) >= 2
    # the batch call was a transcription call: the channels result is gone
    assert product_lib.wmi_channels_select(node.ctx, -1) == -1 and product_lib.wmi_channels_select(node.ctx, 0) == -1


def test_multilingual_auto_and_a_device_resident_clip(product_lib, hip):
    """the multilingual model with the language left to the call (the language token matters, per channel), the clip already on the device,
    one frame behind a 16-byte boundary"""
    node = host.SpeechToText(product_lib); node.set_language_model(synth.make_model("micro", seed=77)); node.language = "auto"
    lib, ctx = product_lib, node.ctx
    d = C.c_void_p()
    try:
        data = _clip(wr.S16, 44100, 4.0, seed=70)
        pcms = cr.convert_channels(data, wr.S16, 44100, 2)
        host_route = _channels_route(node, data, wr.S16, 44100, 2)
        assert hip.hipMalloc(C.byref(d), C.c_size_t(len(data) + 64)) == 0
        src = C.c_void_p(d.value + 4)
        assert hip.hipMemcpy(src, data, C.c_size_t(len(data)), 1) == 0
        before = _counters(lib, ctx)
        w = abi.wmi_wav(src, len(data), wr.S16, 1, 44100, 1)
        assert lib.wmi_full_wav_channels(ctx, _params(node), C.byref(w), 2) == 0
        assert _stats(lib, ctx)[:4] == [0, 4 * 44100, 2 * pcms[0].size, 1]           # nothing is uploaded
        rec, dev_dialogue = abi.wmi_channel_segment(), []
        for i, (t0, t1, text) in enumerate(node.segments()):                        # the call leaves the dialogue view selected
            assert lib.wmi_channels_get_segment(ctx, i, C.byref(rec)) == 0
            dev_dialogue.append({"channel": rec.channel, "index": rec.index, "t0": t0, "t1": t1, "text": text})
        per, delta = _per_chunk(node, before)
        assert (dev_dialogue, per, delta) == (host_route[0], host_route[2], host_route[3])
        _check_dialogue(node, dev_dialogue, per)
        want_listed, want_per, want_delta = _batch_route(node, pcms)
        assert (host_route[1], per, delta) == (want_listed, want_per, want_delta)
        assert all(len(r) > 1 for r in want_listed)
    finally:
        if d.value:
            hip.hipFree(d)
        node.close()


def test_a_following_whisper_full_invalidates_the_view(product_lib, node):
    lib, ctx = product_lib, node.ctx
    assert lib.wmi_channels_select(ctx, -1) == -1                                   # no channels call yet
    data = _clip(wr.S16, 16000, 3.0, seed=80)
    dialogue = node.transcribe_wav_channels(data, wr.S16, 16000, params=_params(node))
    assert node.last_ret == 0 and lib.wmi_channels_select(ctx, -1) == len(dialogue) and lib.wmi_channels_select(ctx, 1) >= 0
    pcm = synth.make_pcm(2.0, seed=81)
    one = node.transcribe(pcm, params=_params(node))
    assert node.last_ret == 0
    rec = abi.wmi_channel_segment()
    assert lib.wmi_channels_select(ctx, -1) == lib.wmi_channels_select(ctx, 0) == lib.wmi_channels_select(ctx, 1) == -1
    assert lib.wmi_channels_get_segment(ctx, 0, C.byref(rec)) == -1
    assert node.collect() == one                                                     # the refused selections changed nothing
    # and a failed channels call leaves none behind either
    node.transcribe_wav_channels(data, wr.S16, 16000, params=_params(node))
    mono = host.SpeechToText._wav(data, wr.S16, 0, 16000)
    assert lib.wmi_full_wav_channels(ctx, _params(node), C.byref(mono[0]), 2) == -112
    assert lib.wmi_channels_select(ctx, -1) == len(dialogue)                         # (decided before anything was touched: the view stays)


@pytest.mark.parametrize("no_speech", [0, abi.NO_SPEECH_REPORT], ids=["plain", "no-speech-report"])
def test_one_silent_channel_equals_the_batch_call(product_lib, model, no_speech):
    node = host.SpeechToText(product_lib, no_speech=no_speech); node.set_language_model(model)
    try:
        data = _clip(wr.S16, 48000, 4.0, seed=90, silent=1)
        pcms = cr.convert_channels(data, wr.S16, 48000, 2)
        assert not pcms[1].any() and pcms[0].any()
        dialogue, listed, per, delta = _channels_route(node, data, wr.S16, 48000, 2)
        _check_dialogue(node, dialogue, per)
        assert (listed, per, delta) == _batch_route(node, pcms)
        if no_speech:
            assert all(p[4] and all(0.0 <= w["no_speech_prob"] <= 1.0 for w in p[4]) for p in per)     # windows per channel
        else:
            assert all(p[4] == [] for p in per)
    finally:
        node.close()


def test_token_dtw_passes_through(product_lib, model):
    node = host.SpeechToText(product_lib, token_dtw=True); node.set_language_model(model)
    try:
        data = _clip(wr.S8, 48000, 4.0, seed=50)
        pcms = cr.convert_channels(data, wr.S8, 48000, 1)
        dialogue, listed, per, delta = _channels_route(node, data, wr.S8, 48000, 1)
        _check_dialogue(node, dialogue, per)                                          # t_dtw of the view = the per-channel results'
        assert any(t[6] >= 0 for p in per for seg in p[0] for t in seg[3])
        assert (listed, per, delta) == _batch_route(node, pcms)
    finally:
        node.close()


def test_a_speaker_mode_is_ignored(product_lib, model):
    node = host.SpeechToText(product_lib, speaker_labels=True); node.set_language_model(model)
    plain = host.SpeechToText(product_lib); plain.set_language_model(model)
    try:
        data = _clip(wr.S16, 44100, 3.0, seed=95)
        got = _channels_route(node, data, wr.S16, 44100, 2)
        assert got == _channels_route(plain, data, wr.S16, 44100, 2)
        sp = abi.wmi_speaker()
        for c in (0, 1, -1):
            if product_lib.wmi_channels_select(node.ctx, c) > 0:
                assert product_lib.wmi_full_get_segment_speaker(node.ctx, 0, C.byref(sp)) == -2
        s4 = (C.c_int64 * 4)()
        assert product_lib.wmi_speaker_stats(node.ctx, s4) == 0 and list(s4)[2:] == [0, 0]      # no table was copied, nothing launched
    finally:
        node.close(); plain.close()


def test_the_other_calls_are_untouched_around_a_channels_call(product_lib, model):
    """whisper_full, wmi_full_wav and wmi_full_batch_wav give the same bytes and counters before and after a channels call on the same
    context; a context that never makes one reports nothing"""
    pcm = synth.make_pcm(4.0, seed=8)
    fresh = host.SpeechToText(product_lib); fresh.set_language_model(model)
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    lib = product_lib
    try:
        data = _clip(wr.S16, 44100, 3.0, seed=21)
        clips = [(data, wr.S16, 1, 44100), (data[:len(data) // 2], wr.S8, 0, 22050)]

        def three():
            out = []
            for i, run in enumerate((lambda: node.transcribe(pcm, params=_params(node)),
                                     lambda: node.transcribe_wav(data, wr.S16, 1, 44100, params=_params(node)),
                                     lambda: node.transcribe_wav_batch(clips, params=_params(node)))):
                before = _counters(lib, node.ctx)
                r = run()
                assert node.last_ret == 0
                # (the WAV counters are those of the last WAV call: whisper_full leaves them as they were)
                out.append((r, node.segments(), list(_counters(lib, node.ctx) - before), _stats(lib, node.ctx)[:4] if i else None))
            return out
        first = three()
        assert len(node.transcribe_wav_channels(data, wr.S16, 44100, params=_params(node))) >= 2 and node.last_ret == 0
        assert three() == first
        assert fresh.transcribe(pcm, params=_params(fresh)) == first[0][0]
        assert _stats(lib, fresh.ctx) == [0, 0, 0, 0, 0]                             # no work set was ever made
        assert lib.wmi_channels_select(fresh.ctx, -1) == -1
    finally:
        node.close(); fresh.close()

"""-m gpu: wmi_full_wav / wmi_full_long_wav / wmi_full_batch_wav (include/wmi_device.h) — an AudioStreamWAV's bytes transcribed as they are.

Each call must give what the call it ends in gives on the judge's samples (tests/wav_ref.py: decode, fold, resample on the CPU): the same
tokens, segments, times and counters, strictly — the converted samples are the judge's bit for bit (tests/test_gpu_wav_pcm.py), and behind
them the same code runs on the same build."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import wav_ref as wr
from godot_whisper_amd import abi, host, synth

pytestmark = pytest.mark.gpu

SR = 16000


@pytest.fixture(scope="module")
def model():
    return synth.make_model("micro.en", seed=2024)


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


def _clip(fmt, stereo, rate, seconds, seed):
    """synthetic speech at `rate` (the 16 kHz generator's samples played at that rate: any signal will do), two different channels"""
    n = int(seconds * rate)
    chans = [synth.make_pcm(n / SR, seed=seed + c)[:n] for c in range(2 if stereo else 1)]
    return wr.pack(np.stack(chans, axis=1).reshape(-1), fmt)


def _both(node, run_wav, run_plain):
    """-> (result, segments, windows, counter deltas) of both routes, the new one first"""
    out = []
    for run in (run_wav, run_plain):
        before = _counters(node.lib, node.ctx)
        r = run()
        assert node.last_ret == 0, node.last_ret
        out.append((r, node.segments(), list(node.last_windows), list(_counters(node.lib, node.ctx) - before)))
    return out


def test_jfk_data_chunk_equals_whisper_full(product_lib, node):
    """the node's own case: s16 mono 16 kHz, the bytes Godot's importer keeps — one decode launch in front of the log-mel"""
    data, channels, rate, bits = wr.riff_data(gu.GOLDEN / "jfk.wav")
    assert (channels, rate, bits) == (1, 16000, 16)
    pcm = wr.convert(data, wr.S16, 0, rate, 2)
    assert pcm.tobytes() == synth.read_wav_mono16(gu.GOLDEN / "jfk.wav").tobytes()
    got, want = _both(node, lambda: node.transcribe_wav(data, wr.S16, 0, rate, params=_params(node)), lambda: node.transcribe(pcm, params=_params(node)))
    assert got == want and len(got[0]) > 1
    assert node.transcribe_wav(data, wr.S16, 0, rate, params=_params(node)) == got[0]
    assert _stats(product_lib, node.ctx)[:4] == [len(data), pcm.size, pcm.size, 1]
    text = host.AudioStreamToText.get_text_wav(node, data, wr.S16, 0, rate)
    assert text == host.AudioStreamToText.get_text(node, pcm)


@pytest.mark.parametrize("fmt,stereo,rate,conv", [(wr.S16, 1, 44100, 2), (wr.S8, 0, 22050, 4)], ids=["s16x2-44100-sinc", "s8-22050-linear"])
def test_other_formats_and_rates_equal_whisper_full_on_the_judges_samples(product_lib, node, fmt, stereo, rate, conv):
    data = _clip(fmt, stereo, rate, 4.0, seed=40)
    pcm = wr.convert(data, fmt, stereo, rate, conv)
    assert abs(pcm.size - 4 * SR) <= 1
    got, want = _both(node, lambda: node.transcribe_wav(data, fmt, stereo, rate, interpolator_type=conv, params=_params(node)),
                      lambda: node.transcribe(pcm, params=_params(node)))
    assert got == want and len(got[0]) > 1
    s = _stats(product_lib, node.ctx)
    assert s[:4] == [len(data) + (12 * pcm.size if rate == 22050 else 0), int(4.0 * rate), pcm.size, 1] and s[4] >= 0
    # what the reference node's loop would have transcribed instead: the interleaved samples as 16 kHz mono — another signal
    assert wr.samples(data, fmt).size != pcm.size


def test_long_recording_equals_full_long(product_lib, node):
    """about 40 s of gated bursts at 48 kHz s16 stereo: plan, pieces and the merged view of wmi_full_long on the judge's samples"""
    import segment_f64 as sj
    parts = [1.5, -0.8, 2.0, -2.5, 12.0, -0.5, 1.2, -3.0, 6.0, -2.0, 5.0, -1.5, 2.0]
    x16 = np.concatenate([synth.make_pcm(s, seed=900 + i) if s > 0 else np.zeros(int(round(-s * SR)), np.float32) for i, s in enumerate(parts)])
    x48 = np.repeat(x16, 3)                                                        # zeros stay zeros: the silences survive the format
    data = wr.pack(np.stack([x48, 0.5 * x48], axis=1).reshape(-1), wr.S16)
    pcm = wr.convert(data, wr.S16, 1, 48000, 2)
    assert 39 * SR < pcm.size < 42 * SR
    lp = sj.params(max_piece_ms=5000)
    views = []
    for run in (lambda: node.transcribe_wav_long(data, wr.S16, 1, 48000, 2, _params(node), lp), lambda: node.transcribe_long(pcm, _params(node), lp)):
        before = _counters(product_lib, node.ctx)
        merged = run()
        assert node.last_ret == 0
        pieces = list(node.last_pieces)
        per_piece = []
        for i in range(len(pieces)):
            assert product_lib.wmi_long_select(node.ctx, i) == pieces[i]["n_segments"]
            per_piece.append((node.collect(), node.segments()))
        assert product_lib.wmi_long_select(node.ctx, -1) == len(node.last_segments)
        views.append((merged, pieces, list(node.last_modes), list(node.last_segments), per_piece, list(_counters(product_lib, node.ctx) - before)))
    assert views[0] == views[1]
    assert len(views[0][1]) >= 6 and len(views[0][0]) > 1
    node.transcribe_wav_long(data, wr.S16, 1, 48000, 2, _params(node), lp)
    assert _stats(product_lib, node.ctx)[:4] == [len(data), x48.size, pcm.size, 1]


def test_batch_of_three_formats_equals_full_batch(product_lib):
    """three clips, three formats and rates, on a multilingual model with the language left to the call: the language token matters"""
    node = host.SpeechToText(product_lib); node.set_language_model(synth.make_model("micro", seed=77)); node.language = "auto"
    try:
        specs = [(wr.S16, 1, 48000, 3.0, 11), (wr.S8, 0, 22050, 2.5, 12), (wr.F32, 1, 16000, 3.5, 13)]
        clips = [(_clip(f, st, r, sec, seed), f, st, r) for f, st, r, sec, seed in specs]
        pcms = [wr.convert(d, f, st, r, 2) for d, f, st, r in clips]
        outs = []
        for run in (lambda: node.transcribe_wav_batch(clips, params=_params(node)), lambda: node.transcribe_batch(pcms, params=_params(node))):
            before = _counters(product_lib, node.ctx)
            r = run()
            assert node.last_ret == 0
            outs.append((r, list(node.last_modes), list(node.last_langs), list(node.last_batch_windows), list(_counters(product_lib, node.ctx) - before)))
        assert outs[0] == outs[1]
        assert len(outs[0][0]) == 3 and all(len(r) > 1 for r in outs[0][0])
        node.transcribe_wav_batch(clips, params=_params(node))
        s = _stats(product_lib, node.ctx)
        assert s[:4] == [sum(len(c[0]) for c in clips) + 12 * pcms[1].size, sum(int(sec * r) for _, _, r, sec, _ in specs), sum(p.size for p in pcms), 3]
    finally:
        node.close()


def test_no_speech_report_passes_through(product_lib, model):
    node = host.SpeechToText(product_lib, no_speech=abi.NO_SPEECH_REPORT); node.set_language_model(model)
    try:
        data = _clip(wr.S16, 1, 44100, 4.0, seed=40)
        pcm = wr.convert(data, wr.S16, 1, 44100, 2)
        got, want = _both(node, lambda: node.transcribe_wav(data, wr.S16, 1, 44100, params=_params(node)), lambda: node.transcribe(pcm, params=_params(node)))
        assert got == want and got[2] and all(0.0 <= w["no_speech_prob"] <= 1.0 for w in got[2])
    finally:
        node.close()


def test_token_dtw_passes_through(product_lib, model):
    node = host.SpeechToText(product_lib, token_dtw=True); node.set_language_model(model)
    try:
        data = _clip(wr.S8, 1, 48000, 4.0, seed=50)
        pcm = wr.convert(data, wr.S8, 1, 48000, 1)
        got, want = _both(node, lambda: node.transcribe_wav(data, wr.S8, 1, 48000, interpolator_type=1, params=_params(node)),
                          lambda: node.transcribe(pcm, params=_params(node)))
        assert got == want and any(d["t_dtw"] >= 0 for d in got[0][1:])
    finally:
        node.close()


def test_error_codes_and_empty_clips(product_lib, node):
    lib, ctx, p = product_lib, node.ctx, _params(node)
    data = _clip(wr.S16, 0, 48000, 1.0, seed=3)

    def wav(d=data, fmt=wr.S16, st=0, rate=48000):
        return SpeechToTextWav(d, fmt, st, rate)
    for kw, conv, e in ((dict(fmt=2), 2, -11), (dict(fmt=7), 2, -1), (dict(st=3), 2, -1), (dict(rate=0), 2, -1), (dict(), 0, -10), (dict(), 9, -1)):
        w = wav(**kw)
        assert lib.wmi_full_wav(ctx, p, C.byref(w.c), conv) == -100 + e, kw
        assert lib.wmi_full_long_wav(ctx, p, C.byref(w.c), conv, None) == -100 + e, kw
        assert lib.wmi_full_batch_wav(ctx, p, C.byref(w.c), 1, conv) == -100 + e, kw
    # an empty clip: what the call it ends in answers for no samples
    one = np.zeros(1, np.float32)
    for rate in (16000, 44100):
        w = wav(d=b"", rate=rate)
        assert lib.wmi_full_wav(ctx, p, C.byref(w.c), 2) == lib.whisper_full(ctx, p, host._fptr(one), 0)
        assert lib.whisper_full_n_segments(ctx) == 0
        assert lib.wmi_full_long_wav(ctx, p, C.byref(w.c), 2, None) == lib.wmi_full_long(ctx, p, one.ctypes.data, 0, 0, None) == -3
        ptrs, lens = (C.c_void_p * 1)(one.ctypes.data), (C.c_int * 1)(0)
        assert lib.wmi_full_batch_wav(ctx, p, C.byref(w.c), 1, 2) == lib.wmi_full_batch(ctx, p, ptrs, lens, 1, 0)
    # a clip below one second transcribes to nothing, as its samples do
    short = _clip(wr.S16, 0, 48000, 0.5, seed=4)
    assert node.transcribe_wav(short, wr.S16, 0, 48000, params=p) == node.transcribe(wr.convert(short, wr.S16, 0, 48000, 2), params=p)


class SpeechToTextWav:
    """a wmi_wav over host bytes that stay referenced"""

    def __init__(self, data, fmt, stereo, rate):
        self.c, self.keep = host.SpeechToText._wav(data, fmt, stereo, rate)


def test_whisper_full_is_untouched_around_the_new_calls(product_lib, model):
    """the same whisper_full before and after the three calls gives the same bytes; a context that never makes them reports zeros"""
    pcm = synth.make_pcm(5.0, seed=8)
    fresh = host.SpeechToText(product_lib); fresh.set_language_model(model)
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    try:
        first = node.transcribe(pcm, params=_params(node)); first_seg = node.segments()
        assert _stats(product_lib, node.ctx) == [0, 0, 0, 0, 0]
        data = _clip(wr.S16, 1, 44100, 3.0, seed=21)
        assert len(node.transcribe_wav(data, wr.S16, 1, 44100, params=_params(node))) > 1
        assert node.transcribe_wav_batch([(data, wr.S16, 1, 44100), (data[:len(data) // 2], wr.S8, 0, 22050)], params=_params(node)) and node.last_ret == 0
        node.transcribe_wav_long(data, wr.S16, 1, 44100, params=_params(node)); assert node.last_ret == 0
        again = node.transcribe(pcm, params=_params(node))
        assert again == first and node.segments() == first_seg
        assert fresh.transcribe(pcm, params=_params(fresh)) == first
        assert _stats(product_lib, fresh.ctx) == [0, 0, 0, 0, 0]
    finally:
        node.close(); fresh.close()

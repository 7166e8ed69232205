"""-m gpu: IMA-ADPCM clips (format 2) through every WAV call in mode 1 of wmi_set_wav_adpcm (include/wmi_device.h).

The contract is one sentence: a format-2 clip gives exactly what the same call gives for WMI_WAV_S16 data equal to the judge's decoded
samples (tests/adpcm_ref.py), with the same stereo and mix_rate — tokens, segments, times, windows, counters, speaker records, both
channels and the dialogue view, strictly.  Also: a batch of mixed formats, a device-resident source, mode 0's -111, PCM results untouched
by the mode, and wmi_wav_stats."""
import ctypes as C

import numpy as np
import pytest

import adpcm_ref as ar
import wav_ref as wr
from godot_whisper_amd import abi, host, synth

pytestmark = pytest.mark.gpu

SR = 16000


def _launches(lib):
    """the decode's launches per clip, as the kernel file exports them"""
    out = (C.c_int * 5)()
    assert lib.wmi_selftest_adpcm_shape(out) == 0
    return out[4]


@pytest.fixture(scope="module")
def model():
    return synth.make_model("micro.en", seed=2024)


@pytest.fixture(scope="module")
def clips():
    """name -> (ADPCM bytes, the judge's samples as s16 bytes, stereo, rate): encoded once, decoded by the judge once."""
    out = {}
    for name, stereo, rate, seconds, seed in (("mono16k", 0, 16000, 2.0, 31), ("stereo44k", 1, 44100, 2.0, 33), ("mono22k", 0, 22050, 1.5, 35)):
        n = int(seconds * rate)
        chans = [(1.0, 0.35)[c] * synth.make_pcm(n / SR, seed=seed + c)[:n] for c in range(2 if stereo else 1)]
        data = ar.encode_clip(np.stack(chans, axis=1).reshape(-1), stereo)
        s16 = ar.decode(data, stereo)
        assert s16.size == n // 2 * 2 * (2 if stereo else 1) and int(np.abs(s16.astype(np.int32)).max()) > 2000
        out[name] = (data, s16.astype("<i2").tobytes(), stereo, rate)
    return out


@pytest.fixture
def node(product_lib, model):
    n = host.SpeechToText(product_lib, wav_adpcm=True); n.set_language_model(model)
    yield n
    n.close()


def _params(node, token_timestamps=False):
    p = node.full_params("", 0); p.temperature_inc = 0.0; p.token_timestamps = token_timestamps
    return p


def _counters(lib, ctx):
    t6, n5 = (C.c_int64 * 6)(), (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return np.array(list(n5))


def _stats(lib, ctx):
    s = (C.c_int64 * 5)()
    assert lib.wmi_wav_stats(ctx, s) == 0
    return list(s)


def _both(node, run):
    """run(data, format) on the ADPCM bytes and on the judge's s16 bytes -> the two views, the new route first"""
    out = []
    for which in (0, 1):
        before = _counters(node.lib, node.ctx)
        r = run(which)
        assert node.last_ret == 0, node.last_ret
        out.append((r, node.segments(), list(node.last_windows), list(_counters(node.lib, node.ctx) - before)))
    return out


def _speaker_records(lib, ctx):
    out = []
    for i in range(lib.whisper_full_n_segments(ctx)):
        o = abi.wmi_speaker()
        rc = lib.wmi_full_get_segment_speaker(ctx, i, C.byref(o))
        out.append(("segment", i, rc, o.speaker, o.is0, o.is1, o.e0, o.e1))
        for j in range(lib.whisper_full_n_tokens(ctx, i)):
            rc = lib.wmi_full_get_token_speaker(ctx, i, j, C.byref(o))
            out.append(("token", i, j, rc) + ((o.speaker, o.is0, o.is1, o.e0, o.e1) if rc == 0 else ()))
    return out


@pytest.mark.parametrize("name,conv", [("mono16k", 2), ("stereo44k", 2), ("mono22k", 4)])
def test_full_wav_equals_the_call_on_the_judges_samples(product_lib, node, clips, name, conv):
    data, s16, stereo, rate = clips[name]
    got, want = _both(node, lambda w: node.transcribe_wav((data, s16)[w], (ar.ADPCM, wr.S16)[w], stereo, rate, interpolator_type=conv, params=_params(node)))
    assert got == want and len(got[0]) > 1
    node.transcribe_wav(data, ar.ADPCM, stereo, rate, interpolator_type=conv, params=_params(node))
    frames = ar.frames_of(len(data), stereo)
    n_out = wr.convert(s16, wr.S16, stereo, rate, conv).size
    s = _stats(product_lib, node.ctx)
    assert s[:4] == [len(data) + (12 * n_out if rate == 22050 else 0), frames, n_out, 1 + _launches(product_lib)] and s[4] >= 0       # the ADPCM bytes went up, not s16
    text = host.AudioStreamToText.get_text_wav(node, data, ar.ADPCM, stereo, rate, interpolator_type=conv)
    assert text == host.AudioStreamToText.get_text_wav(node, s16, wr.S16, stereo, rate, interpolator_type=conv)


def test_samples_are_the_judges_bit_for_bit(product_lib, node, clips):
    lib, ctx = product_lib, node.ctx
    for name, conv in (("mono16k", 2), ("stereo44k", 2), ("stereo44k", 4), ("mono22k", 3)):
        data, s16, stereo, rate = clips[name]
        want = wr.convert(s16, wr.S16, stereo, rate, conv)
        got = np.full(want.size + 3, np.nan, np.float32)
        w, _keep = host.SpeechToText._wav(data, ar.ADPCM, stereo, rate)
        assert lib.wmi_wav_to_pcm(ctx, C.byref(w), conv, got.ctypes.data_as(C.c_void_p), got.size, 0) == want.size
        assert got[:want.size].tobytes() == want.tobytes() and np.all(np.isnan(got[want.size:]))
        if stereo:
            a, b = np.full(want.size, np.nan, np.float32), np.full(want.size, np.nan, np.float32)
            a2, b2 = a.copy(), b.copy()
            ws, _k2 = host.SpeechToText._wav(s16, wr.S16, 1, rate)
            assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), conv, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.size, 0) == want.size
            assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(ws), conv, a2.ctypes.data_as(C.c_void_p), b2.ctypes.data_as(C.c_void_p), a.size, 0) == want.size
            assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes() and not np.any(np.isnan(a)) and a.tobytes() != b.tobytes()


def test_long_form_equals_full_long_wav_on_the_judges_samples(product_lib, node, clips):
    data, s16, stereo, rate = clips["stereo44k"]
    views = []
    for which in (0, 1):
        before = _counters(product_lib, node.ctx)
        merged = node.transcribe_wav_long((data, s16)[which], (ar.ADPCM, wr.S16)[which], stereo, rate, 2, _params(node))
        assert node.last_ret == 0
        views.append((merged, list(node.last_pieces), list(node.last_modes), list(node.last_segments), list(_counters(product_lib, node.ctx) - before)))
    assert views[0] == views[1] and len(views[0][0]) > 1


def test_a_batch_of_s16_s8_and_adpcm_clips(product_lib, node, clips):
    pcm_a = wr.pack(synth.make_pcm(1.5, seed=61), wr.S16)
    pcm_b = wr.pack(np.stack([synth.make_pcm(1.2, seed=62)] * 2, axis=1).reshape(-1), wr.S8)
    fixed = [(pcm_a, wr.S16, 0, 16000), (pcm_b, wr.S8, 1, 16000)]
    mixed = [fixed[0]] + [(clips[n][0], ar.ADPCM, clips[n][2], clips[n][3]) for n in ("stereo44k", "mono16k")] + [fixed[1], (clips["mono22k"][0], ar.ADPCM, 0, 22050)]
    plain = [fixed[0]] + [(clips[n][1], wr.S16, clips[n][2], clips[n][3]) for n in ("stereo44k", "mono16k")] + [fixed[1], (clips["mono22k"][1], wr.S16, 0, 22050)]
    outs = []
    for batch in (mixed, plain):
        before = _counters(product_lib, node.ctx)
        r = node.transcribe_wav_batch(batch, params=_params(node))
        assert node.last_ret == 0
        outs.append((r, list(node.last_modes), list(node.last_batch_windows), list(_counters(product_lib, node.ctx) - before)))
        if batch is mixed:
            s_mixed = _stats(product_lib, node.ctx)
        else:
            s_plain = _stats(product_lib, node.ctx)
    assert outs[0] == outs[1] and len(outs[0][0]) == 5 and all(len(r) > 1 for r in outs[0][0])
    saved = sum(len(clips[n][1]) - len(clips[n][0]) for n in ("stereo44k", "mono16k", "mono22k"))
    assert s_mixed[0] == s_plain[0] - saved and s_mixed[1:3] == s_plain[1:3] and s_mixed[3] == s_plain[3] + 3 * _launches(product_lib) == 5 + 3 * _launches(product_lib)


def test_speaker_modes_pass_through(product_lib, model, clips):
    lib = product_lib
    node = host.SpeechToText(lib, speaker_labels="tokens", wav_adpcm=True); node.set_language_model(model)
    try:
        data, s16, stereo, rate = clips["stereo44k"]
        views = []
        for which in (0, 1):
            r = node.transcribe_wav((data, s16)[which], (ar.ADPCM, wr.S16)[which], 1, rate, params=_params(node, True))
            assert node.last_ret == 0
            st = (C.c_int64 * 4)()
            assert lib.wmi_speaker_stats(node.ctx, st) == 0
            views.append((r, node.segments(), _speaker_records(lib, node.ctx), list(st)))
        assert views[0] == views[1]
        recs = views[0][2]
        assert any(x[0] == "segment" and x[2] == 0 and x[3] == 0 for x in recs)      # the left channel is the louder one
        assert any(x[0] == "token" and x[3] == 0 for x in recs)
        # ranges of the caller's own
        t0, t1 = (C.c_int64 * 3)(0, 50, 120), (C.c_int64 * 3)(50, 120, 400)
        outs = []
        for which in (0, 1):
            w, _keep = host.SpeechToText._wav((data, s16)[which], (ar.ADPCM, wr.S16)[which], 1, rate)
            o = (abi.wmi_speaker * 3)()
            assert lib.wmi_wav_speaker(node.ctx, C.byref(w), t0, t1, 3, 0.0, o) == 0
            outs.append([(x.speaker, x.is0, x.is1, x.e0, x.e1) for x in o])
        assert outs[0] == outs[1] and outs[0][0][3] > 0
    finally:
        node.close()


def test_both_channels_and_the_dialogue_view(product_lib, node, clips):
    data, s16, stereo, rate = clips["stereo44k"]
    views = []
    for which in (0, 1):
        before = _counters(product_lib, node.ctx)
        dlg = node.transcribe_wav_channels((data, s16)[which], (ar.ADPCM, wr.S16)[which], rate, params=_params(node))
        assert node.last_ret == 0
        views.append((dlg, list(node.last_channels), list(node.last_modes), list(_counters(product_lib, node.ctx) - before)))
    assert views[0] == views[1]
    assert len(views[0][1]) == 2 and all(len(r) > 1 for r in views[0][1]) and {d["channel"] for d in views[0][0]} == {0, 1}
    s = _stats(product_lib, node.ctx)
    node.transcribe_wav_channels(data, ar.ADPCM, rate, params=_params(node))
    s2 = _stats(product_lib, node.ctx)
    assert s2[0] == len(data) and s2[1:3] == s[1:3] and s2[3] == s[3] + _launches(product_lib) == 1 + _launches(product_lib)
    # a mono clip: -112, decided as for the PCM formats
    mono = clips["mono16k"]
    w, _keep = host.SpeechToText._wav(mono[0], ar.ADPCM, 0, 16000)
    assert product_lib.wmi_full_wav_channels(node.ctx, _params(node), C.byref(w), 2) == -112


def test_a_device_resident_adpcm_clip_at_an_odd_address(product_lib, node, clips):
    lib, ctx = product_lib, node.ctx
    hip = C.CDLL("libamdhip64.so")
    d = C.c_void_p()
    data, s16, stereo, rate = clips["stereo44k"]
    assert hip.hipMalloc(C.byref(d), C.c_size_t(len(data) + 64)) == 0
    try:
        want = node.transcribe_wav(s16, wr.S16, 1, rate, params=_params(node)); want_seg = node.segments()
        for off in (7, 10):                                                       # odd: every chunk by bytes; even: a head of byte pairs
            src = C.c_void_p(d.value + off)
            assert hip.hipMemcpy(src, data, C.c_size_t(len(data)), 1) == 0
            w = abi.wmi_wav(src, len(data), ar.ADPCM, 1, rate, 1)
            assert lib.wmi_full_wav(ctx, _params(node), C.byref(w), 2) == 0
            assert node.collect() == want and node.segments() == want_seg and len(want) > 1
            s = _stats(lib, ctx)
            assert s[0] == 0 and s[3] == 1 + _launches(lib)                                # nothing was uploaded
    finally:
        hip.hipFree(d)


def test_mode_0_refuses_and_pcm_results_do_not_move(product_lib, model, clips):
    lib = product_lib
    node = host.SpeechToText(lib); node.set_language_model(model)                # the mode is never touched at first
    try:
        assert not node._adpcm_called
        data, s16, stereo, rate = clips["stereo44k"]
        assert node.transcribe_wav(data, ar.ADPCM, 1, rate, params=_params(node)) == [] and node.last_ret == -111
        assert node.transcribe_wav_batch([(data, ar.ADPCM, 1, rate)], params=_params(node)) == [] and node.last_ret == -111
        assert node.transcribe_wav_channels(data, ar.ADPCM, rate, params=_params(node)) == [] and node.last_ret == -111
        pcm_clip = wr.pack(np.stack([synth.make_pcm(2.0, seed=71), synth.make_pcm(2.0, seed=72)], axis=1).reshape(-1), wr.S8)

        def pcm_views():
            a = node.transcribe_wav(s16, wr.S16, 1, rate, params=_params(node)); sa = node.segments()
            b = node.transcribe_wav_batch([(pcm_clip, wr.S8, 1, 16000), (s16, wr.S16, 1, rate)], params=_params(node))
            c = node.transcribe_wav_channels(pcm_clip, wr.S8, 16000, params=_params(node))
            return a, sa, b, c, _stats(lib, node.ctx)[:4]
        before = pcm_views()
        assert len(before[0]) > 1
        assert node.set_wav_adpcm(True) == 0
        assert len(node.transcribe_wav(data, ar.ADPCM, 1, rate, params=_params(node))) > 1 and node.last_ret == 0
        assert pcm_views() == before                                              # with the mode on ...
        assert node.set_wav_adpcm(False) == 1
        assert pcm_views() == before                                              # ... and off again
        assert node.transcribe_wav(data, ar.ADPCM, 1, rate, params=_params(node)) == [] and node.last_ret == -111
        w, _keep = host.SpeechToText._wav(data, 3, 1, rate)                          # QOA: refused in both modes
        assert lib.wmi_full_wav(node.ctx, _params(node), C.byref(w), 2) == -111
        assert node.set_wav_adpcm(True) == 0 and lib.wmi_full_wav(node.ctx, _params(node), C.byref(w), 2) == -111
    finally:
        node.close()

"""-m gpu: the speaker modes of wmi_set_speaker through the transcription calls that take them — wmi_full_wav, wmi_full_long_wav,
wmi_full_batch_wav, wmi_capture_full — on synthetic models and clips of a few seconds.

Mode 0 is what the calls were: the result of a context on which wmi_set_speaker was never called, byte for byte, and the accessors answer
-2.  Modes 1 and 2 change no token, segment, time or counter, and every record equals the judge (tests/speaker_ref.py: main.cpp's
sequential loop) evaluated on the result's own t0 / t1: with `==` for s16 and s8 clips, within 2 m 2^-53 for f32 ones."""
import ctypes as C

import numpy as np
import pytest

import speaker_ref as sr
import stage_compare as sc
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


def _params(node, token_timestamps=True):
    p = node.full_params("", 0); p.temperature_inc = 0.0; p.token_timestamps = token_timestamps
    return p


def _counters(lib, ctx):
    t6, n5 = (C.c_int64 * 6)(), (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return np.array(list(n5))


def _clip(fmt, stereo, rate, seconds, seed, gains=(1.0, 0.3)):
    """synthetic speech at `rate`, two different channels of different loudness"""
    n = int(seconds * rate)
    chans = [gains[c] * synth.make_pcm(n / SR, seed=seed + c)[:n] for c in range(2 if stereo else 1)]
    return wr.pack(np.stack(chans, axis=1).reshape(-1).astype(np.float32), fmt)


def _rec(o):
    return dict(speaker=o.speaker, is0=o.is0, is1=o.is1, e0=o.e0, e1=o.e1)


def _segment_records(lib, ctx):
    """-> [(t0, t1, record)] of the selected result, or the accessor's error code"""
    out = []
    for i in range(lib.whisper_full_n_segments(ctx)):
        o = abi.wmi_speaker()
        rc = lib.wmi_full_get_segment_speaker(ctx, i, C.byref(o))
        if rc != 0:
            return rc
        out.append((lib.whisper_full_get_segment_t0(ctx, i), lib.whisper_full_get_segment_t1(ctx, i), _rec(o)))
    return out


def _token_records(lib, ctx):
    out = []
    for i in range(lib.whisper_full_n_segments(ctx)):
        for j in range(lib.whisper_full_n_tokens(ctx, i)):
            o = abi.wmi_speaker()
            rc = lib.wmi_full_get_token_speaker(ctx, i, j, C.byref(o))
            t = lib.whisper_full_get_token_data(ctx, i, j)
            out.append((t.t0, t.t1, rc, _rec(o)))
    return out


def _hold(x, fmt, rate, t0, t1, got, what, ratio=sr.RATIO):
    """one record against the judge on the same times"""
    want = sr.speaker(x, rate, t0, t1, ratio)
    if fmt != sr.F32:
        assert got == want, (what, t0, t1, got, want)
        return
    assert (got["is0"], got["is1"]) == (want["is0"], want["is1"]), (what, got, want)
    m = max(want["is1"] - want["is0"], 0)
    for c in ("e0", "e1"):
        lim = sr.f32_bound(m, want[c])
        if lim > 0:
            sc.hold("speaker records f32: |dE| / (2 m 2^-53 E)", abs(got[c] - want[c]), lim, (what, t0, t1, c))
        else:
            assert got[c] == want[c], (what, got, want)
    assert sr.f32_label_safe(want, ratio), (what, want)              # (the clips are chosen so: none is skipped)
    assert got["speaker"] == want["speaker"], (what, got, want)


def _run(node, data, fmt, stereo, rate, p, conv=2):
    before = _counters(node.lib, node.ctx)
    r = node.transcribe_wav(data, fmt, stereo, rate, interpolator_type=conv, params=p)
    assert node.last_ret == 0, node.last_ret
    return r, node.segments(), list(_counters(node.lib, node.ctx) - before)


def test_mode_0_is_the_call_as_it_was(product_lib, model, node):
    lib = product_lib
    data = _clip(wr.S16, 1, 44100, 4.0, seed=40)
    fresh = host.SpeechToText(lib); fresh.set_language_model(model)          # wmi_set_speaker is never called on this one
    try:
        assert not fresh._speaker_called
        want = _run(fresh, data, wr.S16, 1, 44100, _params(fresh))
        assert len(want[0]) > 1 and len(want[1]) >= 1
        assert _segment_records(lib, fresh.ctx) == -2
        st = (C.c_int64 * 4)(9, 9, 9, 9)
        assert lib.wmi_speaker_stats(fresh.ctx, st) == 0 and list(st) == [0, 0, 0, 0]
    finally:
        fresh.close()
    assert lib.wmi_set_speaker(node.ctx, 1, 0.0) == 0
    assert _run(node, data, wr.S16, 1, 44100, _params(node)) == want
    assert lib.wmi_set_speaker(node.ctx, 0, 0.0) == 1
    assert _run(node, data, wr.S16, 1, 44100, _params(node)) == want         # back in mode 0: the same bytes ...
    assert _segment_records(lib, node.ctx) == -2                             # ... and no table
    o = abi.wmi_speaker()
    assert lib.wmi_full_get_token_speaker(node.ctx, 0, 0, C.byref(o)) == -2
    assert lib.wmi_full_get_segment_speaker(node.ctx, 99, C.byref(o)) == -1 and lib.wmi_full_get_segment_speaker(node.ctx, 0, None) == -1


@pytest.mark.parametrize("fmt,rate,conv", [(wr.S16, 44100, 2), (wr.S8, 22050, 4), (wr.F32, 16000, 2)], ids=["s16-44100", "s8-22050", "f32-16000"])
def test_modes_1_and_2_change_nothing_and_equal_the_judge(product_lib, node, fmt, rate, conv):
    lib, ctx = product_lib, node.ctx
    data = _clip(fmt, 1, rate, 4.0, seed=40)
    x = sr.channels(data, fmt)
    base = _run(node, data, fmt, 1, rate, _params(node), conv)
    assert len(base[1]) >= 1
    for mode in (1, 2):
        assert lib.wmi_set_speaker(ctx, mode, 0.0) == mode - 1
        assert _run(node, data, fmt, 1, rate, _params(node), conv) == base, mode
        segs = _segment_records(lib, ctx)
        assert isinstance(segs, list) and len(segs) == len(base[1]) >= 1
        for t0, t1, got in segs:
            _hold(x, fmt, rate, t0, t1, got, (fmt, rate, mode, "segment"))
        toks = _token_records(lib, ctx)
        if mode == 1:
            assert toks and all(rc == -2 for _, _, rc, _ in toks)
            continue
        timed = [(t0, t1, got) for t0, t1, rc, got in toks if rc == 0]
        assert len(timed) >= 1 and all(rc in (0, -2) for _, _, rc, _ in toks)
        assert all((rc == 0) == (t0 >= 0 and t1 >= 0) for t0, t1, rc, _ in toks)
        for t0, t1, got in timed:
            _hold(x, fmt, rate, t0, t1, got, (fmt, rate, mode, "token"))
    st = (C.c_int64 * 4)()
    assert lib.wmi_speaker_stats(ctx, st) == 0
    nb = sr.n_bins(x.shape[0], rate)
    assert list(st) == [1, nb, 16 * (nb + 1), 1]
    # mode 2 without token timestamps: segments as before, no token record
    _run(node, data, fmt, 1, rate, _params(node, False), conv)
    assert all(rc == -2 for _, _, rc, _ in _token_records(lib, ctx)) and isinstance(_segment_records(lib, ctx), list)
    # another ratio: the same energies, the judge's label under it
    assert lib.wmi_set_speaker(ctx, 1, 4.0) == 2
    _run(node, data, fmt, 1, rate, _params(node), conv)
    for t0, t1, got in _segment_records(lib, ctx):
        _hold(x, fmt, rate, t0, t1, got, (fmt, rate, "ratio 4"), ratio=4.0)
    # a transcription call of another family drops the table
    node.transcribe(synth.make_pcm(2.0, seed=1), params=_params(node))
    assert _segment_records(lib, ctx) in (-2, [])


def test_a_mono_clip_in_mode_1_is_what_it_was(product_lib, node):
    data = _clip(wr.S16, 0, 48000, 3.0, seed=9)
    base = _run(node, data, wr.S16, 0, 48000, _params(node))
    assert len(base[1]) >= 1
    assert product_lib.wmi_set_speaker(node.ctx, 1, 0.0) == 0
    assert _run(node, data, wr.S16, 0, 48000, _params(node)) == base
    assert _segment_records(product_lib, node.ctx) == -2
    st = (C.c_int64 * 4)()
    assert product_lib.wmi_speaker_stats(node.ctx, st) == 0 and list(st) == [0, 0, 0, 0]


def test_a_device_resident_clip(product_lib, node):
    lib, ctx = product_lib, node.ctx
    hip = C.CDLL("libamdhip64.so")
    data = _clip(wr.S16, 1, 44100, 3.0, seed=12)
    x = sr.channels(data, wr.S16)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(len(data) + 64)) == 0
    try:
        src = C.c_void_p(d.value + 2 * 3)                                        # three samples in: off the frame grid
        assert hip.hipMemcpy(src, data, C.c_size_t(len(data)), 1) == 0
        w = abi.wmi_wav(src, len(data), wr.S16, 1, 44100, 1)
        assert lib.wmi_set_speaker(ctx, 2, 0.0) == 0
        assert lib.wmi_full_wav(ctx, _params(node), C.byref(w), 2) == 0
        segs = _segment_records(lib, ctx)
        assert isinstance(segs, list) and len(segs) >= 1
        for t0, t1, got in segs:
            _hold(x, wr.S16, 44100, t0, t1, got, "device clip")
        st = (C.c_int64 * 5)()
        assert lib.wmi_wav_stats(ctx, st) == 0 and st[0] == 0                    # nothing was uploaded
    finally:
        hip.hipFree(d)


def test_long_form_merged_view_and_a_selected_piece(product_lib, node):
    import segment_f64 as sj
    lib, ctx = product_lib, node.ctx
    parts = [1.5, -0.8, 2.0, -2.5, 4.0, -1.0, 1.2]
    x16 = np.concatenate([synth.make_pcm(s, seed=900 + i) if s > 0 else np.zeros(int(round(-s * SR)), np.float32) for i, s in enumerate(parts)])
    x48 = np.repeat(x16, 3)                                                      # zeros stay zeros: the silences survive the format
    loud = (np.arange(x48.size) // (3 * 48000)) % 2                              # the louder channel changes every three seconds
    data = wr.pack(np.stack([np.where(loud == 0, 1.0, 0.2) * x48, np.where(loud == 0, 0.2, 1.0) * x48], axis=1).reshape(-1).astype(np.float32), wr.S16)
    x = sr.channels(data, wr.S16)
    lp = sj.params(max_piece_ms=5000)

    def run():
        before = _counters(lib, ctx)
        merged = node.transcribe_wav_long(data, wr.S16, 1, 48000, 2, _params(node), lp)
        assert node.last_ret == 0
        return merged, list(node.last_pieces), list(node.last_segments), list(_counters(lib, ctx) - before)
    base = run()
    assert len(base[1]) >= 2 and len(base[2]) >= 2
    assert _segment_records(lib, ctx) == -2
    assert lib.wmi_set_speaker(ctx, 2, 0.0) == 0
    assert run() == base
    merged = _segment_records(lib, ctx)
    assert isinstance(merged, list) and len(merged) == len(base[2])
    for t0, t1, got in merged:
        _hold(x, wr.S16, 48000, t0, t1, got, "merged")
    for t0, t1, rc, got in _token_records(lib, ctx):
        if rc == 0:
            _hold(x, wr.S16, 48000, t0, t1, got, "merged token")
    # a piece shows the records of its segments in the merged view
    pieces = base[1]
    i = max(range(len(pieces)), key=lambda k: pieces[k]["n_segments"])
    assert pieces[i]["n_segments"] >= 1
    assert lib.wmi_long_select(ctx, i) == pieces[i]["n_segments"]
    own = _segment_records(lib, ctx)
    assert [r for _, _, r in own] == [r for _, _, r in merged[pieces[i]["i_segment"]:pieces[i]["i_segment"] + pieces[i]["n_segments"]]]
    assert lib.wmi_long_select(ctx, -1) == len(merged)
    assert _segment_records(lib, ctx) == merged


def test_batch_of_four_clips_a_table_per_stereo_clip(product_lib):
    lib = product_lib
    node = host.SpeechToText(lib); node.set_language_model(synth.make_model("micro", seed=77)); node.language = "auto"
    try:
        ctx = node.ctx
        specs = [(wr.S16, 1, 48000, 3.0, 11, (1.0, 0.3)), (wr.S16, 0, 22050, 2.5, 12, (1.0, 1.0)), (wr.S8, 1, 44100, 3.0, 13, (0.3, 1.0)),
                 (wr.F32, 1, 16000, 3.5, 14, (1.0, 0.25))]
        clips = [(_clip(f, st, r, sec, seed, g), f, st, r) for f, st, r, sec, seed, g in specs]

        def run():
            before = _counters(lib, ctx)
            r = node.transcribe_wav_batch(clips, params=_params(node))
            assert node.last_ret == 0
            segs = []
            for c in range(len(clips)):
                assert lib.wmi_batch_select(ctx, c) >= 0
                segs.append(node.segments())
            return r, segs, list(node.last_modes), list(node.last_langs), list(_counters(lib, ctx) - before)
        base = run()
        assert all(len(s) >= 1 for s in base[1])
        assert lib.wmi_set_speaker(ctx, 2, 0.0) == 0
        assert run() == base
        for c, (data, fmt, st, rate) in enumerate(clips):
            assert lib.wmi_batch_select(ctx, c) == len(base[1][c])
            segs = _segment_records(lib, ctx)
            if not st:
                assert segs == -2                                                # the mono clip carries no table
                continue
            assert isinstance(segs, list) and len(segs) == len(base[1][c])
            x = sr.channels(data, fmt)
            for t0, t1, got in segs:
                _hold(x, fmt, rate, t0, t1, got, ("batch", c))
            for t0, t1, rc, got in _token_records(lib, ctx):
                if rc == 0:
                    _hold(x, fmt, rate, t0, t1, got, ("batch token", c))
        st4 = (C.c_int64 * 4)()
        assert lib.wmi_speaker_stats(ctx, st4) == 0 and st4[0] == 3 and st4[3] == 3
        # the plain lock-step call on caller-made mono carries none
        node.transcribe_batch([wr.convert(d, f, s, r, 2) for d, f, s, r in clips[:2]], params=_params(node))
        assert lib.wmi_batch_select(ctx, 0) >= 0 and _segment_records(lib, ctx) in (-2, [])
    finally:
        node.close()


def test_capture_session_after_two_pushes_and_a_keep_last(product_lib, node):
    lib, ctx = product_lib, node.ctx
    rate = 44100
    pcm = synth.make_pcm(4.0, seed=21)
    t = np.arange(int(4.0 * rate)) * (SR / rate)
    mono = np.interp(t, np.arange(pcm.size), pcm).astype(np.float32)
    fr = np.stack([mono, (0.25 * mono).astype(np.float32)], axis=1)

    def step(sess):
        n, _ = sess.resample()
        p = node.full_params("", int(n / SR * 1500 / 30 + 128))
        before = _counters(lib, ctx)
        assert sess.full(p) == 0
        return node.collect(), node.segments(), list(_counters(lib, ctx) - before)
    with host.CaptureSession(node, rate, 2) as sess:
        sess.push(fr[:rate]); sess.push(fr[rate:])
        keep = int(3.2 * rate)
        assert sess.keep_last(keep) == keep
        base = step(sess)
        assert len(base[1]) >= 1 and _segment_records(lib, ctx) == -2
        assert lib.wmi_set_speaker(ctx, 2, 0.0) == 0
        assert step(sess) == base
        segs = _segment_records(lib, ctx)
        held = np.ascontiguousarray(fr[-keep:])                                  # the accumulation the session holds: f32 stereo at the mix rate
        assert isinstance(segs, list) and len(segs) == len(base[1])
        for t0, t1, got in segs:
            _hold(held, sr.F32, rate, t0, t1, got, "capture")
        timed = [(t0, t1, got) for t0, t1, rc, got in _token_records(lib, ctx) if rc == 0]
        assert timed
        for t0, t1, got in timed:
            _hold(held, sr.F32, rate, t0, t1, got, "capture token")
        st4 = (C.c_int64 * 4)()
        assert lib.wmi_speaker_stats(ctx, st4) == 0 and list(st4)[0::3] == [1, 1]

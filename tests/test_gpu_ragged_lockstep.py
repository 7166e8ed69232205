"""-m gpu: lock-step chunks with an encoder length each (include/wmi_device.h wmi_full_batch_ctx) and the capture sessions of one
context transcribed together (wmi_capture_full_batch).

Every chunk must be what whisper_full with params.audio_ctx = its own length returns for it on a fresh context — bit for bit in the
exact mode (wmi_set_lockstep_exact: the rows' kernels are the one-chunk path's), up to the first near-tie in the default mode (MFMA
rows, tests/test_gpu_parity.py _assert_same_transcription) — while all of them stay rows of the same launches: every call below asserts
that no chunk left lock-step (last_modes all 0); a chunk quietly run alone would pass everything else."""
import ctypes as C

import numpy as np
import pytest

from godot_whisper_amd import host, runtime, synth
from test_gpu_parity import _assert_same_transcription

pytestmark = pytest.mark.gpu

SR = 16000
CTX8 = [0, 428, 278, 129, 64, 1500, 50, 777]
SECS8 = [30, 6, 3, 2.5, 1.2, 30, 1.0, 13]


@pytest.fixture(params=["mfma", "exact"])
def lockstep_mode(request, product_lib):
    product_lib.wmi_set_lockstep_exact(1 if request.param == "exact" else 0)
    yield request.param
    product_lib.wmi_set_lockstep_exact(0)


@pytest.fixture
def exact(product_lib):
    product_lib.wmi_set_lockstep_exact(1)
    yield
    product_lib.wmi_set_lockstep_exact(0)


def _params(node):
    p = node.full_params("", 0); p.temperature_inc = 0.0          # no fallback: no chunk may leave lock-step
    return p


def _pcms8():
    return [synth.make_pcm(s, seed=700 + i, gate=(i % 3 == 1)) for i, s in enumerate(SECS8)]


def _one_at_a_time(product_lib, model, pcms, ctxs):
    """whisper_full per chunk with its own audio_ctx, each on a fresh context"""
    want = []
    for b, a in zip(pcms, ctxs):
        node = host.SpeechToText(product_lib); node.set_language_model(model)
        p = _params(node); p.audio_ctx = int(a)
        want.append(node.transcribe(b, params=p))
        assert node.last_ret == 0
        node.close()
    return want


def _batch_equals_one_at_a_time(product_lib, model, pcms, ctxs, strict, what):
    want = _one_at_a_time(product_lib, model, pcms, ctxs)
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    try:
        got = node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and len(got) == len(pcms)
        assert list(node.last_modes) == [0] * len(pcms), node.last_modes
        for c, (g, w) in enumerate(zip(got, want)):
            _assert_same_transcription(g, w, (what, c, ctxs[c]), strict)
        return got
    finally:
        node.close()


def test_per_chunk_lengths_equal_whisper_full_per_chunk(product_lib, lockstep_mode):
    """Lengths that are no multiple of 16 (129, 278, 777), of one key tile and below (64, 50), with 1 / 2 / 3 / 5 / 8 key slices of the
    cross-attention in one launch (50, 278, 428, 777, 1500), the model's default beside an explicit 1500, a row period far above a row's
    own length."""
    model = synth.make_model("micro.en", seed=2024)
    got = _batch_equals_one_at_a_time(product_lib, model, _pcms8(), CTX8, lockstep_mode == "exact", "eight lengths")
    assert len(got[0]) > 1 and len(got[5]) > 1


def test_default_length_and_explicit_full_length_agree(product_lib, exact):
    model = synth.make_model("micro.en", seed=2024)
    pcm = synth.make_pcm(30, seed=700)
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    try:
        got = node.transcribe_batch([pcm, pcm, pcm], params=_params(node), audio_ctxs=[0, 1500, 428])
        assert node.last_ret == 0 and list(node.last_modes) == [0, 0, 0]
        assert got[0] == got[1] and len(got[0]) > 1
    finally:
        node.close()


def test_audio_longer_than_its_window(product_lib, lockstep_mode):
    """11 s of audio against 2.58 s and 5.56 s of encoder context (129, 278) beside a chunk at the model's full length: the seek windows
    of the three rows are whatever whisper_full walks for each."""
    model = synth.make_model("micro.en", seed=2024)
    pcms = [synth.make_pcm(11.0, seed=720 + i) for i in range(3)]
    _batch_equals_one_at_a_time(product_lib, model, pcms, [129, 278, 0], lockstep_mode == "exact", "several windows")


def test_uniform_array_is_the_old_call(product_lib, lockstep_mode):
    model = synth.make_model("micro.en", seed=5)
    pcms = [synth.make_pcm(6.0, seed=40 + i) for i in range(3)]
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    try:
        p = _params(node); p.audio_ctx = 428
        old = node.transcribe_batch(pcms, params=p)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * 3
        new = node.transcribe_batch(pcms, params=_params(node), audio_ctxs=[428] * 3)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * 3
        assert new == old
        none = node.transcribe_batch(pcms, params=p, audio_ctxs=None)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * 3
        assert none == old
        rows, period, row_T = C.c_int(0), C.c_int(0), (C.c_int * 16)()
        assert product_lib.wmi_batch_enc_dims(node.ctx, C.byref(rows), C.byref(period), row_T) == 0
        assert rows.value >= 1 and period.value == 428 and list(row_T[:rows.value]) == [428] * rows.value     # the common T for a uniform call
    finally:
        node.close()


def test_order_and_grouping_do_not_matter_in_exact_mode(product_lib, exact):
    model = synth.make_model("micro.en", seed=2024)
    rng = np.random.default_rng(18)
    more = [int(x) for x in rng.choice([200, 333, 600, 901, 1200], size=10)]
    ctxs = CTX8 + more
    pcms = _pcms8() + [synth.make_pcm(2.0 + 0.4 * i, seed=740 + i) for i in range(10)]        # <= 5.6 s
    n = len(pcms)
    assert n == 18
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    try:
        product_lib.wmi_set_lockstep_groups(node.ctx, 1)
        given = node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * n
        rev = node.transcribe_batch(pcms[::-1], params=_params(node), audio_ctxs=ctxs[::-1])
        assert node.last_ret == 0 and list(node.last_modes) == [0] * n
        product_lib.wmi_set_lockstep_groups(node.ctx, 2)
        grouped = node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * n
        product_lib.wmi_set_lockstep_groups(node.ctx, 1)
        for c in range(n):
            assert rev[n - 1 - c] == given[c], ("reversed", c, ctxs[c])
            assert grouped[c] == given[c], ("two groups", c, ctxs[c])
            alone = node.transcribe_batch([pcms[c]], params=_params(node), audio_ctxs=[ctxs[c]])
            assert node.last_ret == 0 and list(node.last_modes) == [0]
            assert alone[0] == given[c], ("alone", c, ctxs[c])
    finally:
        product_lib.wmi_set_lockstep_groups(node.ctx, 0)
        node.close()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_stage_values_of_a_ragged_pass(product_lib, exact):
    """Row r of the stacked encoder pass holds, in its first T_r rows, the one-chunk encoder's values at audio_ctx = T_r, bit for bit."""
    model = synth.make_model("micro.en", seed=2024)
    ctxs = [278, 129, 428, 64]
    pcms = [synth.make_pcm(min(T / 50.0, 5.0) - 0.1, seed=760 + i) for i, T in enumerate(ctxs)]     # one window each, no longer than it
    lib = product_lib
    node = host.SpeechToText(lib); node.set_language_model(model)
    one = host.SpeechToText(lib); one.set_language_model(model)
    try:
        node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * 4
        rows, period, row_T = C.c_int(0), C.c_int(0), (C.c_int * 16)()
        assert lib.wmi_batch_enc_dims(node.ctx, C.byref(rows), C.byref(period), row_T) == 0
        R, P = rows.value, period.value
        assert R == 4 and P % 16 == 0 and P >= 428, (R, P)
        lens = list(row_T[:R])
        assert sorted(lens) == sorted(ctxs), lens                     # (the call orders its chunks by length)
        S = lib.whisper_model_n_audio_state(node.ctx); Lt = lib.whisper_model_n_text_layer(node.ctx)
        bx = runtime.get_tensor(lib, node.ctx, "batch_enc_x").reshape(R, P, S)
        bk = runtime.get_tensor(lib, node.ctx, "batch_cross_k").reshape(Lt, R, P, S)
        bv = runtime.get_tensor(lib, node.ctx, "batch_cross_v").reshape(Lt, R, P, S)      # [layer][ctx][state], as "cross_v"
        for r, T in enumerate(lens):
            pcm = pcms[ctxs.index(T)]
            assert lib.wmi_set_audio_ctx(one.ctx, T) == 0
            assert lib.whisper_pcm_to_mel(one.ctx, _fp(pcm), pcm.size, 1) == 0 and lib.whisper_encode(one.ctx, 0, 1) == 0
            x = runtime.get_tensor(lib, one.ctx, "enc_x").reshape(T, S)
            k = runtime.get_tensor(lib, one.ctx, "cross_k").reshape(Lt, T, S)
            v = runtime.get_tensor(lib, one.ctx, "cross_v").reshape(Lt, T, S)
            assert bx[r, :T].tobytes() == x.tobytes(), ("enc_x", r, T)
            assert bk[:, r, :T].tobytes() == k.tobytes(), ("cross_k", r, T)
            assert bv[:, r, :T].tobytes() == v.tobytes(), ("cross_v", r, T)
    finally:
        node.close(); one.close()


def test_ragged_batch_equals_the_compiled_reference(product_lib, checker_lib):
    if checker_lib is None:
        pytest.skip("needs the compiled reference")
    model = synth.make_model("micro.en", seed=1234)
    secs = [6.0 + 1.5 * i for i in range(5)]
    pcms = [synth.make_pcm(s, seed=500 + i) for i, s in enumerate(secs)]
    ctxs = [int(s * 50 + 128) for s in secs]
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    ref = host.SpeechToText(checker_lib); ref.set_language_model(model)
    try:
        got = node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and len(got) == 5 and list(node.last_modes) == [0] * 5
        for c, b in enumerate(pcms):
            pr = _params(ref); pr.audio_ctx = ctxs[c]
            want = ref.transcribe(b, params=pr)
            assert ref.last_ret == 0
            _assert_same_transcription(got[c], want, ("ragged batch vs reference", c, ctxs[c]), False, ref_last_t1=True)
    finally:
        node.close(); ref.close()


def test_block_quantised_model(product_lib, lockstep_mode):
    model = synth.quantize_model(synth.make_model("micro.en", seed=77), "q5_1")
    ctxs = [0, 278, 278, 129]
    pcms = [synth.make_pcm(s, seed=780 + i, gate=(i % 3 == 2)) for i, s in enumerate([30.0, 5.0, 4.0, 2.5])]
    _batch_equals_one_at_a_time(product_lib, model, pcms, ctxs, lockstep_mode == "exact", "q5_1")


# ------------------------------------------------------------------------------------------------ capture sessions
def _speech_frames(seconds, rate, seed):
    """as tests/test_gpu_capture_session.py builds its own: the synthetic speech carried to the mix rate, two slightly different channels"""
    pcm = synth.make_pcm(seconds, seed=seed)
    t = np.arange(int(seconds * rate)) * (SR / rate)
    mono = np.interp(t, np.arange(pcm.size), pcm).astype(np.float32)
    return np.stack([mono, (0.8 * mono).astype(np.float32)], axis=1)


@pytest.fixture
def stream_node(product_lib):
    n = host.CaptureStreamToText(product_lib); n.set_language_model(synth.make_model("micro.en", seed=1))
    yield n
    n.close()


def test_capture_sessions_in_lockstep(product_lib, stream_node, lockstep_mode):
    node = stream_node
    rates, secs = [48000, 44100, 16000], [2.0, 4.1, 6.3]
    sessions = [host.CaptureSession(node, r, 2) for r in rates]
    try:
        ctxs, want = [], []
        for i, (s, r, t) in enumerate(zip(sessions, rates, secs)):
            s.push(_speech_frames(t, r, seed=800 + i))
            n, _ = s.resample()
            assert n > 0
            ctxs.append(min(int(n / SR * 1500 / 30 + 128), 1500))
        p = node.full_params("", 0); p.temperature_inc = 0.0
        for s, a in zip(sessions, ctxs):
            pi = node.full_params("", a); pi.temperature_inc = 0.0
            assert s.full(pi) == 0
            want.append(node.collect())
        before = [s.stats() for s in sessions]
        assert host.CaptureSession.full_batch(sessions, p, ctxs) == 0
        got = node.collect_batch(3)
        assert list(node.last_modes) == [0, 0, 0]
        assert [s.stats() for s in sessions] == before                 # nothing uploaded, nothing resampled again: the PCM was there
        for c, (g, w) in enumerate(zip(got, want)):
            assert len(w) > 1
            _assert_same_transcription(g, w, ("sessions", c, ctxs[c]), lockstep_mode == "exact")
    finally:
        for s in sessions:
            s.close()


def test_stream_capture_many_equals_stream_capture_per_speaker(product_lib, stream_node, exact):
    node = stream_node
    rates = [48000, 44100, 16000]
    frames = [_speech_frames(8.0, r, seed=820 + i) for i, r in enumerate(rates)]
    calls = 6
    # the temperature fallback off in both loops: a session that asked for it would be run alone through whisper_full and equal
    # stream_capture's call trivially — with it off every session of every pass must have been a lock-step row
    want = [list(node.stream_capture(f, r, max_calls=calls, temperature_inc=0.0)) for f, r in zip(frames, rates)]
    got = [[], [], []]
    for t in node.stream_capture_many(frames, rates, max_calls=calls, temperature_inc=0.0):
        got[t[0]].append(t[1:])
    assert node.pass_modes == [[0, 0, 0]] * calls, node.pass_modes
    for i in range(3):
        assert len(got[i]) == len(want[i]) == calls, (i, len(got[i]), len(want[i]))
        for j, (g, w) in enumerate(zip(got[i], want[i])):
            # (finish, text, size, audio_ctx, tokens, no_activity): the tokens as the strict comparison of the lock-step tests holds them
            assert (g[0], g[1], g[2], g[3], g[5]) == (w[0], w[1], w[2], w[3], w[5]), (i, j, g[:4], w[:4])
            _assert_same_transcription([g[1].encode()] + g[4], [w[1].encode()] + w[4], ("speaker", i, "call", j), True)


def test_argument_errors(product_lib, stream_node):
    node = stream_node
    other = host.CaptureStreamToText(product_lib); other.set_language_model(synth.make_model("micro.en", seed=1))
    lib = product_lib
    pcm = synth.make_pcm(2.0, seed=1)
    p = node.full_params("", 0)

    def steps():
        t4, n = (C.c_int64 * 4)(), C.c_int32(0)
        lib.wmi_get_batch_timings(node.ctx, t4, C.byref(n))
        return n.value
    try:
        assert node.transcribe_batch([pcm, pcm], params=p, audio_ctxs=[0, 64]) and node.last_ret == 0
        base = steps()
        assert base > 0
        assert node.transcribe_batch([pcm, pcm], params=p, audio_ctxs=[0, 1501]) == [] and node.last_ret == -5
        assert node.transcribe_batch([pcm, pcm], params=p, audio_ctxs=[-1, 64]) == [] and node.last_ret == -1
        assert steps() == base                                         # the refused calls ran nothing (the counters are the last real call's)
        with host.CaptureSession(node, 44100, 2) as a, host.CaptureSession(other, 44100, 2) as b, host.CaptureSession(node, 16000, 2) as e:
            fr = _speech_frames(1.5, 44100, seed=3)
            a.push(fr); b.push(fr)
            assert host.CaptureSession.full_batch([a, b], p, [200, 200]) == -1          # sessions of two contexts
            assert host.CaptureSession.full_batch([a, e], p, [200, 200]) == -3          # an empty session
            assert host.CaptureSession.full_batch([a, e], p, None) == -3
            assert lib.wmi_capture_full_batch((C.c_void_p * 1)(a.cap), 0, p, None) == -1
            assert lib.wmi_capture_full_batch((C.c_void_p * 2)(a.cap, None), 2, p, None) == -1
            assert host.CaptureSession.full_batch([a], p, [1501]) == -5
            assert host.CaptureSession.full_batch([a], p, [-1]) == -1
            assert steps() == base
            assert host.CaptureSession.full_batch([a], p, [203]) == 0 and node.collect_batch(1)[0]
    finally:
        other.close()

"""-m gpu: lock-step chunks with an encoder length each on BLOCK-QUANTISED models (include/wmi_device.h wmi_full_batch_ctx).

The chunks of such a call are stacked in one encoder pass with a common row period, as on f16 models, and every projection of the pass
runs in the form — block-dot kernel or f16 MFMA — that the chunk's own one-chunk pass takes (the two do not give the same bits and the
stacked row count would pick another); the call is cut only where the lengths cross that threshold (256 rows).  Every chunk must be what
whisper_full with params.audio_ctx = its own length returns for it on a fresh context: bit for bit in the exact mode
(wmi_set_lockstep_exact), up to the first near-tie in the default mode (the encoder attention's key split follows the grid;
tests/test_gpu_parity.py _assert_same_transcription) — while all of them stay rows of the same launches (last_modes all 0)."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
from godot_whisper_amd import host, runtime, synth
from test_gpu_parity import _assert_same_transcription

pytestmark = pytest.mark.gpu

SR = 16000
_cache = {}


def _model(shape, qtype, seed=77):
    key = (shape, qtype, seed)
    if key not in _cache:
        _cache[key] = synth.quantize_model(synth.make_model(shape, seed=seed), qtype)
    return _cache[key]


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


def _params(node, language=None):
    p = node.full_params("", 0); p.temperature_inc = 0.0          # no fallback: no chunk may leave lock-step
    if language is not None:
        node._lang_keep = language
        p.language = language
    return p


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dims(lib, ctx):
    rows, period, row_T = C.c_int(0), C.c_int(0), (C.c_int * 16)()
    assert lib.wmi_batch_enc_dims(ctx, C.byref(rows), C.byref(period), row_T) == 0
    return rows.value, period.value, list(row_T[:rows.value])


def _one_at_a_time(lib, model, pcms, ctxs, language=None):
    """whisper_full per chunk with its own audio_ctx, each on a fresh context"""
    want = []
    for b, a in zip(pcms, ctxs):
        node = host.SpeechToText(lib); node.set_language_model(model)
        p = _params(node, language); p.audio_ctx = int(a)
        want.append(node.transcribe(b, params=p))
        assert node.last_ret == 0
        node.close()
    return want


def _batch_equals_one_at_a_time(lib, model, pcms, ctxs, strict, what):
    want = _one_at_a_time(lib, model, pcms, ctxs)
    node = host.SpeechToText(lib); node.set_language_model(model)
    try:
        got = node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and len(got) == len(pcms)
        assert list(node.last_modes) == [0] * len(pcms), node.last_modes
        for c, (g, w) in enumerate(zip(got, want)):                  # (the caller's order: chunk c against ITS length and PCM)
            _assert_same_transcription(g, w, (what, c, ctxs[c]), strict)
        return got, _dims(lib, node.ctx)
    finally:
        node.close()


# ------------------------------------------------------------------------------------------------ 1. one stacked pass
def test_lengths_above_the_threshold_are_one_stacked_pass(product_lib):
    lib = product_lib
    model = _model("micro.en", "q5_1")
    ctxs = [0, 428, 278, 777]
    pcms = [synth.make_pcm(s, seed=900 + i) for i, s in enumerate([30.0, 6.0, 3.0, 13.0])]
    node = host.SpeechToText(lib); node.set_language_model(model)
    try:
        got = node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * 4
        assert len(got[0]) > 1
        rows, period, row_T = _dims(lib, node.ctx)
        assert rows == 4, (rows, period, row_T)                      # (set by set, the last pass would hold one chunk)
        assert period % 16 == 0 and period >= 1500, period
        assert sorted(row_T) == [278, 428, 777, 1500], row_T
    finally:
        node.close()


# ------------------------------------------------------------------------------------------------ 2. equals whisper_full per chunk
CTX6 = [0, 777, 428, 278, 256, 1500]
SECS6 = [30, 13, 6, 3, 2.5, 30]


@pytest.mark.parametrize("qtype", ["q5_1", "q8_0", "q4_0"])
def test_per_chunk_lengths_equal_whisper_full_per_chunk(product_lib, lockstep_mode, qtype):
    """Lengths that are no multiple of 16 (777, 278), exactly the threshold (256: the f16 form in its own pass), the model's default beside
    an explicit 1500; q5_1 (d, m and a fifth bit), q8_0 (f16 d on the activation side), q4_0 (offset-binary nibbles)."""
    model = _model("micro.en", qtype)
    pcms = [synth.make_pcm(s, seed=910 + i, gate=(i % 3 == 1)) for i, s in enumerate(SECS6)]
    got, (rows, period, row_T) = _batch_equals_one_at_a_time(product_lib, model, pcms, CTX6, lockstep_mode == "exact", qtype)
    assert len(got[0]) > 1 and len(got[5]) > 1
    want_rows = sorted(a or 1500 for a in CTX6)
    if lockstep_mode == "exact":                                     # (8 rows per group in the exact mode: all six in one)
        assert rows == 6 and sorted(row_T) == want_rows, (rows, row_T)
    assert period % 16 == 0 and period >= max(row_T)


# ------------------------------------------------------------------------------------------------ 3. the short side, and straddling
def test_short_lengths_keep_the_block_dot_form_in_a_stack(product_lib, lockstep_mode):
    """129 + 64 + 50 + 200 rows, every chunk below the threshold, stack to 4 x 208 = 832 rows: by its row count the launch would take the f16
    form, and no chunk would equal its own whisper_full any more."""
    model = _model("micro.en", "q5_1")
    ctxs = [129, 64, 50, 200]
    pcms = [synth.make_pcm(s, seed=930 + i) for i, s in enumerate([2.5, 1.3, 1.2, 3.9])]       # (each above 1 s: below it a chunk has no window)
    got, (rows, period, row_T) = _batch_equals_one_at_a_time(product_lib, model, pcms, ctxs, lockstep_mode == "exact", "short side")
    assert rows == 4 and period == 208 and sorted(row_T) == [50, 64, 129, 200], (rows, period, row_T)
    assert len(got[3]) > 1


def test_lengths_on_both_sides_make_two_sets(product_lib, lockstep_mode):
    model = _model("micro.en", "q5_1")
    ctxs = [428, 129, 278, 64]
    pcms = [synth.make_pcm(s, seed=940 + i) for i, s in enumerate([6.0, 2.5, 3.0, 1.2])]
    got, (rows, period, row_T) = _batch_equals_one_at_a_time(product_lib, model, pcms, ctxs, lockstep_mode == "exact", "both sides")
    assert rows == 2 and period == 144 and row_T == [129, 64], (rows, period, row_T)      # the last pass: the short set
    assert len(got[0]) > 1


# ------------------------------------------------------------------------------------------------ 4. stage values
def test_stage_values_of_a_ragged_quantised_pass(product_lib, exact):
    """Row r of the stacked pass holds, in its first T_r rows, the one-chunk encoder's values at audio_ctx = T_r, bit for bit: the residual
    stream behind the last layer and the cross K / V of every decoder layer."""
    lib = product_lib
    model = _model("micro.en", "q5_1")
    ctxs = [777, 428, 278, 256]
    pcms = [synth.make_pcm(min(T / 50.0, 5.0) - 0.1, seed=960 + i) for i, T in enumerate(ctxs)]      # one window each, no longer than it
    node = host.SpeechToText(lib); node.set_language_model(model)
    one = host.SpeechToText(lib); one.set_language_model(model)
    try:
        node.transcribe_batch(pcms, params=_params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * 4
        R, P, lens = _dims(lib, node.ctx)
        assert R == 4 and P == 784 and lens == ctxs, (R, P, lens)
        S = lib.whisper_model_n_audio_state(node.ctx); Lt = lib.whisper_model_n_text_layer(node.ctx)
        bx = runtime.get_tensor(lib, node.ctx, "batch_enc_x").reshape(R, P, S)
        bk = runtime.get_tensor(lib, node.ctx, "batch_cross_k").reshape(Lt, R, P, S)
        bv = runtime.get_tensor(lib, node.ctx, "batch_cross_v").reshape(Lt, R, P, S)
        assert np.isfinite(bx).all() and np.isfinite(bk).all() and np.isfinite(bv).all()      # the rows behind a chunk's length too
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


# ------------------------------------------------------------------------------------------------ 5. the widest shape
def test_widest_shape(product_lib, exact):
    """S = 1280, 20 heads, 128 mel bands: three 512-column chunks per row in the rows kernels, K = 5120 in mlp.2."""
    model = _model("v3-slice", "q5_1", seed=31)
    ctxs = [428, 278, 300]
    pcms = [synth.make_pcm(s, seed=970 + i) for i, s in enumerate([6.0, 3.0, 4.5])]
    got, (rows, period, row_T) = _batch_equals_one_at_a_time(product_lib, model, pcms, ctxs, True, "v3-slice q5_1")
    assert rows == 3 and period == 432 and row_T == [428, 300, 278], (rows, period, row_T)
    assert len(got[0]) > 1


# ------------------------------------------------------------------------------------------------ 6. "auto" with lengths
def test_language_auto_with_lengths(product_lib, exact):
    """The detection runs on a uniform pass at the full audio context (as whisper_full's does, before audio_ctx takes effect); the ragged
    first window behind it is encoded again.  Ids and probabilities are whisper_full's / wmi_lang_detect's per chunk, bit for bit."""
    lib = product_lib
    model = _model("micro", "q5_1", seed=31)
    ctxs = [428, 0, 278, 777]
    pcms = [synth.make_pcm(s, seed=980 + i) for i, s in enumerate([6.0, 20.0, 3.0, 13.0])]
    want = []
    for pcm, a in zip(pcms, ctxs):
        n1 = host.SpeechToText(lib); n1.set_language_model(model)
        p = _params(n1, b"auto"); p.audio_ctx = a
        tr = n1.transcribe(pcm, params=p)
        assert n1.last_ret == 0
        lid = lib.whisper_full_lang_id(n1.ctx)
        probs = np.zeros(99 + 1, np.float32)
        assert lib.wmi_set_audio_ctx(n1.ctx, 0) == 0 and lib.wmi_lang_detect(n1.ctx, 0, _fp(probs)) == lid
        want.append((tr, lid, probs))
        n1.close()
    node = host.SpeechToText(lib); node.set_language_model(model)
    try:
        got = node.transcribe_batch(pcms, params=_params(node, b"auto"), audio_ctxs=ctxs)
        assert node.last_ret == 0 and list(node.last_modes) == [0] * 4
        assert node.last_langs == [w[1] for w in want], (node.last_langs, [w[1] for w in want])
        for c in range(4):
            probs = np.zeros(99 + 1, np.float32)
            assert lib.wmi_batch_lang_probs(node.ctx, c, _fp(probs)) == 0
            assert np.array_equal(probs.view(np.uint32), want[c][2].view(np.uint32)), (c, np.abs(probs - want[c][2]).max())
            g, w = gu.tokens_array(got[c]), gu.tokens_array(want[c][0])
            assert g.shape == w.shape and np.array_equal(g[:, 0], w[:, 0]), (c, g[:, 0], w[:, 0])
        rows, period, row_T = _dims(lib, node.ctx)
        assert rows == 4 and sorted(row_T) == [278, 428, 777, 1500], (rows, row_T)      # the ragged windows were encoded behind the detection
    finally:
        node.close()


# ------------------------------------------------------------------------------------------------ 7. capture sessions
def _speech_frames(seconds, rate, seed):
    """as tests/test_gpu_capture_session.py builds its own: the synthetic speech carried to the mix rate, two slightly different channels"""
    pcm = synth.make_pcm(seconds, seed=seed)
    t = np.arange(int(seconds * rate)) * (SR / rate)
    mono = np.interp(t, np.arange(pcm.size), pcm).astype(np.float32)
    return np.stack([mono, (0.8 * mono).astype(np.float32)], axis=1)


def test_stream_capture_many_equals_stream_capture_per_speaker(product_lib, exact):
    """Three speakers with 3 - 9 s of audio: their accumulations never have equal lengths (total_time * 50 + 128), so every pass is a
    ragged lock-step call of the quantised model — and every transcription is stream_capture's for that speaker."""
    node = host.CaptureStreamToText(product_lib); node.set_language_model(_model("micro.en", "q5_1", seed=1))
    try:
        rates, secs = [48000, 44100, 16000], [9.0, 6.0, 3.0]
        frames = [_speech_frames(t, r, seed=990 + i) for i, (r, t) in enumerate(zip(rates, secs))]
        calls = 4
        want = [list(node.stream_capture(f, r, max_calls=calls, temperature_inc=0.0)) for f, r in zip(frames, rates)]
        got = [[], [], []]
        for t in node.stream_capture_many(frames, rates, max_calls=calls, temperature_inc=0.0):
            got[t[0]].append(t[1:])
        assert node.pass_modes and all(m == [0] * len(m) for m in node.pass_modes), node.pass_modes
        for i in range(3):
            assert len(got[i]) == len(want[i]) and len(want[i]) > 0, (i, len(got[i]), len(want[i]))
            for j, (g, w) in enumerate(zip(got[i], want[i])):
                assert (g[0], g[1], g[2], g[3], g[5]) == (w[0], w[1], w[2], w[3], w[5]), (i, j, g[:4], w[:4])
                _assert_same_transcription([g[1].encode()] + g[4], [w[1].encode()] + w[4], ("speaker", i, "call", j), True)
    finally:
        node.close()


# ------------------------------------------------------------------------------------------------ 8. the epilogue hook
SENT = 0x7B7B                                                         # an f16 pattern (61 248) no projection of these operands produces


def _qkv_q(lib, qtype_id, M, S, Tpad, rpc, x, blocks, bias, out_rows):
    chunks = M // rpc if rpc else 1
    q = np.zeros((out_rows, S), np.uint16); k = np.zeros((out_rows, S), np.uint16); vt = np.zeros((chunks, S, Tpad), np.uint16)
    w = np.frombuffer(blocks, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.wmi_selftest_qkv_encoder_q(0, qtype_id, M, S, Tpad, rpc, p(x), p(w), p(bias), SENT, out_rows, p(q), p(k), p(vt))
    return rc, q, k, vt


@pytest.mark.parametrize("qtype", ["q5_1", "q8_0"])
def test_block_dot_qkv_epilogue_with_rows_per_chunk(product_lib, qtype):
    """Three chunks of 48 rows in ONE launch of the block-dot GEMM (M = 144: two 64-row tiles and a guarded one, every chunk boundary inside
    a tile, V^T of three chunks at their own images) against three launches of one chunk each: the same bytes, nothing else written."""
    lib = product_lib
    S, Tpad, rpc, n = 128, 64, 48, 3
    M = n * rpc
    rng = np.random.default_rng(4242)
    x = rng.standard_normal((M, S)).astype(np.float32)
    W = (rng.standard_normal((3 * S, S)) * 0.08).astype(np.float32)
    bias = (rng.standard_normal(3 * S) * 0.1).astype(np.float32)
    blocks = synth.quantize_blocks(W, qtype)
    qid = synth.QTYPES[qtype][0]
    out_rows = M + 5
    rc, q, k, vt = _qkv_q(lib, qid, M, S, Tpad, rpc, x, blocks, bias, out_rows)
    assert rc == 0
    assert (q[M:] == SENT).all() and (k[M:] == SENT).all()            # rows behind M: untouched
    assert (q[:M] != SENT).all() and (k[:M] != SENT).all()
    for c in range(n):
        rc1, q1, k1, vt1 = _qkv_q(lib, qid, rpc, S, Tpad, rpc, np.ascontiguousarray(x[c * rpc:(c + 1) * rpc]), blocks, bias, rpc)
        assert rc1 == 0
        assert q[c * rpc:(c + 1) * rpc].tobytes() == q1.tobytes(), ("q", c)
        assert k[c * rpc:(c + 1) * rpc].tobytes() == k1.tobytes(), ("k", c)
        assert vt[c].tobytes() == vt1[0].tobytes(), ("vt", c)
        # V^T columns: the chunk's 48 time steps (a permutation inside each group of 16), the 16 behind them untouched
        assert (vt[c][:, :rpc] != SENT).all() and (vt[c][:, rpc:] == SENT).all(), c
    # argument errors: before the device is touched
    assert _qkv_q(lib, qid, M, S, Tpad, 80, x, blocks, bias, out_rows)[0] == -1
    assert _qkv_q(lib, 5, M, S, Tpad, rpc, x, blocks, bias, out_rows)[0] == -1
    assert _qkv_q(lib, qid, M, S, Tpad, rpc, x, blocks, bias, M - 1)[0] == -1


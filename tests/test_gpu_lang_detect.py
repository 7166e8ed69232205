"""Language detection on the device: the language head (k_lang_head: the 100 language logits of the <sot> step instead of the vocabulary
projection) behind wmi_lang_detect, whisper_full with language "auto" (one encoder pass for the detection and the first window) and
wmi_full_batch with language "auto" (detection as one lock-step step, the chunks stay in lock-step).

The inputs are the six 6 s chunks below on synth.make_model("micro", seed=31); the compiled reference (whisper_lang_auto_detect) gives them
the ids in IDS with log(p1 / p2) between 0.65 and 2.27 — twenty times the project's logit bound and more, so the ids are asserted outright.
Audio alone hardly moves the pick on synthetic weights, hence the tones."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import stage_compare as sc
from godot_whisper_amd import host, synth
from test_gpu_parity import _assert_same_transcription
from test_lang_head import N_LANG, lang_codes, restate

pytestmark = pytest.mark.gpu

IDS = [71, 71, 49, 49, 49, 71]
_cache = {}


def inputs():
    if "pcm" not in _cache:
        t = np.arange(96000, dtype=np.float64) / 16000.0
        _cache["pcm"] = [
            synth.make_pcm(6.0, seed=701),
            synth.make_pcm(6.0, seed=700),
            (0.5 * np.sin(2 * np.pi * 200.0 * t)).astype(np.float32),
            (0.5 * np.sin(2 * np.pi * (100.0 * t + 300.0 * t * t))).astype(np.float32),
            (0.5 * np.sin(2 * np.pi * 3000.0 * t)).astype(np.float32),
            (np.float32(0.001) * synth.make_pcm(6.0, seed=700)).astype(np.float32),
        ]
    return [np.ascontiguousarray(x, np.float32) for x in _cache["pcm"]]


def model(kind):
    if kind not in _cache:
        if kind in ("micro", "v3-slice", "medium-slice"): _cache[kind] = synth.make_model(kind, seed=31)
        else:                    _cache[kind] = synth.quantize_model(model("micro"), kind.split("-")[1])
    return _cache[kind]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _node(lib, kind="micro"):
    node = host.SpeechToText(lib); node.set_language_model(model(kind))
    assert node.ctx
    return node


def _params(node, language=b"auto", audio_ctx=0):
    """the host's parameter set (one window, one segment, token timestamps) with the temperature fallback off"""
    p = node.full_params("", audio_ctx)
    node._lang_keep = language
    p.language = language; p.temperature_inc = 0.0
    return p


def _segments(lib, ctx):
    out = []
    for i in range(lib.whisper_full_n_segments(ctx)):
        toks = [lib.whisper_full_get_token_data(ctx, i, j) for j in range(lib.whisper_full_n_tokens(ctx, i))]
        out.append((lib.whisper_full_get_segment_t0(ctx, i), lib.whisper_full_get_segment_t1(ctx, i), bytes(lib.whisper_full_get_segment_text(ctx, i)),
                    [(t.id, t.tid, t.p, t.plog, t.pt, t.ptsum, t.t0, t.t1, t.vlen) for t in toks]))
    return out


def _n_encode(lib, ctx):
    t6 = (C.c_int64 * 6)(); n5 = (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return n5[0]


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("kind", ["micro", "medium-slice", "v3-slice", "micro-q5_1", "micro-q8_0"])      # S = 128 / 1024 / 1280: k_lang_head<1 / 2 / 3>
def test_language_head_equals_the_projection_slice_bit_for_bit(product_lib, kind):
    """wmi_lang_detect (language head) against whisper_lang_auto_detect (full vocabulary projection) and against whisper_decode's logits
    soft-maxed here: the same ids and the same 100 probabilities, bit for bit — i.e. the head's 100 logits are the projection's entries
    sot + 1 .. sot + 100 (f16 rows: k_gemv1's LayerNorm + dot products; block-quantised: k_qrows over the covering tiles + gather)."""
    lib = product_lib
    node = _node(lib, kind); ctx = node.ctx
    try:
        codes = lang_codes(lib)
        sot = lib.whisper_token_sot(ctx); nv = lib.whisper_n_vocab(ctx)
        seen = set()
        for i in (0, 2, 3):
            pcm = inputs()[i]
            if kind in ("v3-slice", "medium-slice"):
                pcm = np.ascontiguousarray(pcm[:48000])
            assert lib.whisper_pcm_to_mel(ctx, _fp(pcm), pcm.size, 1) == 0
            full = np.zeros(N_LANG, np.float32); head = np.zeros(N_LANG, np.float32)
            id_full = lib.whisper_lang_auto_detect(ctx, 0, 1, _fp(full))
            id_head = lib.wmi_lang_detect(ctx, 0, _fp(head))
            assert 0 <= id_full < N_LANG and id_head == id_full, (kind, i, id_full, id_head)
            assert np.array_equal(_bits(head), _bits(full)), (kind, i, np.abs(head - full).max())
            assert lib.wmi_lang_detect(ctx, 0, None) == id_full                                     # probabilities are optional
            # the stage calls: encoder, <sot> at position 0, the logits of the whole vocabulary
            assert lib.whisper_encode(ctx, 0, 1) == 0
            tok = (C.c_int32 * 1)(sot)
            assert lib.whisper_decode(ctx, tok, 1, 0, 1) == 0
            logits = np.ctypeslib.as_array(lib.whisper_get_logits(ctx), (nv,)).copy()
            want_id, want = restate(logits[sot + 1: sot + 1 + N_LANG], codes)
            assert want_id == id_head and np.array_equal(_bits(head), _bits(want)), (kind, i, np.abs(head - want).max())
            if kind == "micro":
                assert id_head == IDS[i], (i, id_head)
                # 51 865 entries hold 99 language tokens: the hundredth value is the token behind them (W/whisper.cpp:3603-3606 walks all 100)
                assert nv == 51865 and head[N_LANG - 1] != 0.0 and _bits(head)[N_LANG - 1] == _bits(want)[N_LANG - 1]
            seen.add(id_head)
        assert lib.wmi_lang_detect(ctx, 600000, None) == -2 and lib.wmi_lang_detect(ctx, -10, None) == -1     # whisper_lang_auto_detect's codes
        if kind == "micro":
            assert seen == {71, 49}
    finally:
        node.close()


# ------------------------------------------------------------------------------------------------ 2. whisper_full
def _full(lib, pcm, language, audio_ctx=0, offset_ms=0, cb=None, kind="micro"):
    node = _node(lib, kind); ctx = node.ctx
    try:
        p = _params(node, language, audio_ctx)
        p.offset_ms = offset_ms
        if cb is not None:
            p.encoder_begin_callback = C.cast(cb, C.c_void_p)
        n0 = _n_encode(lib, ctx)
        ret = lib.whisper_full(ctx, p, _fp(pcm), pcm.size)
        return ret, _segments(lib, ctx), lib.whisper_full_lang_id(ctx), _n_encode(lib, ctx) - n0
    finally:
        node.close()


def test_whisper_full_auto_runs_one_encoder_pass_and_gives_the_same_result(product_lib):
    """language "auto" on a fresh context == the same call with the detected language spelled out (segments, every token field, t0 / t1),
    with ONE encoder pass where the detection has encoded the first window (offset 0, same audio context) and two where it has not."""
    lib = product_lib
    for i, pcm in enumerate(inputs()):
        ret, seg, lid, n_enc = _full(lib, pcm, b"auto")
        assert ret == 0 and lid == IDS[i] and n_enc == 1, (i, ret, lid, n_enc)
        ret2, seg2, lid2, n_enc2 = _full(lib, pcm, bytes(lib.whisper_lang_str(lid)))
        assert ret2 == 0 and lid2 == lid and n_enc2 == 1
        assert seg and seg == seg2, (i, seg, seg2)
    pcm12 = synth.make_pcm(12.0, seed=701)                                 # still one 30 s window
    ret, seg, lid, n_enc = _full(lib, pcm12, b"auto")
    assert ret == 0 and n_enc == 1 and seg
    assert seg == _full(lib, pcm12, bytes(lib.whisper_lang_str(lid)))[1]
    # the detection of a fresh context runs at the full audio context (W/whisper.cpp:5102 sets the call's afterwards): nothing to reuse
    pcm = inputs()[0]
    ret, seg, lid, n_enc = _full(lib, pcm, b"auto", audio_ctx=300)
    assert ret == 0 and lid == IDS[0] and n_enc == 2, (ret, lid, n_enc)
    assert seg and seg == _full(lib, pcm, bytes(lib.whisper_lang_str(lid)), audio_ctx=300)[1]
    ret, seg, lid, n_enc = _full(lib, pcm, b"auto", offset_ms=2000)        # the detection is at 0, the first window is not
    assert ret == 0 and lid == IDS[0] and n_enc == 2, (ret, lid, n_enc)
    assert seg == _full(lib, pcm, bytes(lib.whisper_lang_str(lid)), offset_ms=2000)[1]
    # encoder_begin_callback is still asked before the (skipped) pass, and its "no" still ends the call: code 0, no segments
    calls = []
    cb = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.c_void_p)(lambda c, s, u: (calls.append(1), False)[1])
    ret, seg, lid, n_enc = _full(lib, pcm, b"auto", cb=cb)
    assert (ret, seg, lid, n_enc, len(calls)) == (0, [], IDS[0], 1, 1)
    ret2, seg2, _, n_enc2 = _full(lib, pcm, bytes(lib.whisper_lang_str(lid)), cb=cb)
    assert (ret2, seg2, n_enc2, len(calls)) == (0, [], 0, 2)


# ------------------------------------------------------------------------------------------------ 3. the compiled reference
def test_detected_language_and_probabilities_against_the_compiled_reference(product_lib, checker_lib):
    """whisper_full_lang_id equal, |d lang_probs| <= 1e-2 (the project's token-probability bound)."""
    if checker_lib is None:
        pytest.skip("needs the compiled reference")
    res = []
    for L in (product_lib, checker_lib):
        node = host.SpeechToText(L); node.set_language_model(model("micro"))
        if L is checker_lib:
            node.n_threads = 4
        out = []
        for pcm in inputs():
            p = _params(node)
            assert L.whisper_full(node.ctx, p, _fp(pcm), pcm.size) == 0
            lid = L.whisper_full_lang_id(node.ctx)
            probs = np.zeros(N_LANG, np.float32)
            got = (L.wmi_lang_detect(node.ctx, 0, _fp(probs)) if L is product_lib else L.whisper_lang_auto_detect(node.ctx, 0, 4, _fp(probs)))
            assert got == lid
            out.append((lid, probs))
        node.close()
        res.append(out)
    for i, ((lp, pp), (lr, pr)) in enumerate(zip(*res)):
        assert lp == lr == IDS[i], (i, lp, lr)
        sc.hold("language probabilities max |d|", float(np.abs(pp.astype(np.float64) - pr.astype(np.float64)).max()), 1e-2, i)


# ------------------------------------------------------------------------------------------------ 4. lock-step, exact mode
@pytest.mark.parametrize("kind", ["micro", "micro-q5_1"])
def test_lockstep_auto_exact_mode_equals_whisper_full_per_chunk(product_lib, kind):
    """wmi_full_batch with language "auto" in the exact mode: every chunk in lock-step, language ids and probabilities those of a
    fresh-context whisper_full / wmi_lang_detect on the chunk (bit for bit: the same language-head kernel, rows on grid.y), token streams
    equal, compared field by field as the exact-mode parity tests compare this shape; the chunk shorter than 1 s is detected and has no
    segments."""
    lib = product_lib
    x = inputs()
    chunks = [x[0], x[2], x[3], x[5], np.ascontiguousarray(x[0][:8000])]
    lib.wmi_set_lockstep_exact(1)                    # process-wide, before both sides: it also pins the one-chunk encoder's attention form
    node = None
    try:
        want = []
        for pcm in chunks:
            n1 = _node(lib, kind)
            tr = n1.transcribe(pcm, params=_params(n1))
            assert n1.last_ret == 0
            probs = np.zeros(N_LANG, np.float32)
            lid = lib.whisper_full_lang_id(n1.ctx)
            assert lib.wmi_lang_detect(n1.ctx, 0, _fp(probs)) == lid
            want.append((tr, lid, probs))
            n1.close()
        node = _node(lib, kind)
        got = node.transcribe_batch(chunks, params=_params(node))
        assert node.last_ret == 0 and len(got) == 5
        assert list(node.last_modes)[:4] == [0, 0, 0, 0], node.last_modes
        ids = [lib.wmi_batch_lang_id(node.ctx, c) for c in range(5)]
        assert ids == node.last_langs == [w[1] for w in want], (ids, [w[1] for w in want])
        if kind == "micro":
            assert ids[:4] == [71, 49, 49, 71], ids
        for c in range(5):
            probs = np.zeros(N_LANG, np.float32)
            assert lib.wmi_batch_lang_probs(node.ctx, c, _fp(probs)) == 0
            assert np.array_equal(_bits(probs), _bits(want[c][2])), (c, np.abs(probs - want[c][2]).max())
            assert lib.wmi_batch_select(node.ctx, c) >= 0 and lib.whisper_full_lang_id(node.ctx) == ids[c]
            # the token stream itself is equal; the other fields under the rules the exact-mode lock-step tests apply to this shape
            # (test_lockstep_chunks_equal_one_at_a_time[micro-host]: a multilingual prompt is fed as one batch by whisper_full and
            # token by token by the rows, so the probabilities are not bit-identical between the two)
            g, w = gu.tokens_array(got[c]), gu.tokens_array(want[c][0])
            assert g.shape == w.shape and np.array_equal(g[:, 0], w[:, 0]), (kind, c, g[:, 0], w[:, 0])
            _assert_same_transcription(got[c], want[c][0], (kind, c), False)
        assert gu.tokens_array(got[4]).shape[0] == 0 and lib.wmi_batch_select(node.ctx, 4) == 0       # < 1 s: no segments
        assert gu.tokens_array(got[0]).shape[0] > 0
    finally:
        lib.wmi_set_lockstep_exact(0)
        if node is not None:
            node.close()


# ------------------------------------------------------------------------------------------------ 5. lock-step, default mode, groups
def test_lockstep_auto_default_mode_with_groups(product_lib):
    """Eight chunks, two lock-step groups side by side (the second on a replica context), default (matrix-core) rows: all chunks stay in
    lock-step, the ids are the table's, and every chunk's transcription is the one a known-language wmi_full_batch call gives it (compared
    like the other default-mode lock-step tests: up to the first near-tie).  With audio_ctx = 300 the detection still runs at full length."""
    lib = product_lib
    x = inputs()
    chunks = x + [x[0], x[2]]
    ids_want = IDS + [IDS[0], IDS[2]]
    node = _node(lib)
    try:
        prev = lib.wmi_set_lockstep_groups(node.ctx, 2)
        for actx in (0, 300):
            got = node.transcribe_batch(chunks, params=_params(node, audio_ctx=actx))
            assert node.last_ret == 0 and len(got) == 8
            assert list(node.last_modes) == [0] * 8, node.last_modes
            assert list(node.last_langs) == ids_want, node.last_langs
            known = {}
            for lid in sorted(set(ids_want)):
                known[lid] = node.transcribe_batch(chunks, params=_params(node, bytes(lib.whisper_lang_str(lid)), audio_ctx=actx))
                assert node.last_ret == 0 and list(node.last_modes) == [0] * 8 and list(node.last_langs) == [lid] * 8
            for c in range(8):
                assert gu.tokens_array(got[c]).shape[0] > 0
                _assert_same_transcription(got[c], known[ids_want[c]][c], ("auto vs known", actx, c), False)
    finally:
        lib.wmi_set_lockstep_groups(node.ctx, max(prev, 0))
        node.close()


# ------------------------------------------------------------------------------------------------ 6. edges
def test_lockstep_auto_edges(product_lib):
    """detect_language ends the call behind the detection (ids and probabilities, no segments); an empty chunk is whisper_full's -3; the
    accessors refuse a bad index.
    An English-only model (micro.en) with language "auto": as before this feature the chunks leave lock-step and run one at a time through
    whisper_full — wmi_full_batch returns 0, wmi_batch_chunk_mode is 1 for every chunk, and each chunk's transcription is whisper_full's on
    a fresh context (derived from the parent's full_batch, not observed on a parent build: `lang_known` is false there, so no lock-step)."""
    lib = product_lib
    x = inputs()
    node = _node(lib)
    try:
        p = _params(node); p.detect_language = True
        got = node.transcribe_batch([x[0], x[2], x[5]], params=p)
        assert node.last_ret == 0 and [gu.tokens_array(g).shape[0] for g in got] == [0, 0, 0]
        assert list(node.last_langs) == [71, 49, 71]
        for c in range(3):
            probs = np.zeros(N_LANG, np.float32)
            assert lib.wmi_batch_lang_probs(node.ctx, c, _fp(probs)) == 0
            assert abs(float(probs.sum()) - 1.0) < 1e-4 and int(np.argmax(probs)) == node.last_langs[c]
        assert lib.wmi_batch_lang_id(node.ctx, 3) == -1 and lib.wmi_batch_lang_id(node.ctx, -1) == -1
        assert lib.wmi_batch_lang_probs(node.ctx, 3, _fp(np.zeros(N_LANG, np.float32))) == -1
        node.transcribe_batch([x[0], np.zeros(0, np.float32), x[2]], params=_params(node))
        assert node.last_ret == -3
        got = node.transcribe_batch([x[0], x[2]], params=_params(node))                     # the context is fine afterwards
        assert node.last_ret == 0 and list(node.last_langs) == [71, 49] and list(node.last_modes) == [0, 0]
    finally:
        node.close()
    # English-only
    m_en = synth.make_model("micro.en", seed=31)
    want = []
    for pcm in x[:3]:
        n1 = host.SpeechToText(lib); n1.set_language_model(m_en)
        want.append((n1.transcribe(pcm, params=_params(n1)), lib.whisper_full_lang_id(n1.ctx)))
        assert n1.last_ret == 0
        n1.close()
    node = host.SpeechToText(lib); node.set_language_model(m_en)
    try:
        got = node.transcribe_batch(x[:3], params=_params(node))
        assert node.last_ret == 0 and list(node.last_modes) == [1, 1, 1], (node.last_ret, node.last_modes)
        for c in range(3):
            _assert_same_transcription(got[c], want[c][0], ("micro.en auto", c), True)
            assert node.last_langs[c] == want[c][1]
    finally:
        node.close()

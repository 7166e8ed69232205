"""-m gpu: wmi_full_long (include/wmi_device.h) — a recording cut at its silences on the device and decoded in lock-step.

The merged result must be what transcribe_batch returns on the slices the plan names (wmi_long_get_piece), with the times shifted by each
piece's first frame: strictly, since wmi_full_long makes that very call on the same build.  In the exact mode (wmi_set_lockstep_exact)
every piece must also be what whisper_full returns for its slice on a fresh context.  The plan itself is held to the restatement of
tests/segment_f64.py on the energies of the definition."""
import ctypes as C

import numpy as np
import pytest

import segment_f64 as sj
from godot_whisper_amd import abi, host, synth
from test_gpu_parity import _assert_same_transcription, _hip

pytestmark = pytest.mark.gpu

SR = 16000


@pytest.fixture(params=["mfma", "exact"])
def lockstep_mode(request, product_lib):
    product_lib.wmi_set_lockstep_exact(1 if request.param == "exact" else 0)
    yield request.param
    product_lib.wmi_set_lockstep_exact(0)


@pytest.fixture(scope="module")
def model():
    return synth.make_model("micro.en", seed=2024)


@pytest.fixture
def node(product_lib, model):
    n = host.SpeechToText(product_lib); n.set_language_model(model)
    yield n
    n.close()


def _params(node):
    p = node.full_params("", 0); p.temperature_inc = 0.0          # no fallback: no piece may leave lock-step
    return p


def _recording(parts, seed):
    """parts: seconds of synthetic speech (> 0) or of exact zeros (< 0), one after the other"""
    out = [synth.make_pcm(s, seed=seed + i) if s > 0 else np.zeros(int(round(-s * SR)), np.float32) for i, s in enumerate(parts)]
    return np.concatenate(out)


@pytest.fixture(scope="module")
def rec20():
    """20.5 s: two bursts a short gap apart, a gap above max_gap_ms, a 12 s burst (cut at energy minima with max_piece_ms = 5000), a last burst"""
    return _recording([1.5, -0.8, 2.0, -2.5, 12.0, -0.5, 1.2], seed=900)


def _slices(pcm, pieces):
    return [pcm[160 * p["frame0"]:min(160 * p["frame1"], pcm.size)] for p in pieces]


def _shifted(results, pieces):
    """the per-piece results (collect() form) as one merged result with the times moved by each piece's first frame"""
    text, toks = b"", []
    for r, p in zip(results, pieces):
        text += r[0]
        for d in r[1:]:
            d = dict(d)
            for k in ("t0", "t1", "t_dtw"):
                if k in d and d[k] >= 0:
                    d[k] += p["frame0"]
            toks.append(d)
    return [text] + toks


def _check_plan(pcm, pieces, lp, n_audio_ctx=1500):
    want = sj.plan(sj.energies(pcm), pcm.size, lp, n_audio_ctx)
    assert [(p["frame0"], p["frame1"]) for p in pieces] == [w[:2] for w in want]
    if lp.fit_audio_ctx:
        assert [p["audio_ctx"] for p in pieces] == [w[2] for w in want]


def _long_equals_batch(node, pcm, lp, modes_zero=True, device_ptr=None):
    got = node.transcribe_long(pcm if device_ptr is None else pcm.size, params=_params(node), long_params=lp, device_ptr=device_ptr)
    assert node.last_ret == 0
    pieces, segs = list(node.last_pieces), list(node.last_segments)
    _check_plan(pcm, pieces, lp)
    if modes_zero:
        assert list(node.last_modes) == [0] * len(pieces), node.last_modes
    # the pieces' own views, then the merged one again
    per_piece, per_piece_segs = [], []
    for i in range(len(pieces)):
        assert node.lib.wmi_long_select(node.ctx, i) == pieces[i]["n_segments"]
        per_piece.append(node.collect()); per_piece_segs.append(node.segments())
    assert node.lib.wmi_long_select(node.ctx, -1) == len(segs) and node.collect() == got and node.segments() == segs
    assert node.lib.wmi_long_select(node.ctx, len(pieces)) == -1 and node.lib.wmi_long_select(node.ctx, -2) == -1
    # segment bookkeeping: i_segment / n_segments index the merged list, the segments' times are the pieces' shifted
    at = 0
    for p, ps in zip(pieces, per_piece_segs):
        assert p["i_segment"] == at and p["n_segments"] == len(ps)
        assert segs[at:at + len(ps)] == [(t0 + p["frame0"], t1 + p["frame0"], tx) for t0, t1, tx in ps]
        at += len(ps)
    assert at == len(segs)
    assert got == _shifted(per_piece, pieces)
    # the very call on the plan's slices
    actx = [p["audio_ctx"] for p in pieces] if lp.fit_audio_ctx else None
    want = node.transcribe_batch(_slices(pcm, pieces), params=_params(node), audio_ctxs=actx)
    assert node.last_ret == 0
    assert want == per_piece
    return got, pieces, per_piece


def test_equals_the_batch_call_on_the_plans_slices(product_lib, model, node, rec20, lockstep_mode):
    lp = sj.params(max_piece_ms=5000)
    got, pieces, per_piece = _long_equals_batch(node, rec20, lp)
    assert len(pieces) >= 3 and len(got) > 1
    covered = np.zeros((rec20.size + 159) // 160, bool)
    for p in pieces:
        assert p["frame1"] - p["frame0"] <= 500 and not covered[p["frame0"]:p["frame1"]].any()
        covered[p["frame0"]:p["frame1"]] = True
    assert not covered[450:660].any()                            # the 2.5 s gap (frames 430 .. 680) is decoded by no piece, but for the pads
    cuts = [a["frame1"] for a, b in zip(pieces, pieces[1:]) if a["frame1"] == b["frame0"] and 680 < a["frame1"] < 1880]
    assert len(cuts) >= 2, pieces                                # the 12 s burst (frames 680 .. 1880) was cut inside, at energy minima
    e = sj.energies(rec20)
    for c in cuts:
        s = [p["frame0"] for p in pieces if p["frame1"] == c][0]
        assert e[c] == e[s + 500 - 166:s + 501].min()
    if lockstep_mode == "exact":                                 # and every piece is whisper_full on its slice, on a fresh context
        for i, (sl, p) in enumerate(zip(_slices(rec20, pieces), pieces)):
            one = host.SpeechToText(product_lib); one.set_language_model(model)
            try:
                want = one.transcribe(sl, params=_params(one))
                assert one.last_ret == 0
                _assert_same_transcription(per_piece[i], want, ("piece", i, p), True)
            finally:
                one.close()


def test_seventeen_pieces_cross_the_group_of_sixteen(node, lockstep_mode):
    parts = []
    for i in range(17):
        parts += [1.2, -2.1]
    pcm = _recording(parts, seed=930)
    got, pieces, per_piece = _long_equals_batch(node, pcm, sj.params())
    assert len(pieces) == 17
    assert [p["frame0"] for p in pieces] == [330 * i - (10 if i else 0) for i in range(17)]      # in order: burst i begins at 3.3 s * i
    assert all(len(r) > 1 for r in per_piece)
    assert len({bytes(r[0]) for r in per_piece}) > 1             # different bursts, different texts: the order is checkable


def test_fit_audio_ctx(node, rec20, lockstep_mode):
    lp = sj.params(max_piece_ms=5000, fit_audio_ctx=1)
    got, pieces, _ = _long_equals_batch(node, rec20, lp)
    assert [p["audio_ctx"] for p in pieces] == [min(1500, (p["frame1"] - p["frame0"] + 1) // 2 + 128) for p in pieces]
    assert len(set(p["audio_ctx"] for p in pieces)) > 1


def test_no_speech_windows_are_shifted_and_rebased(product_lib, model, rec20):
    node = host.SpeechToText(product_lib, no_speech=abi.NO_SPEECH_REPORT); node.set_language_model(model)
    try:
        node.transcribe_long(rec20, params=_params(node), long_params=sj.params(max_piece_ms=5000))
        assert node.last_ret == 0
        pieces, merged = list(node.last_pieces), list(node.last_windows)
        assert list(node.last_modes) == [0] * len(pieces) and len(pieces) >= 3 and merged
        want = []
        for i, p in enumerate(pieces):
            assert product_lib.wmi_long_select(node.ctx, i) >= 0
            for w in node.windows():
                assert 0.0 <= w["no_speech_prob"] <= 1.0
                want.append(dict(w, seek=w["seek"] + p["frame0"], i_segment=w["i_segment"] + p["i_segment"]))
        assert merged == want
        assert product_lib.wmi_long_select(node.ctx, -1) >= 0
        n_seg = product_lib.whisper_full_n_segments(node.ctx)
        assert sum(w["n_segments"] for w in merged) == n_seg
        for w in merged:
            assert 0 <= w["i_segment"] <= n_seg - w["n_segments"]
            for s in range(w["i_segment"], w["i_segment"] + w["n_segments"]):
                assert product_lib.wmi_full_get_segment_no_speech_prob(node.ctx, s) == np.float32(w["no_speech_prob"])
    finally:
        node.close()


def test_device_resident_pcm(node, rec20):
    hip = _hip()
    lp = sj.params(max_piece_ms=5000)
    want = node.transcribe_long(rec20, params=_params(node), long_params=lp)
    assert node.last_ret == 0 and len(want) > 1
    want_pieces = list(node.last_pieces)
    dptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(rec20.nbytes + 16)) == 0
    try:
        for off in (0, 4):                                       # a 16-byte aligned buffer, and one that is not
            assert hip.hipMemcpy(C.c_void_p(dptr.value + off), rec20.ctypes.data_as(C.c_void_p), C.c_size_t(rec20.nbytes), 1) == 0
            got = node.transcribe_long(rec20.size, params=_params(node), long_params=lp, device_ptr=dptr.value + off)
            assert node.last_ret == 0
            assert node.last_pieces == want_pieces and got == want, off
    finally:
        hip.hipFree(dptr)


def _counters(lib, ctx):
    t6, n5 = (C.c_int64 * 6)(), (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return list(n5)


def test_silence_decodes_nothing(product_lib, node, rec20):
    assert len(node.transcribe(synth.make_pcm(2.0, seed=3), params=_params(node))) > 1
    before = _counters(product_lib, node.ctx)
    got = node.transcribe_long(np.zeros(20 * SR, np.float32), params=_params(node))
    assert node.last_ret == 0 and got == [b""] and node.last_pieces == []
    assert product_lib.wmi_long_n_pieces(node.ctx) == 0 and product_lib.whisper_full_n_segments(node.ctx) == 0
    assert product_lib.wmi_long_select(node.ctx, -1) == 0 and product_lib.wmi_long_select(node.ctx, 0) == -1
    assert _counters(product_lib, node.ctx) == before
    us, n2 = (C.c_int64 * 3)(), (C.c_int32 * 2)()
    product_lib.wmi_get_long_timings(node.ctx, us, n2)
    assert list(n2) == [2000, 0] and us[1] > 0
    # offset_ms / duration_ms restrict the plan: only the first two bursts of the recording are seen
    p = _params(node); p.duration_ms = 4400
    node.transcribe_long(rec20, params=p, long_params=sj.params(max_piece_ms=5000))
    assert node.last_ret == 0
    assert [(q["frame0"], q["frame1"]) for q in node.last_pieces] == [w[:2] for w in sj.plan(sj.energies(rec20), rec20.size, sj.params(max_piece_ms=5000), 1500, None, 0, 4400)]
    assert node.last_pieces and node.last_pieces[-1]["frame1"] <= 440


def test_refused_calls(product_lib, node, rec20):
    lib = product_lib
    assert len(node.transcribe_long(rec20[:3 * SR], params=_params(node))) > 1
    before = _counters(lib, node.ctx)
    cb = C.CFUNCTYPE(None)(lambda: None)
    for field in ("new_segment_callback", "progress_callback", "encoder_begin_callback", "logits_filter_callback"):
        p = _params(node)
        setattr(p, field, C.cast(cb, C.c_void_p).value)
        assert node.transcribe_long(rec20, params=p) == [] and node.last_ret == -1, field
    assert node.transcribe_long(rec20, params=_params(node), long_params=sj.params(max_piece_ms=999)) == [] and node.last_ret == -1
    assert node.transcribe_long(rec20, params=_params(node), long_params=sj.params(max_piece_ms=30001)) == [] and node.last_ret == -1
    assert lib.wmi_full_long(node.ctx, _params(node), rec20.ctypes.data, 0, 0, None) == -3          # no samples: as whisper_full
    assert _counters(lib, node.ctx) == before
    text = host.AudioStreamToText.get_text(node, rec20[:3 * SR], long_form=True)      # the node's one-shot call, long form
    assert isinstance(text, str)


def test_cpp_host_equals_python_mirror(product_lib, model, node, rec20, tmp_path):
    """godot_whisper::SpeechToText::transcribe_long (host_cpp/) through its command-line driver: the same plan, the same tokens and times"""
    from test_host_cpp import _as_rows, run_demo
    import golden_util as gu
    want = node.transcribe_long(rec20, params=node.full_params("", 0), long_params=sj.params(max_piece_ms=5000))
    assert node.last_ret == 0 and len(want) > 1
    got = run_demo(tmp_path, model, rec20.astype("<f4").tobytes(), "long", 1, "", 5000)
    assert got["pieces"] == [[p["frame0"], p["frame1"]] for p in node.last_pieces]
    tr = got["transcription"]
    assert tr["ok"] and tr["full_text"].encode("latin-1") == bytes(want[0])
    assert np.array_equal(_as_rows(tr)[:, [0, 1, 6, 7]], gu.tokens_array(want)[:, [0, 1, 6, 7]])


def test_token_dtw_times_are_shifted(product_lib, model, rec20):
    """the alignment mode passes through: the pieces take the general driver (chunk mode 1), every t_dtw >= 0 moves with its piece"""
    node = host.SpeechToText(product_lib, token_dtw=True); node.set_language_model(model)
    try:
        got = node.transcribe_long(rec20, params=_params(node), long_params=sj.params(max_piece_ms=5000))
        assert node.last_ret == 0
        pieces = list(node.last_pieces)
        assert list(node.last_modes) == [1] * len(pieces) and len(pieces) >= 3
        per_piece = []
        for i in range(len(pieces)):
            assert product_lib.wmi_long_select(node.ctx, i) == pieces[i]["n_segments"]
            per_piece.append(node.collect())
        assert product_lib.wmi_long_select(node.ctx, -1) >= 0
        assert got == _shifted(per_piece, pieces) and node.collect() == got
        last = [d["t_dtw"] for d in per_piece[-1][1:] if d["t_dtw"] >= 0]
        assert last and pieces[-1]["frame0"] > 0
        merged_last = [d["t_dtw"] for d in got[1:] if d["t_dtw"] >= 0][-len(last):]
        assert merged_last == [t + pieces[-1]["frame0"] for t in last]
    finally:
        node.close()

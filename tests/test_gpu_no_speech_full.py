"""-m gpu: the no-speech modes of the transcription calls (wmi_set_no_speech) on tiny.en — <sot> the last prompt token, and an interior one
with no_timestamps —, tiny (interior) and tiny q5_1, with the host's parameters and n_max_text_ctx = 0 (windows aligned and independent)
on 65 s of audio: three windows.

  mode 1   every token field and segment equals mode 0's; every window's p is within 2 f32 ulp of the float64 value of the definition
           (tests/no_speech_f64.py) on the logits whisper_decode of the prompt cut behind <sot> + whisper_get_logits return on the same
           context (bound A), and |ln p - ln p_checker| <= 2 LOGIT_ABS against the same value from the checker's logits (bound B: ln p =
           l[nosp] - lse(l), each term moves by at most the largest logit difference; block-quantised: twice the bound
           tests/test_gpu_parity.py forms for quantised logits from the checker's response to a 1e-6 perturbation of the samples)
  mode 3   thold between the windows' p: exactly the windows above it are gated (no segments), the others are mode 0's; above all three:
           mode 0; below all three: no segments, and decode counters below the ungated call's that do not depend on max_tokens
  mode 2   logprob_thold on either side of a window's measured avg_logprobs: dropped against emitted, with the host's temperature_inc
           and never a fallback
  lock-step  wmi_full_batch_ctx in the exact mode, 4 chunks of different lengths: windows, p and outcomes of every chunk equal whisper_full's
           bit for bit in modes 1 - 3; with all rows gated a window costs the steps up to its <sot> and no more; wmi_capture_full passes the
           mode through
  fallback   a context per leg (every fresh context's generators start alike), logprob_thold = 0: every window goes through all the
           temperatures; mode 1 equals mode 0 token for token and p is the first temperature's
  node     CaptureStreamToText(no_speech_gate=True): a gated step emits nothing, counts towards max_calls, and the loop goes on"""
import ctypes as C
import math

import numpy as np
import pytest

import golden_util as gu
import no_speech_f64 as nf
import stage_compare as sc
from godot_whisper_amd import abi, host, synth
from test_gpu_parity import LOGIT_ABS, _assert_same_transcription, make_checker

pytestmark = pytest.mark.gpu

CONFIGS = [("tiny.en", False), ("tiny.en", True), ("tiny", False), ("tiny-q5_1", False)]      # (model, no_timestamps)
IDS = [f"{m}{'-notimestamps' if nt else ''}" for m, nt in CONFIGS]
SECONDS = 65.0

_models, _pcm = {}, {}


def model_of(name):
    if name not in _models:
        base = name.split("-")[0]
        m = synth.make_model(base, seed=4321)
        _models[name] = synth.quantize_model(m, "q5_1") if name.endswith("q5_1") else m
    return _models[name]


def pcm_of(seconds=SECONDS, seed=31):
    if (seconds, seed) not in _pcm:
        _pcm[(seconds, seed)] = synth.make_pcm(seconds, seed=seed, gate=True)
    return _pcm[(seconds, seed)]


@pytest.fixture(scope="module")
def nodes(product_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = host.SpeechToText(product_lib)
            made[name].set_language_model(model_of(name))
            assert made[name].ctx
        return made[name]
    yield get
    for n in made.values():
        n.close()


def params(node, no_timestamps=False, fallback=False, **kw):
    """the host's parameters with n_max_text_ctx = 0.  fallback = False: temperature_inc = 0, as in every test that compares two calls token
    for token — a window that falls back draws from decoder 0's generator, which (as in the reference) carries its state from call to call
    on one context, so two calls that fall back do not repeat each other whatever the no-speech mode is"""
    p = node.full_params("", 0)
    p.n_max_text_ctx = 0
    p.no_timestamps = bool(no_timestamps)
    if not fallback:
        p.temperature_inc = 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def run(node, mode, p, pcm=None):
    """-> (tokens [n][9], text, segments [(t0, t1, n_tokens)], windows) of whisper_full in `mode`"""
    lib = node.lib
    node.set_no_speech(mode)
    try:
        r = node.transcribe(pcm_of() if pcm is None else pcm, params=p)
    finally:
        node.set_no_speech(0)
    assert node.last_ret == 0, node.last_ret
    segs = [(lib.whisper_full_get_segment_t0(node.ctx, i), lib.whisper_full_get_segment_t1(node.ctx, i), lib.whisper_full_n_tokens(node.ctx, i))
            for i in range(lib.whisper_full_n_segments(node.ctx))]
    node.last_raw = r
    return gu.tokens_array(r), bytes(r[0]), segs, node.last_windows


def window_tokens(toks, segs, w):
    """the token rows of window w's segments"""
    first = sum(n for _, _, n in segs[:w["i_segment"]])
    return toks[first:first + sum(n for _, _, n in segs[w["i_segment"]:w["i_segment"] + w["n_segments"]])]


NOT_TIMES = [0, 1, 2, 3, 4, 5, 8]            # id tid p plog pt ptsum vlen


def same_window(got, want, clean):
    """a window's tokens against mode 0's.  The token times are compared only while no window in front of it was gated or dropped: the
    reference's token-timestamp heuristics carry t_last / tid_last from one emitted segment to the next (W/whisper.cpp:6315-6377: the first
    token of a segment that does not open with a timestamp starts at t_last), so a window that emits nothing changes what the next one
    starts from — in every other field the windows are independent"""
    return np.array_equal(got, want) if clean else got.shape == want.shape and np.array_equal(got[:, NOT_TIMES], want[:, NOT_TIMES])


def pbits(ws):
    return [(w["seek"], int(np.float32(w["no_speech_prob"]).view(np.uint32)), w["outcome"], w["i_segment"], w["n_segments"]) for w in ws]


def sot_logits(node, seek):
    """the raw logits of the prompt cut behind <sot> ([sot] with n_max_text_ctx = 0) for the window at `seek`, on the node's own context"""
    lib, ctx = node.lib, node.ctx
    assert lib.wmi_set_audio_ctx(ctx, 0) == 0 and lib.whisper_encode(ctx, seek, 4) == 0
    t = np.asarray([lib.whisper_token_sot(ctx)], np.int32)
    assert lib.whisper_decode(ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), 1, 0, 4) == 0
    nv = lib.whisper_n_vocab(ctx)
    return np.ctypeslib.as_array(lib.whisper_get_logits(ctx), shape=(nv,)).copy()


@pytest.fixture(scope="module")
def mode1(nodes):
    """mode 0 and mode 1 of every configuration, computed once"""
    got = {}

    def get(cfg):
        if cfg not in got:
            node = nodes(cfg[0])
            got[cfg] = (run(node, 0, params(node, cfg[1])), run(node, 1, params(node, cfg[1])))
        return got[cfg]
    return get


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_report_changes_nothing_and_holds_bound_a(nodes, mode1, cfg):
    node = nodes(cfg[0]); lib = node.lib
    (t0, text0, segs0, w0), (t1, text1, segs1, w1) = mode1(cfg)
    assert w0 == [] and lib.wmi_full_get_segment_no_speech_prob(node.ctx, 0) != -1.0        # (the accessors read the last call: mode 1's)
    assert np.array_equal(t0, t1) and text0 == text1 and segs0 == segs1 and len(t0) > 0
    assert [w["seek"] for w in w1] == [0, 3000, 6000] and all(w["outcome"] == abi.WINDOW_EMITTED for w in w1)
    assert [w["i_segment"] for w in w1] == [0, 1, 2] and all(w["n_segments"] == 1 for w in w1)      # single_segment
    nosp = lib.whisper_token_nosp(node.ctx)
    for i, w in enumerate(w1):
        assert lib.wmi_full_get_segment_no_speech_prob(node.ctx, w["i_segment"]) == np.float32(w["no_speech_prob"])
    assert lib.wmi_full_get_segment_no_speech_prob(node.ctx, len(segs1)) == -1.0
    for w in w1:
        l = sot_logits(node, w["seek"])
        want = nf.spec_p(l, nosp)
        print(f"{IDS[CONFIGS.index(cfg)]} window at {w['seek']}: p = {w['no_speech_prob']:.9g}, float64 {want:.12g}, {nf.ulps_off(w['no_speech_prob'], want):.3f} ulp")
        assert want >= 1e-30
        sc.hold("no-speech whisper_full mode 1: f32 ulp from the float64 value on whisper_decode's logits (bound A)",
                nf.ulps_off(w["no_speech_prob"], want), float(nf.ULPS), (cfg, w["seek"]))
    # mode 0 again: nothing is stored
    assert run(node, 0, params(node, cfg[1]))[3] == [] and lib.wmi_full_n_windows(node.ctx) == 0
    assert lib.wmi_full_get_segment_no_speech_prob(node.ctx, 0) == -1.0


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_bound_b_against_the_checker(nodes, mode1, checker_lib, cfg):
    node = nodes(cfg[0]); lib = node.lib
    _, (_, _, _, w1) = mode1(cfg)
    model, pcm = model_of(cfg[0]), pcm_of()
    quantised = cfg[0].endswith("q5_1")
    sides = [make_checker(model, checker_lib)] + ([make_checker(model, checker_lib)] if quantised else [])
    try:
        for s in sides:
            s.n_threads = 16
        sides[0].mel(pcm)
        if quantised:
            sides[1].mel((pcm * np.float32(1.0 + 1e-6)).astype(np.float32))
        sot, nosp = lib.whisper_token_sot(node.ctx), lib.whisper_token_nosp(node.ctx)
        for w in w1:
            lr = []
            for s in sides:
                s.encode(w["seek"], 0)
                lr.append(s.decode([sot], 0))
            bound = 2.0 * LOGIT_ABS
            if quantised:
                bound = 2.0 * max(LOGIT_ABS, 3.0 * sc.err_stats(lr[1], lr[0])["max_abs"])
            d = abs(math.log(w["no_speech_prob"]) - math.log(nf.exact_p(lr[0], nosp)))
            print(f"{IDS[CONFIGS.index(cfg)]} window at {w['seek']}: |ln p - ln p_checker| = {d:.3e} of {bound:.3e}")
            sc.hold("no-speech |ln p - ln p_checker| (bound B)" + (" quantised" if quantised else ""), d, bound, (cfg, w["seek"]))
    finally:
        for s in sides:
            s.close()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_general_path_takes_the_same_row(nodes, mode1, cfg):
    """beam search leaves the greedy fast path: the whole prompt is one decode() batch and the head runs behind it — on the flagged row's
    logits where <sot> is the last prompt token, on the row's residual (f16) or on a projection of its own (block-quantised) where it is
    interior.  The same windows, each p within bound A of the same logits; a gated beam window is not sampled either"""
    node = nodes(cfg[0]); lib = node.lib
    _, (_, _, _, w1) = mode1(cfg)
    beam = dict(strategy=abi.WHISPER_SAMPLING_BEAM_SEARCH)
    p = params(node, cfg[1], **beam); p.beam_search.beam_size = 2
    _, _, segs, wb = run(node, 1, p)
    assert [w["seek"] for w in wb] == [w["seek"] for w in w1] and sum(w["n_segments"] for w in wb) == len(segs)
    nosp = lib.whisper_token_nosp(node.ctx)
    for w, g in zip(wb, w1):
        want = nf.spec_p(sot_logits(node, w["seek"]), nosp)
        sc.hold("no-speech whisper_full mode 1, beam search: f32 ulp from the float64 value on whisper_decode's logits (bound A)",
                nf.ulps_off(w["no_speech_prob"], want), float(nf.ULPS), (cfg, w["seek"]))
        assert abs(math.log(w["no_speech_prob"]) - math.log(g["no_speech_prob"])) <= 1e-5, (w, g)
    p = params(node, cfg[1], no_speech_thold=min(w["no_speech_prob"] for w in wb) / 2.0, **beam); p.beam_search.beam_size = 2
    t3, _, segs3, w3 = run(node, 3, p)
    assert len(t3) == 0 and segs3 == [] and [w["outcome"] for w in w3] == [abi.WINDOW_GATED] * 3
    assert [np.float32(w["no_speech_prob"]) for w in w3] == [np.float32(w["no_speech_prob"]) for w in wb]


def timings(lib, ctx):
    t6, n5 = (C.c_int64 * 6)(), (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return list(n5)                                            # n_encode, n_decode, n_batchd, n_prompt, n_sample


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_gate(nodes, mode1, cfg):
    node = nodes(cfg[0]); lib = node.lib
    (t0, text0, segs0, _), (_, _, _, w1) = mode1(cfg)
    ps = [float(np.float32(w["no_speech_prob"])) for w in w1]
    srt = sorted(ps)
    assert srt[0] < srt[1] < srt[2], ps
    for thold in (math.sqrt(srt[0] * srt[1]), math.sqrt(srt[1] * srt[2])):
        t3, _, segs3, w3 = run(node, 3, params(node, cfg[1], no_speech_thold=thold))
        assert [(w["seek"], np.float32(w["no_speech_prob"])) for w in w3] == [(w["seek"], np.float32(w["no_speech_prob"])) for w in w1]
        kept, clean = [], True
        for w, wm in zip(w3, w1):
            gated = np.float32(w["no_speech_prob"]) > np.float32(thold)
            assert w["outcome"] == (abi.WINDOW_GATED if gated else abi.WINDOW_EMITTED) and w["n_segments"] == (0 if gated else 1), (thold, w)
            if not gated:
                assert same_window(window_tokens(t3, segs3, w), window_tokens(t0, segs0, wm), clean), (thold, w)
                kept.append(segs0[wm["i_segment"]])
            clean = clean and not gated
        assert segs3 == kept and 0 < len(kept) < 3
    # above all three: mode 0
    t3, text3, segs3, w3 = run(node, 3, params(node, cfg[1], no_speech_thold=min(1.0, srt[2] * 2.0)))
    assert np.array_equal(t3, t0) and text3 == text0 and segs3 == segs0 and pbits(w3) == pbits(w1)
    # below all three: nothing is sampled
    counts = {}
    for mt in (4, 32):
        lib.whisper_reset_timings(node.ctx)
        t3, text3, segs3, w3 = run(node, 3, params(node, cfg[1], no_speech_thold=srt[0] / 2.0, max_tokens=mt))
        assert len(t3) == 0 and segs3 == [] and text3 == b"" and [w["outcome"] for w in w3] == [abi.WINDOW_GATED] * 3
        assert [np.float32(w["no_speech_prob"]) for w in w3] == [np.float32(p) for p in ps]
        counts[mt] = timings(lib, node.ctx)
        lib.whisper_reset_timings(node.ctx)
        run(node, 0, params(node, cfg[1], max_tokens=mt))
        ungated = timings(lib, node.ctx)
        assert counts[mt][0] == ungated[0] == 3 and counts[mt][1] < ungated[1] and counts[mt][4] < ungated[4], (mt, counts[mt], ungated)
    assert counts[4] == counts[32], counts


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_drop(nodes, mode1, cfg):
    node = nodes(cfg[0])
    _, (_, _, _, w1) = mode1(cfg)
    silent = min(float(np.float32(w["no_speech_prob"])) for w in w1) / 2.0             # every window says "no speech"
    # no threshold on the log-probabilities: emitted as decoded (a failed decoder: dropped).  These calls keep the host's temperature_inc:
    # no window of them may take the fallback (its draws would differ from call to call), however poor its log-probabilities are
    tb, _, segsb, wb = run(node, 2, params(node, cfg[1], fallback=True, no_speech_thold=silent, logprob_thold=-1e30))
    avg = {}
    for w in wb:
        if w["outcome"] == abi.WINDOW_EMITTED:
            plog = window_tokens(tb, segsb, w)[:, 3]
            acc = 0.0
            for x in plog:
                acc += float(x)
            avg[w["seek"]] = acc / len(plog)
    assert avg, wb
    for seek, a in avg.items():
        for thold, dropped in ((a + 0.01, True), (a - 0.01, False)):
            t2, _, segs2, w2 = run(node, 2, params(node, cfg[1], fallback=True, no_speech_thold=silent, logprob_thold=thold))
            clean = True
            for w, b in zip(w2, wb):
                assert np.float32(w["no_speech_prob"]) == np.float32(b["no_speech_prob"]) and w["seek"] == b["seek"]
                if b["seek"] in avg and abs(avg[b["seek"]] - thold) > 1e-4:
                    want = abi.WINDOW_DROPPED if avg[b["seek"]] < thold else abi.WINDOW_EMITTED
                    assert w["outcome"] == want, (seek, thold, w, avg)
                    if want == abi.WINDOW_EMITTED:
                        assert same_window(window_tokens(t2, segs2, w), window_tokens(tb, segsb, b), clean)
                    else:
                        assert w["n_segments"] == 0
                clean = clean and w["outcome"] == b["outcome"]
            assert [w for w in w2 if w["seek"] == seek][0]["outcome"] == (abi.WINDOW_DROPPED if dropped else abi.WINDOW_EMITTED)
    # at or below the no-speech threshold the rule is mode 0's
    t0, text0, segs0, _ = run(node, 0, params(node, cfg[1], logprob_thold=-1e30))
    t2, text2, segs2, w2 = run(node, 2, params(node, cfg[1], no_speech_thold=1.0, logprob_thold=-1e30))
    assert np.array_equal(t0, t2) and text0 == text2 and segs0 == segs2 and all(w["outcome"] == abi.WINDOW_EMITTED for w in w2)


LOCKSTEP_SECONDS = (65.0, 41.0, 31.5, 12.0)


@pytest.mark.parametrize("cfg", [("tiny.en", False), ("tiny", False), ("tiny-q5_1", False)], ids=["tiny.en", "tiny", "tiny-q5_1"])
def test_lockstep_rows_equal_whisper_full(nodes, cfg):
    node = nodes(cfg[0]); lib = node.lib
    bufs = [pcm_of(s, seed=40 + i) for i, s in enumerate(LOCKSTEP_SECONDS)]
    lib.wmi_set_lockstep_exact(1)
    try:
        # the windows' p of every chunk, alone, in mode 1: where the thresholds of modes 2 and 3 go
        alone1 = [run(node, 1, params(node, cfg[1]), pcm=b) for b in bufs]
        ps = sorted(float(np.float32(w["no_speech_prob"])) for r in alone1 for w in r[3])
        assert len(ps) == 3 + 2 + 2 + 1 and ps[0] < ps[-1]
        mid = math.sqrt(ps[len(ps) // 2 - 1] * ps[len(ps) // 2])
        plogs = sorted(float(np.mean(window_tokens(r[0], r[2], w)[:, 3])) for r in alone1 for w in r[3])
        settings = [(1, {}), (3, {"no_speech_thold": mid}), (3, {"no_speech_thold": ps[0] / 2.0}),
                    (2, {"no_speech_thold": ps[0] / 2.0, "logprob_thold": 0.5 * (plogs[len(plogs) // 2 - 1] + plogs[len(plogs) // 2])})]
        for mode, kw in settings:
            p = params(node, cfg[1], **kw)
            want = [run(node, mode, p, pcm=b) + (node.last_raw,) for b in bufs]
            node.set_no_speech(mode)
            try:
                got = node.transcribe_batch(bufs, params=p, audio_ctxs=[0] * len(bufs))
            finally:
                node.set_no_speech(0)
            assert node.last_ret == 0 and len(got) == len(bufs)
            for c, (r, ws) in enumerate(zip(got, node.last_batch_windows)):
                assert pbits(ws) == pbits(want[c][3]), (mode, kw, c, ws, want[c][3])
                # (the tokens as every exact-mode comparison holds them: ids, times and text equal, the token probabilities up to the
                #  f32 order of the two forms of the filter statistics)
                _assert_same_transcription(r, want[c][4], (mode, kw, c), True)
            if mode == 3 and kw["no_speech_thold"] < ps[0]:
                # all rows gated: a window costs the steps that feed the prompt up to <sot> — with <sot> first, one
                t4, n_steps = (C.c_int64 * 4)(), C.c_int32(0)
                lib.wmi_get_batch_timings(node.ctx, t4, C.byref(n_steps))
                assert all(w["outcome"] == abi.WINDOW_GATED for ws in node.last_batch_windows for w in ws)
                # (tiny.en with these parameters: the prompt IS <sot>, i.e. the longest chunk's windows x the prompt length)
                assert n_steps.value == 3 * 1, n_steps.value
    finally:
        lib.wmi_set_lockstep_exact(0)


def test_capture_session_passes_the_mode_through(nodes):
    node = nodes("tiny.en"); lib = node.lib
    pcm = pcm_of(12.0, seed=43)
    p = params(node)
    want = run(node, 1, p, pcm=pcm)
    node.set_no_speech(1)
    try:
        with host.CaptureSession(node, abi.WHISPER_SAMPLE_RATE, 2) as sess:
            sess.push(np.stack([pcm, pcm], axis=1))            # (x + x) / 2 = x at equal rates: the session's PCM is pcm
            assert sess.full(p) == 0
            r = node.collect()
    finally:
        node.set_no_speech(0)
    assert pbits(node.last_windows) == pbits(want[3]) and len(want[3]) == 1 and np.array_equal(gu.tokens_array(r), want[0])
    assert lib.wmi_set_no_speech(node.ctx, 0) == 0


def fresh_leg(product_lib, cfg, mode, **kw):
    """one whisper_full on a context of its own: decoder 0's generator starts where every fresh context's does, so two legs that take the
    temperature fallback draw the same numbers.  -> (run()'s result, the call's counters)"""
    node = host.SpeechToText(product_lib)
    node.set_language_model(model_of(cfg[0]))
    try:
        node.lib.whisper_reset_timings(node.ctx)
        r = run(node, mode, params(node, cfg[1], **kw))
        return r, timings(node.lib, node.ctx)
    finally:
        node.close()


@pytest.mark.parametrize("cfg", [("tiny.en", False), ("tiny", False)], ids=["tiny.en", "tiny"])
def test_fallback_takes_p_once(product_lib, mode1, cfg):
    """the host's temperature_inc with logprob_thold = 0: every window's average log-probability is below it, so every window goes through
    all the temperatures (greedy fast path first, then best_of decoders on the general path) and is emitted from the last one.  Mode 1
    changes nothing in that, and each window's p is the first temperature's: bit for bit what the call without a fallback reports"""
    _, (_, _, _, w1) = mode1(cfg)
    fb = dict(fallback=True, logprob_thold=0.0)
    (_, _, _, _), plain = fresh_leg(product_lib, cfg, 0)
    (t0, text0, segs0, w0), n0 = fresh_leg(product_lib, cfg, 0, **fb)
    (t1, text1, segs1, w1f), n1 = fresh_leg(product_lib, cfg, 1, **fb)
    assert sum(n0[1:]) >= 2 * sum(plain[1:]), (n0, plain)                 # (at least a second attempt per window: the fallback is real)
    assert w0 == [] and np.array_equal(t0, t1) and text0 == text1 and segs0 == segs1 and len(t0) > 0 and n0 == n1
    assert pbits(w1f) == pbits(w1), (w1f, w1)
    # mode 2 at or below the threshold falls back as mode 0 does; above it, a window that decoded poorly is dropped at the first
    # temperature: no further attempt is made
    (t2, text2, segs2, w2), n2 = fresh_leg(product_lib, cfg, 2, no_speech_thold=1.0, **fb)
    assert np.array_equal(t0, t2) and text0 == text2 and segs0 == segs2 and n2 == n0 and pbits(w2) == pbits(w1)
    silent = min(float(np.float32(w["no_speech_prob"])) for w in w1) / 2.0
    (t2, _, segs2, w2), n2 = fresh_leg(product_lib, cfg, 2, no_speech_thold=silent, **fb)
    assert len(t2) == 0 and segs2 == [] and [w["outcome"] for w in w2] == [abi.WINDOW_DROPPED] * 3 and n2 == plain, (w2, n2, plain)


def stream_node(product_lib, gate, thold, calls):
    """the streaming node with temperature_inc = 0 (two nodes are compared call for call) and no_speech_thold = thold in every call's
    parameters; calls[0] counts the parameter blocks, one per transcription"""
    node = host.CaptureStreamToText(product_lib, no_speech_gate=gate)
    node.set_language_model(model_of("tiny.en"))
    make = node.full_params

    def full_params(*a, **kw):
        p = make(*a, **kw)
        p.temperature_inc = 0.0
        p.no_speech_thold = thold
        calls[0] += 1
        return p
    node.full_params = full_params
    return node


def test_streaming_node_gate(product_lib):
    """CaptureStreamToText(no_speech_gate=True): a gated step is "no activity" — nothing is emitted and the loop goes on, max_calls still
    counts it —, on stream() and on stream_capture() through the session and through the separate calls; with the threshold out of reach
    the node emits what the node without the gate emits"""
    pcm = pcm_of(6.0, seed=44)
    xy = np.stack([pcm, pcm], axis=1)
    sr = abi.WHISPER_SAMPLE_RATE
    made = []
    try:
        def node(gate, thold, calls):
            made.append(stream_node(product_lib, gate, thold, calls))
            return made[-1]
        c = [0]
        gated = node(True, 0.0, c)                                  # every p is > 0: every step is gated
        assert list(gated.stream(pcm, max_calls=4)) == [] and c[0] == 4
        assert gated.last_windows and all(w["outcome"] == abi.WINDOW_GATED for w in gated.last_windows)
        for use_session in (True, False):
            c[0] = 0
            # (stream_capture transcribes from the first step on: under a second of audio whisper_full has no window — nothing to gate, an
            #  empty result as without the gate —, from a second on every step is gated)
            got = list(gated.stream_capture(xy, sr, max_calls=6, use_session=use_session))
            assert [(g[1], g[4]) for g in got] == [("", [])] * 3 and all(g[2] < sr for g in got) and c[0] == 6, got
        c[0] = 0
        step = int(round(gated.interval * sr))                       # without max_calls: every step that holds a second of audio or more
        assert list(gated.stream(pcm)) == [] and c[0] == sum(1 for pos in range(step, pcm.size + 1, step) if pos >= sr) > 10
        # the threshold out of reach (p <= 1): the plain node's output, call for call
        c1, c2 = [0], [0]
        open_, plain = node(True, 1.0, c1), node(False, 1.0, c2)
        got, want = list(open_.stream(pcm, max_calls=6)), list(plain.stream(pcm, max_calls=6))
        assert got == want and len(want) == 6 and c1 == c2 == [6]
        assert all(w["outcome"] == abi.WINDOW_EMITTED for w in open_.last_windows) and plain.last_windows == []
        got, want = list(open_.stream_capture(xy, sr, max_calls=4)), list(plain.stream_capture(xy, sr, max_calls=4))
        assert got == want and len(want) == 4
    finally:
        for n in made:
            n.close()

"""-m gpu: whisper_full with an armed draft (wmi_set_draft) on synthetic micro.en, micro, tiny.en and micro.en quantised to q5_1,
synth.make_pcm audio of 4 s at a short audio_ctx.

  (a) nothing existing moves: with nothing armed, every accessor's bits before and after a drafted call on the same context
  (b) the product's own earlier result as the draft, that draft with token k replaced, a garbage draft, a draft with ten tokens appended:
      n_accepted is the judge's (tests/draft_ref.py) and tokens, text, t0 / t1 and segments are EQUAL to the plain call's, p within 1e-2 —
      with no near-tie allowance, on inputs whose greedy run on the checker keeps a filtered top-1 / top-2 margin and a
      |ts_logprob - max_text| of at least 4 x LOGIT_ABS at every step.  The (model seed, PCM seed) pairs below were found on the CPU with
      the checker; every test re-asserts the condition before it compares and fails if it does not hold.  Draft lengths put P + n on 8
      and 9 (the weight-streaming against the MFMA form of the projections)
  (c) one long draft, max_tokens = 0, the model's own uncapped result — and drafts that put P + n on 64 and 65 (a GEMM row-tile edge):
      the accepted-prefix property, and every token 0 .. a is the bit-exact host filters' pick (wmi_process_logits) on the logits row the
      verifier saw, with that row's history; every one of those rows lies within LOGIT_ABS / LOGIT_RMS of whisper_decode on
      prompt + tokens[:j] as one ordinary sequence and of the checker on the same sequence (q5_1: tests/test_gpu_score_texts.py's bounds
      per row, max(LOGIT_ABS, 3 x noise) and min(max(LOGIT_RMS, 2 x noise), 5e-2), noise = the checker's response to a 1e-6 change of the PCM)
  (d) no-speech modes 1 and 3 and token DTW with a draft: |ln p - ln p_plain| <= 2 LOGIT_ABS (ln p = l[nosp] - lse(l): each term moves by at most
      the largest logit difference between the batch's <sot> row and the plain path's), a gated window emits nothing, t_dtw equals the undrafted call's under (b)'s condition
  (e) ineligible calls — beam search, best_of > 1 at t > 0, a callback, a grammar, wmi_full_batch — give reason 2, a result equal bit for bit to
      the unarmed call's and a consumed draft
  (f) the session: wmi_capture_set_draft(cap, 1) over a stream_capture run of 14 steps emits the same messages as mode 0, accepts on every
      step that carries a draft, and starts from nothing after keep_last — (b)'s condition re-asserted with the checker for every step, on
      the step's own samples and audio_ctx (four tokens a step, so that a seed pair that keeps the margins throughout exists)

No test reads the reference checkout."""
import ctypes as C
import math

import numpy as np
import pytest

import draft_ref as dr
import filters_f64 as ff
import golden_util as gu
import stage_compare as sc
from godot_whisper_amd import abi, host, synth
from test_gpu_parity import LOGIT_ABS, LOGIT_RMS, make_checker

pytestmark = pytest.mark.gpu

ACTX = 160
MAX_TOKENS = 12                                   # (b): the capped call the condition is asked of
MARGIN = 4 * LOGIT_ABS
# (model seed, PCM seed) per model: the first pair of a search over seeds on the CPU checker whose capped greedy run keeps both margins
# (micro.en: winner 0.133, mass 0.649; micro: 0.347, 4.272; tiny.en: 0.205, 0.854; micro.en q5_1: 0.301, 0.949 — against 4 x LOGIT_ABS = 0.12)
SEEDS = {"micro.en": (1234, 12), "micro": (1234, 9), "tiny.en": (1234, 11), "micro.en q5_1": (1234, 10)}
P_TOL = 1e-2


def model_of(name, seed):
    base = synth.make_model(name.split()[0], seed=seed)
    return synth.quantize_model(base, "q5_1") if name.endswith("q5_1") else base


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Leg:
    """a node on one model and one PCM, the host-only filters of its vocabulary, and its plain results"""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        ms, ps = SEEDS[name]
        self.model = model_of(name, ms)
        self.pcm = synth.make_pcm(4.0, seed=ps)
        self.node = host.SpeechToText(lib); self.node.set_language_model(self.model)
        assert self.node.ctx
        self.ctx = self.node.ctx
        self.hostside = ff.HostSide(lib, self.model)
        self.v = self.hostside.v
        self.m = dr.Model(self.v.n_vocab, self.v.eot, self.v.beg, lib.whisper_n_text_ctx(self.ctx), self.v.n_audio_ctx, self.v.space_id)
        sot = lib.whisper_token_sot(self.ctx)
        self.prompt = [sot] + ([sot + 1, lib.whisper_token_transcribe(self.ctx)] if lib.whisper_is_multilingual(self.ctx) else [])
        self._plain = {}

    def close(self):
        self.node.close(); self.hostside.close()

    def params(self, max_tokens=MAX_TOKENS, **kw):
        p = self.node.full_params("", ACTX)
        p.n_max_text_ctx = 0; p.temperature_inc = 0.0; p.max_tokens = max_tokens
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    def run(self, p, draft=None, want_logits=0):
        """-> dict(tokens [n][9], text, segs, status, t_dtw, logits)"""
        lib, ctx = self.lib, self.ctx
        lo = None
        if want_logits:
            lo = np.full((want_logits, self.m.n_vocab), np.nan, np.float32)
            assert lib.wmi_selftest_draft_logits(ctx, vp(lo), want_logits) == 0
        r = self.node.transcribe(self.pcm, params=p, draft=draft)
        assert self.node.last_ret == 0, self.node.last_ret
        segs = [(lib.whisper_full_get_segment_t0(ctx, i), lib.whisper_full_get_segment_t1(ctx, i), lib.whisper_full_n_tokens(ctx, i))
                for i in range(lib.whisper_full_n_segments(ctx))]
        st = self.node.last_draft_status
        return dict(tokens=gu.tokens_array(r), text=bytes(r[0]), segs=segs, windows=self.node.last_windows, raw=r, logits=lo,
                    status=(st["n_offered"], st["n_rows"], st["n_accepted"], st["n_emitted_from_draft"], st["reason"]))

    def plain(self, max_tokens=MAX_TOKENS):
        if max_tokens not in self._plain:
            self._plain[max_tokens] = self.run(self.params(max_tokens))
            assert self._plain[max_tokens]["status"] == (0, 0, 0, 0, abi.DRAFT_NONE)
        return self._plain[max_tokens]

    def ids(self, res):
        return [int(t) for t in res["tokens"][:, 0]]

    def dr_params(self, p):
        return dr.Params(bool(p.suppress_blank), float(p.max_initial_ts), int(p.max_tokens), bool(p.single_segment))

    def seek_end(self):
        return self.pcm.size // 160


def ff_state(leg, p, hist, has_ts, seek_delta):
    pat = "".join("t" if t >= leg.v.beg else "x" for t in hist[-2:]) if len(hist) >= 2 else ("t" if hist and hist[0] >= leg.v.beg else "x" * len(hist))
    return ff.State("row", hist=pat, has_ts=has_ts, seek_delta=seek_delta, suppress_blank=bool(p.suppress_blank), max_initial_ts=float(p.max_initial_ts),
                    no_timestamps=bool(p.no_timestamps), non_speech=bool(p.suppress_non_speech_tokens), tdrz=bool(p.tdrz_enable))


def checker_greedy(leg, chk, p, pcm=None, actx=ACTX):
    """the checker's greedy run of the call (float64 filters on its logits) -> (tokens, the smallest winner margin, the smallest mass margin)"""
    pcm = leg.pcm if pcm is None else pcm
    chk.mel(pcm); chk.encode(0, actx)
    dp = leg.dr_params(p)
    d = dr.Dec()
    win, mass = np.inf, np.inf
    for i in range(dr.n_max(leg.m)):
        raw = chk.decode(leg.prompt + d.tokens, 0)
        ref = ff.evaluate(raw, leg.v, ff_state(leg, p, d.tokens, d.has_ts, d.seek_delta), 0.0)
        win, mass = min(win, ref.gaps["winner"]), min(mass, ref.gaps["mass"])
        d.tokens.append(ref.id)
        dr.advance(leg.m, dp, d, i, 0, pcm.size // 160)
        if d.completed or d.failed:
            break
    return list(d.tokens), win, mass


_legs = {}


@pytest.fixture(scope="module")
def legs(product_lib):
    def get(name):
        if name not in _legs:
            _legs[name] = Leg(product_lib, name)
        return _legs[name]
    yield get
    for l in _legs.values():
        l.close()
    _legs.clear()


@pytest.fixture(scope="module")
def condition(legs, checker_lib):
    """(b)'s condition, asserted once per model on the checker: fails — never skips — where it does not hold"""
    held = {}

    def get(name):
        if name not in held:
            leg = legs(name)
            chk = make_checker(leg.model, checker_lib)
            try:
                toks, win, mass = checker_greedy(leg, chk, leg.params())
            finally:
                chk.close()
            print(name, "checker margins: winner", win, "mass", mass, "tokens", len(toks))
            assert win >= MARGIN and mass >= MARGIN, (name, "the seeds no longer meet the margin condition", win, mass)
            held[name] = toks
        return held[name]
    return get


@pytest.fixture(scope="module")
def row_refs(legs, checker_lib):
    """per model: the logits of prompt + tokens as ONE ordinary sequence — whisper_decode on the product's own context, the checker, and
    for q5_1 the checker on the PCM scaled by 1 + 1e-6 (the yardstick's noise) — computed once per sequence and shared by the drafts"""
    made = {}

    def get(name):
        if name in made:
            return made[name][0]
        leg = legs(name)
        quant = "q5_1" in name
        chks = [make_checker(leg.model, checker_lib) for _ in range(2 if quant else 1)]
        chks[0].mel(leg.pcm); chks[0].encode(0, ACTX)
        if quant:
            chks[1].mel((leg.pcm * np.float32(1.0 + 1e-6)).astype(np.float32)); chks[1].encode(0, ACTX)
        cache = {}

        def rows(tokens):
            key = tuple(tokens)
            if key not in cache:
                lib = leg.lib
                seq = np.asarray(leg.prompt + list(tokens), np.int32)
                assert lib.wmi_set_audio_ctx(leg.ctx, ACTX) == 0
                assert lib.whisper_decode(leg.ctx, seq.ctypes.data_as(C.POINTER(C.c_int32)), seq.size, 0, 4) == 0
                one = np.ctypeslib.as_array(lib.whisper_get_logits(leg.ctx), shape=(seq.size, leg.m.n_vocab))[-1].copy()
                ref = chks[0].decode(seq.tolist(), 0)
                cache[key] = (one, ref, chks[1].decode(seq.tolist(), 0) if quant else None)
            return cache[key]
        made[name] = (rows, chks)
        return rows
    yield get
    for _, chks in made.values():
        for c in chks:
            c.close()


def same_result(got, want, what):
    assert got["text"] == want["text"] and got["segs"] == want["segs"], what
    g, w = got["tokens"], want["tokens"]
    assert g.shape == w.shape, what
    assert np.array_equal(g[:, [0, 1, 6, 7]], w[:, [0, 1, 6, 7]]), (what, "ids / tids / t0 / t1")
    for col, nm in ((2, "p"), (4, "pt"), (5, "ptsum")):
        assert np.abs(g[:, col] - w[:, col]).max(initial=0.0) <= P_TOL, (what, nm)


MODELS = ["micro.en", "micro", "tiny.en", "micro.en q5_1"]


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", ["micro.en", "micro.en q5_1"])
def test_nothing_armed_nothing_moves(legs, product_lib, name):
    leg = legs(name)
    fresh = Leg(product_lib, name)
    try:
        want = fresh.run(fresh.params())
    finally:
        fresh.close()
    before = leg.run(leg.params())
    drafted = leg.run(leg.params(), draft=leg.ids(before))
    assert drafted["status"][4] == abi.DRAFT_USED
    after = leg.run(leg.params())
    for r in (before, after):
        assert r["status"] == (0, 0, 0, 0, abi.DRAFT_NONE)
        assert r["text"] == want["text"] and r["segs"] == want["segs"]
        assert np.array_equal(r["tokens"].view(np.uint64), want["tokens"].view(np.uint64)), "an accessor's bits moved"


# ---------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", MODELS)
def test_drafts_of_the_own_result(legs, condition, name):
    leg = legs(name)
    chk_tokens = condition(name)
    want = leg.plain()
    own = leg.ids(want)
    assert own == chk_tokens[:len(own)], "the product's greedy run left the checker's although the margins hold"
    p = leg.params()
    P = len(leg.prompt)
    rng = np.random.default_rng(7)
    garbage = lambda n: rng.integers(1000, leg.v.eot - 1, n).tolist()
    drafts = {"own": own, "own + ten": own + garbage(10), "garbage to P + n = 8": garbage(8 - P), "garbage to P + n = 9": garbage(9 - P),
              "own to P + n = 8": (own + garbage(10))[:8 - P], "own to P + n = 9": (own + garbage(10))[:9 - P]}
    for k in (0, 1, len(own) // 2, len(own) - 1):
        d = list(own); d[k] = own[k] + 1 if own[k] + 1 < leg.v.eot else own[k] - 1
        drafts[f"token {k} replaced"] = d
    # the picks of the rows the accepted run can reach are the greedy decode's own tokens (the condition): the judge's accept length
    for what, d in drafts.items():
        got = leg.run(p, draft=d)
        n = dr.clip(leg.m, leg.dr_params(p), P, len(d))
        a = 0
        while a < n and a < len(chk_tokens) and d[a] == chk_tokens[a]:
            a += 1
        assert got["status"][:3] == (len(d), n, a) and got["status"][4] == abi.DRAFT_USED, (name, what, got["status"], (len(d), n, a))
        assert 1 <= got["status"][3] <= a + 1
        same_result(got, want, (name, what))


# ---------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("name", MODELS)
def test_one_long_draft(legs, row_refs, name):
    leg = legs(name)
    lib = leg.lib
    p = leg.params(max_tokens=0)
    want = leg.plain(0)
    own = leg.ids(want)
    P = len(leg.prompt)
    rng = np.random.default_rng(11)
    pad = lambda d, n: (list(d) + rng.integers(1000, leg.v.eot - 1, n).tolist())[:n]
    for what, d in (("own", own), ("P + n = 64", pad(own, 64 - P)), ("P + n = 65", pad(own, 65 - P))):
        n = dr.clip(leg.m, leg.dr_params(p), P, len(d))
        got = leg.run(p, draft=d, want_logits=n + 1)
        off, rows, a, emitted, reason = got["status"]
        assert (off, rows, reason) == (len(d), n, abi.DRAFT_USED), (name, what, got["status"])
        toks = leg.ids(got)
        # the accepted-prefix property (the window's tokens behind result_len are cut: compare what is there)
        assert 0 <= a <= n and 1 <= emitted <= a + 1
        m_ = min(a, len(toks))
        assert toks[:m_] == d[:m_], (name, what, "an accepted token is not the draft's")
        if a < n and a < len(toks) and emitted == a + 1:
            assert toks[a] != d[a], (name, what, "the first refused token equals the draft's")
        # every token 0 .. a is the host filters' pick on the row the verifier saw, with that row's history
        lo = got["logits"]
        assert np.isfinite(lo[:n + 1]).any(axis=1).all(), "a logits row did not arrive"
        pl = dr.plan(leg.m, leg.dr_params(p), P, d, 0, leg.seek_end())
        for j in range(min(emitted, len(toks))):
            hist, has_ts, seek_delta = pl.states[j]
            _, tok = leg.hostside.pick(lo[j], ff_state(leg, p, hist, has_ts, seek_delta), 0.0)
            assert tok[0] == toks[j], (name, what, "row", j, "the host filters pick", tok[0], "the call emitted", toks[j])
        # every one of those rows against whisper_decode on prompt + tokens[:j] as one ordinary sequence and against the checker on the same
        # sequence.  q5_1: the bounds tests/test_gpu_score_texts.py forms per row from the checker's response to a 1e-6 change of the PCM
        rows = row_refs(name)
        for j in range(min(emitted, len(toks))):
            one, ref, noise = rows(toks[:j])
            ab, rm = LOGIT_ABS, LOGIT_RMS
            if noise is not None:
                nz = sc.err_stats(noise, ref)
                ab, rm = max(LOGIT_ABS, 3.0 * nz["max_abs"]), min(max(LOGIT_RMS, 2.0 * nz["rms_rel"]), 5e-2)
            q = " (quantised: vs the checker's self-noise yardstick)" if noise is not None else ""
            for kind, other in (("one ordinary sequence on the product", one), ("the checker", ref)):
                st = sc.err_stats(lo[j], other)
                sc.hold(f"draft rows vs {kind}, max |d|" + q, st["max_abs"], ab, (name, what, j, st))
                sc.hold(f"draft rows vs {kind}, rms-rel" + q, st["rms_rel"], rm, (name, what, j, st))


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("name", ["micro.en", "micro"])
def test_no_speech_modes_and_dtw_with_a_draft(legs, condition, name):
    leg = legs(name)
    condition(name)
    node = leg.node
    own = leg.ids(leg.plain())
    p = leg.params()
    for mode in (1, 3):
        node.set_no_speech(mode)
        try:
            want = leg.run(p)
            got = leg.run(p, draft=own)
        finally:
            node.set_no_speech(0)
        assert got["status"][4] == abi.DRAFT_USED
        assert len(got["windows"]) == len(want["windows"]) == 1
        gw, ww = got["windows"][0], want["windows"][0]
        assert gw["outcome"] == ww["outcome"]
        # ln p = l[nosp] - lse(l): each term moves by at most the largest logit difference between the batch's <sot> row and the plain path's
        d_ln = abs(math.log(gw["no_speech_prob"]) - math.log(ww["no_speech_prob"]))
        print(name, "mode", mode, "p drafted", gw["no_speech_prob"], "plain", ww["no_speech_prob"], "|d ln p|", d_ln)
        sc.hold("drafted window: |ln p - ln p_plain|", d_ln, 2.0 * LOGIT_ABS, (name, mode))
        same_result(got, want, (name, "no-speech mode", mode))
    # a gated window emits nothing, drafted or not
    node.set_no_speech(3)
    try:
        gated = leg.run(leg.params(no_speech_thold=-1.0), draft=own)
    finally:
        node.set_no_speech(0)
    assert gated["windows"][0]["outcome"] == abi.WINDOW_GATED and gated["segs"] == [] and gated["status"][4] == abi.DRAFT_USED
    assert gated["status"][3] == 0
    # token DTW runs behind the window: the same times
    node.set_token_dtw(True)
    try:
        want = leg.run(p)
        got = leg.run(p, draft=own)
    finally:
        node.set_token_dtw(False)
    assert [t["t_dtw"] for t in got["raw"][1:]] == [t["t_dtw"] for t in want["raw"][1:]]
    same_result(got, want, (name, "token dtw"))


# ---------------------------------------------------------------------------------------------- (e)
def test_ineligible_calls(legs, product_lib):
    leg = legs("micro.en")
    lib = leg.lib
    own = leg.ids(leg.plain())
    cb = abi.whisper_logits_filter_callback(lambda ctx, state, tokens, n_tokens, logits, user: None)
    ptrs, n_rules, keep = abi.make_grammar(gu.colour_list_grammar())

    def variant(l, what):
        p = l.params()
        if what == "beam search":
            p.strategy = abi.WHISPER_SAMPLING_BEAM_SEARCH; p.beam_search.beam_size = 3
        elif what == "best_of 2 at t = 0.4":
            p.temperature = 0.4; p.greedy.best_of = 2
        elif what == "a callback":
            p.logits_filter_callback = C.cast(cb, C.c_void_p)
        else:
            p.grammar_rules = C.cast(ptrs, C.c_void_p); p.n_grammar_rules = n_rules; p.i_start_rule = 0; p.grammar_penalty = 100.0
        return p

    for what in ("beam search", "best_of 2 at t = 0.4", "a callback", "a grammar"):
        # (a context each: the decoders' generators carry their state from call to call, so two calls on one context draw differently)
        a, b = Leg(product_lib, "micro.en"), Leg(product_lib, "micro.en")
        try:
            want = a.run(variant(a, what))
            got = b.run(variant(b, what), draft=own)
            assert got["status"] == (len(own), 0, 0, 0, abi.DRAFT_NOT_ELIGIBLE), (what, got["status"])
            assert got["text"] == want["text"] and got["segs"] == want["segs"], what
            assert np.array_equal(got["tokens"].view(np.uint64), want["tokens"].view(np.uint64)), what
            assert b.run(variant(b, what))["status"] == (0, 0, 0, 0, abi.DRAFT_NONE), (what, "the draft was not consumed")
        finally:
            a.close(); b.close()
    del keep
    # wmi_full_batch
    arr = np.asarray(own, np.int32)

    def lock_step():
        r = leg.node.transcribe_batch([leg.pcm, leg.pcm[:48000]], params=leg.params())
        assert leg.node.last_ret == 0 and len(r) == 2
        return r

    want = lock_step()                                       # nothing armed
    assert leg.node.draft_status()["reason"] == abi.DRAFT_NONE
    assert lib.wmi_set_draft(leg.ctx, vp(arr), arr.size) == 0
    got = lock_step()
    assert leg.node.draft_status() == {"n_offered": len(own), "n_rows": 0, "n_accepted": 0, "n_emitted_from_draft": 0, "reason": abi.DRAFT_NOT_ELIGIBLE}
    for g, w in zip(got, want):                              # text and every token field of every chunk, bit for bit
        assert g[0] == w[0] and len(g) == len(w)
        assert np.array_equal(gu.tokens_array(g).view(np.uint64), gu.tokens_array(w).view(np.uint64)) and [t["text"] for t in g[1:]] == [t["text"] for t in w[1:]]
    assert leg.run(leg.params())["status"] == (0, 0, 0, 0, abi.DRAFT_NONE)


# ---------------------------------------------------------------------------------------------- (f)
SESSION_SEEDS = (1235, 12)                        # (model seed, PCM seed) of the session run, found on the CPU: every step keeps (b)'s margins on the checker (worst 0.25)
SESSION_MAX_TOKENS = 3                            # four tokens a step: a dozen steps stay within reach of a seed search
SESSION_STEP = 4800                               # 0.3 s of capture frames at a mix rate of 16 kHz


def session_accumulations(msgs):
    """the samples [start, pos) every call of the loop transcribed, rebuilt from its messages (finish, .., n_samples, .., no_activity): a
    finished sentence with activity keeps the last 0.2 s.  At a mix rate of 16 kHz the session's PCM is the fold of the two equal
    channels: the samples themselves."""
    out, start = [], 0
    for i, m in enumerate(msgs):
        pos = SESSION_STEP * (i + 1)
        assert m[2] == pos - start, (i, m[2], pos, start)
        out.append((start, pos))
        if m[0] and not m[5]:
            start = pos - int(0.2 * 16000)
    return out


def test_the_session_reuses_its_last_result(product_lib, checker_lib):
    model = model_of("micro.en", SESSION_SEEDS[0])
    pcm = synth.make_pcm(6.0, seed=SESSION_SEEDS[1])
    xy = np.repeat(pcm[:, None], 2, axis=1)
    runs = {}
    for reuse in (False, True):
        node = host.CaptureStreamToText(product_lib, draft_reuse=reuse)
        node.settings["audio/input/transcribe/max_tokens"] = SESSION_MAX_TOKENS
        node.set_language_model(model)
        try:
            msgs = [(f, t, n, a, [(d["id"], d["tid"], d["t0"], d["t1"]) for d in toks], na)
                    for f, t, n, a, toks, na in node.stream_capture(xy, 16000, max_calls=14, temperature_inc=0.0, minimum_sentence_time=2.5)]
            runs[reuse] = (msgs, list(node.draft_statuses))
        finally:
            node.close()
    plain, drafted = runs[False], runs[True]
    # (b)'s condition, re-asserted for every step that decoded: the checker's greedy run on the step's own samples at the step's audio_ctx
    leg = Leg(product_lib, "micro.en")
    try:
        chk = make_checker(model, checker_lib)
        try:
            for i, ((start, pos), m) in enumerate(zip(session_accumulations(plain[0]), plain[0])):
                if pos - start < 16000:
                    assert m[4] == []                            # less than a second: the call decodes nothing
                    continue
                p = leg.node.full_params("", m[3]); p.temperature_inc = 0.0; p.max_tokens = SESSION_MAX_TOKENS
                toks, win, mass = checker_greedy(leg, chk, p, pcm[start:pos], m[3])
                print("session step", i, "samples", (start, pos), "audio_ctx", m[3], "checker margins: winner", win, "mass", mass)
                assert win >= MARGIN and mass >= MARGIN, (i, "the session's seeds no longer meet the margin condition", win, mass)
                assert [t[0] for t in m[4]] == toks, (i, "the product's greedy run left the checker's although the margins hold")
        finally:
            chk.close()
    finally:
        leg.close()
    assert len(plain[0]) >= 10 and drafted[0] == plain[0], "the messages differ with draft_reuse"
    assert all(s["reason"] == abi.DRAFT_NONE for s in plain[1])
    st = drafted[1]
    assert st[0]["reason"] == abi.DRAFT_NONE
    msgs = drafted[0]
    # a step starts from nothing behind keep_last (a finished sentence with activity) and behind a result without tokens
    fresh = lambda i: i == 0 or len(msgs[i - 1][4]) == 0 or (msgs[i - 1][0] and not msgs[i - 1][5])
    assert len(st) == len(msgs)
    assert any(fresh(i) for i in range(1, len(st))) and sum(not fresh(i) for i in range(len(st))) >= 6, "the run does not cover both kinds of step"
    for i, s in enumerate(st):
        if fresh(i):
            assert s["reason"] == abi.DRAFT_NONE and s["n_accepted"] == 0, (i, s, "a step behind keep_last carried a draft")
        else:
            assert s["reason"] == abi.DRAFT_USED and s["n_accepted"] > 0, (i, s)

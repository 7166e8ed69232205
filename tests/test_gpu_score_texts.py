"""-m gpu: wmi_score_texts on synthetic micro.en, micro (multilingual prefix), tiny.en and micro.en quantised to q5_1, synth.make_pcm audio.

  (a) token_logprobs equal the judge's value (tests/score_f64.py, bound A) on the logits rows the scorer saw (logits_out); sums, averages and
      posteriors are exactly the judge's float64 recomputation from the returned values
  (b) those logits rows lie within LOGIT_ABS / LOGIT_RMS (tests/test_gpu_parity.py) of whisper_decode on prefix + text as ONE ordinary
      sequence on the product, and for the f16 models of the checker test_gpu_parity.py uses; hence |lp - lp_ref| <= 2 LOGIT_ABS per token
      (the target logit and the denominator move by at most one bound each).  q5_1: that suite's yardstick — max(LOGIT_ABS, 3 x the
      checker's own response to a 1e-6 relative change of the PCM)
  (c) masking on the device: a text alone and among 15 very different ones, in a call of <= 8 rows and in one of > 8 (decode()'s two
      projection forms), in the two-pass call of 30 x 16, and two copies of one text in a call — each within (b)'s bound
  (d) an empty text, with_eot = 0, every error return, -2 on a state without an encoder result
  (e) nothing existing moves: whisper_full's tokens, probabilities and counters before and after a scoring call; the call adds nothing
      to wmi_get_timings; a context that never scores reports zero score calls, launches and time
  (f) wmi_score_pcm equals whisper_pcm_to_mel + whisper_encode + wmi_score_texts bit for bit

Measured figures go to the parity margins through stage_compare.hold.  No test reads the reference checkout."""
import ctypes as C

import numpy as np
import pytest

import score_f64 as sf
import stage_compare as sc
from godot_whisper_amd import abi, synth
from test_gpu_parity import LOGIT_ABS, LOGIT_RMS, make_checker

pytestmark = pytest.mark.gpu

ACTX = 160                                        # a short encoder: the CPU checker stays in seconds
MODELS = {"micro.en": lambda: synth.make_model("micro.en", seed=1234), "micro": lambda: synth.make_model("micro", seed=1234),
          "tiny.en": lambda: synth.make_model("tiny.en", seed=1234),
          "micro.en q5_1": lambda: synth.quantize_model(synth.make_model("micro.en", seed=1234), "q5_1")}


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def params_of(lib, prompt=None, lang_id=0, with_eot=True, length_norm=False):
    p = lib.wmi_score_default_params()
    p.lang_id = lang_id; p.with_eot = int(with_eot); p.length_norm = int(length_norm)
    keep = None
    if prompt is not None and len(prompt):
        keep = np.asarray(prompt, np.int32)
        p.prompt_tokens = keep.ctypes.data_as(C.POINTER(C.c_int32)); p.prompt_n_tokens = keep.size
    return p, keep


def score(prod, texts, want_logits=False, **kw):
    """-> (rc, recs [(sum, avg, posterior, n_scored, first)], lp, logits rows or None)"""
    lib = prod.lib
    p, keep = params_of(lib, **kw)
    toks = np.asarray([t for y in texts for t in y], np.int32)
    nt = np.asarray([len(y) for y in texts], np.int32)
    total = int(sum(len(y) + (1 if kw.get("with_eot", True) else 0) for y in texts))
    out = (abi.wmi_text_score * max(1, len(texts)))()
    lp = np.full(max(1, total), 7.0, np.float32)
    lo = np.full((max(1, total), prod.NV), np.nan, np.float32) if want_logits else None
    rc = lib.wmi_score_texts_with_state(prod.ctx, None, p, vp(toks) if toks.size else None, vp(nt), len(texts), out, vp(lp), vp(lo))
    recs = [(o.sum_logprob, np.float32(o.avg_logprob), np.float32(o.posterior), o.n_scored, o.first) for o in out][:len(texts)]
    return rc, recs, lp[:total], lo


def targets_of(prod, texts, with_eot=True):
    eot = prod.lib.whisper_token_eot(prod.ctx)
    out = []
    for y in texts:
        out += list(y) + ([eot] if with_eot else [])
    return out


def prefix_of(prod, lang_id=0):
    lib = prod.lib
    sot = lib.whisper_token_sot(prod.ctx)
    pre = [sot] + ([sot + 1 + lang_id, lib.whisper_token_transcribe(prod.ctx)] if lib.whisper_is_multilingual(prod.ctx) else [])
    return pre + [lib.whisper_token_not(prod.ctx)]


@pytest.fixture(scope="module")
def pcm():
    return synth.make_pcm(4.0, seed=9)


@pytest.fixture(scope="module")
def sides(product_lib, pcm):
    made = {}

    def get(name):
        if name not in made:
            prod = sc.ProductSide(product_lib, MODELS[name]())
            prod.mel(pcm); prod.encode(0, ACTX)
            made[name] = prod
        return made[name]
    yield get
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def abs_bound(sides, checker_lib, pcm):
    """(b)'s bound on a logit of a model: LOGIT_ABS for the f16 models; for q5_1 the parity suite's yardstick,
    max(LOGIT_ABS, 3 x the checker's own response to a 1e-6 relative change of the PCM), taken once over the rows of one text"""
    made = {}

    def get(name):
        if "q5_1" not in name:
            return LOGIT_ABS
        if name not in made:
            prod = sides(name)
            chks = [make_checker(MODELS[name](), checker_lib) for _ in range(2)]
            try:
                chks[0].mel(pcm); chks[0].encode(0, ACTX)
                chks[1].mel((pcm * np.float32(1.0 + 1e-6)).astype(np.float32)); chks[1].encode(0, ACTX)
                y = texts_for(11, [3])[0]
                pre = prefix_of(prod)
                noise = max(sc.err_stats(chks[1].decode(pre + y[:i], 0), chks[0].decode(pre + y[:i], 0))["max_abs"] for i in range(len(y) + 1))
            finally:
                for c in chks:
                    c.close()
            made[name] = max(LOGIT_ABS, 3.0 * noise)
            print(name, "logit bound from the checker's self-noise:", made[name])
        return made[name]
    return get


def texts_for(seed, lengths):
    rng = np.random.default_rng(seed)
    return [rng.integers(100, 50000, n).tolist() for n in lengths]


def hold_lp_pair(kind, a, b, bound, what):
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), what
    sc.hold(kind, float(np.abs(np.asarray(a, np.float64)[fin] - np.asarray(b, np.float64)[fin]).max()) if fin.any() else 0.0, bound, what)


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("length_norm", [False, True])
def test_values_are_the_judges_on_the_logits_the_scorer_saw(sides, name, length_norm):
    prod = sides(name)
    texts = texts_for(3, [3, 0, 1, 9, 2])
    kw = dict(lang_id=2) if name == "micro" else {}
    rc, recs, lp, lo = score(prod, texts, want_logits=True, length_norm=length_norm, **kw)
    assert rc == 0, rc
    pl = sf.plan(prod.NV, 448, texts, **kw)
    assert [r[4] for r in recs] == pl["first"][:-1] and [r[3] for r in recs] == list(np.diff(pl["first"]))
    tg = targets_of(prod, texts)
    assert not np.isnan(lo).any()
    for i, t in enumerate(tg):
        want = sf.spec_lp(lo[i], t)
        assert sf.judge_lp(lp[i], lo[i], t), (name, i, float(lp[i]), want)
        sc.hold("score texts: f32 ulp from the float64 value on the scorer's own logits (bound A)", sf.ulps_off(lp[i], want), float(sf.ULPS), (name, i))
    for c in range(len(texts)):                                        # every text's first entry comes from ONE row: the prefix's last
        assert np.array_equal(lo[pl["first"][c]], lo[0]), c
    assert sf.judge_texts(recs, lp, pl["first"], length_norm), (name, recs, sf.text_scores(lp, pl["first"], length_norm))
    assert abs(sum(float(r[2]) for r in recs) - 1.0) < 1e-5
    rc2, recs2, lp2, _ = score(prod, texts, length_norm=length_norm, **kw)      # the same call twice, and without the logits beside it
    assert rc2 == 0 and bits(lp2) == bits(lp) and [r[0] for r in recs2] == [r[0] for r in recs] and bits([r[2] for r in recs2]) == bits([r[2] for r in recs])


# ---------------------------------------------------------------------------------------------- (b)
def one_sequence_logits(side, prefix, y):
    """the rows that predict y_0 .. y_{n-1}, <eot>: whisper_decode of prefix + y[:i] as one ordinary sequence, its last row"""
    return [side.decode(prefix + list(y[:i]), 0) for i in range(len(y) + 1)]


@pytest.mark.parametrize("name", list(MODELS))
def test_logits_rows_against_one_ordinary_sequence_and_the_checker(sides, product_lib, checker_lib, pcm, name):
    prod = sides(name)
    kw = dict(lang_id=2) if name == "micro" else {}
    texts = texts_for(5, [3, 2]) + texts_for(6, [2] * 4)              # 6 texts, 13 rows in the candidate pass
    rc, recs, lp, lo = score(prod, texts, want_logits=True, **kw)
    assert rc == 0, rc
    first = sf.plan(prod.NV, 448, texts, **kw)["first"]
    prefix = prefix_of(prod, kw.get("lang_id", 0))
    tg = targets_of(prod, texts)
    quant = "q5_1" in name
    chks = [make_checker(MODELS[name](), checker_lib) for _ in range(2 if quant else 1)]
    try:
        for c in chks:
            c.n_threads = 8
        chks[0].mel(pcm); chks[0].encode(0, ACTX)
        if quant:
            chks[1].mel((pcm * np.float32(1.0 + 1e-6)).astype(np.float32)); chks[1].encode(0, ACTX)
        for c in (0, 1):                                               # two texts row by row
            own = one_sequence_logits(prod, prefix, texts[c])
            ref = one_sequence_logits(chks[0], prefix, texts[c])
            noise = one_sequence_logits(chks[1], prefix, texts[c]) if quant else None
            for i in range(len(texts[c]) + 1):
                g, t = lo[first[c] + i], tg[first[c] + i]
                ab, rm = LOGIT_ABS, LOGIT_RMS
                if quant:
                    n = sc.err_stats(noise[i], ref[i])
                    ab, rm = max(LOGIT_ABS, 3.0 * n["max_abs"]), min(max(LOGIT_RMS, 2.0 * n["rms_rel"]), 5e-2)
                for kind, other in (("one ordinary sequence on the product", own[i]), ("the checker", ref[i])):
                    st = sc.err_stats(g, other)
                    print(name, c, i, kind, st)
                    what = (name, c, i, st)
                    tag = " (quantised: vs the checker's self-noise yardstick)" if quant else ""
                    sc.hold(f"score texts: logits rows vs {kind}, max |d|{tag}", st["max_abs"], ab, what)
                    sc.hold(f"score texts: logits rows vs {kind}, rms-rel{tag}", st["rms_rel"], rm, what)
                    d = abs(float(lp[first[c] + i]) - sf.spec_lp(other, t))
                    print(name, c, i, kind, "|lp - lp_ref|", d)
                    sc.hold(f"score texts: |lp - lp_ref| vs {kind}{tag}", d, 2.0 * ab, what)
    finally:
        for c in chks:
            c.close()


# ---------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("name", list(MODELS))
def test_texts_do_not_see_each_other(sides, abs_bound, name):
    prod = sides(name)
    kw = dict(lang_id=2) if name == "micro" else {}
    bound = 2.0 * abs_bound(name)
    a = texts_for(11, [3])[0]
    rc, _, alone, _ = score(prod, [a], **kw)                           # 4 rows in the pass: the weight-streaming projections
    assert rc == 0
    # <= 8 rows in the pass, another text beside it
    rc, recs, lp, _ = score(prod, [texts_for(12, [2])[0], a], **kw)
    assert rc == 0
    hold_lp_pair("score texts: a text alone vs beside others, |d lp|", lp[recs[1][4]:], alone, bound, (name, "<= 8 rows"))
    # among 15 very different ones: > 8 rows, the tiled projections
    others = texts_for(13, [1, 6, 2, 5, 3, 4, 6, 1, 2, 3, 5, 4, 6, 2, 1])
    many = others[:7] + [a] + others[7:]
    rc, recs, lp, _ = score(prod, many, **kw)
    assert rc == 0
    hold_lp_pair("score texts: a text alone vs beside others, |d lp|", lp[recs[7][4]:recs[7][4] + 4], alone, bound, (name, "> 8 rows"))
    # two copies of one text in a call
    rc, recs, lp, _ = score(prod, [a, others[1], a], **kw)
    assert rc == 0
    hold_lp_pair("score texts: two copies of one text in a call, |d lp|", lp[recs[0][4]:recs[0][4] + 4], lp[recs[2][4]:recs[2][4] + 4], bound, name)
    assert abs(recs[0][0] - recs[2][0]) <= 4 * bound


@pytest.mark.parametrize("name", ["micro.en", "micro.en q5_1"])
def test_two_passes_of_30_texts_of_16(sides, abs_bound, name):
    prod = sides(name)
    bound = 2.0 * abs_bound(name)
    texts = texts_for(21, [16] * 30)
    pl = sf.plan(prod.NV, 448, texts)
    assert len(pl["pass_text0"]) == 3
    rc, recs, lp, _ = score(prod, texts)
    assert rc == 0
    assert sf.judge_texts(recs, lp, pl["first"])
    for c in (0, 27, 28, 29):                                          # the first pass's ends and the second pass's texts
        rc, _, alone, _ = score(prod, [texts[c]])
        assert rc == 0
        hold_lp_pair("score texts: a text alone vs in the two-pass call, |d lp|", lp[pl["first"][c]:pl["first"][c + 1]], alone, bound, (name, c))


# ---------------------------------------------------------------------------------------------- (d)
def test_empty_text_without_eot_and_errors(sides, product_lib):
    prod = sides("micro.en")
    eot = product_lib.whisper_token_eot(prod.ctx)
    texts = texts_for(31, [0, 4])
    rc, recs, lp, lo = score(prod, texts, want_logits=True)
    assert rc == 0 and recs[0][3] == 1 and recs[0][4] == 0 and recs[1][3] == 5 and recs[1][4] == 1
    assert sf.judge_lp(lp[0], lo[0], eot) and recs[0][0] == float(lp[0])           # the empty text: <eot> at the prefix row
    rc, recs0, lp0, lo0 = score(prod, texts[1:], want_logits=True, with_eot=False)
    assert rc == 0 and recs0[0][3] == 4 and len(lp0) == 4
    for i, t in enumerate(texts[1]):
        assert sf.judge_lp(lp0[i], lo0[i], t)
    hold_lp_pair("score texts: with_eot = 0 vs the same rows with <eot>, |d lp|", lp0, lp[1:5], 2.0 * LOGIT_ABS, "with_eot")
    assert sf.judge_texts(recs0, lp0, [0, 4]) and float(recs0[0][2]) == 1.0
    # error returns: nothing is launched, the timer does not move
    us, nc, nl = C.c_int64(), C.c_int32(), C.c_int32()
    product_lib.wmi_get_score_timings(prod.ctx, C.byref(us), C.byref(nc), C.byref(nl))
    before = (us.value, nc.value, nl.value)
    assert score(prod, [[eot]])[0] == -1 and score(prod, [[-1]])[0] == -1
    assert score(prod, [])[0] == -1
    assert score(prod, [[]], with_eot=False)[0] == -1
    assert score(prod, [[5] * 447])[0] == -1 and score(prod, [[5] * 446])[0] == 0
    assert score(prod, [[5] * 223], prompt=list(range(300)))[0] == -1
    assert score(prod, [[5]], prompt=[99999])[0] == -1
    product_lib.wmi_get_score_timings(prod.ctx, C.byref(us), C.byref(nc), C.byref(nl))
    assert nc.value == before[1] + 1                                   # (the one legal call above)
    fresh = sc.ProductSide(product_lib, MODELS["micro.en"]())
    try:
        assert score(fresh, [[5]])[0] == -2                            # no encoder result in the state
        product_lib.wmi_get_score_timings(fresh.ctx, C.byref(us), C.byref(nc), C.byref(nl))
        assert (us.value, nc.value, nl.value) == (0, 0, 0)
    finally:
        fresh.close()


def test_a_prompt_changes_the_prefix_and_is_held_too(sides):
    prod = sides("micro.en")
    texts = texts_for(41, [2, 5])
    prompt = list(range(1000, 1300))
    rc, recs, lp, lo = score(prod, texts, want_logits=True, prompt=prompt)
    assert rc == 0
    pl = sf.plan(prod.NV, 448, texts, prompt=prompt)
    assert len(pl["prefix"]) == 226
    for i, t in enumerate(targets_of(prod, texts)):
        assert sf.judge_lp(lp[i], lo[i], t), i
    assert sf.judge_texts(recs, lp, pl["first"])
    ref = one_sequence_logits(prod, pl["prefix"], texts[1])
    for i in range(6):
        st = sc.err_stats(lo[pl["first"][1] + i], ref[i])
        sc.hold("score texts: logits rows vs one ordinary sequence on the product, max |d|", st["max_abs"], LOGIT_ABS, ("prompt", i, st))
    rc0, _, lp_plain, _ = score(prod, texts)
    assert rc0 == 0 and bits(lp_plain) != bits(lp)


# ---------------------------------------------------------------------------------------------- (e)
def run_full(lib, ctx, pcm):
    p = lib.whisper_full_default_params(abi.WHISPER_SAMPLING_GREEDY)
    p.print_progress = False; p.print_realtime = False; p.print_timestamps = False; p.print_special = False
    lib.whisper_reset_timings(ctx)
    assert lib.whisper_full(ctx, p, fptr(pcm), pcm.size) == 0
    toks = []
    for i in range(lib.whisper_full_n_segments(ctx)):
        for j in range(lib.whisper_full_n_tokens(ctx, i)):
            toks.append((lib.whisper_full_get_token_id(ctx, i, j), np.float32(lib.whisper_full_get_token_p(ctx, i, j)).view(np.uint32).item()))
    t6 = (C.c_int64 * 6)(); n5 = (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return toks, list(n5), list(t6)


@pytest.mark.parametrize("name", ["micro.en", "micro.en q5_1"])
def test_nothing_existing_moves(product_lib, pcm, name):
    lib = product_lib
    prod = sc.ProductSide(lib, MODELS[name]())
    try:
        toks0, n0, _ = run_full(lib, prod.ctx, pcm)
        us, nc, nl = C.c_int64(), C.c_int32(), C.c_int32()
        lib.wmi_get_score_timings(prod.ctx, C.byref(us), C.byref(nc), C.byref(nl))
        assert (us.value, nc.value, nl.value) == (0, 0, 0)             # a context that never scored
        t6 = (C.c_int64 * 6)(); n5 = (C.c_int32 * 5)()
        lib.wmi_get_timings(prod.ctx, t6, n5)
        before = (list(t6), list(n5))
        rc, recs, lp, _ = score(prod, texts_for(51, [3, 1, 12]))       # on whisper_full's encoder result
        assert rc == 0 and np.isfinite(lp).all()
        lib.wmi_get_timings(prod.ctx, t6, n5)
        assert (list(t6), list(n5)) == before                          # nothing in the reference's timers
        lib.wmi_get_score_timings(prod.ctx, C.byref(us), C.byref(nc), C.byref(nl))
        assert nc.value == 1 and us.value > 0 and nl.value == 2 * (1 + 2) + 1      # prefix: 3 items, one chunk; pass: 16 rows, two groups; finish
        toks1, n1, _ = run_full(lib, prod.ctx, pcm)
        assert toks1 == toks0 and n1 == n0
    finally:
        prod.close()


# ---------------------------------------------------------------------------------------------- (f)
def test_score_pcm_is_encode_plus_score_texts(sides, product_lib, pcm):
    lib = product_lib
    prod = sc.ProductSide(lib, MODELS["micro.en"]())
    try:
        texts = texts_for(61, [2, 7, 0, 4])
        toks = np.asarray([t for y in texts for t in y], np.int32); nt = np.asarray([len(y) for y in texts], np.int32)
        total = int(nt.sum()) + len(texts)
        out = (abi.wmi_text_score * len(texts))(); lp = np.zeros(total, np.float32)
        p = lib.wmi_score_default_params()
        assert lib.wmi_score_pcm(prod.ctx, p, vp(pcm), pcm.size, 0, ACTX, vp(toks), vp(nt), len(texts), out, vp(lp)) == 0
        a = ([(o.sum_logprob, o.n_scored, o.first) for o in out], bits([o.avg_logprob for o in out]), bits([o.posterior for o in out]), bits(lp))
        prod.mel(pcm); prod.encode(0, ACTX)
        rc, recs, lp2, _ = score(prod, texts)
        assert rc == 0
        b = ([(r[0], r[3], r[4]) for r in recs], bits([r[1] for r in recs]), bits([r[2] for r in recs]), bits(lp2))
        assert a == b
        assert lib.wmi_score_pcm(prod.ctx, p, vp(pcm), pcm.size, 0, 5000, vp(toks), vp(nt), len(texts), out, vp(lp)) == -1
        assert lib.wmi_score_pcm(prod.ctx, p, None, pcm.size, 0, 0, vp(toks), vp(nt), len(texts), out, vp(lp)) == -1
    finally:
        prod.close()

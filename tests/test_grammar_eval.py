"""The grammar's reject set from csrc/grammar_eval.h — the text k_grammar_reject compiles too — run on the host
(wmi_selftest_grammar, where = 0) on a host-only context, no GPU.

The judge is the host definition the suite already holds to the compiled reference (test_host_logic.py:
test_grammar_penalties_live_against_reference): wmi_process_logits with the grammar and a token history, on raw logits that are
finite everywhere, with no text token banned (suppress_blank and suppress_non_speech_tokens off) and the timestamps 30 below so that
the "timestamp mass beats every text token" rule never fires.  Rejected <=> out_logits[i] == raw[i] - penalty.
"""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import stage_compare as sc
from godot_whisper_amd import abi, host, runtime

RULES = {"colours": gu.colour_list_grammar, "negated": gu.negated_class_grammar, "unicode": gu.unicode_grammar}
# the history texts of test_host_logic.py's grammar test
TEXTS = {"colours": ["", " red", " red,", " red, 12", " red, 120, gre", " blue.", " purple", " red, green, blue, 7"],
         "negated": ["", " hello", " hello world", " café", " 12", " a,b"],
         "unicode": ["", "é", "éβ", "日", "日本ω", "é!", "abc"]}
PENALTY = 57.0


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


def host_ctx(lib, name):
    model, _, _ = gu.case_inputs(name)
    buf = C.create_string_buffer(model, len(model))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(model))
    assert ctx
    return ctx


def histories(lib, ctx, which):
    """test_host_logic.py's histories: tokenised texts, every other unicode one cut inside a multi-byte sequence, number 3 with a
    special token in front"""
    beg = lib.whisper_token_beg(ctx)
    out = []
    for k, text in enumerate(TEXTS[which]):
        buf = (C.c_int32 * 64)()
        n = lib.whisper_tokenize(ctx, text.encode("utf-8"), buf, 64)
        assert n >= 0
        hist = list(buf[:n])
        if which == "unicode" and text and k % 2 == 1:
            hist = hist[:-1] if len(hist) > 1 else hist
        if k == 3:
            hist = [beg + 5] + hist
        out.append(np.asarray(hist, np.int32))
    return out


def grammar_params(lib, node, rules, penalty=PENALTY):
    p = node.full_params("", 0)
    p.suppress_blank = False; p.suppress_non_speech_tokens = False
    ptrs, n_rules, keep = abi.make_grammar(rules)
    p.grammar_rules = C.cast(ptrs, C.c_void_p); p.n_grammar_rules = n_rules; p.i_start_rule = 0; p.grammar_penalty = penalty
    return p, keep


def judge_mask(lib, ctx, p, hist, raw):
    """the reject set by wmi_process_logits"""
    nv = raw.size
    lo, lp, pr = (np.empty(nv, np.float32) for _ in range(3))
    lib.wmi_process_logits(ctx, p, sc._fptr(raw), hist.ctypes.data_as(C.POINTER(C.c_int32)), hist.size, 0, 3000, C.c_float(0.0),
                           sc._fptr(lo), sc._fptr(lp), sc._fptr(pr))
    eot = lib.whisper_token_eot(ctx)
    assert np.all(np.isfinite(lo[:eot])), "a text token was banned: the judge could not see its penalty"
    pen = (raw - np.float32(p.grammar_penalty)).astype(np.float32)
    rej = lo == pen
    assert np.all(rej | (lo == raw) | np.isneginf(lo)), "a logit is neither raw nor raw - penalty"
    return rej.astype(np.uint8)


def selftest_mask(lib, ctx, p, hists, where=0):
    nv = lib.whisper_n_vocab(ctx)
    n = len(hists)
    flat = np.concatenate(hists).astype(np.int32) if sum(h.size for h in hists) else np.zeros(1, np.int32)
    nh = np.asarray([h.size for h in hists], np.int32)
    mask = np.full((n, nv), 7, np.uint8); over = np.full(n, 7, np.uint32)
    rc = lib.wmi_selftest_grammar(ctx, p, where, n, vp(flat), vp(nh), vp(mask), vp(over))
    assert rc == 0, rc
    return mask, over


def same_set(got, want):
    """the comparison the tests rest on: byte for byte"""
    return got.shape == want.shape and bool(np.array_equal(got, want))


@pytest.mark.parametrize("name", ["en30", "ml11"])
@pytest.mark.parametrize("which", ["colours", "negated", "unicode"])
def test_host_evaluator_equals_the_reject_set_of_process_logits(lib, which, name):
    ctx = host_ctx(lib, name)
    node = host.SpeechToText(lib); node.ctx = ctx
    try:
        nv = lib.whisper_n_vocab(ctx); beg = lib.whisper_token_beg(ctx)
        p, keep = grammar_params(lib, node, RULES[which]())
        rng = np.random.default_rng(5)
        counts = []
        for k, hist in enumerate(histories(lib, ctx, which)):
            raw = (rng.standard_normal(nv) * 3.0).astype(np.float32)
            raw[beg:] -= 30.0
            want = judge_mask(lib, ctx, p, hist, raw)
            got, over = selftest_mask(lib, ctx, p, [hist])
            assert over[0] == 0, (which, name, k)
            assert same_set(got[0], want), (which, name, k, int(np.sum(got[0] != want)), np.flatnonzero(got[0] != want)[:8])
            counts.append(int(want.sum()))
            if counts[-1] and counts[-1] < nv:           # the comparison refuses a wrong mask, either way round
                for flip_from in (0, 1):
                    bad = want.copy()
                    bad[np.flatnonzero(want[:lib.whisper_token_eot(ctx)] == flip_from)[0]] ^= 1
                    assert not same_set(bad, got[0])
        print(f"{which}/{name}: rejected per history {counts}")
        # not vacuous: constrained states reject most of the vocabulary, unparsable histories leave no stack and reject nothing
        assert max(counts) > (5000 if which == "negated" else 40000) and min(counts) == 0, counts
        del keep
    finally:
        node.ctx = None
        lib.whisper_free(ctx)


def many_alternatives_grammar(n):
    """root ::= c_0 "x" | c_1 "x" | ...: n alternatives, each beginning with a different character — n stacks at the start"""
    root = []
    for i in range(n):
        root += ([(abi.GRETYPE_ALT, 0)] if i else []) + [(abi.GRETYPE_CHAR, 0x4E00 + i), (abi.GRETYPE_CHAR, ord("x"))]
    return [root]


def test_state_over_capacity_reports_overflow(lib):
    ctx = host_ctx(lib, "en30")
    node = host.SpeechToText(lib); node.ctx = ctx
    try:
        status = abi.wmi_grammar_status()
        assert lib.wmi_grammar_status(ctx, C.byref(status)) == 0
        assert status.cap_stacks > 0 and status.cap_depth > 0 and status.cap_words > 0
        empty = np.zeros(0, np.int32)
        p, keep = grammar_params(lib, node, many_alternatives_grammar(status.cap_stacks + 6))
        mask, over = selftest_mask(lib, ctx, p, [empty])
        assert over[0] == 1 and not mask.any()
        p, keep2 = grammar_params(lib, node, many_alternatives_grammar(status.cap_stacks))      # at the capacity: served
        mask, over = selftest_mask(lib, ctx, p, [empty])
        assert over[0] == 0 and mask.sum() > 40000
        del keep, keep2
    finally:
        node.ctx = None
        lib.whisper_free(ctx)


def test_mode_setter_and_status_without_a_device(lib):
    ctx = host_ctx(lib, "en30")
    try:
        assert lib.wmi_set_grammar_device(None, 1) == -2 and lib.wmi_grammar_status(None, None) == -2
        assert lib.wmi_set_grammar_device(ctx, 1) == 0 and lib.wmi_set_grammar_device(ctx, 5) == 1 and lib.wmi_set_grammar_device(ctx, 0) == 1
        assert lib.wmi_set_grammar_device(ctx, 0) == 0
        status = abi.wmi_grammar_status()
        assert lib.wmi_grammar_status(ctx, C.byref(status)) == 0 and status.steps_device == 0 and status.rows_host == 0
    finally:
        lib.whisper_free(ctx)

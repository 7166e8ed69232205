"""-m gpu: grammar-constrained decoding on the device (wmi_set_grammar_device; csrc/grammar_eval.h, csrc/k_grammar.hip).

  reject kernel     wmi_selftest_grammar(where = 1) — k_grammar_reject — equals where = 0 — the same text on the host, which
                    tests/test_grammar_eval.py holds to wmi_process_logits — byte for byte: every grammar and history of that test on both
                    vocabularies, each history alone and all histories of a grammar as the rows of one launch (grid.y, the per-row state)
  pick and draws    wmi_selftest_grammar_sample on crafted logits against wmi_process_logits (+ wmi_sample_draws) with the same grammar
                    and history on a host-only context: ids exact, p / plog / pt / ptsum within PICK_TOL, the bound tests/test_gpu_filters.py
                    holds the device pick to
  end to end        the grammar parameter sets of tests/test_gpu_parity.py: mode 1 against mode 0 of the same library under that test's
                    rule (equal up to the first near-tie, which lies at or behind token 3; greedy: |dp| <= 2e-2 there), the counters of
                    wmi_grammar_status, the capacity fallback, and mode 0 byte-identical to a context that never heard of the mode

No test reads the reference checkout or oracle/_ref."""
import ctypes as C
import re

import numpy as np
import pytest

import filters_f64 as ff
import golden_util as gu
import stage_compare as sc
from godot_whisper_amd import abi, host, synth
from test_gpu_decode_lengths import PICK_TOL
from test_grammar_eval import RULES, grammar_params, histories, many_alternatives_grammar, selftest_mask, vp

pytestmark = pytest.mark.gpu

FIELDS = ("p", "plog", "pt", "ptsum")
HI = 12.0


# ------------------------------------------------------------------------------------------------ the reject kernel
class Pair:
    """a compute context and a host-only context of one golden case's model"""

    def __init__(self, lib, name):
        model, _, _ = gu.case_inputs(name)
        self.lib = lib
        self.buf = C.create_string_buffer(model, len(model))
        self.ctx = lib.whisper_init_from_buffer_with_params(C.cast(self.buf, C.c_void_p), len(model), abi.whisper_context_params(True))
        self.hctx = lib.wmi_init_host_only(C.cast(self.buf, C.c_void_p), len(model))
        assert self.ctx and self.hctx
        self.node = host.SpeechToText(lib); self.node.ctx = self.hctx

    def close(self):
        self.node.ctx = None
        self.lib.whisper_free(self.ctx); self.lib.whisper_free(self.hctx)


@pytest.fixture(scope="module")
def pairs(product_lib):
    made = {}
    def get(name):
        if name not in made:
            made[name] = Pair(product_lib, name)
        return made[name]
    yield get
    for p in made.values():
        p.close()


@pytest.mark.parametrize("name", ["en30", "ml11"])
@pytest.mark.parametrize("which", ["colours", "negated", "unicode"])
def test_reject_kernel_equals_the_host_evaluator(pairs, which, name):
    pr = pairs(name); lib = pr.lib
    p, keep = grammar_params(lib, pr.node, RULES[which]())
    hists = histories(lib, pr.hctx, which)
    want = [selftest_mask(lib, pr.hctx, p, [h]) for h in hists]
    counts = [int(m.sum()) for m, _ in want]
    assert max(counts) > 5000 and min(counts) == 0 and all(o[0] == 0 for _, o in want), counts
    for k, h in enumerate(hists):                            # each history as a single row
        got, over = selftest_mask(lib, pr.ctx, p, [h], where=1)
        assert over[0] == 0 and np.array_equal(got, want[k][0]), (which, name, k, int(np.sum(got != want[k][0])), np.flatnonzero(got[0] != want[k][0][0])[:8])
    rows = hists[:8]                                         # all of them as the rows of one launch: a different state per row
    got, over = selftest_mask(lib, pr.ctx, p, rows, where=1)
    assert not over.any()
    for r in range(len(rows)):
        assert np.array_equal(got[r], want[r][0][0]), (which, name, "row", r, int(np.sum(got[r] != want[r][0][0])))
    assert len({m.tobytes() for m in got}) >= 2 and got[0].any() and not all(m.any() for m in got) and len(rows) >= 6, "the rows of the launch do not differ"
    del keep


def test_reject_kernel_leaves_an_over_capacity_row_to_the_host(pairs):
    pr = pairs("en30"); lib = pr.lib
    status = abi.wmi_grammar_status()
    assert lib.wmi_grammar_status(pr.ctx, C.byref(status)) == 0
    p, keep = grammar_params(lib, pr.node, many_alternatives_grammar(status.cap_stacks + 6))
    # row 0 at the start (over the capacity), row 1 behind the first character of an alternative (one stack)
    buf = (C.c_int32 * 16)()
    n = lib.whisper_tokenize(pr.hctx, "一".encode("utf-8"), buf, 16)
    assert n > 0
    h1 = np.asarray(list(buf[:n]), np.int32)
    got, over = selftest_mask(lib, pr.ctx, p, [np.zeros(0, np.int32), h1], where=1)
    want1, o1 = selftest_mask(lib, pr.hctx, p, [h1])
    assert list(over) == [1, 0] and o1[0] == 0 and not got[0].any()
    assert np.array_equal(got[1], want1[0]) and want1.sum() > 40000
    del keep


# ------------------------------------------------------------------------------------------------ penalised pick and draws
class Side:
    """micro.en: the compute context, a host-only context (the judge), a parsed history and its reject set"""

    def __init__(self, lib):
        model = synth.make_model("micro.en", seed=1234)
        self.lib = lib
        self.buf = C.create_string_buffer(model, len(model))
        self.ctx = lib.whisper_init_from_buffer_with_params(C.cast(self.buf, C.c_void_p), len(model), abi.whisper_context_params(True))
        assert self.ctx
        self.host = ff.HostSide(lib, model)
        self.v = self.host.v
        self.node = host.SpeechToText(lib); self.node.ctx = self.host.ctx
        self.keep = []

    def close(self):
        self.node.ctx = None
        self.lib.whisper_free(self.ctx); self.host.close()

    def tokens(self, text):
        buf = (C.c_int32 * 64)()
        n = self.lib.whisper_tokenize(self.host.ctx, text.encode("utf-8"), buf, 64)
        assert n > 0
        return np.asarray(list(buf[:n]), np.int32)

    def params(self, penalty=100.0, no_timestamps=False):
        p, keep = grammar_params(self.lib, self.node, RULES["colours"](), penalty)
        p.suppress_blank = True; p.no_timestamps = no_timestamps
        self.keep.append(keep)
        return p

    def rejected(self, p, hist):
        m, over = selftest_mask(self.lib, self.host.ctx, p, [hist])
        assert over[0] == 0
        return m[0].astype(bool)

    def judge(self, p, raw, hist, T):
        """wmi_process_logits with the grammar: (logits, log-probabilities, probabilities)"""
        nv = self.v.n_vocab
        lo, lp, pr = (np.empty(nv, np.float32) for _ in range(3))
        self.lib.wmi_process_logits(self.host.ctx, p, sc._fptr(raw), hist.ctypes.data_as(C.POINTER(C.c_int32)), hist.size, 0, 0, C.c_float(T),
                                    sc._fptr(lo), sc._fptr(lp), sc._fptr(pr))
        return lo, lp, pr

    def sample(self, p, mode, raws, hists, T, u=None, k=1, tid_default=0):
        n = len(raws)
        lg = np.ascontiguousarray(np.stack(raws), np.float32)
        h = np.concatenate(hists).astype(np.int32)
        nh = np.asarray([x.size for x in hists], np.int32)
        z = np.zeros(n, np.int32)
        out = (abi.whisper_token_data * (n * k))()
        uu = None if u is None else np.ascontiguousarray(u, np.float64)
        rc = self.lib.wmi_selftest_grammar_sample(self.ctx, p, mode, n, vp(lg), vp(h), vp(nh), vp(z), vp(z), C.c_float(T),
                                                  None if uu is None else vp(uu), k, tid_default, out)
        assert rc == 0, rc
        return [[(o.id, o.tid, o.p, o.plog, o.pt, o.ptsum) for o in out[r * k:(r + 1) * k]] for r in range(n)]

    def filters(self, p, raw, hist, T):
        """the grammar-free device pick (wmi_selftest_filters mode 0) of the same step"""
        out = (abi.whisper_token_data * 1)()
        nh = np.asarray([hist.size], np.int32); z = np.zeros(1, np.int32)
        rc = self.lib.wmi_selftest_filters(self.ctx, p, 0, 1, vp(np.ascontiguousarray(raw, np.float32)), vp(hist), vp(nh), vp(z), vp(z), C.c_float(T),
                                           None, None, 0, None, None, 1, 0, out)
        assert rc == 0, rc
        o = out[0]
        return (o.id, o.tid, o.p, o.plog, o.pt, o.ptsum)


@pytest.fixture(scope="module")
def side(product_lib):
    s = Side(product_lib)
    yield s
    s.close()


def hold_token(what, got, want):
    """a device token against the host's: ids exact, the four statistics within PICK_TOL (tests/test_gpu_filters.py's bound)"""
    assert got[0] == want[0] and got[1] == want[1], (what, got, want)
    for j, k in enumerate(FIELDS):
        d = abs(got[2 + j] - want[2 + j])
        assert d == d, (what, k, got, want)
        print(f"{d / PICK_TOL:7.3f} of 1  grammar {what}: {k} vs the host filters ({d:.2e} / {PICK_TOL:g})")
        sc.hold(f"grammar sampling: {k} vs the host filters", d, PICK_TOL, what)


def bits(tok):
    return (tok[0], tok[1]) + tuple(np.asarray(tok[2:], np.float32).view(np.uint32).tolist())


def base_row(s, T, seed, ts_shift=-30.0):
    """N(0, 1) noise in the domain behind the temperature division; the timestamps far below, one of them clearly the best"""
    d = np.random.default_rng(seed).standard_normal(s.v.n_vocab)
    d[s.v.beg:] += ts_shift
    d[s.v.beg + 50] += 8.0
    return d


def raw_of(design, T):
    return (design * (T if T > 0 else 1.0)).astype(np.float32)


def sets(s, p, hist):
    rej = s.rejected(p, hist)
    eot = s.v.eot
    r = np.flatnonzero(rej[:eot]); a = np.flatnonzero(~rej[:eot])
    a = np.asarray([i for i in a if len(s.lib.whisper_token_to_str(s.host.ctx, int(i))) > 0])       # (an empty text is never a candidate)
    assert r.size > 1000 and a.size >= 3, (r.size, a.size)
    return r, a


def test_pick_takes_the_accepted_runner_up(side):
    s = side; p = s.params(); hist = s.tokens(" red,")
    r, a = sets(s, p, hist)
    for T in (0.0, 0.5):
        d = base_row(s, T, 1)
        b, ru = int(r[r.size // 2]), int(a[-1])
        d[b] = HI + 3.0; d[ru] = HI                         # the best text token is rejected, the runner-up accepted: ahead of the rest by ~8
        raw = raw_of(d, T)
        lo, lp, pr = s.judge(p, raw, hist, T)
        want = s.host.token(lp, pr, int(np.argmax(pr)))
        assert want[0] == ru and np.sort(lo[np.isfinite(lo)])[-1] - np.sort(lo[np.isfinite(lo)])[-2] >= ff.WIN_GAP
        got = s.sample(p, 0, [raw], [hist], T)[0][0]
        hold_token(f"(a) runner-up, T {T}", got, want)
        assert got[0] == ru and abs(got[3] - float(lp[ru])) <= PICK_TOL       # plog under the PENALISED row
        free = s.filters(p, raw, hist, T)
        assert free[0] == b, "without the grammar the rejected token wins: the case decides nothing"


def test_timestamp_mass_beats_text_leaves_the_grammar_out(side):
    s = side; p = s.params(); hist = s.tokens(" red,")
    r, a = sets(s, p, hist)
    for T in (0.0, 0.5):
        d = base_row(s, T, 2)
        d[int(r[7])] = HI; d[s.v.beg + 60] = HI + 6.0       # the timestamp mass ahead of the best text token by ~6 >= MASS_GAP
        raw = raw_of(d, T)
        lo, lp, pr = s.judge(p, raw, hist, T)
        want = s.host.token(lp, pr, int(np.argmax(pr)))
        assert want[0] == s.v.beg + 60 and np.isneginf(lo[:s.v.beg]).all()
        got = s.sample(p, 0, [raw], [hist], T)[0][0]
        hold_token(f"(b) forced timestamp, T {T}", got, want)
        assert bits(got) == bits(s.filters(p, raw, hist, T)), "not the grammar-free result bit for bit"


def test_every_text_token_rejected_still_picks_the_penalised_arg_max(side):
    s = side; p = s.params(no_timestamps=True); hist = s.tokens(" blue.")       # the grammar is complete: nothing more is accepted
    rej = s.rejected(p, hist)
    eot = s.v.eot
    cand = np.asarray([len(s.lib.whisper_token_to_str(s.host.ctx, i)) > 0 for i in range(eot)])
    assert rej[:eot][cand].all()
    d = base_row(s, 0.0, 3)
    d[eot] = -150.0; d[:eot][~cand] = -150.0                # what the grammar does not penalise stays below the penalised row
    b = int(np.flatnonzero(cand)[31000]); d[b] = HI
    raw = raw_of(d, 0.0)
    lo, lp, pr = s.judge(p, raw, hist, 0.0)
    want = s.host.token(lp, pr, int(np.argmax(pr)))
    assert want[0] == b and lo[b] == np.float32(raw[b] - np.float32(100.0))
    got = s.sample(p, 0, [raw], [hist], 0.0)[0][0]
    hold_token("(c) all rejected", got, want)
    assert got[0] == b and got[0] < s.v.beg and np.isfinite(got[3]) and got[3] > -1.0


def test_exact_ties_take_the_first_index(side):
    s = side; p = s.params(); hist = s.tokens(" red,")
    r, a = sets(s, p, hist)
    a0, a1 = int(a[0]), int(a[-1])
    r_lo, r_hi = int(r[r < a0][-1]) if (r < a0).any() else None, int(r[r > a0][0])
    cases = [("two accepted", {a0: HI, a1: HI}, min(a0, a1)), ("accepted then rejected", {a0: HI, r_hi: HI + 100.0}, a0)]
    if r_lo is not None:
        cases.append(("rejected then accepted", {r_lo: HI + 100.0, a0: HI}, r_lo))
    for name, put, winner in cases:
        d = base_row(s, 0.0, 4)
        for i, val in put.items():
            d[i] = val
        raw = raw_of(d, 0.0)
        lo, lp, pr = s.judge(p, raw, hist, 0.0)
        ids = list(put)
        assert lo[ids[0]] == lo[ids[1]] == np.float32(HI), (name, lo[ids])       # an exact tie on the penalised row
        want = s.host.token(lp, pr, int(np.argmax(pr)))
        assert want[0] == winner, (name, want)
        got = s.sample(p, 0, [raw], [hist], 0.0)[0][0]
        hold_token(f"(d) tie, {name}", got, want)
    assert len(cases) == 3, "no rejected token in front of the first accepted one: one order of the tie is not exercised"


def test_temperature_divides_first_and_penalises_after(side):
    s = side; p = s.params(penalty=3.0); hist = s.tokens(" red,")
    r, a = sets(s, p, hist)
    T = 0.5
    d = base_row(s, T, 5)
    b, ac = int(r[100]), int(a[-1])
    d[b] = HI; d[ac] = HI - 4.0         # divided first: 12 - 3 = 9 beats 8, the rejected token still wins; penalised first: (6 - 3) / 0.5 = 6 loses
    raw = raw_of(d, T)
    lo, lp, pr = s.judge(p, raw, hist, T)
    want = s.host.token(lp, pr, int(np.argmax(pr)))
    assert want[0] == b and lo[b] == np.float32(np.float32(raw[b] / np.float32(T)) - np.float32(3.0))
    got = s.sample(p, 0, [raw], [hist], T)[0][0]
    hold_token("(e) T 0.5, penalty 3", got, want)


def test_draws_return_the_cell_of_the_penalised_cdf(side):
    s = side; p = s.params(penalty=3.0); hist = s.tokens(" red,")
    r, a = sets(s, p, hist)
    for T, k in ((0.5, 1), (1.0, 3)):
        d = base_row(s, T, 6)
        b, a0, a1 = int(r[200]), int(a[0]), int(a[-1])
        d[b] = HI; d[a0] = HI - 2.0; d[a1] = HI - 2.5; d[int(r[-1])] = HI - 1.0
        raw = raw_of(d, T)
        lo, lp, pr = s.judge(p, raw, hist, T)
        drawn = (abi.whisper_token_data * 8)()
        assert s.lib.wmi_sample_draws(s.host.ctx, sc._fptr(pr), sc._fptr(lp), 8, 1, drawn) == 8
        # the crafted tokens and what the host drew; a cell narrower than 1e-4 is not asked for (the device sums carry ~1e-6 of the total)
        targets = sorted(i for i in {int(t.id) for t in drawn} | {b, a0, a1, int(r[-1])} if pr[i] > 1e-4)
        cdf = np.cumsum(pr.astype(np.float64)); total = cdf[-1]
        assert {b, a0, a1, int(r[-1])} <= set(targets), [(i, pr[i]) for i in (b, a0, a1, int(r[-1]))]
        for j0 in range(0, len(targets), k):
            grp = (targets[j0:j0 + k] * k)[:k]
            u = np.asarray([[(cdf[i] - pr[i] / 2.0) / total for i in grp]], np.float64)       # the middle of each cell
            got = s.sample(p, 2, [raw], [hist], T, u=u, k=k, tid_default=s.v.beg if k > 1 else 0)[0]
            for i, g in zip(grp, got):
                hold_token(f"(f) draw of {i}, T {T}, k {k}", g, s.host.token(lp, pr, i, s.v.beg if k > 1 else 0))
        # rows of one launch: a state per row (two histories), the same bits as alone
        h2 = s.tokens(" red, 12")
        u1 = np.asarray([[0.3], [0.6]], np.float64)
        both = s.sample(p, 2, [raw, raw], [hist, h2], T, u=u1, k=1)
        for row, (hh, uu) in enumerate(((hist, 0.3), (h2, 0.6))):
            alone = s.sample(p, 2, [raw], [hh], T, u=np.asarray([[uu]], np.float64), k=1)
            assert bits(both[row][0]) == bits(alone[0][0]), (T, row, both[row][0], alone[0][0])


# ------------------------------------------------------------------------------------------------ end to end
def _params(node, name, rules=None):
    """the `grammar` / `grammar_beam` parameter sets of tests/test_gpu_parity.py"""
    p = node.lib.whisper_full_default_params(abi.WHISPER_SAMPLING_GREEDY)
    p.language = b"en"; p.temperature_inc = 0.0; p.print_progress = False
    ptrs, n_rules, keep = abi.make_grammar(rules if rules is not None else gu.colour_list_grammar())
    node._grammar_keep = keep
    p.grammar_rules = C.cast(ptrs, C.c_void_p); p.n_grammar_rules = n_rules; p.i_start_rule = 0; p.grammar_penalty = 100.0
    p.no_timestamps = True; p.single_segment = True; p.max_tokens = 24
    if name == "grammar_beam":
        p.strategy = abi.WHISPER_SAMPLING_BEAM_SEARCH; p.beam_search.beam_size = 3; p.greedy.best_of = 1
    return p


def _segments(lib, ctx):
    return [(lib.whisper_full_get_segment_t0(ctx, i), lib.whisper_full_get_segment_t1(ctx, i), bytes(lib.whisper_full_get_segment_text(ctx, i)),
             [lib.whisper_full_get_token_id(ctx, i, j) for j in range(lib.whisper_full_n_tokens(ctx, i))]) for i in range(lib.whisper_full_n_segments(ctx))]


def _run(lib, model, pcm, variant, mode, rules=None):
    """mode None: a context that never hears of the mode"""
    node = host.SpeechToText(lib); node.set_language_model(model)
    try:
        if mode is not None:
            assert lib.wmi_set_grammar_device(node.ctx, mode) == 0
        p = _params(node, variant, rules)
        assert lib.whisper_full(node.ctx, p, pcm.ctypes.data_as(C.POINTER(C.c_float)), pcm.size) == 0
        toks = gu.tokens_array([b""] + node.collect()[1:])
        status = abi.wmi_grammar_status()
        assert lib.wmi_grammar_status(node.ctx, C.byref(status)) == 0
        return _segments(lib, node.ctx), toks, (status.steps_device, status.rows_host)
    finally:
        node.close()


def _same_up_to_the_first_near_tie(variant, a, b):
    (sa, ta), (sb, tb) = a, b
    n = min(len(ta), len(tb))
    same = ta[:n, 0] == tb[:n, 0]
    first = n if same.all() else int(np.argmin(same))
    if first < n:
        assert first >= 3, (variant, first, ta[:4, 0], tb[:4, 0])
        if variant != "grammar_beam":
            assert abs(ta[first, 2] - tb[first, 2]) <= 2e-2, (variant, first, ta[first], tb[first])
    else:
        assert len(sa) == len(sb), (variant, len(sa), len(sb))
        for x, y in zip(sa, sb):
            assert x == y, (variant, x, y)
        assert np.abs(ta[:, 2] - tb[:, 2]).max() <= 1e-2
    return first, n


@pytest.fixture(scope="module")
def e2e_inputs():
    return synth.make_model("micro.en", seed=55), synth.make_pcm(20.0, seed=56)


@pytest.mark.parametrize("variant", ["grammar", "grammar_beam"])
def test_device_route_equals_the_host_route(product_lib, e2e_inputs, variant):
    model, pcm = e2e_inputs
    s0, t0, c0 = _run(product_lib, model, pcm, variant, 0)
    s1, t1, c1 = _run(product_lib, model, pcm, variant, 1)
    first, n = _same_up_to_the_first_near_tie(variant, (s0, t0), (s1, t1))
    print(f"{variant}: {n} tokens, equal up to {first}; device steps {c1[0]}, host rows {c1[1]}")
    text = b"".join(a[2] for a in s1).decode()
    assert re.fullmatch(r" ?((red|green|blue|[0-9]+)(, (red|green|blue|[0-9]+))*\.?|(red|green|blue|[0-9]+, )*(r|re|g|gr|gre|gree|b|bl|blu)?)?", text) or \
           re.match(r" ?(red|green|blue|[0-9]+)", text), text
    assert c1[0] > 0 and c1[1] == 0, c1
    assert c0 == (0, 0)
    # mode 0 is byte for byte a context that never heard of the mode
    sn, tn, cn = _run(product_lib, model, pcm, variant, None)
    assert cn == (0, 0) and sn == s0 and tn.tobytes() == t0.tobytes()


def test_over_capacity_grammar_falls_back_to_the_host_and_stays_exact(product_lib, e2e_inputs):
    model, pcm = e2e_inputs
    status = abi.wmi_grammar_status()
    assert product_lib.wmi_grammar_status(None, C.byref(status)) == -2
    probe = host.SpeechToText(product_lib); probe.set_language_model(model)
    assert product_lib.wmi_grammar_status(probe.ctx, C.byref(status)) == 0 and status.cap_stacks > 0
    probe.close()
    rules = many_alternatives_grammar(status.cap_stacks + 6)
    s0, t0, c0 = _run(product_lib, model, pcm, "grammar", 0, rules)
    s1, t1, c1 = _run(product_lib, model, pcm, "grammar", 1, rules)
    first, n = _same_up_to_the_first_near_tie("grammar", (s0, t0), (s1, t1))
    print(f"over capacity: {n} tokens, equal up to {first}; device steps {c1[0]}, host rows {c1[1]}")
    assert c1[1] > 0 and c0 == (0, 0), (c0, c1)

"""The judge of the text scorer (tests/score_f64.py) refuses wrong answers, the defined form sits within bound B of the plain float64
log-soft-max, and csrc/score.cpp's plan (wmi_selftest_score_plan, on a host-only context: no device) is the plan restated there —
prefixes of 2 and 4 rows and with 0 / 3 / 300 prompt tokens, 1 / 2 / 16 texts of 0, 1, 2 and 9 tokens, 7 / 8 / 9 rows in all, 30 texts of
16 tokens (two passes, every text whole), every error return; in every plan no row of a text can see a cell of another text and every
row sees the whole prefix."""
import ctypes as C
import math

import numpy as np
import pytest

import score_f64 as sf
from godot_whisper_amd import abi, runtime, synth

NV = 51864


def rows_of(seed=3, n=4, nv=NV):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(nv) * 4.0).astype(np.float32) for _ in range(n)]


def f32(x):
    return np.float32(x)


# ---------------------------------------------------------------------------------------------- the judge, per value
def test_the_definition_is_accepted_and_within_bound_b_of_the_plain_form():
    rng = np.random.default_rng(1)
    for l in rows_of():
        for t in (0, 127, 128, NV - 1, int(rng.integers(NV))):
            want = sf.spec_lp(l, t)
            assert sf.judge_lp(f32(want), l, t)
            assert abs(want - sf.exact_lp(l, t)) <= sf.bound_b(l, t), (t, want, sf.exact_lp(l, t))
    l = np.full(NV, np.float32(1.25))
    assert abs(sf.spec_lp(l, 5) + math.log(NV)) < 1e-12 and sf.judge_lp(f32(-math.log(NV)), l, 5)
    l = np.full(NV, -np.inf, np.float32); l[77] = 3.0
    assert sf.spec_lp(l, 77) == 0.0 and sf.judge_lp(f32(0.0), l, 77) and not sf.judge_lp(f32(-1e-7), l, 77)
    assert sf.spec_lp(l, 78) == -math.inf and sf.judge_lp(f32(-np.inf), l, 78) and not sf.judge_lp(f32(-1e30), l, 78)
    assert not sf.judge_lp(f32(np.nan), rows_of()[0], 3)


def test_wrong_values_are_refused():
    rows = rows_of()
    l, t = rows[0], 1000
    good = sf.spec_lp(l, t)
    assert not sf.judge_lp(f32(sf.spec_lp(l, t + 1)), l, t)                       # a target one column off
    lm = l.copy(); lm[int(l.argmax())] = -np.inf
    assert not sf.judge_lp(f32(float(l[t] - sf.spec_parts(l)[0]) - math.log(sf.spec_parts(lm)[1])), l, t)      # the maximum left out of the sum
    li = l.copy(); li[::7] = -np.inf; li[t] = l[t]
    M, S = sf.spec_parts(li)
    wrong = float(f32(li[t] - M)) - math.log(S + float((li == -np.inf).sum()))    # -inf entries counted (as exp(0) each)
    assert sf.judge_lp(f32(sf.spec_lp(li, t)), li, t) and not sf.judge_lp(f32(wrong), li, t)
    M1, S1 = sf.spec_parts(rows[1])
    assert not sf.judge_lp(f32(float(f32(l[t] - M1)) - math.log(S1)), l, t)       # a row's denominator taken from its neighbour
    # sums in f32: a left-to-right f32 denominator over the whole vocabulary
    with np.errstate(over="ignore"):
        e = np.exp((l - l.max()).astype(np.float32), dtype=np.float32)
        s32 = np.cumsum(e, dtype=np.float32)[-1]
    assert not sf.judge_lp(f32(np.log(e[t] / s32, dtype=np.float32)), l, t)
    assert sf.judge_lp(f32(good), l, t)


# ---------------------------------------------------------------------------------------------- the judge, per text
def test_wrong_text_sums_and_posteriors_are_refused():
    rng = np.random.default_rng(2)
    first = [0, 3, 4, 9, 10]
    lp = (-rng.uniform(0.5, 12.0, first[-1])).astype(np.float32)
    good = sf.text_scores(lp, first)
    assert sf.judge_texts(good, lp, first)
    assert abs(sum(float(g[2]) for g in good) - 1.0) < 1e-6

    def with_sums(sums):
        vmax = max(sums); den = sum(math.exp(v - vmax) for v in sums)
        return [(s, f32(s / g[3]), f32(math.exp(s - vmax) / den), g[3], g[4]) for s, g in zip(sums, good)]

    # a text's sum taken over the next text's rows
    nxt = [sum(float(x) for x in lp[first[min(c + 1, 3)]:first[min(c + 1, 3) + 1]]) for c in range(4)]
    assert not sf.judge_texts(with_sums(nxt), lp, first)
    # the prefix row's lp credited to text 0 only: the other texts lose their first entry
    cred = [sum(float(x) for x in lp[first[c] + (1 if c else 0):first[c + 1]]) for c in range(4)]
    assert not sf.judge_texts(with_sums(cred), lp, first)
    # <eot> not scored: every text loses its last entry (and its count)
    no_eot = [(sum(float(x) for x in lp[first[c]:first[c + 1] - 1]), g[1], g[2], g[3] - 1, g[4]) for c, g in enumerate(good)]
    assert not sf.judge_texts(no_eot, lp, first)
    # sums added in f32
    big = (-rng.uniform(0.5, 12.0, 400)).astype(np.float32)
    fb = [0, 399, 400]
    s32 = [float(np.cumsum(big[fb[c]:fb[c + 1]], dtype=np.float32)[-1]) for c in range(2)]
    gb = sf.text_scores(big, fb)
    assert s32[0] != gb[0][0]
    assert not sf.judge_texts([(s32[c], gb[c][1], gb[c][2], gb[c][3], gb[c][4]) for c in range(2)], big, fb)
    # length_norm is another posterior
    assert not sf.judge_texts(good, lp, first, length_norm=True) and sf.judge_texts(sf.text_scores(lp, first, True), lp, first, True)


def test_all_texts_minus_infinity_give_zero_posteriors_not_nan():
    first = [0, 2, 3]
    lp = np.array([-1.0, -np.inf, -np.inf], np.float32)
    good = sf.text_scores(lp, first)
    assert [float(g[2]) for g in good] == [0.0, 0.0] and all(g[0] == -math.inf for g in good)
    nan = [(g[0], g[1], f32(np.nan), g[3], g[4]) for g in good]
    assert sf.judge_texts(good, lp, first) and not sf.judge_texts(nan, lp, first)
    lp2 = np.array([-1.0, -np.inf, -2.0], np.float32)
    g2 = sf.text_scores(lp2, first)
    assert float(g2[0][2]) == 0.0 and float(g2[1][2]) == 1.0


# ---------------------------------------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def host_ctx():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    out = {}
    for name in ("micro.en", "micro"):
        mb = synth.make_model(name, seed=1)
        buf = C.create_string_buffer(mb, len(mb))
        ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(mb))
        assert ctx
        out[name] = (ctx, buf)
    yield lib, out
    for ctx, _ in out.values():
        lib.whisper_free(ctx)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def hook_plan(lib, ctx, texts, prompt=(), lang_id=0, translate=False, with_eot=True, n_tokens=None):
    p = lib.wmi_score_default_params()
    pr = np.asarray(prompt, np.int32)
    p.lang_id = lang_id; p.translate = int(translate); p.with_eot = int(with_eot)
    if pr.size:
        p.prompt_tokens = pr.ctypes.data_as(C.POINTER(C.c_int32)); p.prompt_n_tokens = pr.size
    toks = np.asarray([t for y in texts for t in y], np.int32)
    nt = np.asarray([len(y) for y in texts] if n_tokens is None else n_tokens, np.int32)
    cap = 16384
    prefix = np.full(512, -9, np.int32); first = np.full(len(texts) + 1, -9, np.int32); ptg = np.full(max(1, len(texts)), -9, np.int32)
    rows = np.full((cap, 7), -9, np.int32); p0 = np.full(64, -9, np.int32)
    n_prefix, n_rows = C.c_int(-1), C.c_int(-1)
    rc = lib.wmi_selftest_score_plan(ctx, p, vp(toks) if toks.size else None, vp(nt), len(texts), vp(prefix), prefix.size, C.byref(n_prefix), vp(first),
                                     vp(ptg), vp(rows), cap, C.byref(n_rows), vp(p0), p0.size)
    if rc < 0:
        return None
    return dict(prefix=prefix[:n_prefix.value].tolist(), first=first.tolist(), prefix_target=ptg[:len(texts)].tolist(),
                rows=[tuple(r) for r in rows[:n_rows.value].tolist()], pass_text0=p0[:rc + 1].tolist())


def texts_of(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 50000, n).tolist() for n in lengths]


def check_isolation(pl):
    P = len(pl["prefix"])
    for ip in range(len(pl["pass_text0"]) - 1):
        cells = sf.plan_cells(pl, ip)
        for r in (r for r in pl["rows"] if r[0] == ip):
            seen = [c for c in cells if sf.sees(c[0], c[1], r[3], r[2])]
            assert sum(1 for c in seen if c[2] == -1) == P                              # the whole prefix
            assert all(c[2] in (-1, r[3] - 1) for c in seen)                             # and no cell of another text
            assert sum(1 for c in seen if c[2] == r[3] - 1) == r[2] - P + 1              # its own rows up to itself


PLAN_CASES = [
    ("micro.en", [[1]], {}), ("micro.en", [[]], {}), ("micro.en", [[1, 2]], {}), ("micro.en", [list(range(9))], {}),
    ("micro.en", texts_of([0, 1]), {}), ("micro.en", texts_of([2, 9]), {}), ("micro.en", texts_of([0, 1, 2, 9] * 4), {}),
    ("micro.en", texts_of([3, 2]), {}),            # 7 rows in all (5 + the 2 prefix items)
    ("micro.en", texts_of([3, 3]), {}),            # 8
    ("micro.en", texts_of([4, 3]), {}),            # 9, and 7 rows in the candidate pass
    ("micro.en", texts_of([4, 4]), {}), ("micro.en", texts_of([5, 4]), {}),      # 8 and 9 rows in the candidate pass
    ("micro.en", texts_of([3, 4]), dict(with_eot=False)),
    ("micro.en", texts_of([1, 1, 5]), dict(with_eot=False)),
    ("micro.en", texts_of([16] * 30), {}),         # 480 rows > n_text_ctx: two passes
    ("micro.en", texts_of([2, 9]), dict(prompt=[11, 12, 13])), ("micro.en", texts_of([2, 9]), dict(prompt=list(range(300)))),
    ("micro", texts_of([0, 1, 2, 9]), dict(lang_id=2)), ("micro", texts_of([2, 9]), dict(lang_id=0, translate=True, prompt=[5, 6, 7])),
    ("micro", texts_of([16] * 30), dict(prompt=list(range(300)))),
]


@pytest.mark.parametrize("i_case", range(len(PLAN_CASES)))
def test_the_plan_is_the_restated_plan(host_ctx, i_case):
    lib, ctxs = host_ctx
    name, texts, kw = PLAN_CASES[i_case]
    nv = synth.SHAPES[name][0]
    got = hook_plan(lib, ctxs[name][0], texts, **kw)
    want = sf.plan(nv, synth.SHAPES[name][5], texts, **kw)
    assert want is not None and got == want, (name, kw)
    assert len(got["prefix"]) == (4 if nv > NV else 2) + (0 if not kw.get("prompt") else 1 + min(len(kw["prompt"]), 223))
    n_scored = [(len(y) + 1 if kw.get("with_eot", True) else len(y)) for y in texts]
    assert got["first"] == np.concatenate([[0], np.cumsum(n_scored)]).tolist()
    if len(texts) == 30:
        assert len(got["pass_text0"]) == 3 and got["pass_text0"][1] == 448 // 16
        for ip in range(2):                                                              # every text whole, at most n_text_ctx rows
            assert sum(1 for r in got["rows"] if r[0] == ip) <= 448
        assert {r[3] for r in got["rows"] if r[0] == 0}.isdisjoint({r[3] for r in got["rows"] if r[0] == 1})
    check_isolation(got)
    # places: every entry of the per-token results is written exactly once
    places = sorted(got["first"][:-1] + [r[6] for r in got["rows"]])
    assert places == list(range(got["first"][-1]))


def test_plan_errors(host_ctx):
    lib, ctxs = host_ctx
    en, ml = ctxs["micro.en"][0], ctxs["micro"][0]
    assert hook_plan(lib, en, [[1, 2]]) is not None
    assert hook_plan(lib, en, []) is None                                    # n_texts < 1
    assert hook_plan(lib, en, [[50256]]) is None                             # an id >= eot
    assert hook_plan(lib, en, [[-1]]) is None
    assert hook_plan(lib, ml, [[50256]], lang_id=0) is not None and hook_plan(lib, ml, [[50257]]) is None
    assert hook_plan(lib, en, [[]], with_eot=False) is None                  # an empty text without <eot>
    assert hook_plan(lib, en, [[1] * 446]) is not None and hook_plan(lib, en, [[1] * 447]) is None      # longer than n_text_ctx - P
    assert hook_plan(lib, en, [[1] * 222], prompt=list(range(300))) is not None and hook_plan(lib, en, [[1] * 223], prompt=list(range(300))) is None
    assert hook_plan(lib, en, [[1]], n_tokens=[-1]) is None
    assert hook_plan(lib, ml, [[1]], lang_id=99) is None and hook_plan(lib, ml, [[1]], lang_id=-1) is None
    assert hook_plan(lib, en, [[1]], prompt=[60000]) is None
    assert sf.plan(NV, 448, [[1] * 447]) is None and sf.plan(NV, 448, [[]], with_eot=False) is None and sf.plan(NV, 448, [[50256]]) is None
    # the compute entry points on a context without a compute path
    out = (abi.wmi_text_score * 1)()
    nt = np.array([1], np.int32); tk = np.array([1], np.int32)
    assert lib.wmi_score_texts(en, lib.wmi_score_default_params(), vp(tk), vp(nt), 1, out, None) == -2
    assert lib.wmi_score_texts(None, lib.wmi_score_default_params(), vp(tk), vp(nt), 1, out, None) == -1

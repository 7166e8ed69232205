"""The float64 judge of the no-speech probability (tests/no_speech_f64.py) on the CPU: it accepts the definition's own value rounded to
f32, stays next to the plain float64 soft-max, and REFUSES the wrong answers a kernel or a driver could give — so that the GPU tests,
which hold the kernels to it, would see them.  Then the driver's rule (wmi_selftest_no_speech_rule) over its whole table, and the
accessors on a context that has never computed."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import no_speech_f64 as nf
from godot_whisper_amd import abi, runtime, synth


@pytest.fixture(scope="module")
def cases():
    return {nv: dict(nf.make_cases(nv)) for nv in nf.VOCABS}


@pytest.mark.parametrize("nv", nf.VOCABS)
def test_judge_accepts_the_definition_and_knows_the_exact_cases(cases, nv):
    nosp = nf.nosp_of(nv)
    for name, l in cases[nv].items():
        want = nf.spec_p(l, nosp)
        assert want == 0.0 or want >= 1e-30, (name, want)
        assert nf.judge(np.float32(want), l, nosp), name
        if 0.0 < want < 1.0:                                   # three ulp away is refused, on either side
            for k in (-3, 3):
                off = np.float32(want) + np.float32(k) * np.spacing(np.float32(want))
                assert not nf.judge(off, l, nosp), (name, k)
    assert nf.spec_p(cases[nv]["all equal"], nosp) == 1.0 / nv
    assert nf.spec_p(cases[nv]["nosp -inf"], nosp) == 0.0 and nf.spec_p(cases[nv]["only nosp finite"], nosp) == 1.0
    assert not nf.judge(np.float32(np.nan), cases[nv]["normal"], nosp) and not nf.judge(np.float32(1e-45), cases[nv]["nosp -inf"], nosp)
    # integer-valued logits: every f32 difference is exact, a shift changes nothing
    a, b, c = (nf.spec_p(cases[nv][k], nosp) for k in ("integers", "integers + 30000", "integers - 30000"))
    assert a == b == c and a > 0.0


@pytest.mark.parametrize("nv", nf.VOCABS)
def test_the_f32_differences_of_the_definition_stay_next_to_the_plain_float64_soft_max(cases, nv):
    """ln p = (l[nosp] - M) - ln S.  The f32 difference of the numerator is off by at most half an f32 ulp of |l[nosp] - M|; every term of
    S carries a relative error of at most half an f32 ulp of its own difference (twice: block maximum, then row maximum), and the terms
    that matter have small differences — bounded here by the numerator's bound again."""
    nosp = nf.nosp_of(nv)
    for name, l in cases[nv].items():
        s, e = nf.spec_p(l, nosp), nf.exact_p(l, nosp)
        if s == 0.0 or e == 0.0:
            assert s == e, name
            continue
        fin = l[l != -np.inf]
        spread = float(fin.max()) - float(fin.min())
        bound = 3.0 * float(np.spacing(np.float32(max(spread, 1.0)))) / 2.0 + 1e-12
        assert abs(math.log(s) - math.log(e)) <= bound, (name, s, e, bound)


@pytest.mark.parametrize("nv", nf.VOCABS)
def test_judge_refuses_the_wrong_answers(cases, nv):
    nosp = nf.nosp_of(nv); c = cases[nv]
    # a soft-max over the filtered logits: the static ban takes <|nospeech|> itself
    for name in ("normal", "all equal", "nosp the maximum by 20", "maximum at the last entry"):
        assert not nf.judge(nf.wrong_filtered(c[name], nosp), c[name], nosp), name
    # the last prompt row instead of the <sot> row
    rows = np.stack([c["normal"], c["flat random"], c["nosp the maximum by 20"]])
    assert nf.judge(np.float32(nf.spec_p(rows[0], nosp)), rows[0], nosp) and not nf.judge(nf.wrong_row(rows, nosp), rows[0], nosp)
    # a left-to-right f32 sum: behind the row's large terms, each of the ~50 000 small ones is rounded against the running sum's ulp
    assert not nf.judge(nf.wrong_f32_sum(c["normal"], nosp), c["normal"], nosp)
    assert nf.ulps_off(nf.wrong_f32_sum(c["normal"], nosp), nf.spec_p(c["normal"], nosp)) > 8
    # a missing last partial block: 1 / (n - n % 128) instead of 1 / n, and a maximum that lives there
    assert nv % nf.BLOCK != 0
    for name in ("all equal", "flat random", "maximum at the last entry"):
        assert not nf.judge(nf.wrong_missing_last_block(c[name], nosp), c[name], nosp), name
    # a maximum taken over the first block only: the float64 exp overflows where the row's maximum is 800 above it
    w = nf.wrong_first_block_max(c["maximum at the last entry"], nosp)
    assert w != w and not nf.judge(w, c["maximum at the last entry"], nosp)
    step = np.where(np.arange(nv) < nf.BLOCK, 0.0, 1000.0).astype(np.float32)
    assert nf.judge(np.float32(nf.spec_p(step, nosp)), step, nosp) and not nf.judge(nf.wrong_first_block_max(step, nosp), step, nosp)


# ---------------------------------------------------------------------------------------------- the driver's rule
EMIT, FALLBACK, DROP, GATE = range(4)


def test_rule_over_the_whole_table():
    lib = runtime.load_library()
    thold, lp_thold = 0.6, -1.0
    for mode, p, failed, avg in itertools.product(range(4), (0.59, 0.61), (0, 1), (-1.5, -0.5)):
        got = lib.wmi_selftest_no_speech_rule(mode, C.c_float(p), C.c_float(thold), failed, C.c_double(avg), C.c_float(lp_thold))
        poor = bool(failed) or avg < lp_thold
        silent = p > thold
        if mode == 3 and silent:
            want = GATE
        elif mode == 2 and silent:
            want = DROP if poor else EMIT                     # never a fallback for a window that says "no speech"
        else:
            want = FALLBACK if poor else EMIT                 # modes 0 and 1, and every window at or below the threshold
        assert got == want, (mode, p, failed, avg, got, want)
    # the comparisons are strict: p == thold is not silent, avg == logprob_thold is not poor
    f = lambda mode, p, avg: lib.wmi_selftest_no_speech_rule(mode, C.c_float(p), C.c_float(0.5), 0, C.c_double(avg), C.c_float(-1.0))
    assert f(3, 0.5, 0.0) == EMIT and f(2, 0.5, -2.0) == FALLBACK and f(2, 0.75, -1.0) == EMIT and f(2, 0.75, -1.0000001) == DROP


def test_accessors_on_a_context_that_has_not_computed():
    lib = runtime.load_library()
    model = synth.make_model("micro.en", seed=1)
    buf = C.create_string_buffer(model, len(model))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(model))
    assert ctx
    try:
        w = abi.wmi_window()
        assert lib.wmi_full_n_windows(ctx) == 0 and lib.wmi_full_get_window(ctx, 0, C.byref(w)) == -1
        assert lib.wmi_full_get_segment_no_speech_prob(ctx, 0) == -1.0 and lib.wmi_full_get_segment_no_speech_prob(ctx, -1) == -1.0
        assert lib.wmi_set_no_speech(ctx, 3) == 0 and lib.wmi_set_no_speech(ctx, 9) == 3 and lib.wmi_set_no_speech(ctx, -4) == 3
        assert lib.wmi_set_no_speech(ctx, 0) == 0                # (out-of-range values were clamped to 3 and 0)
        assert lib.wmi_full_n_windows(ctx) == 0
    finally:
        lib.whisper_free(ctx)
    assert lib.wmi_set_no_speech(None, 1) == -2 and lib.wmi_full_n_windows(None) == 0
    assert lib.wmi_full_n_windows_from_state(None) == 0 and lib.wmi_full_get_segment_no_speech_prob_from_state(None, 0) == -1.0
    assert lib.wmi_full_get_window_from_state(None, 0, C.byref(abi.wmi_window())) == -1


def test_kernel_hook_refuses_bad_arguments_before_the_device():
    lib = runtime.load_library()
    z = np.zeros(256, np.float32); p = np.zeros(16, np.float32); W = np.zeros((256, 8), np.uint16)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    f = lambda form, rows, nv, nosp, lg, W_, x, K: lib.wmi_selftest_no_speech(0, form, rows, nv, nosp, vp(lg), vp(W_), vp(x), K, None, vp(p))
    assert f(2, 1, 256, 3, z, None, None, 0) == -1 and f(1, 0, 256, 3, z, None, None, 0) == -1 and f(1, 17, 256, 3, z, None, None, 0) == -1
    assert f(1, 1, 256, 256, z, None, None, 0) == -1 and f(1, 1, 256, -1, z, None, None, 0) == -1 and f(1, 1, 65537, 3, z, None, None, 0) == -1
    assert f(1, 1, 256, 3, None, None, None, 0) == -1
    assert f(0, 1, 256, 3, None, None, z, 8) == -1 and f(0, 1, 256, 3, None, W, None, 8) == -1
    assert f(0, 1, 256, 3, None, W, z, 12) == -1 and f(0, 1, 256, 3, None, W, z, 1544) == -1 and f(0, 1, 256, 3, None, W, z, 0) == -1
    assert lib.wmi_selftest_no_speech(0, 1, 1, 256, 3, vp(z), None, None, 0, None, None) == -1

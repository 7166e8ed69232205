"""-m gpu: the scoring kernels (csrc/k_score.hip) on crafted logits, through wmi_selftest_score_rows.

  vocabularies  1, 127, 128, 129, 51864, 51865, 51866 and 65536 entries; 1, 7, 8, 9 and 17 rows (the hook groups them by 8 as decode() does)
  targets       0, n_vocab - 1 and both sides of a block edge
  cases         all logits equal (lp = -ln n_vocab), one dominant logit, target -inf (exactly -inf), everything but the target -inf
                (exactly 0), integer logits shifted by +-30000 (the bits of the unshifted ones), normal rows
  every value is held to the judge (tests/score_f64.py, bound A: 2 f32 ulp of the float64 value of the definition); every row of a
  multi-row call is bit for bit what it gives alone; the same call twice gives the same bits.

No test reads the reference checkout or oracle/_ref."""
import ctypes as C
import math

import numpy as np
import pytest

import score_f64 as sf
import stage_compare as sc

pytestmark = pytest.mark.gpu

VOCABS = (1, 127, 128, 129, 51864, 51865, 51866, 65536)
ROWS = (1, 7, 8, 9, 17)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def score(lib, rows, targets):
    lg = np.ascontiguousarray(np.stack(rows), np.float32)
    tg = np.ascontiguousarray(targets, np.int32)
    lp = np.full(lg.shape[0], 7.0, np.float32)
    rc = lib.wmi_selftest_score_rows(0, lg.shape[0], lg.shape[1], vp(lg), vp(tg), vp(lp))
    assert rc == 0, rc
    return lp


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def targets_of(nv):
    """0, the last entry and both sides of a block edge (the first edge and the last one inside the vocabulary)"""
    t = {0, nv - 1}
    for e in (sf.BLOCK, ((nv - 1) // sf.BLOCK) * sf.BLOCK):
        if 0 < e < nv:
            t |= {e - 1, e}
    return sorted(t)


def hold_lp(got, l, t, what):
    want = sf.spec_lp(l, t)
    assert sf.judge_lp(got, l, t), (what, float(got), want, sf.ulps_off(got, want))
    sc.hold("score rows: f32 ulp from the float64 value (bound A)", sf.ulps_off(got, want), float(sf.ULPS), what)


def make_cases(nv, t, seed=7):
    """[(name, logits)] for target t: every expected lp is -inf, 0, or at least 1e-3 in size (score_f64: bound A)"""
    rng = np.random.default_rng(seed + nv + 31 * t)
    out = [("all equal", np.full(nv, np.float32(1.25)))]
    v = rng.standard_normal(nv).astype(np.float32); v[(t + nv // 2) % nv] = np.float32(12.0)
    out.append(("one dominant logit", v))
    v = (rng.standard_normal(nv) * 6.0).astype(np.float32); v[t] = -np.inf
    out.append(("target -inf", v))
    v = np.full(nv, -np.inf, np.float32); v[t] = np.float32(-3.5)
    out.append(("only the target finite", v))
    ints = rng.integers(-20, 21, nv).astype(np.float32)
    out += [("integers", ints), ("integers + 30000", (ints + np.float32(30000.0)).astype(np.float32)),
            ("integers - 30000", (ints - np.float32(30000.0)).astype(np.float32))]
    out.append(("normal", (rng.standard_normal(nv) * 6.0).astype(np.float32)))
    return out


@pytest.mark.parametrize("nv", VOCABS)
def test_every_case_at_every_target(product_lib, nv):
    for t in targets_of(nv):
        got = {}
        for name, l in make_cases(nv, t):
            lp = score(product_lib, [l], [t])
            hold_lp(lp[0], l, t, (nv, t, name))
            assert bits(score(product_lib, [l], [t])) == bits(lp), (nv, t, name)          # the same call twice
            got[name] = lp[0]
        assert got["target -inf"] == -np.inf and got["only the target finite"] == 0.0, (nv, t)
        assert sf.ulps_off(got["all equal"], -math.log(nv)) <= sf.ULPS, (nv, t)
        assert bits([got["integers"]] * 2) == bits([got["integers + 30000"], got["integers - 30000"]]), (nv, t)


@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("nv", (129, 51864, 51865, 65536))
def test_rows_of_one_call_equal_the_rows_alone(product_lib, nv, n_rows):
    ts = targets_of(nv)
    rows, tg = [], []
    for r in range(n_rows):
        t = ts[r % len(ts)]
        cs = make_cases(nv, t)
        rows.append(cs[(3 * r + n_rows) % len(cs)][1]); tg.append(t)
    got = score(product_lib, rows, tg)
    assert bits(score(product_lib, rows, tg)) == bits(got), (nv, n_rows)
    for r in range(n_rows):
        assert bits(score(product_lib, [rows[r]], [tg[r]])) == bits(got[r:r + 1]), (nv, n_rows, r)
        hold_lp(got[r], rows[r], tg[r], (nv, n_rows, r))


def test_one_row_many_targets_and_bad_arguments(product_lib):
    """the prefix row's form: the same logits under different targets, each what it gives alone; argument errors before the device"""
    nv = 51865
    l = make_cases(nv, 0)[-1][1]
    tg = [0, 5, 127, 128, 50257, nv - 1, 300, 4000, 129]
    got = score(product_lib, [l] * len(tg), tg)
    for r, t in enumerate(tg):
        assert bits(score(product_lib, [l], [t])) == bits(got[r:r + 1]), t
        hold_lp(got[r], l, t, ("one row", t))
    lp = np.zeros(1, np.float32); z = np.zeros(8, np.float32); t = np.zeros(1, np.int32)
    f = product_lib.wmi_selftest_score_rows
    assert f(0, 0, 8, vp(z), vp(t), vp(lp)) == -1 and f(0, 1, 0, vp(z), vp(t), vp(lp)) == -1 and f(0, 1, 65537, vp(z), vp(t), vp(lp)) == -1
    assert f(0, 1, 8, None, vp(t), vp(lp)) == -1 and f(0, 1, 8, vp(z), None, vp(lp)) == -1 and f(0, 1, 8, vp(z), vp(t), None) == -1
    t[0] = 8
    assert f(0, 1, 8, vp(z), vp(t), vp(lp)) == -1
    t[0] = -1
    assert f(0, 1, 8, vp(z), vp(t), vp(lp)) == -1

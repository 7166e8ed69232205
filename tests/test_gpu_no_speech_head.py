"""-m gpu: the no-speech kernels (csrc/k_nospeech.hip) on crafted logits, through wmi_selftest_no_speech, on the three vocabularies.

  form 1   logits from HBM: every case of tests/no_speech_f64.py within 2 f32 ulp of the float64 value of the definition (bound A: one
           rounding by the definition, one ulp for a double exp that is not correctly rounded); exactly 0 / exactly 1 where the definition
           says so; integer-valued logits shifted by +-30000 give the bits of the unshifted ones; the same call twice gives the same bits
  rows     1 / 2 / 8 / 16 rows of different cases in one launch: every row bit for bit what it gives alone
  form 0   the fused head at K = 128, 384, 512 on every case, at K = 768 and 1280 on a reduced set, on the crafted projection of
           tests/test_gpu_filters.py (Side.projection): p equals form 1 on the product's own projection of the same row (logits_out) bit
           for bit, and those logits lie within LOGIT_ABS of the float64 W . LN(x)

Measured on the MI355X: the worst distance from the float64 value over all form 1 cases is printed with the parity margins (bound A).
No test reads the reference checkout or oracle/_ref."""
import ctypes as C
import types

import numpy as np
import pytest

import no_speech_f64 as nf
import stage_compare as sc
from test_gpu_filters import Side
from test_gpu_parity import LOGIT_ABS

pytestmark = pytest.mark.gpu


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def form1(lib, rows, nosp):
    lg = np.ascontiguousarray(np.stack(rows), np.float32)
    p = np.full(lg.shape[0], -7.0, np.float32)
    rc = lib.wmi_selftest_no_speech(0, 1, lg.shape[0], lg.shape[1], nosp, vp(lg), None, None, 0, None, vp(p))
    assert rc == 0, rc
    return p


def form0(lib, W, xs, nosp, want_logits=True):
    x = np.ascontiguousarray(np.stack(xs), np.float32)
    n, K = x.shape
    p = np.full(n, -7.0, np.float32)
    lo = np.empty((n, W.shape[0]), np.float32) if want_logits else None
    rc = lib.wmi_selftest_no_speech(0, 0, n, W.shape[0], nosp, None, vp(W), vp(x), K, vp(lo), vp(p))
    assert rc == 0, rc
    return p, lo


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def hold_p(kind, p, l, nosp, what):
    want = nf.spec_p(l, nosp)
    assert nf.judge(p, l, nosp), (what, float(p), want, nf.ulps_off(p, want))
    sc.hold(f"no-speech {kind}: f32 ulp from the float64 value (bound A)", nf.ulps_off(p, want), float(nf.ULPS), what)


@pytest.fixture(scope="module")
def cases():
    return {nv: nf.make_cases(nv) for nv in nf.VOCABS}


@pytest.mark.parametrize("nv", nf.VOCABS)
def test_form_1_on_every_case(product_lib, cases, nv):
    nosp = nf.nosp_of(nv)
    got = {}
    for name, l in cases[nv]:
        p = form1(product_lib, [l], nosp)
        hold_p("form 1", p[0], l, nosp, (nv, name))
        assert bits(form1(product_lib, [l], nosp)) == bits(p), (nv, name)              # the same call twice
        got[name] = p[0]
    assert got["all equal"] == np.float32(1.0 / nv) and got["nosp -inf"] == 0.0 and got["only nosp finite"] == 1.0
    assert bits([got["integers"]] * 2) == bits([got["integers + 30000"], got["integers - 30000"]]), nv


@pytest.mark.parametrize("n_rows", [1, 2, 8, 16])
@pytest.mark.parametrize("nv", nf.VOCABS)
def test_rows_of_one_launch_equal_the_rows_alone(product_lib, cases, nv, n_rows):
    nosp = nf.nosp_of(nv); cs = cases[nv]
    rows = [cs[(5 * r + n_rows) % len(cs)][1] for r in range(n_rows)]
    got = form1(product_lib, rows, nosp)
    for r, l in enumerate(rows):
        assert bits(form1(product_lib, [l], nosp)) == bits(got[r:r + 1]), (nv, n_rows, r)
        hold_p("form 1", got[r], l, nosp, (nv, n_rows, r))


def fused_case(lib, proj, K, name, want, nosp):
    W, x = Side.projection(proj, K, want)
    p, lo = form0(lib, W, [x], nosp)
    ref = Side.projection_f64(proj, W, x)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(lo[0]), fin) and not np.isnan(lo[0]).any(), (K, name)
    # The projection's activation operand is f16(LN(x)) (SURVEY App. B rule 1; ln_row_compute), here f16(0.999995) = 1: the float64
    # product with THAT operand is held on every case.  The plain W . LN(x) differs from it by 5e-6 of a logit — nothing at a logit's usual
    # size, 0.15 on the entries of +-30000 (measured: 0.150 at K = 128) — so it is held on every case but the two shifted ones.
    xd = x.astype(np.float64)
    a16 = ((xd - xd.mean()) / np.sqrt(xd.var() + 1e-5)).astype(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ref16 = W[:, [8, 10, 12]].astype(np.float64) @ a16[[8, 10, 12]]
    sc.hold("no-speech form 0: the product's projection vs float64 W . f16(LN(x)), max |d|", float(np.abs(lo[0][fin] - ref16[fin]).max()), LOGIT_ABS, (K, name))
    if "30000" not in name:
        sc.hold("no-speech form 0: the product's projection vs float64 W . LN(x), max |d|", float(np.abs(lo[0][fin] - ref[fin]).max()), LOGIT_ABS, (K, name))
    assert bits(p) == bits(form1(lib, [lo[0]], nosp)), (K, name, p)                   # the head's own logits are the projection's bits
    hold_p("form 0", p[0], lo[0], nosp, (K, name))
    assert bits(form0(lib, W, [x], nosp, want_logits=False)[0]) == bits(p), (K, name)   # twice, and without the projection beside it
    return x


@pytest.mark.parametrize("K", [128, 384, 512])
@pytest.mark.parametrize("nv", nf.VOCABS)
def test_fused_head_on_every_case(product_lib, cases, nv, K):
    nosp = nf.nosp_of(nv)
    proj = types.SimpleNamespace(v=types.SimpleNamespace(n_vocab=nv), W={})
    for name, l in cases[nv]:
        fused_case(product_lib, proj, K, name, l, nosp)


@pytest.mark.parametrize("K,nv", [(768, 51865), (1280, 51866)])
def test_fused_head_at_the_wider_projections(product_lib, cases, K, nv):
    nosp = nf.nosp_of(nv)
    proj = types.SimpleNamespace(v=types.SimpleNamespace(n_vocab=nv), W={})
    for name, l in cases[nv]:
        if name in nf.REDUCED:
            fused_case(product_lib, proj, K, name, l, nosp)


@pytest.mark.parametrize("n_rows", [2, 16])
def test_fused_head_rows_of_one_launch_equal_the_rows_alone(product_lib, cases, n_rows):
    """rows with different activations against one matrix: x scaled per row (LayerNorm takes the scale out again up to rounding, so the
    rows' logits differ in their last bits) — every row what it gives alone, and what form 1 gives on the product's projection of it"""
    nv, K = 51865, 384
    nosp = nf.nosp_of(nv)
    proj = types.SimpleNamespace(v=types.SimpleNamespace(n_vocab=nv), W={})
    W, x = Side.projection(proj, K, dict(cases[nv])["normal"])
    rng = np.random.default_rng(8)
    xs = [(x * np.float32(1.0 + 0.37 * r) + rng.standard_normal(K).astype(np.float32) * np.float32(0.01 * (r % 3))).astype(np.float32) for r in range(n_rows)]
    p, lo = form0(product_lib, W, xs, nosp)
    for r in range(n_rows):
        alone, _ = form0(product_lib, W, [xs[r]], nosp, want_logits=False)
        assert bits(alone) == bits(p[r:r + 1]), (n_rows, r)
        assert bits(form1(product_lib, [lo[r]], nosp)) == bits(p[r:r + 1]), (n_rows, r)

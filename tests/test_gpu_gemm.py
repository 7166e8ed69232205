"""-m gpu: every tile form of the f16 GEMMs (csrc/k_gemm.hip, csrc/k_gemm8.hip) and every epilogue (csrc/gemm_epi.h) on crafted operands,
element by element against float64, through wmi_selftest_gemm.

The cases are tests/gemm_f64.py's TABLE: one row per dispatch path at the smallest shape that reaches it — the ten tile forms (64x32, 64x64,
64x128, 96x128, 128x128, 192x128 of k_gemm on the 2- or 4-deep DMA ring or the register-staged loop, in both fragment orientations;
k_gemm8 on 192- and 288-row tiles by the product's dispatch, and on 128, 192 and 288 rows called directly with fewer tiles than compute
units), interior and bounds-checked, under the eight epilogues, plus the paths the enumeration of the product's calls
(tests/test_gemm_f64.py) reaches.  Each case first asserts the plan the hook reports (gemm_plan(): kernel, tile, wavefronts, ring, loop,
orientation rule, k extent of a slot), so a later change of the dispatch rule moves a case visibly instead of silently un-covering a path.
The table's plans are those of a 256-CU device; only the q|k|v launch on k_gemm8's 288-row tiles depends on the CU count, and on a device
with another count its chunk count is derived from wmi_selftest_gemm_plan (plan_for_this_device).

Three operand families per case (gemm_f64.make_case): exact-sparse and exact-dense, compared bit for bit with the one correctly rounded
value of the exact result, and normal, within ulp / 2 + K 2^-24 sum |a||w| + 2^-24 |v| per further f32 step.  Everywhere: rows >= M,
columns >= N, the padding columns, the rows EPI_CONV2's map never stores and the rows between the chunks are still the sentinel.

GELU (gelu16_pair, both through EPI_F16_BIAS_GELU and EPI_CONV2): all 63 488 finite f16 inputs, one per output element
(test_gelu_every_finite_input; the measured figures are in its docstring).

Cross-form checks (same operands, same k order: bit-identical whatever the tile — on all three families): the GELU of the k_gemm8 case
against the 96x128 and the 64x64 form on a common sub-block; gemm8 called directly on 128-row tiles against 192-row tiles; q|k|v on 288-row
tiles against wmi_selftest_qkv_encoder; the in-place residual against the out-of-place one.

WHAT THESE CASES FOUND: no defect in the kernels — all 183 cases hold on the MI355X, the guarded right edge (N = 80, which no product
call has) and gemm8 with empty XCD runs included, and the forms are bit-identical to each other on all three families.  Two claims in
comments were off: gelu16_pair differs from the reference's table on 370 inputs by up to 3 f16 steps, not "271 entries, <= 2 ulp"
(corrected in csrc/gemm_epi.h; the kernel is the one within 0.5001 ulp of float64), and the enumeration of the product's calls reaches 19
(plan, epilogue) pairs beyond the ten tile forms listed when these tests were planned (added to the table, gemm_f64._table).

No test reads the reference checkout or oracle/_ref."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import attn_f64 as af
import gemm_f64 as gf

pytestmark = pytest.mark.gpu


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_CUS = []


def device_cus(lib):
    """the CU count the dispatch uses on this device, as the hook reports it with a launch's plan"""
    if not _CUS:
        c = gf.make_case(gf.Spec("probe", gf.F16_BIAS, 1, 128, 64, gf.kplan(64, 64, 4)), "sparse")
        launch(lib, c)
    return _CUS[0]


def plan_at(lib, s, n_cu):
    out = (C.c_int * 10)()
    assert lib.wmi_selftest_gemm_plan(s.epi, s.M, s.N, s.K, s.S, n_cu, out) == 0
    return tuple(out)[:9]


def plan_for_this_device(lib, s):
    """the table's plan; for the q|k|v launch on k_gemm8's 288-row tiles on a device that has not 256 CUs, the chunk count that reaches it"""
    if s.force8 or device_cus(lib) == 256 or plan_at(lib, s, device_cus(lib)) == s.plan:
        return s
    assert s.epi == gf.QKV_ENC and s.plan[0] == 8, (s.id, "a plan that depends on the CU count", device_cus(lib))
    for chunks in range(16, 0, -1):
        t = dataclasses.replace(s, M=chunks * s.rpc)
        if t.M >= 4096 and plan_at(lib, t, device_cus(lib)) == s.plan:
            return t
    pytest.fail(f"no chunk count sends q|k|v at {s.rpc} rows per chunk to k_gemm8's 288-row tiles on {device_cus(lib)} CUs")


def launch(lib, c):
    """-> (outs, plan): the hook's buffers as gemm_f64.blank_outputs shapes them, and the plan that served the call"""
    s = c.spec
    outs = {k: None if v is None else np.zeros_like(v) for k, v in gf.blank_outputs(c).items()}
    plan = (C.c_int * 11)()
    f32 = s.epi in (gf.RESID, gf.CONV2)
    rc = lib.wmi_selftest_gemm(0, s.epi, s.M, s.N, s.K, c.lda, s.S, c.scale, s.n_layers, s.rpc, s.conv2_out, s.Tpad, s.ld_pad, s.in_place, s.force8,
                               _p(c.A), _p(c.W), _p(c.bias), _p(c.resid), gf.SENTINEL32 if f32 else gf.SENTINEL16, c.out_rows,
                               _p(outs["C"]), _p(outs["aux"]), _p(outs["aux2"]), plan)
    if rc in (-2, -3):                                        # a device error: nothing more is started on this device
        pytest.exit(f"wmi_selftest_gemm: device error {rc} at {c.name}", returncode=3)
    assert rc == 0, (rc, c.name)
    assert plan[9] == s.epi and plan[10] >= 8 and plan[10] % 8 == 0, tuple(plan)
    if not _CUS:
        _CUS.append(plan[10])
    return outs, tuple(plan)[:9]


def run(lib, spec, family, operands=None):
    spec = plan_for_this_device(lib, spec)
    c = gf.make_case(spec, family, operands=operands)
    outs, plan = launch(lib, c)
    assert plan == spec.plan, (c.name, spec.path, "the dispatch no longer sends this shape down the path the case is there for", plan, spec.plan)
    gf.hold_gemm(c, outs)
    return c, outs


def same_bits(what, a, b):
    bad = np.argwhere(a != b)
    assert bad.size == 0, (what, "first differing (.., row, column)", tuple(bad[0]), len(bad))


# ---------------------------------------------------------------------------------------------- the table
GROUPS = {}
for _s in gf.TABLE:
    GROUPS.setdefault((_s.path, gf.EPI_NAMES[_s.epi]), []).append(_s)


@pytest.mark.parametrize("family", gf.FAMILIES)
@pytest.mark.parametrize("path,epi", list(GROUPS), ids=[f"{p} {e}".replace(" ", "_") for p, e in GROUPS])
def test_table(product_lib, path, epi, family):
    for spec in GROUPS[(path, epi)]:
        run(product_lib, spec, family)


def test_in_place_residual_equals_out_of_place(product_lib):
    a, b = [s for s in gf.TABLE if (s.epi, s.M, s.N, s.K) == (gf.RESID, 1500, 768, 64)]
    assert a.in_place != b.in_place
    for family in gf.FAMILIES:
        ca = gf.make_case(a, family)
        cb = gf.make_case(b, family, operands=(ca.A, ca.W, ca.bias, ca.resid))
        same_bits(f"{family} in place / out of place", launch(product_lib, ca)[0]["C"], launch(product_lib, cb)[0]["C"])


# ---------------------------------------------------------------------------------------------- GELU
@pytest.mark.parametrize("epi", [gf.GELU, gf.CONV2], ids=["F16_BIAS_GELU", "CONV2"])
def test_gelu_every_finite_input(product_lib, epi):
    """All 63 488 finite f16 values as acc + bias of one output element each (gemm_f64.gelu_sweep_case), under the bound of gemm_f64's
    docstring, with: no NaN, gelu(+-0) = 0, x returned where the table returns x, a zero where the table's negative tail gives one; for
    EPI_CONV2 x == f32(pe + aux) bit for bit.

    Measured on the MI355X (printed by this test), the same through both epilogues: the kernel's result differs from the table on 370 of the
    63 488 inputs, by at most 3 f16 steps; its largest distance from float64 is 0.5001 ulp where the table's is 2.8116 — the differences
    are the table's error, not the kernel's (gemm_f64.gelu_pair_np, with correctly rounded exp2 and reciprocal: 369 inputs, 0.5001 ulp).
    csrc/gemm_epi.h said "271 entries, <= 2 ulp" from an earlier emulation; its comment now carries these figures."""
    c = gf.gelu_sweep_case(epi)
    outs, plan = launch(product_lib, c)
    assert plan == c.spec.plan, plan
    x = gf.all_finite_f16()
    img = outs["C"] if epi == gf.GELU else outs["aux"]
    got = img[0, :248, :256].view(np.float16) if epi == gf.GELU else img[0, :248, :256].view(np.float32).astype(np.float16)
    tab = gf.gelu_table(x)
    differ = got.view(np.uint16) != tab.view(np.uint16)
    differ &= ~((got == 0) & (tab == 0))                      # (a zero of either sign)
    step = lambda h: np.where(h.view(np.int16) < 0, -(h.view(np.int16) & 0x7FFF).astype(np.int32), h.view(np.int16).astype(np.int32))
    steps = np.abs(step(got) - step(tab))[differ]
    d = gf.gelu_dist(got, x.astype(np.float64))
    print(f"{gf.EPI_NAMES[epi]}: differs from the table on {int(differ.sum())} of {x.size} inputs, by at most {int(steps.max()) if steps.size else 0} f16 steps; "
          f"largest distance from float64 {d.max():.4f} ulp (the table's {gf.gelu_dist(tab, x.astype(np.float64)).max():.4f})")
    gf.hold_gelu_sweep(gf.EPI_NAMES[epi], got, x)
    gf.hold_gemm(c, outs)


# ---------------------------------------------------------------------------------------------- one result whatever the form
@pytest.mark.parametrize("family", gf.FAMILIES)
@pytest.mark.parametrize("K", [64, 320])
def test_gelu_is_the_same_bits_on_k_gemm8_96x128_and_64x64(product_lib, K, family):
    big = next(s for s in gf.TABLE if (s.epi, s.M, s.N, s.K, s.force8) == (gf.GELU, 4100, 4608, K, 0))
    c8 = gf.make_case(big, family)
    o8, p8 = launch(product_lib, c8)
    assert p8 == gf.plan8(192), p8
    s96 = gf.Spec("96x128", gf.GELU, 4100, 1280, K, gf.kplan(96, 128, 2))
    c96 = gf.make_case(s96, family, operands=(c8.A, c8.W[:1280], c8.bias[:1280], None))
    o96, p96 = launch(product_lib, c96)
    assert p96 == s96.plan, p96
    same_bits("k_gemm8 192 rows / 96x128", o8["C"][0, :4116, :1280], o96["C"][0])
    s64 = gf.Spec("64x64", gf.GELU, 100, 128, K, gf.kplan(64, 64, 4))
    c64 = gf.make_case(s64, family, operands=(c8.A[:99 * K + K], c8.W[:128], c8.bias[:128], None))
    o64, p64 = launch(product_lib, c64)
    assert p64 == s64.plan, p64
    same_bits("k_gemm8 192 rows / 64x64", o8["C"][0, :100, :128], o64["C"][0, :100])


@pytest.mark.parametrize("family", gf.FAMILIES)
@pytest.mark.parametrize("epi", [gf.GELU, gf.CROSS_KV], ids=["F16_BIAS_GELU", "CROSS_KV"])
def test_gemm8_direct_128_rows_equals_192_rows(product_lib, epi, family):
    s192, s128 = [next(s for s in gf.TABLE if s.epi == epi and s.force8 == bm) for bm in (192, 128)]
    c192 = gf.make_case(s192, family)
    c128 = gf.make_case(s128, family, operands=(c192.A, c192.W, c192.bias, None))
    a, pa = launch(product_lib, c192)
    b, pb = launch(product_lib, c128)
    assert pa == gf.plan8(192) and pb == gf.plan8(128), (pa, pb)
    for name in ("C", "aux"):
        if a[name] is not None:
            same_bits(f"{gf.EPI_NAMES[epi]} {family} {name}", a[name], b[name])


@pytest.mark.parametrize("family", gf.FAMILIES)
def test_qkv_on_288_row_tiles_equals_the_qkv_hook(product_lib, family):
    spec = plan_for_this_device(product_lib, next(s for s in gf.TABLE if s.epi == gf.QKV_ENC and s.plan[0] == 8 and not s.force8))
    c = gf.make_case(spec, family)
    o, plan = launch(product_lib, c)
    assert plan == spec.plan, plan
    q = np.zeros((c.out_rows, spec.S), np.uint16); k = np.zeros_like(q); vt = np.zeros_like(o["aux2"])
    rc = product_lib.wmi_selftest_qkv_encoder(0, spec.M, spec.S, spec.Tpad, spec.rpc, _p(c.A), _p(c.W), _p(c.bias), af.SENTINEL16, c.out_rows,
                                              _p(q), _p(k), _p(vt))
    assert rc == 0, rc
    same_bits("q", o["C"][0], q); same_bits("k", o["aux"][0], k); same_bits("V^T", o["aux2"], vt)

"""CPU: the judge of the f16 GEMM tests (tests/gemm_f64.py) refuses wrong answers, its GELU yardsticks are what its docstring says, the
table of dispatch plans is what gemm_plan() (wmi_selftest_gemm_plan: host only) answers, and every plan the product can reach is in the
table.  The kernels themselves run in tests/test_gpu_gemm.py."""
import ctypes as C

import numpy as np
import pytest

import gemm_f64 as gf
from godot_whisper_amd import runtime


def spec_of(epi, M, N, K, **kw):
    found = [s for s in gf.TABLE if (s.epi, s.M, s.N, s.K) == (epi, M, N, K) and all(getattr(s, k) == v for k, v in kw.items())]
    assert found, (epi, M, N, K, kw)
    return found[0]


# ---------------------------------------------------------------------------------------------- GELU yardsticks
def test_gelu_emulation_and_table_against_float64():
    x = gf.all_finite_f16()
    xf = x.astype(np.float64)
    d_pair = gf.gelu_dist(gf.gelu_pair_np(x.astype(np.float32)), xf)
    d_tab = gf.gelu_dist(gf.gelu_table(x), xf)
    print(f"gelu16_pair (NumPy) max {d_pair.max():.4f} ulp, table max {d_tab.max():.4f} ulp, "
          f"differ on {int((gf.gelu_pair_np(x.astype(np.float32)) != gf.gelu_table(x)).sum())} inputs")
    assert d_pair.max() <= 0.5001
    assert d_tab.max() <= gf.GELU_TABLE_MAX
    gf.hold_gelu_sweep("emulation", gf.gelu_pair_np(x.astype(np.float32)), x)
    t = np.linspace(-8, 8, 160001)
    assert np.abs(np.gradient(gf.gelu_f64(t), t)).max() <= gf.GELU_SLOPE


@pytest.mark.parametrize("wrong", ["constant", "no_input_rounding", "pair_swapped"])
def test_gelu_bound_refuses_a_wrong_form(wrong):
    x = gf.all_finite_f16()
    f = np.float32
    with np.errstate(over="ignore"):
        if wrong == "constant":                                 # 0.044715 -> 0.04715
            xf = x.astype(f)
            g = (xf / (f(1) + np.exp(f(-2 * gf.K0) * xf * (f(1) + f(0.04715) * xf * xf)))).astype(np.float16)
            xin = x
        elif wrong == "no_input_rounding":                       # x taken a third of an f16 step off its rounded value
            xin = x[100:140]
            off = xin.astype(f) + f(0.33) * np.spacing(np.abs(xin)).astype(f)
            g = (off / (f(1) + np.exp(f(-2 * gf.K0) * off * (f(1) + f(gf.K1) * off * off)))).astype(np.float16)
        else:
            g = gf.gelu_pair_np(x.astype(f)).reshape(248, 128, 2)[:, :, ::-1].reshape(248, 256)
            xin = x
    with pytest.raises(AssertionError):
        gf.hold_gelu_exact(wrong, g, xin)


@pytest.mark.parametrize("epi", [gf.GELU, gf.CONV2])
def test_gelu_sweep_case_reaches_every_finite_input(epi):
    c = gf.gelu_sweep_case(epi)
    assert (c.acc().astype(np.float16).view(np.uint16) == gf.all_finite_f16().view(np.uint16))[gf.all_finite_f16() != 0].all()
    gf.hold_gemm(c, gf.restate(c))


# ---------------------------------------------------------------------------------------------- the judge
ACCEPT = [(gf.F16_BIAS, 100, 128, 128, {}), (gf.F16_BIAS, 100, 80, 128, {}), (gf.GELU, 100, 128, 96, {}), (gf.Q_SCALED, 65, 128, 192, {}),
          (gf.RESID, 100, 128, 128, {}), (gf.RESID, 100, 80, 128, {}), (gf.CONV2, 150, 128, 384, dict(aux_null=False)),
          (gf.CONV2, 150, 128, 384, dict(aux_null=True)), (gf.CONV2, 161, 128, 192, dict(conv2_out=0)), (gf.CONV2, 161, 128, 192, dict(conv2_out=64)),
          (gf.QKV_DEC, 100, 192, 64, {}), (gf.CROSS_KV, 100, 256, 128, {}), (gf.GELU, 200, 128, 256, {})]


@pytest.mark.parametrize("family", ["sparse", "dense"])
@pytest.mark.parametrize("epi,M,N,K,kw", ACCEPT)
def test_judge_accepts_a_correct_restatement(epi, M, N, K, kw, family):
    c = gf.make_case(spec_of(epi, M, N, K, **kw), family)
    gf.hold_gemm(c, gf.restate(c))


FAULTS = [
    ("transpose4", gf.F16_BIAS, 100, 128, 128, {}), ("swap_r8", gf.F16_BIAS, 100, 128, 128, {}), ("shift8", gf.F16_BIAS, 100, 128, 128, {}),
    ("shift16", gf.F16_BIAS, 100, 128, 128, {}), ("shift32", gf.F16_BIAS, 100, 128, 128, {}), ("row_M", gf.F16_BIAS, 100, 128, 128, {}),
    ("transpose4", gf.RESID, 100, 128, 128, {}), ("swap_r8", gf.RESID, 100, 128, 128, {}), ("row_M", gf.RESID, 100, 128, 128, {}),
    ("col_N", gf.F16_BIAS, 100, 80, 128, {}), ("col_N", gf.RESID, 100, 80, 128, {}),
    ("drop_k_tail", gf.GELU, 100, 128, 96, {}), ("drop_k_tail", gf.RESID, 100, 128, 96, {}),
    ("dup_k_tile", gf.F16_BIAS, 100, 128, 128, {}), ("dup_k_tile", gf.RESID, 100, 128, 128, {}),
    ("bias_on_k", gf.QKV_DEC, 100, 192, 64, {}), ("scale_wrong", gf.QKV_DEC, 100, 192, 64, {}),
    ("no_bias_v", gf.CROSS_KV, 100, 256, 128, {}), ("scale_wrong", gf.CROSS_KV, 100, 256, 128, {}), ("stride_short", gf.CROSS_KV, 100, 256, 128, {}),
    ("conv2_P", gf.CONV2, 161, 128, 192, dict(conv2_out=0)), ("conv2_P", gf.CONV2, 161, 128, 192, dict(conv2_out=64)),
    ("conv2_ignore_out", gf.CONV2, 161, 128, 192, dict(conv2_out=64)),
    ("gelu_far", gf.GELU, 100, 128, 128, {}), ("gelu_far", gf.CONV2, 150, 128, 384, dict(aux_null=False)),
    ("gelu_far", gf.CONV2, 150, 128, 384, dict(aux_null=True)),
    ("resid_twice", gf.RESID, 100, 128, 128, {}),
]


@pytest.mark.parametrize("fault,epi,M,N,K,kw", FAULTS)
def test_judge_refuses(fault, epi, M, N, K, kw):
    # the dense family must catch every one of them; the sparse one all but a repeated K tile it may have no weight in
    for family in ("dense", "sparse"):
        c = gf.make_case(spec_of(epi, M, N, K, **kw), family)
        try:
            gf.hold_gemm(c, gf.restate(c, fault))
        except AssertionError:
            continue
        assert family == "sparse" and fault in ("dup_k_tile", "drop_k_tail"), (fault, family, "accepted")


def test_judge_refuses_on_the_normal_family_too():
    """the bound of the normal family is tight enough for a dropped K tail and a bias on the wrong segment"""
    for fault, epi, M, N, K in (("drop_k_tail", gf.RESID, 100, 128, 96), ("bias_on_k", gf.QKV_DEC, 100, 192, 64), ("no_bias_v", gf.CROSS_KV, 100, 256, 128)):
        c = gf.make_case(spec_of(epi, M, N, K), "normal")
        ok = gf.blank_outputs(c)
        rows, W = c.rows().astype(np.float32), c.W.astype(np.float32)
        if fault == "drop_k_tail":
            good = (rows @ W.T + c.bias) + c.resid
            bad = (rows[:, :64] @ W[:, :64].T + c.bias) + c.resid
            ok["C"][0, :M, :N] = good.view(np.uint32)
            gf.hold_gemm(c, ok)
            ok["C"][0, :M, :N] = bad.view(np.uint32)
        else:
            acc = rows @ W.T
            s = np.float32(c.scale); S = c.spec.S
            if epi == gf.QKV_DEC:
                ok["C"][0, :M, :S] = ((acc[:, :S] + c.bias[:S]) * s).astype(np.float16).view(np.uint16)
                ok["aux"][0, :M, :S] = (acc[:, S:2 * S] * s).astype(np.float16).view(np.uint16)
                ok["aux2"][0, :M, :S] = (acc[:, 2 * S:] + c.bias[2 * S:]).astype(np.float16).view(np.uint16)
                gf.hold_gemm(c, ok)
                ok["aux"][0, :M, :S] = ((acc[:, S:2 * S] + c.bias[S:2 * S]) * s).astype(np.float16).view(np.uint16)
            else:
                for il in range(c.spec.n_layers):
                    ok["C"][il, :M, :S] = (acc[:, il * 2 * S:il * 2 * S + S] * s).astype(np.float16).view(np.uint16)
                    ok["aux"][il, :M, :S] = (acc[:, il * 2 * S + S:(il + 1) * 2 * S] + c.bias[il * 2 * S + S:(il + 1) * 2 * S]).astype(np.float16).view(np.uint16)
                gf.hold_gemm(c, ok)
                ok["aux"][1, :M, :S] = acc[:, 3 * S:4 * S].astype(np.float16).view(np.uint16)
        with pytest.raises(AssertionError):
            gf.hold_gemm(c, ok)


def test_qkv_cases_go_through_hold_qkv():
    import attn_f64 as af
    for family in gf.FAMILIES:
        c = gf.make_case(gf.Spec("small", gf.QKV_ENC, 256, 384, 128, gf.kplan(64, 64, 4), S=128, rpc=128, T=120, Tpad=128), family)
        q = gf.qkv_case(c)
        full = q.product()
        assert full.shape == (256, 384) and np.allclose(full, c.rows().astype(np.float64) @ c.W.astype(np.float64).T + c.bias, atol=1e-9)
        if c.exact:
            assert (full.astype(np.float16).astype(np.float64) == full).all()
        o = gf.blank_outputs(c)
        v16 = full.astype(np.float32).astype(np.float16).view(np.uint16)
        o["C"][0, :256, :128] = v16[:, :128]; o["aux"][0, :256, :128] = v16[:, 128:256]
        pos = af.vt_pos(np.arange(128))
        for b in range(2):
            o["aux2"][b][:, pos] = v16[b * 128:(b + 1) * 128, 256:].T
        gf.hold_gemm(c, o)
        o["aux2"][1][:, pos] = v16[:128, 256:].T             # chunk 1 holds chunk 0's V^T
        with pytest.raises(AssertionError):
            gf.hold_gemm(c, o)


# ---------------------------------------------------------------------------------------------- the plans
def plan(lib, epi, M, N, K, S, n_cu):
    out = (C.c_int * 10)()
    rc = lib.wmi_selftest_gemm_plan(epi, M, N, K, S, n_cu, out)
    assert rc == 0, (rc, epi, M, N, K, S, n_cu)
    assert out[9] == epi
    return tuple(out)[:9]


def test_table_plans_are_what_the_dispatch_answers_at_256_cus():
    lib = runtime.load_library()
    for s in gf.TABLE:
        if not s.force8:
            assert plan(lib, s.epi, s.M, s.N, s.K, s.S, 256) == s.plan, (s.id, s.path)
    assert lib.wmi_selftest_gemm_plan(8, 100, 128, 64, 0, 256, (C.c_int * 10)()) == -1
    assert lib.wmi_selftest_gemm_plan(0, 0, 128, 64, 0, 256, (C.c_int * 10)()) == -1
    assert lib.wmi_selftest_gemm_plan(0, 100, 128, 48, 0, 256, (C.c_int * 10)()) == -1
    assert lib.wmi_selftest_gemm_plan(0, 100, 128, 64, 0, 256, None) == -1


def test_every_plan_the_product_reaches_is_in_the_table():
    """the encoder's seven GEMMs at one chunk and at 2 .. 16 lock-step chunks (uniform and ragged row periods), T = 1500 and short audio_ctx,
    the decoder's prompt projections at 9 .. 448 rows, six model widths, 256 and 304 compute units"""
    lib = runtime.load_library()
    missing = {}
    seen = set()
    for n_cu in (256, 304):
        for name, (S, Lt, nm) in gf.MODELS.items():
            calls = set()
            for T in (1500, 1000, 750, 563, 200, 64):
                for nb in range(1, 17):
                    for ragged in ((False,) if nb == 1 else (False, True)):
                        calls.update(gf.product_calls(S, Lt, nm, T, nb, ragged))
            for n in list(range(9, 130)) + [160, 200, 223, 224, 256, 300, 384, 447, 448]:
                calls.update(gf.prompt_calls(S, n))
            for (epi, M, N, K, Sx) in sorted(calls):
                key = plan(lib, epi, M, N, K, Sx, n_cu) + (epi,)
                seen.add(key)
                if key not in gf.TABLE_KEYS:
                    missing.setdefault(key, (name, n_cu, gf.EPI_NAMES[epi], M, N, K))
    assert not missing, ("plans the product reaches that tests/gemm_f64.py TABLE does not hold (first shape of each)", missing)
    # and the table's dispatched product paths are no dead letters: each is reached by some product call
    unreached = {s.key for s in gf.TABLE if s.product and not s.force8} - seen
    print("table plans no enumerated product call reaches:", sorted(unreached))


# ---------------------------------------------------------------------------------------------- the hook's refusals
def test_gemm_hook_refuses_before_the_device_is_touched():
    lib = runtime.load_library()

    def run(epi=0, M=70, N=128, K=64, lda=64, S=0, n_layers=0, rpc=0, conv2_out=0, Tpad=0, ld_pad=0, in_place=0, force8=0, out_rows=None, resid=False,
            aux=False, aux2=False, null=None):
        out_rows = M + 16 if out_rows is None else out_rows
        buf = np.zeros(1 << 20, np.uint32)                    # (every pointer: one buffer large enough for any of them)
        p = lambda name, want=True: None if (null == name or not want) else buf.ctypes.data_as(C.c_void_p)
        return lib.wmi_selftest_gemm(0, epi, M, N, K, lda, S, 1.0, n_layers, rpc, conv2_out, Tpad, ld_pad, in_place, force8, p("A"), p("W"), p("bias"),
                                     p("resid", resid), gf.SENTINEL16, out_rows, p("C"), p("aux", aux), p("aux2", aux2), p("plan"))
    bad = [dict(epi=8), dict(epi=-1), dict(M=0), dict(N=0), dict(N=126), dict(K=0), dict(K=48), dict(lda=0), dict(ld_pad=4), dict(ld_pad=-8),
           dict(out_rows=80), dict(null="A"), dict(null="W"), dict(null="C"), dict(null="plan"), dict(epi=2), dict(epi=0, resid=True),
           dict(epi=0, in_place=1), dict(epi=3, resid=True, in_place=1), dict(epi=0, S=64), dict(epi=0, aux=True), dict(epi=0, rpc=10),
           dict(epi=0, conv2_out=10), dict(epi=0, Tpad=64), dict(epi=5, N=192, S=64), dict(epi=5, N=192, S=60, aux=True, aux2=True),
           dict(epi=5, N=128, S=64, aux=True, aux2=True), dict(epi=6, N=256, S=64, n_layers=1, aux=True), dict(epi=6, N=256, S=64, n_layers=2),
           dict(epi=4, N=192, S=64, aux=True, aux2=True), dict(epi=4, N=192, S=64, aux=True, aux2=True, Tpad=64),
           dict(epi=4, M=128, N=192, S=64, aux=True, aux2=True, Tpad=128, rpc=60),
           dict(epi=3, resid=True, rpc=4), dict(epi=3, M=161, resid=True, rpc=54, conv2_out=40), dict(epi=3, M=161, resid=True, rpc=54, conv2_out=64),
           dict(force8=192), dict(epi=1, N=256, force8=96), dict(epi=1, N=128, force8=192), dict(epi=1, N=256, K=96, force8=192),
           dict(epi=4, N=768, S=256, K=256, M=64, Tpad=64, aux=True, aux2=True, force8=192)]
    for kw in bad:
        assert run(**kw) == -1, kw
    if lib.wmi_device_count() <= 0:
        for kw in (dict(), dict(epi=2, resid=True, in_place=1), dict(epi=1, N=256, force8=192), dict(epi=3, M=161, resid=True, rpc=54, conv2_out=64, out_rows=208)):
            assert run(**kw) in (-2, -3), kw

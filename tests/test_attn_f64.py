"""CPU: the conditions tests/attn_f64.py's cases rest on, the yardstick's own error, the refusals of the two test hooks
(wmi_selftest_attn_encoder, wmi_selftest_qkv_encoder: decided before the device is touched), and the negative controls — restatements
of the attention with one classic mistake each must FAIL the same hold_case() / hold_qkv() tests/test_gpu_attn_encoder.py passes the
kernels' results to.  A control that passed would mean the GPU test cannot see that mistake: sharpen the case, not the control."""
import ctypes as C

import numpy as np
import pytest

import attn_f64 as af
from godot_whisper_amd import runtime


# ---------------------------------------------------------------------------------------------- the generators' conditions
@pytest.mark.parametrize("T", [1, 33, 64, 65, 129, 200, 513, 563, 576, 641, 1500])
def test_selector_margin_and_coverage(T):
    worst = np.inf
    for seed in (0, 1, 2) if T <= 641 else (0,):
        c = af.make_case("selector", T, seed=seed)
        margin, pi = af.selector_margin(c.q[0], c.k[0], T)
        worst = min(worst, margin)
        assert (pi == c.pi[0]).all() and sorted(pi.tolist()) == list(range(T))         # every key is some query's: both sides of every boundary
        assert set(af.boundary_keys(T)) <= set(pi.tolist()) and {0, T - 1} <= set(pi.tolist())
        # the restatement with the reference's rounding points returns the selected rows exactly: every other numerator is 0 in f16
        assert np.array_equal(af.attend_ref_points(c.q[0], c.k[0], c.v[0], T, f16_result=True), c.expected(0))
    assert worst >= af.SELECTOR_MARGIN, worst
    assert np.exp(-af.SELECTOR_MARGIN) < 2.0 ** -25                                   # below half of f16's smallest subnormal


@pytest.mark.parametrize("T", [1, 65, 563, 1500])
def test_uniform_sums_are_exact_in_f32(T):
    c = af.make_case("uniform", [T, max(T - 1, 1), T] if T == 563 else T, ragged=False)
    for b, Tb in enumerate(c.lens):
        v = c.v[b, :Tb]
        assert (c.q[b, :Tb] == 0).all()
        assert ((v.astype(np.float64) * 16) % 1 == 0).all() and np.abs(v.astype(np.float64)).max() <= 8
        exact = v.astype(np.float64).sum(0)
        assert np.abs(v.astype(np.float64)).sum(0).max() * 16 < 2 ** 24                # every partial sum, in any order, is an f32 integer / 16
        for order in (np.arange(Tb), np.arange(Tb)[::-1], np.random.default_rng(0).permutation(Tb)):
            acc = np.zeros(c.S, np.float32)
            for j in order[:200]:
                acc += v[j].astype(np.float32)
            assert np.array_equal(acc.astype(np.float64), v[order[:200]].astype(np.float64).sum(0))
        # one key more or less moves the result by about 1 / T of a value: thousands of times the f32 bound at T = 1500
        if Tb > 1:
            moved = np.abs(v[:Tb - 1].astype(np.float64).sum(0) / (Tb - 1) - exact / Tb)
            assert (moved > 2.0 ** -22 * np.abs(exact / Tb)).any()


@pytest.mark.parametrize("family", ["selector", "uniform", "random"])
def test_poison_is_finite_and_everywhere_behind_the_length(family):
    c = af.make_case(family, [641, 513, 200, 80], Tpad=704, qk_rows=656, out_rows=650)
    assert c.ragged and c.T == 641
    for b, Tb in enumerate(c.lens):
        for a, rows in ((c.q[b], 656), (c.k[b], 656), (c.v[b], 704)):
            tail = a[Tb:].astype(np.float64)
            assert tail.shape[0] == rows - Tb and np.isfinite(tail).all() and (np.abs(tail) == af.POISON).all()
            assert (tail[:, 1:] == -tail[:, :-1]).all() and (tail[1:] == -tail[:-1]).all()            # alternating along both axes
            assert np.isfinite(a[:Tb].astype(np.float64)).all() and np.abs(a[:Tb].astype(np.float64)).max() < 100


def test_vt_pos_swaps_bits_2_and_3():
    t = np.arange(64)
    p = af.vt_pos(t)
    assert sorted(p.tolist()) == t.tolist() and (af.vt_pos(p) == t).all()
    assert p[:16].tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15] and (p[16:32] == p[:16] + 16).all()


# ---------------------------------------------------------------------------------------------- the yardstick's own error
def test_reference_points_distance_from_float64():
    """T = 563, spread 1 (the shape of the existing form test): rms-rel 4.3e-4 with the f32 result, 4.8e-4 with the f16 one; the f16 store
    alone is 2.1e-4.  The bands are +-25 % around the figures: a restatement that lost a rounding point, or gained one, leaves them."""
    c = af.make_case("random", 563, spread=1.0)
    exp = c.expected(0)
    scale = np.sqrt(np.mean(exp * exp))
    r32 = c.ref_error(0, True)[0] / scale
    r16 = c.ref_error(0, False)[0] / scale
    store = np.sqrt(np.mean((exp.astype(np.float16).astype(np.float64) - exp) ** 2)) / scale
    print(f"attend_ref_points vs float64 at T = 563: rms-rel f32 {r32:.3e}, f16 {r16:.3e}; f16 store alone {store:.3e}")
    assert 3.2e-4 <= r32 <= 5.4e-4 and 3.6e-4 <= r16 <= 6.0e-4 and 1.6e-4 <= store <= 2.6e-4
    assert r16 > r32
    for spread in (0.25, 4.0):
        c = af.make_case("random", 200, spread=spread)
        assert 0 < c.ref_error(0, True)[0] < 2e-3 * np.sqrt(np.mean(c.expected(0) ** 2))


# ---------------------------------------------------------------------------------------------- negative controls
FAULTS = ("extra_key", "missing_key", "vt_no_swap", "next_head", "next_chunk", "row_at_T")


def _control_cases():
    return [af.make_case("selector", 563), af.make_case("uniform", 563), af.make_case("selector", 1500), af.make_case("uniform", 1500),
            af.make_case("uniform", [563, 563, 563], qk_rows=576, out_rows=570),
            af.make_case("selector", [641, 513, 200, 80], Tpad=704, qk_rows=656, out_rows=650)]


@pytest.fixture(scope="module")
def control_cases():
    return _control_cases()


@pytest.mark.parametrize("want_f32", [False, True])
def test_faithful_restatement_passes(control_cases, want_f32):
    for c in control_cases + [af.make_case("random", 200, spread=s) for s in (0.25, 1.0, 4.0)]:
        af.hold_case(c, af.restate(c, want_f32), want_f32, "restatement")


@pytest.mark.parametrize("want_f32", [False, True])
@pytest.mark.parametrize("fault", FAULTS)
def test_every_classic_mistake_fails_hold_case(control_cases, fault, want_f32):
    caught = []
    for c in control_cases:
        if fault == "next_chunk" and c.B == 1:
            continue
        try:
            af.hold_case(c, af.restate(c, want_f32, fault), want_f32, fault)
        except AssertionError as e:
            caught.append((c.family, c.name, str(e)[:120]))
    families = {f for f, _, _ in caught}
    assert families & {"selector", "uniform"}, (fault, "passed hold_case on every case")
    if fault in ("missing_key", "next_head", "row_at_T"):
        assert len(caught) == len(control_cases), (fault, caught)               # these are seen by every case, T = 1500 included
    if fault == "vt_no_swap":                                                      # a sum over all keys cannot see a permutation of them: the selector does
        assert sum(f == "selector" for f, _, _ in caught) == sum(c.family == "selector" for c in control_cases)
    if fault == "extra_key":                                                       # 1 / T of a poisoned value: seen by every uniform case
        assert sum(f == "uniform" for f, _, _ in caught) == sum(c.family == "uniform" for c in control_cases)


def test_selector_failure_names_the_key_that_was_read():
    c = af.make_case("selector", 129)
    with pytest.raises(AssertionError, match=r"expected key \d+, the row equals key\(s\) \[\d+"):
        af.hold_case(c, af.restate(c, False, "vt_no_swap"), False)


def test_qkv_controls():
    """hold_qkv() refuses a V^T image in plain time order, a chunk stride taken for a row stride, a store behind M and a written column
    past the 16-step block that holds T."""
    c = af.make_qkv_case(3)
    full = c.product().astype(np.float16)
    S, Tpad, rpc = c.S, c.Tpad, c.rows_per_chunk
    out_rows = c.M + 16
    def images():
        q = np.full((out_rows, S), af.SENTINEL16, np.uint16); k = q.copy()
        q[:c.M] = full[:, :S].view(np.uint16); k[:c.M] = full[:, S:2 * S].view(np.uint16)
        vt = np.full((c.chunks, S, Tpad), af.SENTINEL16, np.uint16)
        for b in range(c.chunks):
            vt[b][:, af.vt_pos(np.arange(rpc))] = full[b * rpc:(b + 1) * rpc, 2 * S:].T.view(np.uint16)
        return q, k, vt
    q, k, vt = images()
    af.hold_qkv(c, q, k, vt, out_rows)
    q, k, vt = images(); vt[1] = vt[1][:, af.vt_pos(np.arange(Tpad))]
    with pytest.raises(AssertionError): af.hold_qkv(c, q, k, vt, out_rows)
    q, k, vt = images(); vt[2] = vt[1]
    with pytest.raises(AssertionError): af.hold_qkv(c, q, k, vt, out_rows)
    q, k, vt = images(); k[c.M] = k[c.M - 1]
    with pytest.raises(AssertionError): af.hold_qkv(c, q, k, vt, out_rows)
    q, k, vt = images(); q[7, 5] ^= 1
    with pytest.raises(AssertionError): af.hold_qkv(c, q, k, vt, out_rows)
    c1 = af.make_qkv_case(0, Tpad=640)
    f1 = c1.product().astype(np.float16)
    q = np.full((c1.M + 16, S), af.SENTINEL16, np.uint16); k = q.copy()
    q[:c1.M] = f1[:, :S].view(np.uint16); k[:c1.M] = f1[:, S:2 * S].view(np.uint16)
    vt = np.full((1, S, 640), af.SENTINEL16, np.uint16)
    vt[0][:, af.vt_pos(np.arange(c1.M))] = f1[:, 2 * S:].T.view(np.uint16)
    with pytest.raises(AssertionError, match="not finite"): af.hold_qkv(c1, q, k, vt, c1.M + 16)       # columns 563..575 must have been written
    vt[0][:, af.vt_pos(np.arange(c1.M, 576))] = 0
    af.hold_qkv(c1, q, k, vt, c1.M + 16)
    vt[0][3, af.vt_pos(576)] = 0
    with pytest.raises(AssertionError, match="past 576"): af.hold_qkv(c1, q, k, vt, c1.M + 16)


def test_exact_qkv_operands_are_exact():
    c = af.make_qkv_case(3)
    full = c.product()
    assert ((full * 8) % 1 == 0).all() and np.abs(full).max() < 32 and np.array_equal(full.astype(np.float16).astype(np.float64), full)
    assert ((c.W != 0).sum(1) == 2).all() and set(np.unique(c.W).tolist()) <= {-1.0, 0.0, 0.5, 1.0}
    assert c.abs_product().max() * 8 < 2 ** 24                      # every partial sum is an f32 integer / 8


# ---------------------------------------------------------------------------------------------- the hooks' refusals
def _attn(lib, B=1, T=65, Tpad=128, S=128, H=2, qk_rows=128, out_rows=70, row_T=None, want_f32=0, form=2, groups=0, null=None):
    q = np.zeros((B, max(qk_rows, 1), max(S, 1)), np.uint16); v = np.zeros((B, max(Tpad, 1), max(S, 1)), np.uint16)
    out = np.zeros((B, max(out_rows, 1), max(S, 1)), np.uint32)
    rt = None if row_T is None else np.asarray(row_T, np.int32)
    p = lambda a, name: None if a is None or null == name else a.ctypes.data_as(C.c_void_p)
    return lib.wmi_selftest_attn_encoder(0, B, T, Tpad, S, H, qk_rows, out_rows, p(rt, "row_T"), want_f32, form, groups, p(q, "q"), p(q, "k"),
                                         p(v, "v"), af.SENTINEL16, p(out, "out"))


def test_attention_hook_refuses_what_the_product_cannot_launch():
    lib = runtime.load_library()
    bad = [dict(S=128, H=3), dict(S=96, H=2), dict(Tpad=100), dict(Tpad=64), dict(T=129, Tpad=128), dict(B=17), dict(B=0), dict(T=0),
           dict(B=2, row_T=[65, 66]), dict(B=2, row_T=[0, 65]), dict(B=3, row_T=[65, 1, -4]),
           dict(groups=1, T=511, Tpad=512, qk_rows=512, out_rows=512, form=2), dict(groups=1, T=511, Tpad=512, qk_rows=512, out_rows=512, form=1),
           dict(groups=1, T=255, Tpad=256, qk_rows=256, out_rows=256, form=0), dict(groups=1, T=200, Tpad=256, qk_rows=256, out_rows=256),
           dict(qk_rows=64), dict(out_rows=64), dict(form=3), dict(form=-1), dict(groups=2), dict(groups=-2),
           dict(null="q"), dict(null="k"), dict(null="v"), dict(null="out")]
    for kw in bad:
        assert _attn(lib, **kw) == -1, kw
    if lib.wmi_device_count() <= 0:
        # what is well-formed gets as far as the device, and says so
        for kw in (dict(), dict(B=2, row_T=[65, 1]), dict(groups=1, T=512, Tpad=512, qk_rows=512, out_rows=512),
                   dict(groups=1, form=0, T=256, Tpad=256, qk_rows=256, out_rows=256), dict(groups=-1, T=200, Tpad=256, qk_rows=256, out_rows=256)):
            assert _attn(lib, **kw) in (-2, -3), kw


def test_qkv_hook_refusals():
    lib = runtime.load_library()
    def run(M=70, S=128, Tpad=128, rpc=0, out_rows=None, null=None):
        out_rows = M if out_rows is None else out_rows
        x = np.zeros((max(M, 1), max(S, 1)), np.uint16); W = np.zeros((3 * max(S, 1), max(S, 1)), np.uint16); b = np.zeros(3 * max(S, 1), np.float32)
        q = np.zeros((max(out_rows, 1), max(S, 1)), np.uint16); vt = np.zeros((16, max(S, 1), max(Tpad, 1)), np.uint16)
        p = lambda a, name: None if null == name else a.ctypes.data_as(C.c_void_p)
        return lib.wmi_selftest_qkv_encoder(0, M, S, Tpad, rpc, p(x, "xn"), p(W, "W"), p(b, "bias"), af.SENTINEL16, out_rows, p(q, "q"), p(q, "k"),
                                            p(vt, "vt"))
    for kw in (dict(M=0), dict(S=96), dict(S=0), dict(Tpad=100), dict(Tpad=0), dict(M=129), dict(M=140, rpc=60), dict(M=256, rpc=192, Tpad=128),
               dict(M=17 * 64, rpc=64), dict(rpc=-1), dict(out_rows=69), dict(null="xn"), dict(null="W"), dict(null="bias"), dict(null="q"),
               dict(null="k"), dict(null="vt")):
        assert run(**kw) == -1, kw
    if lib.wmi_device_count() <= 0:
        assert run() in (-2, -3) and run(M=128, rpc=64) in (-2, -3)

"""CPU: the conditions tests/dec_attn_f64.py's cases rest on, the refusals of the two test hooks (wmi_selftest_attn_decoder,
wmi_selftest_attn_cross: decided before the device is touched), and the negative controls — restatements of the decoder's attention with one
classic mistake each must FAIL the same hold_case() tests/test_gpu_attn_decoder.py passes the kernels' results to.  A control that passed
would mean the GPU test cannot see that mistake: sharpen the case, not the control.

Three (fault, family) pairs are blind by arithmetic and not for want of a key (dec_attn_f64.BLIND): with q = 0 every slice maximum is
0, so exp(m_s - M) IS 1 and "weight_one" leaves the uniform family's result unchanged — it is held on the selector and the random family; a
key counted twice is counted twice in the soft-max sum too, so where it holds all the weight ("slice_overlap", "quarter_twice" on the selector) the result is
still its value — it is held on the uniform family, where every key weighs 1 / n."""
import ctypes as C

import numpy as np
import pytest

import attn_f64 as af
import dec_attn_f64 as df
from godot_whisper_amd import runtime

FAMILIES = ("selector", "uniform", "random")


def shapes():
    """(name, family -> cases) for every shape tests/test_gpu_attn_decoder.py launches"""
    out = []
    for c in df.SELF_CELLS:
        out.append((f"self cells={c}", lambda f, c=c: df.self_cases(f, c)))
        if c > 64:                                            # (the long form is launched where a row has more than 64 cells)
            out.append((f"self long cells={c}", lambda f, c=c: df.self_cases(f, c, long_form=True)))
    for cap in (64, 448):
        out.append((f"self full cache {cap}", lambda f, cap=cap: df.self_cases(f, cap, cap=cap)))
    out.append(("self long full cache 448", lambda f: df.self_cases(f, 448, cap=448, long_form=True)))
    for lf in (False, True):
        out.append((f"self lock-step{' long' if lf else ''}", lambda f, lf=lf: df.self_lockstep_cases(f, long_form=lf)))
    for H in df.HEADS:
        for c in df.HEAD_CELLS:
            out.append((f"self H={H} cells={c}", lambda f, H=H, c=c: df.self_cases(f, c, H=H, rows=4, limit=2)))
    for c in df.SELF_CELLS:
        out.append((f"dec n=1 cells={c}", lambda f, c=c: df.dec_row_cases(f, c)))
    for n, n_past in df.DEC_PROMPTS:
        out.append((f"dec n={n} n_past={n_past}", lambda f, n=n, p=n_past: df.dec_prompt_cases(f, n, p, cap=448 if n < 448 else None)))
    for T in df.CROSS_T:
        out.append((f"cross T={T}", lambda f, T=T: df.cross_cases(f, T)))
    for H in (6, 8):
        out.append((f"cross T=1500 H={H}", lambda f, H=H: df.cross_cases(f, 1500, n=3, H=H, limit=2)))
    out.append(("cross lock-step", lambda f: df.cross_lockstep_cases(f)))
    out.append(("cross lock-step H=12", lambda f: df.cross_lockstep_cases(f, lens=(385, 193, 97, 1), H=12)[:3]))
    for H, T in ((2, 385), (2, 1500), (12, 385), (20, 193)):
        out.append((f"cross one query T={T}{'' if H == 2 else f' H={H}'}", lambda f, H=H, T=T: df.cross_cases(f, T, n=3, H=H, same_q=True, limit=2)))
    out.append(("cross lock-step one query", lambda f: df.cross_lockstep_cases(f, same_q=True)[:2]))
    return out


SHAPES = shapes()


# ---------------------------------------------------------------------------------------------- the generators' conditions
def test_values_are_distinct_per_head_and_exact():
    v = df.values(3, 1500, 128).astype(np.float64)
    assert ((v * 16) % 1 == 0).all() and np.abs(v).max() < 8 and np.abs(v).sum(0).max() * 16 < 2 ** 24       # every partial sum is an f32 integer / 16
    for h in range(2):
        assert len({r.tobytes() for r in v[:, 64 * h:64 * h + 64]}) == 1500
    assert np.exp(-af.SELECTOR_MARGIN) < 2.0 ** -25                                   # below half of f16's smallest subnormal


def test_plans_and_boundaries():
    assert [df.xattn_plan(T) for T in (1, 192, 193, 1344, 1345, 1500)] == [(1, 1), (1, 192), (2, 97), (7, 192), (8, 169), (8, 188)]
    assert {df.xattn_plan(T)[0] for T in df.CROSS_T} == set(range(1, 9))
    keys = df.boundary_keys("cross", 1500)
    assert {0, 1499} <= set(keys) and all({s * 188 - 1, s * 188} <= set(keys) for s in range(1, 8))
    assert all({s * 188 + w * 48 - 1, s * 188 + w * 48} <= set(keys) for s in range(8) for w in range(1, 4))          # kpw = roundup8(47) = 48
    keys = df.boundary_keys("self", 257, long_form=True)
    assert all({m - 1, m} <= set(keys) for m in list(range(8, 257, 8)) + [65, 130, 195])                                # quarters of 65
    assert {0, 256, 64 + 8, 65 + 8} <= set(keys)
    assert set(df.boundary_keys("dec", 300)) >= {0, 299, 31, 32, 255, 256}
    assert df.boundary_keys("self", 1) == [0] and df.boundary_keys("cross", 2) == [0, 1]


@pytest.mark.parametrize("family", FAMILIES)
def test_poison_is_finite_and_behind_every_length(family):
    for c in (df.self_lockstep_cases(family)[0], df.cross_lockstep_cases(family)[0], df.dec_prompt_cases(family, 5, 60, cap=448)[0]):
        for r in range(c.rows):
            seen = max(c.vis[i] for i in range(c.n) if c.crow[i] == r)
            for a in (c.k[r], c.v[r]):
                tail = a[seen:].astype(np.float64)
                assert tail.shape[0] == c.cells - seen and (np.abs(tail) == af.POISON).all()
                assert np.isfinite(a[:seen].astype(np.float64)).all() and np.abs(a[:seen].astype(np.float64)).max() < 100
    full = df.self_cases(family, 64, cap=64)[0]
    assert np.abs(full.k.astype(np.float64)).max() < 100                                # a full cache: nothing poisoned


def test_selector_lead_holds_at_every_row():
    for c in df.cross_cases("selector", 1500, limit=2) + df.self_cases("selector", 448, limit=2) + df.dec_prompt_cases("selector", 200, 0) + \
            df.cross_cases("selector", 385, n=3, same_q=True, limit=2) + df.cross_lockstep_cases("selector")[:2]:
        assert df.selector_lead(c) >= af.SELECTOR_MARGIN
        # the restatement with the reference's rounding points returns the selected rows exactly: every other numerator is 0 in f16
        assert np.array_equal(df.attend_ref_points(c.q, c.k, c.v, c.vis, c.crow, f16_result=True), c.expected())
    c = df.dec_prompt_cases("selector", 200, 0)[0]
    assert all(c.pi[i] <= i for i in range(200)) and sum(c.pi[i] == i for i in range(200)) >= 66 and c.mask().shape == (200, 200)
    assert (c.mask()[7, :8] == 0).all() and np.isneginf(c.mask()[7, 8:]).all()


def test_uniform_bound_sees_one_key():
    """one key more or less moves some element by more than the derived bound, in both result types, at the longest rows of every kind"""
    for c in (df.cross_cases("uniform", 1500)[0], df.self_cases("uniform", 448, cap=448)[0], df.dec_prompt_cases("uniform", 448, 0)[0]):
        i = c.n - 1
        v = c.v[c.crow[i], :c.vis[i]].astype(np.float64)
        moved = np.abs(c.uniform_p(i) * v[:-1].sum(0) - c.expected()[i])
        for want_f32 in (False, True):
            assert (moved > 2 * c.uniform_bound(want_f32)[i]).any(), c.name


# ---------------------------------------------------------------------------------------------- the judge accepts the faithful restatement
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=[n for n, _ in SHAPES])
def test_faithful_restatement_passes(shape, family):
    worst = {}
    def hold(kind, measured, limit, what=None):
        worst[kind] = max(worst.get(kind, 0.0), measured)
        assert measured <= limit, (kind, what, measured, limit)
    for c in SHAPES[shape][1](family):
        for variant in ("slices", "global") if c.kind == "cross" else ("points",):
            for want_f32 in (False, True):
                raw, parts = df.restate(c, want_f32, variant=variant)
                df.hold_case(c, raw, want_f32, variant, hold, partials=parts if c.ragged else None)


# ---------------------------------------------------------------------------------------------- negative controls
CONTROL_SHAPES = [n for n, _ in SHAPES if n in ("self cells=33", "self cells=257", "self long cells=257", "self long cells=66", "self lock-step",
                                                  "self lock-step long", "self H=12 cells=40", "dec n=1 cells=257", "dec n=5 n_past=60",
                                                  "dec n=200 n_past=0", "cross T=193", "cross T=1345", "cross T=1500", "cross T=1500 H=6",
                                                  "cross lock-step", "cross one query T=385")]


def _refused(c, fault, want_f32):
    raw, _ = df.restate(c, want_f32, fault)
    try:
        df.hold_case(c, raw, want_f32, fault)
    except AssertionError:
        return True
    return False


def test_every_classic_mistake_fails_hold_case():
    by_name = dict(SHAPES)
    pairs = skipped = 0
    refused_somewhere = set()
    for name in CONTROL_SHAPES:
        cases = {family: by_name[name](family) for family in ("selector", "uniform")}
        probe = cases["uniform"][0]
        for fault in df.FAULTS_OF[df.fault_kind(probe)]:
            pairs += 1
            seen = {}
            for family in ("selector", "uniform"):
                if (fault, family) in df.BLIND:
                    continue                                   # (module docstring)
                for want_f32 in (False, True):
                    got = []
                    for c in cases[family]:
                        try:
                            got.append(_refused(c, fault, want_f32))
                        except df.NoSuchKey:
                            pass
                    if got:
                        seen[(family, want_f32)] = any(got)
            if not seen:
                skipped += 1
                continue
            assert all(seen.values()), (name, fault, "passed hold_case", seen)
            refused_somewhere.add(fault)
    assert refused_somewhere == set(df.FAULTS), set(df.FAULTS) - refused_somewhere
    assert skipped * 4 < pairs, (skipped, pairs)


def test_weight_one_is_seen_by_the_random_family():
    assert df.BLIND == {("weight_one", "uniform"), ("slice_overlap", "selector"), ("quarter_twice", "selector")}
    for T in (193, 1500):
        for c in df.cross_cases("random", T):
            raw, _ = df.restate(c, True, "weight_one")
            with pytest.raises(AssertionError):
                df.hold_case(c, raw, True, "weight_one")


def test_stale_partials_fail_the_neutral_check_on_their_own():
    c = df.cross_lockstep_cases("uniform")[0]
    raw, parts = df.restate(c, True)
    df.hold_case(c, raw, True, "", partials=parts)
    _, stale = df.restate(c, True, "stale_partial")
    with pytest.raises(AssertionError, match="not neutral"):
        df.hold_case(c, raw, True, "", partials=stale)


def test_selector_failure_names_the_key_that_was_read():
    c = df.cross_cases("selector", 193)[0]
    raw, _ = df.restate(c, False)
    raw[0] = raw[1]                                          # row 0 read row 1's key
    assert c.pi[0] != c.pi[1]
    with pytest.raises(AssertionError, match=r"expected key \d+ of 193, the row equals key\(s\) \[\d+"):
        df.hold_case(c, raw, False)
    c = df.self_cases("selector", 33)[0]
    raw, _ = df.restate(c, True)
    raw[c.n] = raw[0]
    with pytest.raises(AssertionError, match="rows behind the launch"):
        df.hold_case(c, raw, True)


# ---------------------------------------------------------------------------------------------- the random family's ratios of the restatements
@pytest.mark.parametrize("variant,T", [("points", 33), ("points", 257), ("points", 448), ("slices", 193), ("slices", 777), ("slices", 1500),
                                       ("global", 193), ("global", 1500)])
def test_restatement_ratios_stay_within_the_limits(variant, T):
    seen = []
    def hold(kind, measured, limit, what=None):
        seen.append((measured, limit))
        assert measured <= limit, (kind, what, measured, limit)
    for c in (df.self_cases("random", T) if variant == "points" else df.cross_cases("random", T)):
        for want_f32 in (False, True):
            raw, _ = df.restate(c, want_f32, variant=variant)
            df.hold_case(c, raw, want_f32, variant, hold)
    assert len(seen) == 12 and {lim for _, lim in seen} == {af.RMS_LIMIT, af.MAX_LIMIT} and min(m for m, _ in seen) > 0
    print(variant, T, "worst rms ratio %.3f, worst max ratio %.3f" % (max(m for m, l in seen if l == af.RMS_LIMIT), max(m for m, l in seen if l == af.MAX_LIMIT)))


# ---------------------------------------------------------------------------------------------- the hooks' refusals
def _p(a, null=False):
    return None if a is None or null else a.ctypes.data_as(C.c_void_p)


def _dec(lib, form=1, n=2, S=128, H=2, cap=64, cache_rows=None, n_kv=(5, 64), via_dev=0, long_cache=0, want_f32=0, out_rows=None, null=None):
    cache_rows = (1 if form == 0 else n) if cache_rows is None else cache_rows
    out_rows = n if out_rows is None else out_rows
    q = np.zeros((max(n, 1), max(S, 1)), np.uint16); kc = np.zeros((max(cache_rows, 1), max(cap, 1), max(S, 1)), np.uint16)
    nk = np.asarray(n_kv, np.int32); mask = np.zeros((max(n, 1), max(int(nk[0]), 1)), np.float32)
    out = np.zeros((max(out_rows, 1), max(S, 1)), np.uint32)
    return lib.wmi_selftest_attn_decoder(0, form, n, S, H, cap, cache_rows, _p(nk, null == "n_kv"), _p(mask, null == "mask"), via_dev, long_cache, want_f32,
                                         _p(q, null == "q"), _p(kc, null == "k"), _p(kc, null == "v"), af.SENTINEL16, out_rows, _p(out, null == "out"))


def test_decoder_hook_refuses_what_the_product_cannot_launch():
    lib = runtime.load_library()
    bad = [dict(form=3), dict(form=-1), dict(n=0), dict(n=17), dict(S=96), dict(S=128, H=3), dict(H=0, S=0), dict(S=1344, H=21), dict(cap=0), dict(cap=4),
           dict(n_kv=(0, 5)), dict(n_kv=(5, 65)), dict(cache_rows=1), dict(out_rows=1), dict(null="q"), dict(null="k"), dict(null="v"), dict(null="out"),
           dict(null="n_kv"), dict(form=0, n=2, n_kv=(9,), null="mask"), dict(form=0, n=2, n_kv=(1,)), dict(form=0, n=2, n_kv=(65,)),
           dict(form=0, n=2, n_kv=(9,), cache_rows=2), dict(form=0, n=2, n_kv=(9,), long_cache=1), dict(form=1, via_dev=1), dict(long_cache=1), dict(long_cache=1, n_kv=(64, 64)), dict(form=2, want_f32=0),
           dict(form=2, want_f32=1, long_cache=1), dict(form=0, n=449, cap=449, n_kv=(449,))]
    for kw in bad:
        assert _dec(lib, **kw) == -1, kw
    if lib.wmi_device_count() <= 0:
        for kw in (dict(), dict(long_cache=1, cap=128, n_kv=(5, 65)), dict(form=0, n=2, n_kv=(9,)), dict(form=0, n=2, n_kv=(9,), via_dev=1), dict(form=2, want_f32=1),
                   dict(form=2, want_f32=1, n=1, n_kv=(64,))):
            assert _dec(lib, **kw) in (-2, -3), kw


def _cross(lib, form=0, consumer=0, n=2, S=128, H=2, T=200, kv_rows=1, row_lens=None, want_f32=0, lanes=0, qscale=1.0, out_rows=None, null=None):
    out_rows = n if out_rows is None else out_rows
    q = np.zeros((max(n, 1), max(S, 1)), np.float32 if form == 2 else np.uint16)
    kc = np.zeros((max(kv_rows, 1), max(T, 1), max(S, 1)), np.uint16)
    rl = None if row_lens is None else np.asarray(row_lens, np.int32)
    out = np.zeros((max(out_rows, 1), max(S, 1)), np.uint32)
    pm = np.zeros((max(n, 1), max(H, 1), 16), np.float32); po = np.zeros((max(n, 1), max(H, 1), 16, 64), np.float32); info = np.zeros(2, np.int32)
    return lib.wmi_selftest_attn_cross(0, form, consumer, n, S, H, T, kv_rows, _p(rl), want_f32, lanes, _p(q, null == "q"), C.c_float(qscale),
                                       _p(kc, null == "k"), _p(kc, null == "v"), af.SENTINEL16, out_rows, _p(out, null == "out"),
                                       _p(pm, null == "pmax"), _p(pm.copy(), null == "part_l"), _p(po, null == "part_o"), _p(info, null == "info"))


def test_cross_hook_refuses_what_the_product_cannot_launch():
    lib = runtime.load_library()
    bad = [dict(form=3), dict(form=-1), dict(consumer=2), dict(form=0, consumer=1), dict(n=0), dict(n=17), dict(S=96), dict(S=128, H=3), dict(T=0), dict(T=1501),
           dict(kv_rows=3), dict(kv_rows=0), dict(out_rows=1), dict(null="q"), dict(null="k"), dict(null="v"), dict(null="out"), dict(null="info"),
           dict(form=1, null="pmax"), dict(form=1, null="part_l"), dict(form=1, null="part_o"),
           dict(form=0, row_lens=[200, 5], kv_rows=2), dict(form=1, row_lens=[200, 0], kv_rows=2), dict(form=1, row_lens=[201, 5], kv_rows=2),
           dict(form=1, row_lens=[200, 5]), dict(form=1, row_lens=[150, 5], kv_rows=2),
           dict(form=1, consumer=1, want_f32=0), dict(form=1, consumer=1, want_f32=1, n=9), dict(form=1, consumer=1, want_f32=1, n=1, lanes=1),
           dict(form=1, consumer=0, lanes=1), dict(form=2, S=1600, H=25), dict(form=2, consumer=1, want_f32=1), dict(form=2, qscale=float("nan"))]
    for kw in bad:
        assert _cross(lib, **kw) == -1, kw
    if lib.wmi_device_count() <= 0:
        for kw in (dict(), dict(form=1), dict(form=1, row_lens=[200, 5], kv_rows=2), dict(form=1, consumer=1, want_f32=1), dict(form=1, consumer=1, want_f32=1, lanes=1),
                   dict(form=2), dict(form=2, S=1280, H=20)):
            assert _cross(lib, **kw) in (-2, -3), kw


def test_hooks_are_bound():
    lib = runtime.load_library()
    assert lib.wmi_selftest_attn_decoder.restype is C.c_int and len(lib.wmi_selftest_attn_decoder.argtypes) == 18
    assert lib.wmi_selftest_attn_cross.restype is C.c_int and len(lib.wmi_selftest_attn_cross.argtypes) == 22

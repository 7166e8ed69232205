"""The float64 restatement of the logit filters (tests/filters_f64.py) against the host definition (csrc/host_logic.cpp through
wmi_process_logits) on a host-only context — no GPU — for EVERY case tests/test_gpu_filters.py runs on the device:

    the allowed set matches exactly . id and tid match exactly . p, plog, pt and ptsum of the picked entry lie within PICK_TOL of the
    float64 values . the case meets the conditions on the inputs (filters_f64.check_conditions) and does what its pattern is about

That proves the yardstick before a GPU is involved, and that the host definition alone stays inside the bound on the chosen inputs
(a left-to-right f32 soft-max over 51 864 terms loses the terms that fall under half an ulp of the running sum: measured here up to
7.6e-5 in plog and 2.5e-5 in p on the N(0, 3^2) pattern, under 1.4e-5 on the draw cases).
The worst host-vs-float64 difference per field is printed per vocabulary.  The hook's argument checks are held here as well: on a
host-only context every one of them must answer before the "cannot compute" code, i.e. before anything could touch a device."""
import ctypes as C

import numpy as np
import pytest

import filters_f64 as ff
from godot_whisper_amd import abi, runtime, synth

PICK_TOL = 1e-4                  # tests/test_gpu_decode_lengths.py (not imported: that module is -m gpu)
FIELDS = ("p", "plog", "pt", "ptsum")


def host_model(label):
    """a model of the vocabulary `label` for a host-only context: the filters read the vocabulary and n_audio_ctx only, so the
    51 866-token vocabulary rides on micro's widths"""
    if label == "v3-slice":
        return synth.make_model((51866, 1500, 128, 2, 2, 448, 128, 2, 3, 128), seed=1234)
    return synth.make_model(label, seed=1234)


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


@pytest.fixture(scope="module", params=ff.VOCABS)
def host(lib, request):
    h = ff.HostSide(lib, host_model(request.param))
    h.label = request.param
    yield h
    h.close()


def compare(host, case, worst, tid_default=0):
    r = ff.evaluate(case.raw, host.v, case.state, case.temperature)
    ff.check_conditions(r, case.name)
    lo, got = host.pick(case.raw, case.state, case.temperature, tid_default)
    assert np.array_equal(lo > -np.inf, r.cand), (case.name, np.flatnonzero((lo > -np.inf) != r.cand)[:8])
    want = r.pick(tid_default)
    assert got[:2] == want[:2], (case.name, got, want, r.gaps)
    for k, a, b in zip(FIELDS, got[2:], want[2:]):
        d = abs(a - b)
        worst[k] = max(worst[k], d)
        assert d <= PICK_TOL, (case.name, k, a, b)
    e = case.expect
    if "id" in e:
        assert r.id == e["id"], (case.name, r.id, e)
    if "force_ts" in e:
        assert r.force_ts == e["force_ts"], (case.name, r.gaps)
    if e.get("tid0"):
        assert want[1] == tid_default and want[4] == 0.0 and want[5] < 1e-30, (case.name, want)
    if e.get("flat"):
        assert r.id == int(np.flatnonzero(r.cand)[0]) and abs(r.p - 1.0 / int(r.allowed.sum())) < 1e-12, case.name
    return r


def test_host_filters_agree_with_float64_on_every_case(host):
    worst = dict.fromkeys(FIELDS, 0.0)
    n = 0
    for sn in ff.states_of(host.label):
        for temps in (ff.TEMPS, (0.0, 0.5)):                 # modes 0 / 2, and the fused form's temperatures
            cases, dropped = ff.make_cases(host.v, ff.STATE[sn], temps=temps)
            names = set()
            for c in cases:
                assert c.name not in names, c.name
                names.add(c.name)
                compare(host, c, worst); n += 1
    print(f"\n{host.label}: {n} cases, worst |host - float64| " + ", ".join(f"{k} {worst[k]:.2e}" for k in FIELDS))
    assert n > 0


def test_draw_cases_and_their_targets(host):
    worst = dict.fromkeys(FIELDS, 0.0)
    stretch = 0
    for sn, forced in ff.DRAW_STATES:
        for T in ff.TEMPS:
            c = ff.make_draw_case(host.v, ff.STATE[sn], T, forced)
            r = compare(host, c, worst, tid_default=host.v.beg)
            idx, cdf = r.cdf()
            assert (r.logprobs[idx] >= ff.POS).all(), c.name       # "p > 0" means the same set in f32 and in float64
            assert r.draw(0.0) == idx[0] and r.draw(1.0 - 2.0 ** -53) == idx[-1], c.name
            for t in c.targets:
                assert r.probs[t] >= 1e-5, (c.name, t, r.probs[t])
                assert r.draw(r.cell_mid(t)) == t, (c.name, t)
            stretch += c.expect["empty_stretch"] is not None
    assert stretch >= 2, "two states must leave a stretch of empty blocks in front of a positive token"
    print(f"\n{host.label}: draw cases, worst |host - float64| " + ", ".join(f"{k} {worst[k]:.2e}" for k in FIELDS))


def test_dropped_products_are_named(host):
    v = host.v
    drop = {sn: ff.make_cases(v, ff.STATE[sn])[1] for sn in ff.states_of(host.label)}
    assert "ts-mass wins" in drop["no_timestamps"] and "ts underflow" in drop["no_timestamps"]
    if "[ts,ts]" in drop:
        assert "ts-mass wins" in drop["[ts,ts]"] and "all equal" in drop["has_ts seek 3000"]
    assert drop["[text,text]"] == [] and drop["initial"] == []


def _call(lib, ctx, mode=0, n_rows=1, logits=True, out=True, W=None, x=None, K=0, lo=None, u=None, k=1, n_hist=True, nv=51864):
    z = np.zeros(nv * max(n_rows, 1) if logits else 1, np.float32)
    td = (abi.whisper_token_data * 64)()
    nh = (C.c_int * 16)(); hs = (C.c_int * 16)(); sd = (C.c_int * 16)()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return lib.wmi_selftest_filters(ctx, lib.whisper_full_default_params(0), mode, n_rows, vp(z) if logits else None, None,
                                    nh if n_hist else None, hs, sd, C.c_float(0.0), vp(W), vp(x), K, vp(lo), vp(u), k, 0,
                                    td if out else None)


def test_hook_argument_checks_come_before_the_device(lib, host):
    ctx, nv = host.ctx, host.v.n_vocab
    c = lambda **kw: _call(lib, ctx, nv=nv, **kw)
    x = np.ones(128, np.float32); W = np.zeros((8, 128), np.float16); lo = np.zeros(nv, np.float32); u = np.zeros(64, np.float64)
    assert _call(lib, None) == -1
    for bad in (dict(mode=-1), dict(mode=3), dict(n_rows=0), dict(n_rows=17), dict(logits=False), dict(out=False), dict(n_hist=False),
                dict(mode=1, W=W, x=x, K=128, lo=lo, n_rows=2), dict(mode=1, x=x, K=128, lo=lo), dict(mode=1, W=W, K=128, lo=lo),
                dict(mode=1, W=W, x=x, K=128), dict(mode=1, W=W, x=x, K=0, lo=lo),
                dict(mode=2, u=u, n_rows=0), dict(mode=2, u=u, n_rows=9), dict(mode=2, u=u, k=0), dict(mode=2, u=u, k=9), dict(mode=2),
                dict(mode=2, u=u, logits=False)):
        assert c(**bad) == -1, bad
    # a projection that cannot take the fused path: its own code, before the context is asked whether it can compute
    for K in (12, 1544, 2048):
        assert c(mode=1, W=W, x=x, K=K, lo=lo) == -4, K
    # well-formed calls reach "cannot compute" on a host-only context
    assert c() == -2 and c(n_rows=16) == -2 and c(mode=1, W=W, x=x, K=128, lo=lo) == -2 and c(mode=2, u=u, n_rows=8, k=8) == -2

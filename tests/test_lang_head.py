"""Language detection, the host half (csrc/host_logic.cpp: lang_probs_from_logits): 100 f32 logits -> (id, probs[100]).  Every
detection route — the full vocabulary projection of whisper_lang_auto_detect, the language head of whisper_full / wmi_lang_detect and
the lock-step rows of wmi_full_batch — ends in this one helper, so the routes agree bit for bit whenever their 100 logits do.  Held
here, without a device, against a restatement of W/whisper.cpp:3600-3641 with the product's tie order."""
import ctypes as C
import math

import numpy as np

from godot_whisper_amd import runtime

N_LANG = 100


def lang_codes(lib):
    return [bytes(lib.whisper_lang_str(i)) for i in range(N_LANG)]


def restate(logits, codes):
    """W/whisper.cpp:3600-3641: (logit, id) pairs in the order of the reference's std::map (by language code; bytes compare as strcmp does),
    sorted by logit descending — stable, so equal logits keep the code order —, exp relative to the maximum in double, summed in that
    order, divided, narrowed to float."""
    cand = sorted(range(N_LANG), key=lambda i: codes[i])
    cand.sort(key=lambda i: -float(logits[i]))                  # list.sort is stable
    mx = float(logits[cand[0]])
    e = [math.exp(float(logits[i]) - mx) for i in cand]
    s = 0.0
    for x in e:
        s += x
    probs = np.zeros(N_LANG, np.float32)
    for i, x in zip(cand, e):
        probs[i] = np.float32(x / s)
    return cand[0], probs


def product(lib, logits):
    lg = np.ascontiguousarray(logits, np.float32)
    out = np.full(N_LANG, -1.0, np.float32)
    lid = lib.wmi_selftest_lang_probs(lg.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    return lid, out


def vectors():
    rng = np.random.default_rng(3100)
    out = []
    for scale in (0.05, 1.0, 7.0):
        for _ in range(4):
            out.append(("random x%g" % scale, (rng.standard_normal(N_LANG) * scale).astype(np.float32)))
    v = (rng.standard_normal(N_LANG) * 2.0).astype(np.float32)
    top = np.float32(v.max() + 1.5)
    v[[83, 12]] = top                                            # two exact ties at the top ...
    v[[40, 41, 7]] = np.float32(v.min() - 0.25)                  # ... and three at the bottom
    out.append(("ties", v))
    out.append(("all equal", np.full(N_LANG, np.float32(-3.25))))
    v = (rng.standard_normal(N_LANG) * 3.0).astype(np.float32); v[57] = -np.inf
    out.append(("one -inf", v))
    v = np.linspace(-45.0, 15.0, N_LANG).astype(np.float32); rng.shuffle(v)
    out.append(("60-unit spread", v))
    return out


def test_language_probabilities_equal_the_restated_reference():
    lib = runtime.load_library()
    codes = lang_codes(lib)
    assert len(set(codes)) == N_LANG and codes[0] == b"en"
    for name, v in vectors():
        want_id, want = restate(v, codes)
        got_id, got = product(lib, v)
        assert got_id == want_id, (name, got_id, want_id)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, np.abs(got - want).max())
        assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-5, name


def test_ties_go_to_the_first_language_code():
    lib = runtime.load_library()
    codes = lang_codes(lib)
    v = np.zeros(N_LANG, np.float32)
    lid, probs = product(lib, v)
    assert codes[lid] == min(codes)                              # all equal: the smallest code, not id 0
    assert np.array_equal(probs, np.full(N_LANG, np.float32(0.01)))
    v[:] = -1.0; v[[90, 5, 33]] = 2.0
    lid, probs = product(lib, v)
    assert codes[lid] == min(codes[i] for i in (90, 5, 33))
    assert probs[90] == probs[5] == probs[33] > probs[0]
    v[57] = -np.inf
    lid2, probs2 = product(lib, v)
    assert lid2 == lid and probs2[57] == 0.0


def test_bad_arguments_are_refused():
    lib = runtime.load_library()
    v = np.zeros(N_LANG, np.float32)
    assert lib.wmi_selftest_lang_probs(None, v.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lib.wmi_selftest_lang_probs(v.ctypes.data_as(C.POINTER(C.c_float)), None) == product(lib, v)[0]       # probabilities are optional

"""CPU side of the SRC_ZERO_ORDER_HOLD (3) and SRC_LINEAR (4) converters of wmi_resample.

Ground truth is data: tests/golden/resample_zoh_linear.npz holds what libsamplerate's own src_simple, compiled from the reference
(tests/golden/make_resample_goldens.py), returned for every case of tests/resample_ref.py — frame counts and output bits.
* the product's host plan (wmi_selftest_resample_plan, no GPU needed) reports the library's output_frames_gen / input_frames_used
  and walks the double recurrence;
* the sequential Python restatement (tests/resample_ref.py), which the GPU tests use for inputs the fixture does not hold, equals
  the library bit for bit on every case.
Left out by name: SRC_LINEAR on one frame at 8000 and 11025 Hz, where the library reads data_in[-1] (resample_ref.undefined);
the product answers it with 0 frames, asserted on its own below.
"""
import ctypes as C
import math

import numpy as np
import pytest

import resample_ref as rr


@pytest.fixture(scope="module")
def fixture_cases():
    recs = rr.load_fixture()
    assert [(r["seed"], r["length"], r["rate"], r["converter"]) for r in recs] == rr.cases()      # no case dropped from the file
    assert len(recs) == len(rr.LENGTHS) * len(rr.RATES) * 2 - 2
    return recs


@pytest.fixture(scope="module")
def product_host():
    from godot_whisper_amd import runtime
    return runtime.load_library()


def _plan(lib, n, src_rate, converter, n_pos=0):
    gen, used, closed = C.c_longlong(-1), C.c_longlong(-1), C.c_int(-1)
    pos = np.zeros(max(n_pos, 1), np.int64); frac = np.zeros(max(n_pos, 1), np.float64)
    r = lib.wmi_selftest_resample_plan(n, src_rate, rr.DST_RATE, converter, C.byref(gen), C.byref(used), C.byref(closed), n_pos,
                                       C.c_void_p(pos.ctypes.data), C.c_void_p(frac.ctypes.data))
    return r, gen.value, used.value, closed.value, pos[:n_pos], frac[:n_pos]


def _exact(inc):
    """csrc/k_resample.hip: with inc = m * 2^q, m odd, no partial sum x + inc (x < 1) is ever rounded when inc + 1 <= 2^(q + 53); the
    positions then come from the 128-bit product n * m (closed form), else from the host's table."""
    m, e = math.frexp(inc)
    m, q = int(math.ldexp(m, 53)), e - 53
    while m % 2 == 0:
        m //= 2; q += 1
    return 1 if inc + 1.0 <= math.ldexp(1.0, q + 53) else 0


def test_fixture_is_what_the_host_asks_for(fixture_cases):
    """Every case ran to the capacity the host passes (no "size differ" for these converters) and consumed a sane number of frames."""
    for r in fixture_cases:
        _, cap = rr.ratio_and_capacity(r["length"], r["rate"])
        assert r["frames_gen"] == cap == r["out"].size, r
        assert 0 <= r["frames_used"] <= r["length"], r


def test_plan_reports_the_library_frame_counts(product_host, fixture_cases):
    for r in fixture_cases:
        got, gen, used, closed, _, _ = _plan(product_host, r["length"], r["rate"], r["converter"])
        key = (r["length"], r["rate"], r["converter"])
        assert got == 0, key
        assert (gen, used) == (r["frames_gen"], r["frames_used"]), key
        assert closed == _exact(1.0 / (16000.0 / r["rate"])), key
    assert {_exact(1.0 / (16000.0 / rate)) for rate in rr.RATES} == {0, 1}                      # both forms of the positions are exercised


@pytest.mark.parametrize("converter", rr.CONVERTERS)
def test_plan_positions_are_the_double_recurrence(product_host, converter):
    for rate in rr.RATES:
        for n in rr.LENGTHS:
            ratio, cap = rr.ratio_and_capacity(n, rate)
            if cap == 0 or rr.undefined(n, rate, converter):
                continue
            got, gen, _, closed, pos, frac = _plan(product_host, n, rate, converter, n_pos=cap)
            assert got == 0 and gen == cap
            want_p, want_f = rr.positions(ratio, cap)
            assert np.array_equal(pos, want_p), (rate, n, closed)
            assert frac.tobytes() == want_f.tobytes(), (rate, n, closed)


def test_restatement_equals_the_library_bit_for_bit(fixture_cases):
    for r in fixture_cases:
        ratio, cap = rr.ratio_and_capacity(r["length"], r["rate"])
        out, used = rr.src_simple(rr.make_input(r["seed"], r["length"]), ratio, r["converter"], cap)
        key = (r["length"], r["rate"], r["converter"])
        assert (out.size, used) == (r["frames_gen"], r["frames_used"]), key
        assert out.tobytes() == r["out"].tobytes(), key


def test_plan_edges(product_host):
    # SRC_LINEAR on one frame at a ratio above 1: the library reads data_in[-1]; the plan refuses it, ZOH repeats the frame
    for rate in (8000, 11025):
        assert _plan(product_host, 1, rate, rr.SRC_LINEAR)[0] == -31
        with pytest.raises(IndexError):
            rr.src_simple(np.ones(1, np.float32), 16000.0 / rate, rr.SRC_LINEAR, int(16000.0 / rate))
    assert _plan(product_host, 1, 8000, rr.SRC_ZERO_ORDER_HOLD)[:3] == (0, 2, 1)
    # a single frame going down gives nothing, whatever the converter
    assert _plan(product_host, 1, 48000, rr.SRC_LINEAR)[:3] == (0, 0, 0)
    for conv in rr.CONVERTERS:
        assert _plan(product_host, 1000, 16000 * 300, conv)[0] == -6         # SRC_ERR_BAD_SRC_RATIO, as for the SINC converters
        assert _plan(product_host, 1000, 50, conv)[0] == -6
    assert _plan(product_host, 1000, 48000, 0)[0] == -10                      # SRC_SINC_BEST_QUALITY: unchanged
    assert _plan(product_host, 1000, 48000, 5)[0] == -10                      # no such converter

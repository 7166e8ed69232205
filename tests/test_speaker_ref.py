"""CPU: the judge of the speaker labels (tests/speaker_ref.py) refuses the usual wrong answers, and the library's host side
(csrc/speaker_ranges.h through wmi_selftest_speaker_ranges) equals it on the judge's own tables — with `==`: for s16 and s8 also against
the straight sequential loop over the samples (every partial sum of that loop is a multiple of 2^-15 or 2^-7 below 2^31, so the order of
addition cannot show), for f32 against the same left-to-right addition of the judge's bins.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

import speaker_ref as sr
from godot_whisper_amd import abi, runtime, synth

RATES = [16000, 44100, 22050, 11025, 150, 63, 4096000]
COUNTS = [0, 1, 2, 159, 160, 161, 48001]
FORMATS = [sr.S16, sr.S8, sr.F32]


@pytest.fixture(scope="module")
def lib():
    return runtime.load_library()


def _ranges(n, rate):
    nb = sr.n_bins(n, rate)
    big = 2 ** 40                                               # t * rate far beyond 2^31 (and, at 4.096 MHz, beyond 2^61)
    out = [(0, 0), (0, 1), (1, 0), (3, 3), (0, nb), (0, max(nb - 1, 0)), (max(nb - 1, 0), nb), (max(nb - 2, 0), nb + 7), (nb, nb + 5),
           (nb + 1, nb + 2), (0, nb + 100), (nb // 3, 2 * nb // 3), (2 * nb // 3, nb // 3), (1, 2), (0, big), (big, 2 * big),
           (nb // 2, 2 ** 62 // max(rate, 1)), (0, 2 ** 62)]
    return out


def _selftest(lib, bins, last2, fmt, n, rate, ranges, ratio=0.0):
    t0 = np.array([r[0] for r in ranges], np.int64); t1 = np.array([r[1] for r in ranges], np.int64)
    out = (abi.wmi_speaker * len(ranges))()
    b = np.ascontiguousarray(bins)
    rc = lib.wmi_selftest_speaker_ranges(b.ctypes.data if b.size else None, b.shape[0], last2.ctypes.data, fmt, n, rate, ratio,
                                         t0.ctypes.data, t1.ctypes.data, len(ranges), out)
    assert rc == 0, rc
    return [dict(speaker=o.speaker, is0=o.is0, is1=o.is1, e0=o.e0, e1=o.e1) for o in out]


@pytest.mark.parametrize("fmt", FORMATS, ids=["s16", "s8", "f32"])
@pytest.mark.parametrize("rate", RATES)
def test_host_ranges_equal_the_judge(lib, fmt, rate):
    for n in COUNTS:
        data = sr.crafted(fmt, n, seed=rate % 1000 + n)
        bins, last2 = sr.table(data, fmt, rate)
        assert bins.shape[0] == sr.n_bins(n, rate)
        ranges = _ranges(n, rate)
        got = _selftest(lib, bins, last2, fmt, n, rate, ranges)
        x = sr.channels(data, fmt)
        for (t0, t1), g in zip(ranges, got):
            want = sr.speaker_from_table(bins, fmt, n, rate, t0, t1)
            assert g == want, (fmt, rate, n, t0, t1, g, want)
            straight = sr.speaker(x, rate, t0, t1)
            assert (g["is0"], g["is1"]) == (straight["is0"], straight["is1"])
            if fmt != sr.F32:
                assert g == straight, (fmt, rate, n, t0, t1, g, straight)          # bit for bit, labels included
            else:
                m = straight["is1"] - straight["is0"]
                for c in ("e0", "e1"):
                    assert abs(g[c] - straight[c]) <= sr.f32_bound(m, straight[c]), (rate, n, t0, t1, c, g[c], straight[c])


def test_ties_and_the_ratio(lib):
    """equal channel sums, and one channel exactly 1.1 times the other as nearly as integers allow, on either side"""
    rate, n = 16000, 321
    for l, r, ratio in [(1000, 1000, 0.0), (1100, 1000, 0.0), (1101, 1000, 0.0), (1099, 1000, 0.0), (1000, 1100, 0.0), (1000, 1101, 0.0),
                        (2000, 1000, 2.0), (2001, 1000, 2.0), (1000, 2000, 2.0), (11, 10, 0.0), (0, 0, 0.0), (0, 1, 0.0), (32768 * 160, 1, 0.0)]:
        v = np.zeros((n, 2), np.int64)
        v[:160, 0] = l // 160; v[0, 0] += l % 160
        v[:160, 1] = -(r // 160); v[1, 1] -= r % 160
        v[:, 0] = np.clip(v[:, 0], -32768, 32767)
        data = sr.pack(v.reshape(-1), sr.S16)
        bins, last2 = sr.table(data, sr.S16, rate)
        got = _selftest(lib, bins, last2, sr.S16, n, rate, [(0, 1), (0, 3)], ratio)
        for (t0, t1), g in zip([(0, 1), (0, 3)], got):
            want = sr.speaker_of_clip(data, sr.S16, rate, t0, t1, ratio if ratio > 0 else sr.RATIO)
            assert g == want, (l, r, ratio, g, want)
    # the three outcomes all occur above
    assert {sr.label(1100.0 / 32768, 1000.0 / 32768), sr.label(1101.0 / 32768, 1000.0 / 32768), sr.label(1000.0 / 32768, 1101.0 / 32768)} == {-1, 0, 1}


def _case(name):
    """a clip, a range and a ratio on which the mistake shows"""
    rng = np.random.default_rng(5)
    n = 2000
    v = np.stack([rng.integers(-20000, 20000, n), rng.integers(-3000, 3000, n)], axis=1)
    if name == "abs_narrow":
        v[500] = (-32768, -32768)
    s16 = sr.pack(v.reshape(-1), sr.S16)
    if name == "s8_unsigned":
        return sr.pack(np.stack([rng.integers(-128, 0, n), rng.integers(0, 127, n)], axis=1).reshape(-1), sr.S8), sr.S8, 16000, 0, 5, sr.RATIO
    if name == "f32_accumulators":
        x = (rng.random((40000, 2)) + 0.5).astype(np.float32)
        return sr.pack(x.reshape(-1), sr.F32), sr.F32, 16000, 0, 240, sr.RATIO
    if name == "no_clamp":
        return s16, sr.S16, 16000, 3, 500, sr.RATIO
    if name == "clamp_is1_only":
        return s16, sr.S16, 16000, 400, 500, sr.RATIO
    if name == "ratio_wrong_side":
        w = np.zeros((400, 2), np.int64); w[:160, 0] = 105; w[:160, 1] = 100
        return sr.pack(w.reshape(-1), sr.S16), sr.S16, 16000, 0, 1, sr.RATIO
    if name == "ge":
        w = np.zeros((400, 2), np.int64); w[:160, 0] = 200; w[:160, 1] = 100
        return sr.pack(w.reshape(-1), sr.S16), sr.S16, 16000, 0, 1, 2.0
    if name == "rate_16000":
        return s16, sr.S16, 44100, 1, 3, sr.RATIO
    return s16, sr.S16, 16000, 2, 7, sr.RATIO


@pytest.mark.parametrize("name", sr.VARIANTS)
def test_the_judge_refuses(name):
    data, fmt, rate, t0, t1, ratio = _case(name)
    good = sr.speaker_of_clip(data, fmt, rate, t0, t1, ratio)
    bad = sr.variant(name, data, fmt, rate, t0, t1, ratio)
    assert bad != good, (name, good)
    # and the unmistaken restatement is the judge
    assert sr.variant("none", data, fmt, rate, t0, t1, ratio) == good


def test_the_reference_at_16k_is_the_definition():
    """main.cpp:41-43: min(max(0, (t * 16000) / 100), n_samples - 1) = is(t) at rate 16000"""
    for n in (1, 160, 161, 48001):
        for t in (0, 1, 2, 299, 300, 301, 10 ** 9):
            assert sr.sample_of(t, n, 16000) == min(max(0, t * 16000 // 100), n - 1)


def test_error_codes_without_a_device(lib):
    assert lib.wmi_set_speaker(None, 1, 1.1) == -2
    assert lib.wmi_full_get_segment_speaker(None, 0, None) == -1
    assert lib.wmi_full_get_token_speaker(None, 0, 0, None) == -1
    mb = synth.make_model("micro.en", seed=1)
    buf = C.create_string_buffer(mb, len(mb))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(mb))
    assert ctx
    try:
        assert lib.wmi_set_speaker(ctx, 3, 1.1) == -1 and lib.wmi_set_speaker(ctx, -1, 1.1) == -1
        assert lib.wmi_set_speaker(ctx, 1, 1.1) == 0 and lib.wmi_set_speaker(ctx, 2, -5.0) == 1 and lib.wmi_set_speaker(ctx, 0, float("nan")) == 2
        rec = abi.wmi_speaker()
        assert lib.wmi_full_get_segment_speaker(ctx, 0, C.byref(rec)) == -1            # no segment 0
        raw = C.create_string_buffer(bytes(64), 64)
        t = np.zeros(1, np.int64)
        out = (abi.wmi_speaker * 1)()

        def call(fmt=sr.S16, stereo=1, rate=48000, n_bytes=64, data=raw, n=1, t0=t, on_device=0):
            w = abi.wmi_wav(C.cast(data, C.c_void_p) if data is not None else None, n_bytes, fmt, stereo, rate, on_device)
            return lib.wmi_wav_speaker(ctx, C.byref(w), t0.ctypes.data if t0 is not None else None, t.ctypes.data, n, 0.0, out)
        assert call(stereo=0) == -12
        assert call(fmt=2) == -11 and call(fmt=3) == -11
        assert call(fmt=7) == -1 and call(stereo=2) == -1 and call(rate=0) == -1 and call(n_bytes=-1) == -1 and call(data=None) == -1
        assert call(n=-1) == -1 and call(t0=None) == -1
        assert lib.wmi_wav_speaker(None, None, None, None, 0, 0.0, None) == -1
        assert call() == -2                                                              # a context that cannot compute: after every argument
        assert call(rate=7) == -2                                                        # any positive rate is an argument the call takes
        nb = C.c_longlong(-1)
        w = abi.wmi_wav(C.cast(raw, C.c_void_p), 64, sr.S16, 0, 16000, 0)
        assert lib.wmi_selftest_channel_bins(0, C.byref(w), None, 0, C.byref(nb), out) == -12
        st = (C.c_int64 * 4)(1, 1, 1, 1)
        assert lib.wmi_speaker_stats(ctx, st) == 0 and list(st) == [0, 0, 0, 0]
    finally:
        lib.whisper_free(ctx)


def test_selftest_ranges_arguments(lib):
    bins = np.zeros((1, 2), np.uint64); last2 = np.zeros(2, np.uint64); t = np.zeros(1, np.int64); out = (abi.wmi_speaker * 1)()
    f = lib.wmi_selftest_speaker_ranges
    assert f(bins.ctypes.data, 1, last2.ctypes.data, sr.S16, 160, 16000, 0.0, t.ctypes.data, t.ctypes.data, 1, out) == 0
    assert f(bins.ctypes.data, 2, last2.ctypes.data, sr.S16, 160, 16000, 0.0, t.ctypes.data, t.ctypes.data, 1, out) == -1     # not the clip's count
    assert f(bins.ctypes.data, 1, last2.ctypes.data, 5, 160, 16000, 0.0, t.ctypes.data, t.ctypes.data, 1, out) == -1
    assert f(bins.ctypes.data, 1, last2.ctypes.data, sr.S16, 160, 0, 0.0, t.ctypes.data, t.ctypes.data, 1, out) == -1
    assert f(None, 0, last2.ctypes.data, sr.S16, 0, 16000, 0.0, t.ctypes.data, t.ctypes.data, 1, out) == 0 and out[0].speaker == -1

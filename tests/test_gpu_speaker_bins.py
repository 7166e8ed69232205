"""-m gpu: k_channel_bins (csrc/k_speaker.hip) through wmi_selftest_channel_bins, and wmi_wav_speaker on top of it, against the judge
(tests/speaker_ref.py).

s16 and s8: the table, the energies and the labels equal the judge's sequential loop with `==` (every partial sum of that loop is exactly
representable, so no order of addition can show), ties included.  f32: |E_device - E_judge| <= 2 m 2^-53 E_judge for the m terms of a
bin or a range — the textbook bound for two orders of adding m non-negative doubles —, labels compared where the judge's inequality
holds with that margin (every case here does; the test asserts that none was skipped), and two runs give the same bits."""
import ctypes as C

import numpy as np
import pytest

import speaker_ref as sr
import stage_compare as sc
from godot_whisper_amd import abi, host, synth

pytestmark = pytest.mark.gpu

KINDS = [sr.S16, sr.S8, sr.F32]
RATES = [16000, 44100, 22050, 150, 48000, 4096000]
COUNTS = [0, 1, 2, 63, 64, 65, 159, 160, 161, 4097, 48001]
THIRD_BIN = 2 * 40960 + 17123                  # at 4.096 MHz (40 960 frames a bin): two bins and a part of a third
PAD = 4                                        # sentinel pairs behind the table


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(scope="module")
def node(product_lib):
    n = host.SpeechToText(product_lib); n.set_language_model(synth.make_model("micro.en", seed=3))
    yield n
    n.close()


@pytest.fixture(scope="module")
def judged():
    """(format, rate, frames) -> (bytes, judge's bins, last2, channels), computed once and shared"""
    memo = {}

    def get(fmt, rate, n):
        key = (fmt, rate, n)
        if key not in memo:
            data = sr.crafted(fmt, n, seed=7 * fmt + rate % 977 + n)
            memo[key] = (data,) + sr.table(data, fmt, rate) + (sr.channels(data, fmt),)
        return memo[key]
    return get


def _bins(lib, data, fmt, rate, nb, on_device=None):
    """-> (bins [nb][2], last2 [2]) in the format's table type; sentinels behind both must survive"""
    dt = np.float64 if fmt == sr.F32 else np.uint64
    buf = np.full((nb + PAD, 2), 0x5A5A5A5A5A5A5A5A, np.uint64)
    last = np.full(4, 0x5A5A5A5A5A5A5A5A, np.uint64)
    if on_device is None:
        keep = C.create_string_buffer(bytes(data), max(len(data), 1))
        w = abi.wmi_wav(C.cast(keep, C.c_void_p), len(data), fmt, 1, rate, 0)
    else:
        w = abi.wmi_wav(on_device, len(data), fmt, 1, rate, 1)
    got_nb = C.c_longlong(-1)
    rc = lib.wmi_selftest_channel_bins(0, C.byref(w), buf.ctypes.data, nb + PAD, C.byref(got_nb), last.ctypes.data)
    assert rc == 0, (rc, fmt, rate, len(data))
    assert got_nb.value == nb, (got_nb.value, nb)
    assert np.all(buf[nb:] == 0x5A5A5A5A5A5A5A5A) and np.all(last[2:] == 0x5A5A5A5A5A5A5A5A)
    return buf[:nb].view(dt).copy(), last[:2].view(dt).copy()


def _hold_f32(kind, got, want, m, what):
    """got within 2 m 2^-53 want; returns nothing, records the margin"""
    lim = sr.f32_bound(m, want)
    if lim > 0 and np.isfinite(lim):
        sc.hold(kind, abs(got - want), lim, what)
    else:
        assert got == want, (kind, what, got, want)


def _check_table(fmt, rate, n, got_bins, got_last, want_bins, want_last, what):
    if fmt != sr.F32:
        assert got_bins.tobytes() == want_bins.tobytes(), (what, np.argwhere(got_bins != want_bins)[:4])
        assert got_last.tobytes() == want_last.tobytes(), (what, got_last, want_last)
        return
    assert got_last.tobytes() == want_last.tobytes(), (what, got_last, want_last)
    edges = sr.bin_edges(n, rate)
    bad = np.argwhere(got_bins != want_bins)
    for b, c in bad.tolist():                                       # (most bins are equal bit for bit: few terms)
        _hold_f32("speaker bins f32: |dE| / (2 m 2^-53 E)", float(got_bins[b, c]), float(want_bins[b, c]), edges[b + 1] - edges[b], (what, b, c))


def _ranges(n, rate):
    nb = sr.n_bins(n, rate)
    return [(0, 0), (0, 1), (1, 0), (0, nb), (0, max(nb - 1, 0)), (max(nb - 1, 0), nb), (max(nb - 2, 0), nb + 7), (nb, nb + 5), (0, nb + 100),
            (nb // 3, 2 * nb // 3), (1, 2), (0, 2 ** 40), (2 ** 40, 2 ** 41)]


def _wav_speaker(lib, ctx, data, fmt, rate, ranges, ratio=0.0):
    keep = C.create_string_buffer(bytes(data), max(len(data), 1))
    w = abi.wmi_wav(C.cast(keep, C.c_void_p), len(data), fmt, 1, rate, 0)
    t0 = np.array([r[0] for r in ranges], np.int64); t1 = np.array([r[1] for r in ranges], np.int64)
    out = (abi.wmi_speaker * len(ranges))()
    rc = lib.wmi_wav_speaker(ctx, C.byref(w), t0.ctypes.data, t1.ctypes.data, len(ranges), ratio, out)
    assert rc == 0, rc
    return [dict(speaker=o.speaker, is0=o.is0, is1=o.is1, e0=o.e0, e1=o.e1) for o in out]


@pytest.mark.parametrize("fmt", KINDS, ids=["s16", "s8", "f32"])
@pytest.mark.parametrize("rate", RATES)
def test_table_and_ranges_equal_the_judge(product_lib, node, judged, fmt, rate):
    skipped = compared = 0
    for n in COUNTS + ([THIRD_BIN] if rate == 4096000 else []):
        data, want_bins, want_last, x = judged(fmt, rate, n)
        nb = sr.n_bins(n, rate)
        got_bins, got_last = _bins(product_lib, data, fmt, rate, nb)
        _check_table(fmt, rate, n, got_bins, got_last, want_bins, want_last, (fmt, rate, n))
        ranges = _ranges(n, rate)
        for (t0, t1), g in zip(ranges, _wav_speaker(product_lib, node.ctx, data, fmt, rate, ranges)):
            want = sr.speaker(x, rate, t0, t1)
            what = (fmt, rate, n, t0, t1)
            if fmt != sr.F32:
                assert g == want, (what, g, want)                     # energies and label, bit for bit
                continue
            assert (g["is0"], g["is1"]) == (want["is0"], want["is1"]), (what, g, want)
            m = want["is1"] - want["is0"]
            for c in ("e0", "e1"):
                _hold_f32("speaker ranges f32: |dE| / (2 m 2^-53 E)", g[c], want[c], max(m, 0), (what, c))
            if sr.f32_label_safe(want):
                assert g["speaker"] == want["speaker"], (what, g, want)
                compared += 1
            else:
                skipped += 1
    assert skipped == 0, skipped
    if fmt == sr.F32:
        print(f"f32 rate {rate}: {compared} labels compared; worst fractions of the bound:",
              {k: round(v["worst_ratio"], 4) for k, v in sc.MARGINS.items() if k.startswith("speaker")})


@pytest.mark.parametrize("fmt", KINDS, ids=["s16", "s8", "f32"])
def test_device_sources_at_every_sample_offset(product_lib, hip, judged, fmt):
    """the clip starts 0 .. 7 SAMPLES into an allocation: every 16-byte phase a sample-aligned pointer can have at 16 bit (half of them
    at 8 bit, all four at 32 bit twice), a stereo source off its frame grid included"""
    bs = sr.SAMPLE_BYTES[fmt]
    cases = [(16000, 161), (16000, 4097), (44100, 4097), (150, 65)]
    room = 8 * 4097 + 8 * bs + 64
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(room)) == 0
    try:
        for rate, n in cases:
            data, want_bins, want_last, _ = judged(fmt, rate, n)
            for off in range(8):
                src = C.c_void_p(d.value + off * bs)
                assert hip.hipMemcpy(src, data, C.c_size_t(len(data)), 1) == 0
                got_bins, got_last = _bins(product_lib, data, fmt, rate, sr.n_bins(n, rate), on_device=src)
                _check_table(fmt, rate, n, got_bins, got_last, want_bins, want_last, (fmt, rate, n, "offset", off))
    finally:
        hip.hipFree(d)


def test_the_most_negative_samples(product_lib):
    """|-32768| = 32768 and |-128| = 128 do not fit the sample's own type: a clip of nothing else"""
    for fmt, lo in ((sr.S16, -32768), (sr.S8, -128)):
        for n in (1, 2, 161, 4097):
            v = np.full((n, 2), lo, np.int64); v[::3, 1] = lo + 1
            data = sr.pack(v.reshape(-1), fmt)
            want_bins, want_last = sr.table(data, fmt, 16000)
            got_bins, got_last = _bins(product_lib, data, fmt, 16000, sr.n_bins(n, 16000))
            assert got_bins.tobytes() == want_bins.tobytes() and got_last.tobytes() == want_last.tobytes(), (fmt, n)
            assert int(got_last[0]) == -lo


def test_ties_and_the_ratio_on_either_side(product_lib, node):
    """equal channel sums, and one channel 1.1 times the other as nearly as integers allow: just below, at, and just above, both ways"""
    seen = set()
    for fmt in (sr.S16, sr.S8):
        for l, r, ratio in [(1000, 1000, 0.0), (1100, 1000, 0.0), (1101, 1000, 0.0), (1099, 1000, 0.0), (1000, 1100, 0.0), (1000, 1101, 0.0),
                            (1000, 1099, 0.0), (2000, 1000, 2.0), (2001, 1000, 2.0), (1000, 2000, 2.0), (1000, 2001, 2.0), (0, 0, 0.0), (0, 1, 0.0)]:
            n = 321
            v = np.zeros((n, 2), np.int64)
            v[:160, 0] = l // 160; v[:l % 160, 0] += 1                  # the sums are l and r exactly, every sample within 8 bits
            v[:160, 1] = -(r // 160); v[:r % 160, 1] -= 1
            data = sr.pack(v.reshape(-1), fmt)
            ranges = [(0, 1), (0, 3), (1, 3)]
            got = _wav_speaker(product_lib, node.ctx, data, fmt, 16000, ranges, ratio)
            for (t0, t1), g in zip(ranges, got):
                want = sr.speaker_of_clip(data, fmt, 16000, t0, t1, ratio if ratio > 0 else sr.RATIO)
                assert g == want, (fmt, l, r, ratio, t0, t1, g, want)
                seen.add(g["speaker"])
    assert seen == {-1, 0, 1}


def test_two_runs_on_the_same_f32_input_give_the_same_bits(product_lib, judged):
    for rate, n in ((16000, 48001), (4096000, THIRD_BIN), (44100, 4097)):
        data = judged(sr.F32, rate, n)[0]
        a = _bins(product_lib, data, sr.F32, rate, sr.n_bins(n, rate))
        b = _bins(product_lib, data, sr.F32, rate, sr.n_bins(n, rate))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (rate, n)


def test_mono_and_capacity_errors(product_lib, node):
    lib = product_lib
    raw = C.create_string_buffer(bytes(4 * 400), 1600)
    nb = C.c_longlong(-1); last = np.zeros(2, np.uint64); buf = np.zeros((8, 2), np.uint64)
    w = abi.wmi_wav(C.cast(raw, C.c_void_p), 1600, sr.S16, 1, 16000, 0)
    assert lib.wmi_selftest_channel_bins(0, C.byref(w), buf.ctypes.data, 2, C.byref(nb), last.ctypes.data) == -4 and nb.value == 3
    mono = abi.wmi_wav(C.cast(raw, C.c_void_p), 1600, sr.S16, 0, 16000, 0)
    out = (abi.wmi_speaker * 1)(); t = np.zeros(1, np.int64)
    assert lib.wmi_wav_speaker(node.ctx, C.byref(mono), t.ctypes.data, t.ctypes.data, 1, 0.0, out) == -12
    empty = abi.wmi_wav(C.cast(raw, C.c_void_p), 0, sr.S16, 1, 16000, 0)
    assert lib.wmi_wav_speaker(node.ctx, C.byref(empty), t.ctypes.data, t.ctypes.data, 1, 0.0, out) == 0
    assert (out[0].speaker, out[0].is0, out[0].is1, out[0].e0, out[0].e1) == (-1, 0, 0, 0.0, 0.0)

"""The judge of the two-channel WAV calls (tests/channels_ref.py) on the CPU: it REFUSES the wrong answers a split could give, the
library's merge rule (wmi_selftest_channels_merge, csrc/channel_merge.h) equals the judge's, every conversion error of the two calls is
answered on a context without a device, and every case of the GPU table has two equal, defined counts."""
import ctypes as C

import numpy as np
import pytest

import channels_ref as cr
import wav_ref as wr
from godot_whisper_amd import abi, runtime, synth


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


def _wav(data, fmt, stereo, rate, on_device=0, n_bytes=None):
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    w = abi.wmi_wav(C.cast(buf, C.c_void_p), len(data) if n_bytes is None else n_bytes, fmt, stereo, rate, on_device)
    w._keep = buf
    return w


# ------------------------------------------------------------------------------------------------ the judge refuses wrong answers

def _refused(got0, got1, want):
    with pytest.raises(AssertionError):
        cr.hold(got0, got1, want)


def test_make_stereo_is_asymmetric():
    for fmt, lo, hi in ((wr.S16, -1.0, 32767 / 32768), (wr.S8, -1.0, 127 / 128), (wr.F32, -1.0, 1.0)):
        l, r = cr.split(cr.make_stereo(fmt, 257, 3), fmt)
        assert l.size == r.size == 257
        assert (l[0], r[0], l[-1], r[-1]) == (np.float32(lo), np.float32(hi), np.float32(hi), np.float32(lo))
        assert abs(np.corrcoef(l, r)[0, 1]) < 0.2                                 # independent channels
        assert cr.make_stereo(fmt, 0, 3) == b"" and len(cr.make_stereo(fmt, 1, 3)) == 2 * wr.SAMPLE_BYTES[fmt]
    l, r = cr.split(cr.make_stereo(wr.S16, 1, 3), wr.S16)
    assert (l[0], r[0]) == (-1.0, np.float32(32767 / 32768))


@pytest.mark.parametrize("rate", [48000, 16000])
def test_the_judge_accepts_the_definition_and_refuses_wrong_splits(rate):
    conv, n = 2, 257
    data = cr.make_stereo(wr.S16, n, 11)
    want = cr.convert_channels(data, wr.S16, rate, conv)
    assert want[0].size == want[1].size == wr.convert(data, wr.S16, 1, rate, conv).size > 0
    cr.hold(want[0].copy(), want[1].copy(), want)

    def res(x):
        return wr.resample(np.ascontiguousarray(x, np.float32), rate, conv)
    l, r = cr.split(data, wr.S16)
    # channels swapped
    _refused(want[1], want[0], want)
    # the fold in both
    folded = wr.convert(data, wr.S16, 1, rate, conv)
    _refused(folded, folded, want)
    # channel 0 twice
    _refused(want[0], want[0], want)
    # the interleaved stream read as mono and halved (every second SAMPLE of the stream resampled as if it were the clip)
    inter = wr.samples(data, wr.S16)
    _refused(res(inter[:n]), res(inter[n:]), want)
    _refused(res(inter)[:want[0].size], res(inter)[want[0].size:2 * want[0].size], want)
    # one frame late
    _refused(res(np.append(np.float32(0), l[:-1])), res(np.append(np.float32(0), r[:-1])), want)
    # one sample short
    _refused(want[0][:-1], want[1][:-1], want)
    _refused(want[0], want[1][:-1], want)
    # unsigned 8-bit (on the 8-bit clip of the same shape)
    d8 = cr.make_stereo(wr.S8, n, 11)
    want8 = cr.convert_channels(d8, wr.S8, rate, conv)
    u8 = (np.frombuffer(d8, "u1").astype(np.float32) - 128) / np.float32(128.0)
    _refused(res(u8[0::2]), res(u8[1::2]), want8)
    u8 = np.frombuffer(d8, "u1").astype(np.float32) / np.float32(128.0)
    _refused(res(u8[0::2]), res(u8[1::2]), want8)
    # channel 1 resampled with the other SINC table (48 kHz only: nothing is resampled at 16 kHz)
    if rate != wr.DST_RATE:
        _refused(want[0], wr.resample(r, rate, 1)[:want[1].size], want)
    # out1 left at zeros
    _refused(want[0], np.zeros_like(want[1]), want)


def test_split_ignores_the_odd_tail():
    data = cr.make_stereo(wr.S16, 9, 5)
    want = cr.split(data, wr.S16)
    for tail in (b"\x7f", b"\x7f\x7f", b"\x7f\x7f\x7f"):                           # an odd byte, an odd sample, both
        got = cr.split(data + tail, wr.S16)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ------------------------------------------------------------------------------------------------ the merge rule

def _lib_merge(lib, a, b):
    ta, tb = (C.c_int64 * max(len(a), 1))(*a), (C.c_int64 * max(len(b), 1))(*b)
    n = len(a) + len(b)
    ch, ix = (C.c_int * (n + 2))(*([-7] * (n + 2))), (C.c_int * (n + 2))(*([-7] * (n + 2)))
    got = lib.wmi_selftest_channels_merge(ta, len(a), tb, len(b), ch, ix)
    assert got == n and list(ch[n:]) == [-7, -7] and list(ix[n:]) == [-7, -7]      # nothing behind the n entries is written
    return list(zip(ch[:n], ix[:n]))


def test_merge_rule_equals_the_judges(lib):
    assert hasattr(lib, "wmi_selftest_channels_merge")
    by_hand = [
        ([], [], []),
        ([5], [], [(0, 0)]),
        ([], [5, 6], [(1, 0), (1, 1)]),
        ([3], [3], [(0, 0), (1, 0)]),                                              # equal t0: channel 0 first
        ([0, 0, 0], [0, 0], [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]),             # runs of equal t0 within a side
        ([1, 4, 4, 9], [4, 4, 10], [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (0, 3), (1, 2)]),
        ([1, 2, 3], [7, 8], [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]),             # one side wholly before the other
        ([7, 8], [1, 2, 3], [(1, 0), (1, 1), (1, 2), (0, 0), (0, 1)]),
        ([5, 2], [3], [(1, 0), (0, 0), (0, 1)]),                                   # a side that does not ascend keeps its own order
    ]
    for a, b, want in by_hand:
        assert cr.merge(a, b) == want, (a, b)
        assert _lib_merge(lib, a, b) == want, (a, b)
    rng = np.random.default_rng(2718)
    for _ in range(200):
        a = np.sort(rng.integers(0, 30, rng.integers(0, 13))).tolist()
        b = np.sort(rng.integers(0, 30, rng.integers(0, 13))).tolist()
        want = cr.merge(a, b)
        assert _lib_merge(lib, a, b) == want, (a, b)
        # the rule's properties: each side in its own order, the start times never fall, ties put channel 0 first
        assert [i for c, i in want if c == 0] == list(range(len(a))) and [i for c, i in want if c == 1] == list(range(len(b)))
        ts = [(a, b)[c][i] for c, i in want]
        assert ts == sorted(ts)
        assert all(not (c0 == 1 and c1 == 0 and t0 == t1) for (c0, _), (c1, _), t0, t1 in zip(want, want[1:], ts, ts[1:]))
    one = (C.c_int64 * 1)(1)
    out = (C.c_int * 4)()
    assert lib.wmi_selftest_channels_merge(one, -1, one, 1, out, out) == -1 and lib.wmi_selftest_channels_merge(None, 1, one, 1, out, out) == -1
    assert lib.wmi_selftest_channels_merge(one, 1, one, 1, None, out) == -1 and lib.wmi_selftest_channels_merge(one, 1, one, 1, out, None) == -1
    assert lib.wmi_selftest_channels_merge(None, 0, None, 0, None, None) == 0


def test_struct_layout_and_symbols(lib):
    assert C.sizeof(abi.wmi_channel_segment) == 8
    assert [getattr(abi.wmi_channel_segment, f).offset for f, _ in abi.wmi_channel_segment._fields_] == [0, 4]
    import pathlib
    text = (pathlib.Path(__file__).resolve().parent.parent / "include" / "wmi_device.h").read_text()
    for name in ("wmi_wav_to_pcm_channels", "wmi_full_wav_channels", "wmi_channels_select", "wmi_channels_get_segment", "wmi_selftest_channels_merge"):
        assert name + "(" in text and hasattr(lib, name)


# ------------------------------------------------------------------------------------------------ the table of the GPU test

def test_every_case_of_the_gpu_table_has_two_equal_defined_counts(lib):
    table = cr.cases()
    assert len(table) == 3 * (15 + 4 * 4 * 15 - 1)                                 # SRC_LINEAR upsampling one frame is the one exclusion
    zeros = bytes(8 * max(wr.COUNTS))
    counted = {}
    for fmt, rate, conv, n in table:
        key = (rate, conv, n)                                                      # the count depends on these alone
        if key not in counted:
            counted[key] = wr.resample(np.zeros(n, np.float32), rate, conv).size
        if fmt == wr.S16:                                                          # the judge itself, once per key
            a, b = cr.convert_channels(zeros[:4 * n], wr.S16, rate, conv)
            assert a.size == b.size == counted[key], (key, a.size, b.size)
        # the library's host-side plan for the clip: the count wmi_wav_to_pcm reports
        frames, n_out = C.c_longlong(-1), C.c_longlong(-1)
        w = _wav(zeros[:2 * n * wr.SAMPLE_BYTES[fmt]], fmt, 1, rate)
        assert lib.wmi_selftest_wav_plan(C.byref(w), conv, C.byref(frames), C.byref(n_out)) == 0
        assert (frames.value, n_out.value) == (n, counted[key]), (fmt, key)
        wr.hold_count(n_out.value, n, rate, conv, counted[key])


# ------------------------------------------------------------------------------------------------ errors, without a device

def test_every_conversion_error_without_a_device(lib):
    mb = synth.make_model("micro.en", seed=1)
    buf = C.create_string_buffer(mb, len(mb))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(mb))
    p = lib.whisper_full_default_params(0)
    data = cr.make_stereo(wr.S16, 4800, 1)
    d0, d1 = np.full(4800, np.nan, np.float32), np.full(4800, np.nan, np.float32)
    p0, p1 = d0.ctypes.data_as(C.c_void_p), d1.ctypes.data_as(C.c_void_p)
    ok = dict(data=data, fmt=wr.S16, stereo=1, rate=48000)

    def codes(conv=2, cap=4800, **kw):
        a = dict(ok, **kw)
        w = _wav(a["data"], a["fmt"], a["stereo"], a["rate"], a.get("on_device", 0), a.get("n_bytes"))
        if a.get("null"):
            w.data = None
        return lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), conv, p0, p1, cap, 0), lib.wmi_full_wav_channels(ctx, p, C.byref(w), conv)
    try:
        for kw, e in ((dict(stereo=0), -12), (dict(stereo=0, rate=16000), -12), (dict(fmt=2), -11), (dict(fmt=3), -11), (dict(conv=0), -10),
                      (dict(null=True), -1), (dict(n_bytes=-2), -1), (dict(fmt=5), -1), (dict(stereo=2), -1), (dict(stereo=-1), -1),
                      (dict(rate=0), -1), (dict(n_bytes=8 * (2 ** 31)), -1), (dict(conv=5), -1), (dict(conv=-1), -1),
                      (dict(stereo=0, fmt=2), -11), (dict(stereo=0, conv=0), -10)):     # a mono clip is decided behind the others
            kw = dict(kw); conv = kw.pop("conv", 2)
            one, full = codes(conv=conv, **kw)
            assert (one, full) == (e, -100 + e), (kw, conv, one, full)
        w = _wav(data, wr.S16, 1, 48000)
        # NULL arguments of the calls themselves
        assert lib.wmi_wav_to_pcm_channels(None, C.byref(w), 2, p0, p1, 4800, 0) == -1 and lib.wmi_wav_to_pcm_channels(ctx, None, 2, p0, p1, 4800, 0) == -1
        assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), 2, None, p1, 4800, 0) == -1 and lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), 2, p0, None, 4800, 0) == -1
        assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), 2, p0, p1, -1, 0) == -1
        assert lib.wmi_full_wav_channels(None, p, C.byref(w), 2) == -101 and lib.wmi_full_wav_channels(ctx, p, None, 2) == -101
        # a device pointer off its sample grid (decided from the pointer's value alone)
        wd = abi.wmi_wav(C.c_void_p(0x7f0000001001), 9600, wr.S16, 1, 48000, 1)
        assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(wd), 2, p0, p1, 4800, 0) == -1 and lib.wmi_full_wav_channels(ctx, p, C.byref(wd), 2) == -101
        # the capacity is per channel: 4800 frames at 48 kHz are 1600 samples each
        assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), 2, p0, p1, 1599, 0) == -4
        # a clip in order: the context cannot compute, and the device was never reached
        w16 = _wav(data, wr.S16, 1, 16000)
        for ww, conv, cap in ((w, 2, 1600), (w16, 0, 4800)):
            assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(ww), conv, p0, p1, cap, 0) == -2
            assert lib.wmi_full_wav_channels(ctx, p, C.byref(ww), conv) == -102
        assert np.all(np.isnan(d0)) and np.all(np.isnan(d1))                       # nothing was written
        # no channels result, no work set
        assert lib.wmi_channels_select(ctx, -1) == lib.wmi_channels_select(ctx, 0) == lib.wmi_channels_select(None, 0) == -1
        rec = abi.wmi_channel_segment(9, 9)
        assert lib.wmi_channels_get_segment(ctx, 0, C.byref(rec)) == -1 and lib.wmi_channels_get_segment(ctx, 0, None) == -1 and (rec.channel, rec.index) == (9, 9)
        st = (C.c_int64 * 5)(7, 7, 7, 7, 7)
        assert lib.wmi_wav_stats(ctx, st) == 0 and list(st) == [0, 0, 0, 0, 0]
    finally:
        lib.whisper_free(ctx)

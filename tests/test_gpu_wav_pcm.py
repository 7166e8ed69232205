"""-m gpu: wmi_wav_to_pcm (csrc/k_wav.hip k_wav_decode; csrc/k_resample.hip in_frame over packed frames) against the judge
tests/wav_ref.py — bit equality everywhere: a decoded sample is one exact division, a folded frame one f32 add and one halving, and a
resampled frame the sequential converter's own operations in its order.

The table (wav_ref.cases()): s8 / s16 / f32, mono and stereo, at 16 kHz (decode only), 48 and 44.1 kHz (closed-form positions), 22.05 kHz
(table positions) and 8 kHz (upsampling), converters 1 - 4, frame counts around a group of eight, a 16-byte piece and a 256-thread block,
and 3 s per format at 44.1 and 48 kHz with converter 2.  SRC_LINEAR upsampling one frame is left out by name (the library reads
data_in[-1]); its 0-sample answer is an edge below.
"""
import ctypes as C

import numpy as np
import pytest

import wav_ref as wr
from godot_whisper_amd import abi, host, synth

pytestmark = pytest.mark.gpu

GUARD = 64
SMALL = [c for c in wr.cases() if c[4] <= max(wr.COUNTS)]
LONG = [c for c in wr.cases() if c[4] > max(wr.COUNTS)]


@pytest.fixture(scope="module")
def node(product_lib):
    n = host.SpeechToText(product_lib); n.set_language_model(synth.make_model("micro.en", seed=1))
    yield n
    n.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(scope="module")
def wants():
    """the judge's result per case, computed once and shared: (format, stereo, rate, converter, frames) -> (bytes, samples)"""
    memo = {}

    def get(case):
        if case not in memo:
            fmt, st, rate, conv, n = case
            data = wr.make_bytes(fmt, st, n, seed=1000 + n % 997 + 7 * fmt + st)
            want = wr.convert(data, fmt, st, rate, conv)
            want.setflags(write=False)
            memo[case] = (data, want)
        return memo[case]
    return get


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _wav(data, fmt, st, rate):
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    w = abi.wmi_wav(C.cast(buf, C.c_void_p), len(data), fmt, st, rate, 0)
    w._keep = buf
    return w


def _stats(lib, ctx):
    s = (C.c_int64 * 5)()
    assert lib.wmi_wav_stats(ctx, s) == 0
    return list(s)


def _to_host(lib, ctx, w, conv, n_want):
    """-> (count, the samples written, the guard behind them): dst is all sentinels beforehand, its capacity exactly the count"""
    out = np.full(n_want + GUARD, np.nan, np.float32)
    got = lib.wmi_wav_to_pcm(ctx, C.byref(w), conv, _p(out), n_want, 0)
    return got, out[:max(got, 0)], out[max(got, 0):]


@pytest.mark.parametrize("fmt,st", wr.FORMATS, ids=["s8", "s8x2", "s16", "s16x2", "f32", "f32x2"])
def test_host_bytes_equal_the_judge_on_the_small_counts(product_lib, node, wants, fmt, st):
    lib, ctx = product_lib, node.ctx
    for case in SMALL:
        if case[:2] != (fmt, st):
            continue
        _, _, rate, conv, n = case
        data, want = wants(case)
        got, out, guard = _to_host(lib, ctx, _wav(data, fmt, st, rate), conv, want.size)
        assert got == want.size, (case, got)
        wr.hold(out, want, case)
        assert np.all(np.isnan(guard)), case
        # one launch whatever the rate — none for an empty result —, the bytes as bytes, the table's 12 bytes per sample at 22.05 kHz
        s = _stats(lib, ctx)
        table = 12 * want.size if rate == 22050 else 0
        assert s[:4] == [(len(data) + table) if want.size else 0, n, want.size, 1 if want.size else 0], (case, s)
        assert want.size == 0 or fmt == wr.F32 or s[0] - table != 4 * n * (2 if st else 1), case


@pytest.mark.parametrize("case", LONG, ids=[f"{f}-{s}-{r}" for f, s, r, _, _ in LONG])
def test_three_seconds_equal_the_judge(product_lib, node, wants, case):
    fmt, st, rate, conv, n = case
    data, want = wants(case)
    got, out, guard = _to_host(product_lib, node.ctx, _wav(data, fmt, st, rate), conv, want.size)
    assert got == want.size and abs(got - n * 16000 // rate) <= 1, (case, got)
    wr.hold(out, want, case)
    assert np.all(np.isnan(guard))
    assert _stats(product_lib, node.ctx)[:4] == [len(data), n, want.size, 1]


DEV_COUNTS = [1, 7, 9, 17, 257, 4097]


@pytest.mark.parametrize("fmt,st", wr.FORMATS, ids=["s8", "s8x2", "s16", "s16x2", "f32", "f32x2"])
def test_device_pointers_at_every_sample_offset(product_lib, node, hip, wants, fmt, st):
    """the source starts 0, 1, 2 and 3 SAMPLES into a larger allocation — every alignment a sample-aligned pointer can have, a stereo
    source off its frame grid included —, dst is a device pointer 0 .. 3 floats into its allocation with a guard behind the result"""
    lib, ctx = product_lib, node.ctx
    bs = wr.SAMPLE_BYTES[fmt]
    room_in = 8 * max(DEV_COUNTS) + 64
    room_out = 2 * max(DEV_COUNTS) + GUARD + 16
    d_in, d_out = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_in), C.c_size_t(room_in)) == 0 and hip.hipMalloc(C.byref(d_out), C.c_size_t(4 * room_out)) == 0
    try:
        for case in SMALL:
            if case[:2] != (fmt, st) or case[4] not in DEV_COUNTS or case[3] in (1, 3):
                continue
            _, _, rate, conv, n = case
            data, want = wants(case)
            for off in (0, 1, 2, 3):
                if rate != 16000 and off not in (0, 1 + n % 3):                       # every offset at 16 kHz (the vector body), two at the others
                    continue
                key = (case, off)
                marks = np.full(room_out, np.nan, np.float32)
                assert hip.hipMemcpy(d_out, _p(marks), C.c_size_t(marks.nbytes), 1) == 0
                src = C.c_void_p(d_in.value + off * bs)
                assert hip.hipMemcpy(src, data, C.c_size_t(len(data)), 1) == 0
                dst = C.c_void_p(d_out.value + 4 * off)
                w = abi.wmi_wav(src, len(data), fmt, st, rate, 1)
                got = lib.wmi_wav_to_pcm(ctx, C.byref(w), conv, dst, want.size, 1)
                assert got == want.size, (key, got)
                back = np.zeros(room_out, np.float32)
                assert hip.hipMemcpy(_p(back), d_out, C.c_size_t(back.nbytes), 2) == 0
                wr.hold(back[off:off + got], want, key)
                assert np.all(np.isnan(back[:off])) and np.all(np.isnan(back[off + got:])), key
                # nothing but the table is uploaded
                assert _stats(lib, ctx)[:4] == [12 * want.size if rate == 22050 else 0, n, want.size, 1 if want.size else 0], key
    finally:
        hip.hipFree(d_in); hip.hipFree(d_out)


def test_extreme_samples_and_odd_tails(product_lib, node):
    lib, ctx = product_lib, node.ctx
    for fmt, lo, hi in ((wr.S16, -32768, 32767), (wr.S8, -128, 127)):
        scale = 32768.0 if fmt == wr.S16 else 128.0
        # extremes at the first and the last frame, by hand: mono, and stereo pairs whose sum is -2, just under 2, and 0 from both ends
        v = np.zeros(41, np.int32); v[0] = lo; v[-1] = hi
        got, out, _ = _to_host(lib, ctx, _wav(wr.pack(v, fmt), fmt, 0, 16000), 2, 41)
        assert got == 41 and out[0] == -1.0 and out[-1] == np.float32(hi / scale) and not out[1:-1].any()
        vs = np.zeros(2 * 19, np.int32); vs[0:2] = lo; vs[2:4] = (lo, hi); vs[-2:] = hi
        got, out, _ = _to_host(lib, ctx, _wav(wr.pack(vs, fmt), fmt, 1, 16000), 2, 19)
        assert got == 19 and out[0] == -1.0 and out[1] == np.float32(-1.0 / scale / 2.0) and out[-1] == np.float32(hi / scale)
        wr.hold(out, wr.decode(wr.pack(vs, fmt), fmt, 1))
    # a trailing incomplete sample or frame is ignored: every count of bytes around whole frames, 16 kHz and resampled
    for fmt, st in wr.FORMATS:
        fb = wr.SAMPLE_BYTES[fmt] * (2 if st else 1)
        whole = wr.make_bytes(fmt, st, 300, seed=9)
        for rate, conv in ((16000, 2), (48000, 4)):
            for cut in range(len(whole) - 2 * fb, len(whole) + 1):
                data = whole[:cut]
                want = wr.convert(data, fmt, st, rate, conv)
                assert wr.frames_of(cut, fmt, st) == cut // fb
                got, out, guard = _to_host(lib, ctx, _wav(data, fmt, st, rate), conv, want.size)
                assert got == want.size, (fmt, st, rate, cut)
                wr.hold(out, want, (fmt, st, rate, cut))
                assert np.all(np.isnan(guard))
                assert _stats(lib, ctx)[:2] == [cut, cut // fb]                      # the bytes as handed over, the whole frames read


@pytest.mark.parametrize("rate,conv", [(48000, 2), (44100, 1), (22050, 2), (8000, 3), (48000, 4), (16000, 2)])
def test_f32_input_equals_downmix_and_resample(product_lib, node, rate, conv):
    """the packed-frame reader against the calls it stands in for, on the same f32 samples"""
    lib, ctx = product_lib, node.ctx
    n = 5003
    fr = np.random.default_rng(rate + conv).uniform(-1, 1, size=(n, 2)).astype(np.float32)
    mono = np.zeros(n, np.float32)
    assert lib.wmi_downmix_stereo(ctx, _p(fr), n, 0, _p(mono)) == 0
    cap = max(wr.capacity(n, rate), n) + 8
    ref = np.full(cap, np.nan, np.float32)
    n_ref = lib.wmi_resample(ctx, _p(mono), n, rate, 16000, conv, 0, _p(ref), cap)
    assert n_ref > 0
    for st, data in ((1, fr.tobytes()), (0, mono.tobytes())):
        got, out, guard = _to_host(lib, ctx, _wav(data, wr.F32, st, rate), conv, n_ref)
        assert got == n_ref
        wr.hold(out, ref[:n_ref], (rate, conv, st))
        assert np.all(np.isnan(guard))


def test_edges(product_lib, node):
    lib, ctx = product_lib, node.ctx
    out = np.full(64, np.nan, np.float32)
    one = _wav(wr.pack(np.array([20000], np.int32), wr.S16), wr.S16, 0, 8000)
    assert lib.wmi_wav_to_pcm(ctx, C.byref(one), 4, _p(out), 64, 0) == 0 and np.all(np.isnan(out))      # SRC_LINEAR upsampling one frame
    assert _stats(lib, ctx)[:4] == [0, 1, 0, 0]
    assert lib.wmi_wav_to_pcm(ctx, C.byref(one), 3, _p(out), 64, 0) == 2                                # zero-order hold repeats it
    assert out[:2].tobytes() == np.array([20000 / 32768] * 2, np.float32).tobytes() and np.all(np.isnan(out[2:]))
    out[:] = np.nan
    far = _wav(bytes(9600), wr.S16, 0, 16000 * 300)                                                     # ratio outside libsamplerate's range
    assert lib.wmi_wav_to_pcm(ctx, C.byref(far), 2, _p(out), 64, 0) == 0 and np.all(np.isnan(out))
    empty = _wav(b"", wr.S16, 1, 44100)
    assert lib.wmi_wav_to_pcm(ctx, C.byref(empty), 2, _p(out), 0, 0) == 0 and _stats(lib, ctx)[:4] == [0, 0, 0, 0]
    w = _wav(bytes(9600), wr.S16, 0, 48000)
    assert lib.wmi_wav_to_pcm(ctx, C.byref(w), 2, _p(out), 63, 0) == -4 and lib.wmi_wav_to_pcm(ctx, C.byref(w), 0, _p(out), 64, 0) == -10
    assert np.all(np.isnan(out))

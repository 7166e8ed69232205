"""-m gpu: wmi_wav_to_pcm_channels (csrc/k_wav.hip k_wav_split; csrc/k_resample.hip k_resample_split / k_resample_simple_split) against
the judge tests/channels_ref.py — bit equality per channel: a decoded sample is one exact division, and a resampled sample receives the
sequential converter's own operations in its order, whichever channel shares the thread with it.

The table (channels_ref.cases()): s8 / s16 / f32 stereo at 16 kHz (decode only), 48 and 44.1 kHz (closed-form positions), 22.05 kHz (table
positions) and 8 kHz (upsampling), converters 1 - 4, frame counts around a group of eight, a 16-byte piece and a 256-thread block (inputs
shorter than the SINC reach among them), and 3 s of s16 at 44.1 and 48 kHz with converter 2.  The clips are channels_ref.make_stereo's:
independent channels with asymmetric extremes, so a swap, a fold or a copy of one channel fails."""
import ctypes as C

import numpy as np
import pytest

import channels_ref as cr
import wav_ref as wr
from godot_whisper_amd import abi, host, synth

pytestmark = pytest.mark.gpu

GUARD = 64
FORMATS = [wr.S8, wr.S16, wr.F32]
IDS = ["s8x2", "s16x2", "f32x2"]


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
    """the judge's result per case, computed once and shared: (format, rate, converter, frames) -> (bytes, (pcm0, pcm1))"""
    memo = {}

    def get(case):
        if case not in memo:
            fmt, rate, conv, n = case
            data = cr.make_stereo(fmt, n, seed=2000 + n % 997 + 7 * fmt)
            want = cr.convert_channels(data, fmt, rate, conv)
            for w in want:
                w.setflags(write=False)
            memo[case] = (data, want)
        return memo[case]
    return get


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _wav(data, fmt, rate):
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    w = abi.wmi_wav(C.cast(buf, C.c_void_p), len(data), fmt, 1, rate, 0)
    w._keep = buf
    return w


def _stats(lib, ctx):
    s = (C.c_int64 * 5)()
    assert lib.wmi_wav_stats(ctx, s) == 0
    return list(s)


def _to_host(lib, ctx, w, conv, n_want):
    """-> (count, [the samples written per channel], [the guard behind them]): both dsts are all sentinels beforehand, the capacity
    exactly the count"""
    outs = [np.full(n_want + GUARD, np.nan, np.float32) for _ in range(2)]
    got = lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), conv, _p(outs[0]), _p(outs[1]), n_want, 0)
    g = max(got, 0)
    return got, [o[:g] for o in outs], [o[g:] for o in outs]


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_host_bytes_equal_the_judge_on_the_small_counts(product_lib, node, wants, fmt):
    lib, ctx = product_lib, node.ctx
    ran = 0
    for case in cr.cases():
        if case[0] != fmt:
            continue
        _, rate, conv, n = case
        data, want = wants(case)
        k = want[0].size
        got, out, guard = _to_host(lib, ctx, _wav(data, fmt, rate), conv, k)
        assert got == k == want[1].size, (case, got)
        cr.hold(out[0], out[1], want, case)
        assert np.all(np.isnan(guard[0])) and np.all(np.isnan(guard[1])), case
        # one launch for both channels — none for an empty result —, the bytes once, the table's 12 bytes per sample once at 22.05 kHz
        table = 12 * k if rate == 22050 else 0
        assert _stats(lib, ctx)[:4] == [(len(data) + table) if k else 0, n, 2 * k, 1 if k else 0], case
        ran += 1
    assert ran == 15 + 4 * 4 * 15 - 1 and len(cr.cases()) == 3 * ran               # no filter emptied the table


@pytest.mark.parametrize("case", cr.LONG, ids=[f"s16x2-{c[1]}" for c in cr.LONG])
def test_three_seconds_equal_the_judge(product_lib, node, wants, case):
    fmt, rate, conv, n = case
    data, want = wants(case)
    k = want[0].size
    got, out, guard = _to_host(product_lib, node.ctx, _wav(data, fmt, rate), conv, k)
    assert got == k and abs(got - n * 16000 // rate) <= 1, (case, got)
    cr.hold(out[0], out[1], want, case)
    assert np.all(np.isnan(guard[0])) and np.all(np.isnan(guard[1]))
    assert _stats(product_lib, node.ctx)[:4] == [len(data), n, 2 * k, 1]
    # a second run gives the same bits
    got2, out2, _ = _to_host(product_lib, node.ctx, _wav(data, fmt, rate), conv, k)
    assert got2 == k and out2[0].tobytes() == out[0].tobytes() and out2[1].tobytes() == out[1].tobytes()


DEV_COUNTS = [1, 7, 9, 17, 257, 4097]


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_device_pointers_at_every_sample_offset(product_lib, node, hip, wants, fmt):
    """the source starts 0 .. 7 SAMPLES into a larger allocation — odd offsets are off the frame grid: no group of eight, sample-sized
    loads, the unaligned f32 reader —, the two destinations are device pointers 0 .. 3 floats into their allocations, differently
    aligned, each with a guard around its result"""
    lib, ctx = product_lib, node.ctx
    bs = wr.SAMPLE_BYTES[fmt]
    room_in = 8 * max(DEV_COUNTS) + 128
    room_out = 2 * max(DEV_COUNTS) + GUARD + 16                                     # (8 kHz doubles the count)
    d_in, d_o0, d_o1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_in), C.c_size_t(room_in)) == 0
    assert hip.hipMalloc(C.byref(d_o0), C.c_size_t(4 * room_out)) == 0 and hip.hipMalloc(C.byref(d_o1), C.c_size_t(4 * room_out)) == 0
    ran = 0
    try:
        for case in cr.cases():
            if case[0] != fmt or case[3] not in DEV_COUNTS or case[2] in (1, 3):
                continue
            _, rate, conv, n = case
            data, want = wants(case)
            k = want[0].size
            for off in range(8):
                if rate != 16000 and off not in (0, 1 + n % 7):                       # every offset at 16 kHz (the vector body), two at the others
                    continue
                key = (case, off)
                o0, o1 = off % 4, (off + 1 + off // 4) % 4                              # the pair of destination alignments differs and varies
                assert max(o0, o1) + k + GUARD <= room_out and off * bs + len(data) <= room_in, key      # the call writes inside the allocations
                marks = np.full(room_out, np.nan, np.float32)
                assert hip.hipMemcpy(d_o0, _p(marks), C.c_size_t(marks.nbytes), 1) == 0 and hip.hipMemcpy(d_o1, _p(marks), C.c_size_t(marks.nbytes), 1) == 0
                src = C.c_void_p(d_in.value + off * bs)
                assert hip.hipMemcpy(src, data, C.c_size_t(len(data)), 1) == 0
                w = abi.wmi_wav(src, len(data), fmt, 1, rate, 1)
                got = lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), conv, C.c_void_p(d_o0.value + 4 * o0), C.c_void_p(d_o1.value + 4 * o1), k, 1)
                assert got == k, (key, got)
                backs = [np.zeros(room_out, np.float32), np.zeros(room_out, np.float32)]
                assert hip.hipMemcpy(_p(backs[0]), d_o0, C.c_size_t(backs[0].nbytes), 2) == 0 and hip.hipMemcpy(_p(backs[1]), d_o1, C.c_size_t(backs[1].nbytes), 2) == 0
                cr.hold(backs[0][o0:o0 + k], backs[1][o1:o1 + k], want, key)
                for b, o in ((backs[0], o0), (backs[1], o1)):
                    assert np.all(np.isnan(b[:o])) and np.all(np.isnan(b[o + k:])), key
                # nothing but the table is uploaded
                assert _stats(lib, ctx)[:4] == [12 * k if rate == 22050 else 0, n, 2 * k, 1 if k else 0], key
                ran += 1
        # 16 kHz: 6 counts x 8 offsets; elsewhere 4 rates x 2 converters x 6 counts, less SRC_LINEAR on one frame at 8 kHz, x 2 offsets
        assert ran == 6 * 8 + (4 * 2 * 6 - 1) * 2
    finally:
        hip.hipFree(d_in); hip.hipFree(d_o0); hip.hipFree(d_o1)


def test_odd_tails_are_ignored(product_lib, node):
    lib, ctx = product_lib, node.ctx
    for fmt in FORMATS:
        fb = 2 * wr.SAMPLE_BYTES[fmt]
        whole = cr.make_stereo(fmt, 300, seed=9)
        for rate, conv in ((16000, 2), (48000, 4)):
            for cut in range(len(whole) - 2 * fb, len(whole) + 1):                   # every count of bytes around whole frames
                data = whole[:cut]
                want = cr.convert_channels(data, fmt, rate, conv)
                got, out, guard = _to_host(lib, ctx, _wav(data, fmt, rate), conv, want[0].size)
                assert got == want[0].size, (fmt, rate, cut)
                cr.hold(out[0], out[1], want, (fmt, rate, cut))
                assert np.all(np.isnan(guard[0])) and np.all(np.isnan(guard[1]))
                assert _stats(lib, ctx)[:2] == [cut, cut // fb]


def test_two_runs_give_the_same_bits_and_the_fold_is_left_alone(product_lib, node, wants):
    lib, ctx = product_lib, node.ctx
    for case in ((wr.S16, 44100, 1, 4097), (wr.F32, 22050, 2, 4095), (wr.S8, 16000, 2, 4097)):
        fmt, rate, conv, n = case
        data, want = wants(case)
        k = want[0].size
        a = _to_host(lib, ctx, _wav(data, fmt, rate), conv, k)
        b = _to_host(lib, ctx, _wav(data, fmt, rate), conv, k)
        assert a[0] == b[0] == k and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
        # the folding call on the same clip still gives the judge's fold
        mono = np.full(k + GUARD, np.nan, np.float32)
        w = _wav(data, fmt, rate)
        assert lib.wmi_wav_to_pcm(ctx, C.byref(w), conv, _p(mono), k, 0) == k
        wr.hold(mono[:k], wr.convert(data, fmt, 1, rate, conv), case)


def test_edges(product_lib, node):
    lib, ctx = product_lib, node.ctx
    o0, o1 = np.full(64, np.nan, np.float32), np.full(64, np.nan, np.float32)
    one = _wav(wr.pack(np.array([20000, -30000], np.int32), wr.S16), wr.S16, 8000)
    assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(one), 4, _p(o0), _p(o1), 64, 0) == 0 and np.all(np.isnan(o0)) and np.all(np.isnan(o1))
    assert _stats(lib, ctx)[:4] == [0, 1, 0, 0]                                       # SRC_LINEAR upsampling one frame: 0 samples
    assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(one), 3, _p(o0), _p(o1), 64, 0) == 2  # zero-order hold repeats it
    assert o0[:2].tobytes() == np.array([20000 / 32768] * 2, np.float32).tobytes() and o1[:2].tobytes() == np.array([-30000 / 32768] * 2, np.float32).tobytes()
    assert np.all(np.isnan(o0[2:])) and np.all(np.isnan(o1[2:]))
    o0[:] = np.nan; o1[:] = np.nan
    empty = _wav(b"", wr.S16, 44100)
    assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(empty), 2, _p(o0), _p(o1), 0, 0) == 0 and _stats(lib, ctx)[:4] == [0, 0, 0, 0]
    w = _wav(bytes(4 * 4800), wr.S16, 48000)
    assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), 2, _p(o0), _p(o1), 63, 0) == -4
    assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(w), 0, _p(o0), _p(o1), 64, 0) == -10
    mono = abi.wmi_wav(w.data, w.n_bytes, wr.S16, 0, 48000, 0)
    assert lib.wmi_wav_to_pcm_channels(ctx, C.byref(mono), 2, _p(o0), _p(o1), 64, 0) == -12
    assert np.all(np.isnan(o0)) and np.all(np.isnan(o1))

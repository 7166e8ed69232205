"""The judge of the AudioStreamWAV ingest (tests/wav_ref.py) on the CPU: it REFUSES the wrong decoders a port could write — the
reference node's own among them —, the library's host-side plan (wmi_selftest_wav_plan) gives the judge's counts on every case of the
GPU table, and every conversion error is answered on a context without a device."""
import ctypes as C

import numpy as np
import pytest

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

def _refused(got, want):
    with pytest.raises(AssertionError):
        wr.hold(got, want)


def test_the_judge_accepts_the_definition_and_refuses_wrong_decoders():
    b8 = wr.make_bytes(wr.S8, 0, 64, 1)
    b16 = wr.make_bytes(wr.S16, 0, 64, 2)
    b16s = wr.make_bytes(wr.S16, 1, 64, 3)
    want8, want16, want16s = wr.decode(b8, wr.S8, 0), wr.decode(b16, wr.S16, 0), wr.decode(b16s, wr.S16, 1)
    # the definition by hand on the extreme values
    assert want8[0] == -1.0 and want8[-1] == np.float32(127 / 128) and want16[0] == -1.0 and want16[-1] == np.float32(32767 / 32768)
    assert want16s[0] == -1.0 and want16s[-1] == np.float32(32767 / 32768) and want16s.size == 64
    wr.hold(want16.copy(), want16)
    # unsigned 8-bit (a plain `char` on a platform where it is unsigned, or a WAV file's own 8-bit convention)
    _refused((np.frombuffer(b8, "u1").astype(np.float32) / np.float32(128.0)), want8)
    _refused(((np.frombuffer(b8, "u1").astype(np.float32) - 128) / np.float32(128.0)), want8)
    # big-endian 16-bit
    _refused((np.frombuffer(b16, ">i2").astype(np.float32) / np.float32(32768.0)), want16)
    # / 32767
    _refused((np.frombuffer(b16, "<i2").astype(np.float64) / 32767.0).astype(np.float32), want16)
    # the left channel instead of the fold
    _refused(wr.samples(b16s, wr.S16)[0::2], want16s)
    # the reference node's 8-bit branch: range(size / 2) with decode_s8(i * 2) — every second byte, half the samples
    node8 = (np.frombuffer(b8, "i1")[0:2 * (len(b8) // 2):2].astype(np.float32) / np.float32(128.0))
    _refused(node8, want8)
    # the reference node on a stereo asset: interleaved samples read as mono
    _refused(wr.samples(b16s, wr.S16), want16s)
    # an extra frame from a trailing odd byte / an odd trailing sample
    odd = b16 + b"\x7f"
    assert wr.decode(odd, wr.S16, 0).tobytes() == want16.tobytes() and wr.frames_of(len(odd), wr.S16, 0) == 64
    _refused(np.append(want16, np.float32(0x7f / 32768)), wr.decode(odd, wr.S16, 0))
    odd_s = b16s + b16[:2]
    assert wr.decode(odd_s, wr.S16, 1).tobytes() == want16s.tobytes() and wr.frames_of(len(odd_s), wr.S16, 1) == 64
    _refused(np.append(want16s, wr.samples(b16[:2], wr.S16)), wr.decode(odd_s, wr.S16, 1))


def test_the_judge_refuses_the_f32_capacity():
    """90 959 frames at 44.1 kHz: int(uint32(n) * (16000.0 / 44100.0)) = 33 000, the same product in f32 33 001 — one frame more than the
    converter is given room for."""
    n, rate = 90959, 44100
    assert wr.capacity(n, rate) == 33000
    f32_cap = int(np.float32(n) * np.float32(16000.0 / rate))
    assert f32_cap == 33001
    wr.hold_count(33000, n, rate, 3)
    with pytest.raises(AssertionError):
        wr.hold_count(f32_cap, n, rate, 3)
    # and the resampled wrong rate: a 44.1 kHz asset read as 16 kHz keeps its frame count
    with pytest.raises(AssertionError):
        wr.hold_count(n, n, rate, 3)


def test_the_builder_round_trips():
    v = np.array([-32768, -1, 0, 1, 32767], np.int32)
    assert wr.samples(wr.pack(v, wr.S16), wr.S16).tobytes() == (v / 32768.0).astype(np.float32).tobytes()
    v8 = np.array([-128, -1, 0, 127], np.int32)
    assert wr.pack(v8, wr.S8) == b"\x80\xff\x00\x7f"
    assert wr.pack(np.array([-2.0, -1.0, 0.0, 0.5, 1.0]), wr.S16) == np.array([-32768, -32767, 0, 16384, 32767], "<i2").tobytes()
    with pytest.raises(AssertionError):
        wr.pack(np.array([40000]), wr.S16)
    for fmt, st in wr.FORMATS:
        for n in (0, 1, 2, 9):
            b = wr.make_bytes(fmt, st, n, 5)
            assert wr.frames_of(len(b), fmt, st) == n and wr.decode(b, fmt, st).size == n


# ------------------------------------------------------------------------------------------------ the library's plan

def test_struct_layout_and_symbols(lib):
    assert C.sizeof(abi.wmi_wav) == 32
    assert [getattr(abi.wmi_wav, f).offset for f, _ in abi.wmi_wav._fields_] == [0, 8, 16, 20, 24, 28]
    assert (abi.WMI_WAV_S8, abi.WMI_WAV_S16, abi.WMI_WAV_F32) == (wr.S8, wr.S16, wr.F32) == (0, 1, 32)
    import pathlib
    text = (pathlib.Path(__file__).resolve().parent.parent / "include" / "wmi_device.h").read_text()
    for name in ("wmi_wav_to_pcm", "wmi_full_wav", "wmi_full_long_wav", "wmi_full_batch_wav", "wmi_selftest_wav_plan", "wmi_wav_stats"):
        assert name + "(" in text and hasattr(lib, name)


def test_plan_gives_the_judges_counts_on_every_case_of_the_gpu_table(lib):
    zeros = bytes(8 * max(wr.LONG_FRAMES.values()) + 8)
    counted = {}
    for fmt, st, rate, conv, n in wr.cases():
        nb = n * wr.SAMPLE_BYTES[fmt] * (2 if st else 1)
        for extra in (0, 1) if n <= 17 else (0,):                                  # an odd trailing byte adds no frame
            if extra and fmt == wr.S8 and not st:
                continue                                                           # (one more byte IS one more 8-bit mono frame)
            w = _wav(zeros[:nb + extra], fmt, st, rate)
            frames, n_out = C.c_longlong(-1), C.c_longlong(-1)
            assert lib.wmi_selftest_wav_plan(C.byref(w), conv, C.byref(frames), C.byref(n_out)) == 0, (fmt, st, rate, conv, n)
            assert frames.value == n == wr.frames_of(nb + extra, fmt, st)
            key = (rate, conv, n)                                                  # the count depends on these alone
            if key not in counted:
                counted[key] = wr.resample(np.zeros(n, np.float32), rate, conv).size
            assert n_out.value == counted[key], (fmt, st, rate, conv, n, n_out.value, counted[key])
            wr.hold_count(n_out.value, n, rate, conv, counted[key])
    # SRC_LINEAR upsampling one frame: undefined in the library, 0 samples
    w = _wav(bytes(2), wr.S16, 0, 8000)
    frames, n_out = C.c_longlong(-1), C.c_longlong(-1)
    assert lib.wmi_selftest_wav_plan(C.byref(w), 4, C.byref(frames), C.byref(n_out)) == 0 and (frames.value, n_out.value) == (1, 0)
    # the capacity with the uint32 cast in double
    w = _wav(bytes(90959), wr.S8, 0, 44100)
    assert lib.wmi_selftest_wav_plan(C.byref(w), 3, C.byref(frames), C.byref(n_out)) == 0 and n_out.value == 33000


# ------------------------------------------------------------------------------------------------ errors, without a device

def test_every_conversion_error_without_a_device(lib):
    mb = synth.make_model("micro.en", seed=1)
    buf = C.create_string_buffer(mb, len(mb))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(mb))
    p = lib.whisper_full_default_params(0)
    data = wr.make_bytes(wr.S16, 0, 4800, 1)
    dst = np.full(4800, np.nan, np.float32)
    dp = dst.ctypes.data_as(C.c_void_p)
    ok = dict(data=data, fmt=wr.S16, stereo=0, rate=48000)

    def codes(conv=2, cap=4800, d=dp, **kw):
        a = dict(ok, **kw)
        w = _wav(a["data"], a["fmt"], a["stereo"], a["rate"], a.get("on_device", 0), a.get("n_bytes"))
        if a.get("null"):
            w.data = None
        wp = C.byref(w)
        one = lib.wmi_wav_to_pcm(ctx, wp, conv, d, cap, 0)
        fulls = (lib.wmi_full_wav(ctx, p, wp, conv), lib.wmi_full_long_wav(ctx, p, wp, conv, None), lib.wmi_full_batch_wav(ctx, p, wp, 1, conv))
        plan = lib.wmi_selftest_wav_plan(wp, conv, None, None)
        return one, fulls, plan
    try:
        for kw, e in ((dict(null=True), -1), (dict(fmt=5), -1), (dict(fmt=-1), -1), (dict(fmt=16), -1), (dict(stereo=2), -1), (dict(stereo=-1), -1),
                      (dict(rate=0), -1), (dict(rate=-16000), -1), (dict(n_bytes=-2), -1), (dict(n_bytes=2 * (2 ** 31)), -1),
                      (dict(fmt=2), -11), (dict(fmt=3), -11), (dict(conv=0), -10), (dict(conv=5), -1), (dict(conv=-1), -1)):
            kw = dict(kw); conv = kw.pop("conv", 2)
            one, fulls, plan = codes(conv=conv, **kw)
            assert one == e and plan == e and fulls == (-100 + e,) * 3, (kw, conv, one, fulls, plan)
        # a device pointer that is not sample-aligned (decided from the pointer's value alone; nothing is read)
        w = abi.wmi_wav(C.c_void_p(0x7f0000001001), 9600, wr.S16, 0, 48000, 1)
        assert lib.wmi_wav_to_pcm(ctx, C.byref(w), 2, dp, 4800, 0) == -1 and lib.wmi_full_wav(ctx, p, C.byref(w), 2) == -101
        w = abi.wmi_wav(C.c_void_p(0x7f0000001002), 9600, wr.F32, 1, 48000, 1)
        assert lib.wmi_selftest_wav_plan(C.byref(w), 2, None, None) == -1
        w = abi.wmi_wav(C.c_void_p(0x7f0000001001), 9600, wr.S8, 1, 48000, 1)      # 8-bit: every address is sample-aligned
        assert lib.wmi_selftest_wav_plan(C.byref(w), 2, None, None) == 0
        # NULL arguments of the calls themselves
        w = _wav(data, wr.S16, 0, 48000)
        assert lib.wmi_wav_to_pcm(None, C.byref(w), 2, dp, 4800, 0) == -1 and lib.wmi_wav_to_pcm(ctx, None, 2, dp, 4800, 0) == -1
        assert lib.wmi_wav_to_pcm(ctx, C.byref(w), 2, None, 4800, 0) == -1 and lib.wmi_wav_to_pcm(ctx, C.byref(w), 2, dp, -1, 0) == -1
        assert lib.wmi_full_wav(None, p, C.byref(w), 2) == -101 and lib.wmi_full_batch_wav(ctx, p, None, 1, 2) == -101
        assert lib.wmi_full_batch_wav(ctx, p, C.byref(w), -1, 2) == -101
        assert lib.wmi_wav_stats(None, (C.c_int64 * 5)()) == -1 and lib.wmi_wav_stats(ctx, None) == -1
        # the capacity: 4800 frames at 48 kHz are 1600 samples
        assert lib.wmi_wav_to_pcm(ctx, C.byref(w), 2, dp, 1599, 0) == -4
        # the converter is not looked at at 16 kHz; the context cannot compute: -2, and the device was never reached
        w16 = _wav(data, wr.S16, 0, 16000)
        assert lib.wmi_selftest_wav_plan(C.byref(w16), 0, None, None) == 0 and lib.wmi_selftest_wav_plan(C.byref(w16), 77, None, None) == 0
        for ww, conv, cap in ((w, 2, 1600), (w16, 0, 4800)):
            assert lib.wmi_wav_to_pcm(ctx, C.byref(ww), conv, dp, cap, 0) == -2
            assert lib.wmi_full_wav(ctx, p, C.byref(ww), conv) == -102
            assert lib.wmi_full_long_wav(ctx, p, C.byref(ww), conv, None) == -102
            assert lib.wmi_full_batch_wav(ctx, p, C.byref(ww), 1, conv) == -102
        assert np.all(np.isnan(dst))                                                # nothing was written
        st = (C.c_int64 * 5)(7, 7, 7, 7, 7)
        assert lib.wmi_wav_stats(ctx, st) == 0 and list(st) == [0, 0, 0, 0, 0]      # no work set was ever made
    finally:
        lib.whisper_free(ctx)

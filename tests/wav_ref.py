"""The judge of the AudioStreamWAV ingest (include/wmi_device.h wmi_wav_to_pcm, wmi_full_*_wav): the definition in NumPy, and the
16 kHz step through the sequential converters the resampler tests already use.

  sample   16 bit: np.frombuffer(..., "<i2") / 32768, 8 bit: np.frombuffer(..., "i1") / 128 — the division in float64, rounded to f32
           (exact either way: a power of two under at most 16 significant bits); f32: as is
  frame    mono: the sample; stereo: (l + r) in f32, then / 2 in float64, rounded to f32 (src/speech_to_text.cpp:45-51)
  tails    a trailing incomplete sample or frame is ignored
  rate     16000: done.  Else src_simple(mono, 16000 / rate, converter) with room for int(uint32(frames) * ratio) frames:
           converters 1, 2 by oracle/liboracle_dsp.so's oracle_resample_audio_buffer (loaded as tests/test_gpu_host_dsp.py loads it),
           3, 4 by tests/resample_ref.py

hold() is what a result is judged by: the count, then every bit.  tests/test_wav_ref.py shows it refusing the wrong decoders.
"""
import ctypes as C
import functools
import pathlib
import struct

import numpy as np

import resample_ref as rr

ROOT = pathlib.Path(__file__).resolve().parent.parent
S8, S16, F32 = 0, 1, 32                       # wmi_device.h WMI_WAV_*; 0 / 1 = AudioStreamWAV.FORMAT_8_BITS / FORMAT_16_BITS
SAMPLE_BYTES = {S8: 1, S16: 2, F32: 4}
DST_RATE = 16000

# the table of the GPU test (tests/test_gpu_wav_pcm.py) and of the CPU plan test
FORMATS = [(S8, 0), (S8, 1), (S16, 0), (S16, 1), (F32, 0), (F32, 1)]
RATES = [16000, 48000, 44100, 22050, 8000]    # decode only | closed-form positions (two) | table positions | upsampling
CONVERTERS = [1, 2, 3, 4]
COUNTS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4095, 4097]      # around a group of 8, a 16-byte piece, a 256-thread block
LONG_FRAMES = {44100: 3 * 44100 + 1, 48000: 3 * 48000 + 5}                   # the 3 s cases: converter 2 only


def undefined(frames, rate, converter):
    return rate != DST_RATE and rr.undefined(frames, rate, converter)       # SRC_LINEAR upsampling one frame reads data_in[-1]


def cases():
    """(format, stereo, rate, converter, frames) of every case of the table: the full cross at the small counts (one converter at
    16 kHz, where it is not looked at), then 3 s per format at 44.1 and 48 kHz with converter 2."""
    out = []
    for fmt, st in FORMATS:
        for rate in RATES:
            for conv in ([2] if rate == DST_RATE else CONVERTERS):
                for n in COUNTS:
                    if not undefined(n, rate, conv):
                        out.append((fmt, st, rate, conv, n))
        for rate, n in LONG_FRAMES.items():
            out.append((fmt, st, rate, 2, n))
    return out


def frames_of(n_bytes, fmt, stereo):
    return n_bytes // SAMPLE_BYTES[fmt] // (2 if stereo else 1)


def capacity(frames, rate):
    """int(uint32(frames) * (16000.0 / rate)), the room the host gives the converter (src/speech_to_text.cpp:25-29)"""
    return int(np.uint32(frames) * (float(DST_RATE) / float(rate)))


def samples(data, fmt):
    """every whole sample of the bytes as f32"""
    data = bytes(data)
    bs = SAMPLE_BYTES[fmt]
    n = len(data) // bs
    if fmt == S16:
        return (np.frombuffer(data, "<i2", n).astype(np.float64) / 32768.0).astype(np.float32)
    if fmt == S8:
        return (np.frombuffer(data, "i1", n).astype(np.float64) / 128.0).astype(np.float32)
    return np.frombuffer(data, "<f4", n).copy()


def fold(x):
    """interleaved stereo samples -> mono; an odd trailing sample is ignored"""
    n = x.size // 2
    xy = x[:2 * n].reshape(n, 2)
    with np.errstate(over="ignore"):
        return ((xy[:, 0] + xy[:, 1]).astype(np.float64) / 2.0).astype(np.float32)


def decode(data, fmt, stereo):
    """the mono f32 frames at the asset's own rate"""
    x = samples(data, fmt)
    return fold(x) if stereo else x


@functools.lru_cache(maxsize=None)
def dsp():
    so = ROOT / "oracle" / "liboracle_dsp.so"
    assert so.exists(), "oracle/liboracle_dsp.so not built (python __graft_entry__.py build)"
    lib = C.CDLL(str(so))
    lib.oracle_resample_audio_buffer.restype = C.c_uint32
    lib.oracle_resample_audio_buffer.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


@functools.lru_cache(maxsize=None)
def _table(converter):
    name = {2: "sinc_fastest.bin", 1: "sinc_medium.bin"}[converter]
    raw = (ROOT / "godot-whisper_amd" / "csrc" / "data" / name).read_bytes()
    inc, cnt = struct.unpack("<ii", raw[:8])
    return inc, np.frombuffer(raw[8:], "<f4", cnt).copy()


def resample(mono, rate, converter):
    """mono f32 frames at `rate` -> 16 kHz, what src_simple returns"""
    mono = np.ascontiguousarray(mono, np.float32)
    if rate == DST_RATE:
        return mono.copy()
    if mono.size == 0:
        return np.zeros(0, np.float32)
    if converter in (1, 2):
        inc, tab = _table(converter)
        out = np.zeros(max(capacity(mono.size, rate) + 8, mono.size + 8), np.float32)
        got = dsp().oracle_resample_audio_buffer(mono.ctypes.data, mono.size, rate, DST_RATE, tab.ctypes.data, tab.size, inc, out.ctypes.data)
        return out[:got].copy()
    assert converter in (3, 4), converter
    ratio, cap = rr.ratio_and_capacity(mono.size, rate)
    return rr.src_simple(mono, ratio, converter, cap)[0]


def convert(data, fmt, stereo, rate, converter):
    """the mono 16 kHz f32 samples the transcription reads"""
    return resample(decode(data, fmt, stereo), rate, converter)


def hold(got, want, what=""):
    """the result `got` (a float32 array of exactly the samples reported) against the definition's: the count, then every bit"""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    assert got.size == want.size, (what, "count", got.size, want.size)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, "bits", int(bad.size), "first at", int(bad[0]), float(got[bad[0]]), float(want[bad[0]])))


def hold_count(n_out, frames, rate, converter, want=None):
    """the count a call reports: the definition's own (`want` when the caller has it already; it depends on the frame count, the rate
    and the converter alone), which lies within the capacity"""
    if want is None:
        want = frames if rate == DST_RATE else resample(np.zeros(frames, np.float32), rate, converter).size
    assert n_out == want, ("count", n_out, want)
    assert rate == DST_RATE or n_out <= capacity(frames, rate), ("capacity", n_out, capacity(frames, rate))


def pack(values, fmt):
    """bytes of samples (interleaved for stereo).  Integer arrays are taken as the stored values (they must fit); float arrays are
    quantised as an exporter does: round(x * 32767) / round(x * 127), clipped; F32 takes floats as they are."""
    v = np.asarray(values)
    if fmt == F32:
        return np.ascontiguousarray(v, "<f4").tobytes()
    lo, hi, scale, dt = (-32768, 32767, 32767.0, "<i2") if fmt == S16 else (-128, 127, 127.0, "i1")
    if np.issubdtype(v.dtype, np.floating):
        v = np.clip(np.rint(v.astype(np.float64) * scale), lo, hi)
    assert v.size == 0 or (v.min() >= lo and v.max() <= hi), (fmt, v.min(), v.max())
    return v.astype(dt).tobytes()


def make_bytes(fmt, stereo, frames, seed, extremes=True):
    """`frames` frames of seeded noise over the whole range of the format; with `extremes` the first and the last frame hold the
    format's extreme values (-32768 / 32767, -128 / 127; f32: -1 / 1)"""
    rng = np.random.default_rng(seed)
    n = frames * (2 if stereo else 1)
    if fmt == F32:
        v = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        v[::37] *= np.float32(1e-3)
        lo, hi = np.float32(-1.0), np.float32(1.0)
    else:
        lo, hi = (-32768, 32767) if fmt == S16 else (-128, 127)
        v = rng.integers(lo, hi + 1, n).astype(np.int32)
    if extremes and frames > 0:
        if stereo:
            v[0], v[1] = lo, lo                                   # the fold of two minima: -1 exactly
            v[-2], v[-1] = hi, hi
        else:
            v[0] = lo; v[-1] = hi
    return pack(v, fmt)


def riff_data(path):
    """(data chunk bytes, channels, rate, bits) of a PCM RIFF file — what Godot's importer hands AudioStreamWAV.data / .stereo / .mix_rate / .format"""
    b = pathlib.Path(path).read_bytes()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    off, fmt, data = 12, None, None
    while off + 8 <= len(b):
        cid, sz = b[off:off + 4], struct.unpack_from("<I", b, off + 4)[0]
        if cid == b"fmt ":
            fmt = struct.unpack_from("<HHIIHH", b, off + 8)
        elif cid == b"data":
            data = b[off + 8:off + 8 + sz]
        off += 8 + sz + (sz & 1)
    assert fmt is not None and data is not None and fmt[0] == 1, fmt
    return data, fmt[1], fmt[2], fmt[5]

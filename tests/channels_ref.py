"""The judge of the two-channel WAV calls (include/wmi_device.h wmi_wav_to_pcm_channels, wmi_full_wav_channels): the definition in NumPy
on top of tests/wav_ref.py, and the dialogue view's merge rule in plain Python.

  split     wav_ref.samples(data, fmt) de-interleaved: channel c = samples[c::2] over the whole frames (an odd trailing sample is dropped;
            wav_ref.samples has dropped an incomplete sample already) — no fold
  rate      16000: done.  Else wav_ref.resample(channel, rate, converter) per channel: two runs of the sequential converter
  merge     a stable two-way merge by start time: while both sides have entries, side 0's head if its t0 <= side 1's head's t0, else side
            1's; then the rest.  A side's own order is never changed.

hold() judges a pair of results: each channel by wav_ref.hold — the count, then every bit.  make_stereo() builds clips on which a swap, a
fold or a copy of one channel cannot pass: independent noise, (minimum, maximum) in frame 0 and (maximum, minimum) in the last frame.
tests/test_channels_ref.py shows the judge refusing the wrong answers.
"""
import numpy as np

import wav_ref as wr


def split(data, fmt):
    """-> (left, right): the two channels' f32 samples at the asset's own rate"""
    x = wr.samples(data, fmt)
    n = x.size // 2
    return x[0:2 * n:2].copy(), x[1:2 * n:2].copy()


def convert_channels(data, fmt, rate, converter):
    """-> (pcm0, pcm1): the mono 16 kHz f32 samples of each channel"""
    return tuple(wr.resample(ch, rate, converter) for ch in split(data, fmt))


def hold(got0, got1, want, what=""):
    """a pair of results against the judge's pair: per channel the count, then every bit"""
    wr.hold(got0, want[0], (what, "channel 0"))
    wr.hold(got1, want[1], (what, "channel 1"))


def merge(t0_a, t0_b):
    """-> [(channel, index)] of the dialogue view for the two channels' segment start times"""
    out, a, b = [], 0, 0
    while a < len(t0_a) and b < len(t0_b):
        if t0_a[a] <= t0_b[b]:
            out.append((0, a)); a += 1
        else:
            out.append((1, b)); b += 1
    out += [(0, i) for i in range(a, len(t0_a))]
    out += [(1, i) for i in range(b, len(t0_b))]
    return out


def make_stereo(fmt, frames, seed):
    """bytes of `frames` stereo frames: seeded noise over the whole range of the format, the two channels independent, frame 0 =
    (minimum, maximum) and the last frame = (maximum, minimum) — with one frame the first rule wins"""
    rng = np.random.default_rng([seed, 0xC4A7])
    if fmt == wr.F32:
        v = rng.uniform(-1.0, 1.0, (frames, 2)).astype(np.float32)
        v[::37, 0] *= np.float32(1e-3); v[5::41, 1] *= np.float32(1e-3)
        lo, hi = np.float32(-1.0), np.float32(1.0)
    else:
        lo, hi = (-32768, 32767) if fmt == wr.S16 else (-128, 127)
        v = rng.integers(lo, hi + 1, (frames, 2)).astype(np.int32)
    if frames > 0:
        v[-1] = (hi, lo)
        v[0] = (lo, hi)
    return wr.pack(v.reshape(-1), fmt)


def cases():
    """(format, rate, converter, frames) of the GPU table: wav_ref's grid for the three stereo formats — the full cross at the small
    counts (one converter at 16 kHz), without what wav_ref.undefined excludes"""
    out = []
    for fmt in (wr.S8, wr.S16, wr.F32):
        for rate in wr.RATES:
            for conv in ([2] if rate == wr.DST_RATE else wr.CONVERTERS):
                for n in wr.COUNTS:
                    if not wr.undefined(n, rate, conv):
                        out.append((fmt, rate, conv, n))
    return out


LONG = [(wr.S16, rate, 2, n) for rate, n in wr.LONG_FRAMES.items()]      # the 3 s cases

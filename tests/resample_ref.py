"""libsamplerate's SRC_ZERO_ORDER_HOLD and SRC_LINEAR converters restated in sequential Python, as src_simple runs them for the
host (src/speech_to_text.cpp:16-43: one channel, one src_process call, a constant ratio, last_position 0):
thirdparty/libsamplerate/src/src_zoh.c:59-126 and src_linear.c:61-135, loop for loop.  Python floats are C doubles and round() is
lrint() (round half to even); the f32 steps go through numpy.float32 scalars.

tests/test_resample_converters.py pins this file to the recorded results of the compiled library
(tests/golden/resample_zoh_linear.npz, written by tests/golden/make_resample_goldens.py) bit for bit; the GPU tests use it for
inputs the fixture does not hold.  The inputs of the fixture's cases come from make_input() below.
"""
import pathlib

import numpy as np

SRC_ZERO_ORDER_HOLD, SRC_LINEAR = 3, 4
DST_RATE = 16000
FIXTURE = pathlib.Path(__file__).resolve().parent / "golden" / "resample_zoh_linear.npz"

# The fixture's cases: every length at every rate with both converters, but for SRC_LINEAR on one frame at a ratio above 1, where the
# library reads data_in[-1] (src_linear.c:96-108 with in_used 0) and has no defined result.
LENGTHS = [0, 1, 2, 3, 57, 255, 256, 257, 441, 4096, 14669]
RATES = [48000, 32000, 44100, 22050, 47999, 8000, 11025, 16001]
CONVERTERS = [SRC_ZERO_ORDER_HOLD, SRC_LINEAR]
TILE = 441


def undefined(n, rate, converter):
    return converter == SRC_LINEAR and n == 1 and rate < DST_RATE


def cases():
    """(seed, length, rate, converter) of every fixture case, in the fixture's order."""
    out = []
    for i, n in enumerate(LENGTHS):
        for j, rate in enumerate(RATES):
            for conv in CONVERTERS:
                if not undefined(n, rate, conv):
                    out.append((1000 + 16 * i + j, n, rate, conv))
    return out


def make_input(seed, n):
    """n mono frames: TILE seeded full-mantissa f32 values of mixed magnitude, repeated.  Up to TILE frames that is plain noise.  The
    longer cases repeat it so that the recorded outputs, which then nearly repeat as well (441 frames at 44.1 kHz are 160 at 16 kHz),
    compress: the fixture stays a small file.  Inputs that never repeat run against this restatement instead."""
    rng = np.random.default_rng(seed)
    tile = rng.uniform(-1.0, 1.0, TILE)
    tile[::37] *= 1e-3
    return np.resize(tile.astype(np.float32), n)


def ratio_and_capacity(n, rate):
    ratio = float(DST_RATE) / float(rate)                       # src/speech_to_text.cpp:28-29
    return ratio, int(np.uint32(n) * ratio)


def fmod_one(x):                                                # thirdparty/libsamplerate/src/common.h:149-158
    res = x - round(x)
    return res + 1.0 if res < 0.0 else res


def positions(ratio, count):
    """(pos, frac) of the first `count` outputs: the recurrence all converters share (src_linear.c:113-117, src_sinc.c:411-416)."""
    inc = 1.0 / ratio
    pos = np.zeros(count, np.int64); frac = np.zeros(count, np.float64)
    x, p = 0.0, 0
    for i in range(count):
        pos[i] = p; frac[i] = x
        x += inc
        rem = fmod_one(x)
        p += int(round(x - rem))
        x = rem
    return pos, frac


def src_simple(x, ratio, converter, out_frames):
    """-> (output frames, input_frames_used).  Raises where the library would read outside data_in."""
    assert converter in (SRC_ZERO_ORDER_HOLD, SRC_LINEAR)
    linear = converter == SRC_LINEAR
    x = np.ascontiguousarray(x, np.float32)
    in_count = int(x.size)
    out = np.zeros(max(out_frames, 0), np.float32)
    if in_count <= 0:
        return out[:0], 0
    f32 = np.float32
    last_value = x[0]
    in_used = out_gen = 0
    input_index = 0.0
    inc = 1.0 / ratio
    # samples before the first sample of the input array
    while input_index < 1.0 and out_gen < out_frames:
        if (in_used + (1.0 + input_index) >= in_count) if linear else (in_used + input_index >= in_count):
            break
        if linear:
            out[out_gen] = f32(float(last_value) + input_index * float(f32(x[0] - last_value)))
        else:
            out[out_gen] = last_value
        out_gen += 1
        input_index += inc
    rem = fmod_one(input_index)
    in_used += int(round(input_index - rem))
    input_index = rem
    # main loop
    while out_gen < out_frames and ((in_used + input_index < in_count) if linear else (in_used + input_index <= in_count)):
        if in_used < 1:
            raise IndexError("the converter reads data_in[-1]")
        a = x[in_used - 1]
        if linear:
            out[out_gen] = f32(float(a) + input_index * float(f32(x[in_used] - a)))
        else:
            out[out_gen] = a
        out_gen += 1
        input_index += inc
        rem = fmod_one(input_index)
        in_used += int(round(input_index - rem))
        input_index = rem
    return out[:out_gen], min(in_used, in_count)


def load_fixture():
    """-> list of dicts: seed, length, rate, converter, frames_gen, frames_used, out (float32 array with the recorded bits)."""
    z = np.load(FIXTURE)
    bits = z["out_bits"]
    recs = []
    for k in range(z["seed"].size):
        a, b = int(z["offset"][k]), int(z["offset"][k + 1])
        recs.append(dict(seed=int(z["seed"][k]), length=int(z["length"][k]), rate=int(z["rate"][k]), converter=int(z["converter"][k]),
                         frames_gen=int(z["frames_gen"][k]), frames_used=int(z["frames_used"][k]), out=bits[a:b].view(np.float32)))
    return recs

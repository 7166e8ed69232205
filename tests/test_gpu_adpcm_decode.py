"""-m gpu: the IMA-ADPCM decode kernels alone (wmi_selftest_adpcm_decode, csrc/k_adpcm.hip) against the judge (tests/adpcm_ref.py), strictly
equal: mono and stereo, contents that sit in both clamps, counts around every edge of the launch shape (taken from
wmi_selftest_adpcm_shape), every source byte offset 0 - 15, an odd trailing byte, the guard around the image, the clip whose additive term
wraps 32 bits twice, and two runs bit for bit."""
import ctypes as C

import numpy as np
import pytest

import adpcm_ref as ar
from godot_whisper_amd import runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = runtime.require_gpu()
    runtime.silence_logs(lib)
    return lib


@pytest.fixture(scope="module")
def shape(lib):
    out = (C.c_int * 5)()
    assert lib.wmi_selftest_adpcm_shape(out) == 0
    chunk, lanes, wg, tile, launches = list(out)
    return dict(chunk=chunk, wave=chunk * lanes, group=chunk * wg, tile=tile)


def _decode(lib, data, stereo, offset=0, cap=None):
    data = bytes(data)
    frames = ar.frames_of(len(data), stereo)
    nch = 2 if stereo else 1
    out = np.full(frames * nch + 8, 0x5A5A, np.int16)
    got = C.c_longlong(-1)
    buf = C.create_string_buffer(data, max(len(data), 1))
    r = lib.wmi_selftest_adpcm_decode(0, buf, len(data), stereo, offset, out.ctypes.data_as(C.c_void_p), frames if cap is None else cap, C.byref(got))
    assert got.value == frames, (got.value, frames)
    if r != 0:
        return r
    assert np.all(out[frames * nch:] == 0x5A5A)                               # nothing behind the caller's samples
    return out[:frames * nch]


def _clip(kinds, n, seed):
    """A clip of n nibbles per channel (n even), one content per channel."""
    return ar.pack([ar.content(kind, n, seed + 17 * c) for c, kind in enumerate(kinds)])


def _edge_counts(shape):
    c, w, g = shape["chunk"], shape["wave"], shape["group"]
    raw = [1, 2, c - 1, c, c + 1, w - 1, w, w + 1, g - 1, g, g + 1, 2 * g + 1]
    return sorted({n + (n & 1) for n in raw} | {c - 2, w - 2, g - 2, w + 2, g + 2})       # a byte holds two nibbles: even counts either side


@pytest.mark.parametrize("stereo", [0, 1])
def test_counts_around_every_edge_of_the_launch_shape(lib, shape, stereo):
    other = {"random": "small", "sevens": "fifteens", "fifteens": "zeros", "zeros": "runs", "runs": "random", "small": "sevens"}
    for n in _edge_counts(shape):
        for kind in ar.CONTENTS:
            data = _clip((kind, other[kind]) if stereo else (kind,), n, seed=n)
            got = _decode(lib, data, stereo)
            assert not isinstance(got, int), (n, kind, got)
            ar.hold(got, ar.decode(data, stereo))


def test_every_source_byte_offset(lib, shape):
    """The head in front of the first 16-byte boundary is 0 - 15 bytes (stereo: whole byte pairs, or none at an odd address: every chunk
    by bytes); the image's place moves with it."""
    n = shape["wave"] + 3 * shape["chunk"] + 6
    mono, stereo = _clip(("random",), n, 3), _clip(("runs", "random"), n, 4)
    want_m, want_s, want_odd = ar.decode(mono, 0), ar.decode(stereo, 1), ar.decode(stereo + b"\xc3", 1)
    ar.hold(want_odd, want_s)
    for offset in range(16):
        ar.hold(_decode(lib, mono, 0, offset), want_m)
        ar.hold(_decode(lib, stereo, 1, offset), want_s)
        ar.hold(_decode(lib, stereo + b"\xc3", 1, offset), want_s)           # an odd trailing byte adds nothing
    # clips shorter than the head
    for nb in (1, 2, 3, 5, 14, 15, 16, 17):
        for offset in (0, 1, 2, 9, 15):
            d = bytes(np.random.default_rng(nb * 16 + offset).integers(0, 256, nb, dtype=np.uint8))
            ar.hold(_decode(lib, d, 0, offset), ar.decode(d, 0))
            ar.hold(_decode(lib, d, 1, offset), ar.decode(d, 1))            # (one byte: no frame, an empty clip)


@pytest.mark.parametrize("stereo", [0, 1])
def test_more_partials_than_one_tile_of_the_cross_workgroup_walk(lib, shape, stereo):
    n = shape["group"] * shape["tile"] + shape["group"] + shape["chunk"] + 2  # tile + 2 workgroups: the walk makes a second pass with a carry
    data = _clip(("random", "small") if stereo else ("random",), n, seed=11)
    want = ar.decode(data, stereo)
    got = _decode(lib, data, stereo, offset=5 if not stereo else 6)
    ar.hold(got, want)
    ar.hold(_decode(lib, data, stereo, offset=5 if not stereo else 6), got)   # two runs, bit for bit


def test_an_additive_term_beyond_32_bits(lib):
    sat = ar.saturation_nibbles()
    mono = ar.pack([sat])
    want = ar.decode(mono, 0)
    assert want[69999] == 32767 and want[-1] == -32768
    ar.hold(_decode(lib, mono, 0), want)
    stereo = ar.pack([sat, sat[::-1]])
    ar.hold(_decode(lib, stereo, 1, offset=3), ar.decode(stereo, 1))
    ar.hold(_decode(lib, stereo, 1, offset=3), ar.decode(stereo, 1))


def test_capacity_empty_clips_and_argument_errors(lib, shape):
    data = _clip(("random",), shape["chunk"] * 4, 1)
    frames = ar.frames_of(len(data), 0)
    assert _decode(lib, data, 0, cap=frames - 1) == -4
    assert isinstance(_decode(lib, data, 0, cap=frames), np.ndarray)
    out = np.zeros(8, np.int16)
    got = C.c_longlong(-1)
    assert lib.wmi_selftest_adpcm_decode(0, None, 0, 0, 0, out.ctypes.data_as(C.c_void_p), 0, C.byref(got)) == 0 and got.value == 0
    assert lib.wmi_selftest_adpcm_decode(0, b"\x11", 1, 1, 0, out.ctypes.data_as(C.c_void_p), 0, C.byref(got)) == 0 and got.value == 0
    assert lib.wmi_selftest_adpcm_decode(0, b"\x11", 1, 2, 0, out.ctypes.data_as(C.c_void_p), 8, C.byref(got)) == -1
    assert lib.wmi_selftest_adpcm_decode(0, b"\x11", 1, 0, -1, out.ctypes.data_as(C.c_void_p), 8, C.byref(got)) == -1
    assert lib.wmi_selftest_adpcm_decode(-1, b"\x11", 1, 0, 0, out.ctypes.data_as(C.c_void_p), 8, C.byref(got)) == -1
    assert lib.wmi_selftest_adpcm_decode(0, b"\x11", 1, 0, 0, None, 8, C.byref(got)) == -1
    ms = (C.c_float * 2)()
    assert lib.wmi_bench_adpcm_decode(0, data, len(data), 0, 0, 2, ms) == 0 and ms[0] > 0 and ms[1] > 0
    assert lib.wmi_bench_adpcm_decode(0, data, len(data), 0, 0, 0, ms) == -1

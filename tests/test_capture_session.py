"""CPU side of the capture session (include/wmi_device.h wmi_capture_*; csrc/capture.cpp, k_resample.hip, k_mel.hip):

* the host's decision which resampled outputs survive a push (wmi_selftest_capture_plan): the outputs below first_dirty are the same
  bytes for the old and for the grown input, by the sequential converters themselves (oracle/liboracle_dsp.so for the SINC converters,
  tests/resample_ref.py for zero-order hold and linear);
* the block scheme of the parallel VAD filter, restated in numpy with its hand-over check and re-run, against host.high_pass_filter;
* argument errors and NULL safety of every new entry point on a context without a device.
"""
import ctypes as C
import math
import pathlib
import struct

import numpy as np
import pytest

import resample_ref as rr
from godot_whisper_amd import host, runtime, synth

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


@pytest.fixture(scope="module")
def dsp():
    so = ROOT / "oracle" / "liboracle_dsp.so"
    assert so.exists(), "oracle/liboracle_dsp.so not built (python __graft_entry__.py build)"
    d = C.CDLL(str(so))
    d.oracle_resample_audio_buffer.restype = C.c_uint32
    d.oracle_resample_audio_buffer.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return d


def _table(name):
    raw = (ROOT / "godot-whisper_amd" / "csrc" / "data" / name).read_bytes()
    inc, cnt = struct.unpack("<ii", raw[:8])
    return inc, np.frombuffer(raw[8:], "<f4", cnt).copy()


TABLES = {2: _table("sinc_fastest.bin"), 1: _table("sinc_medium.bin")}


def _sequential(dsp, x, rate, converter):
    """What src_simple gives the host for mono frames x at `rate` -> 16 kHz."""
    x = np.ascontiguousarray(x, np.float32)
    if converter in (1, 2):
        inc, tab = TABLES[converter]
        out = np.zeros(max(int(x.size * 16000.0 / rate) + 8, x.size + 8), np.float32)
        got = dsp.oracle_resample_audio_buffer(x.ctypes.data, x.size, rate, 16000, tab.ctypes.data, tab.size, inc, out.ctypes.data)
        return out[:got]
    ratio, cap = rr.ratio_and_capacity(x.size, rate)
    return rr.src_simple(x, ratio, converter, cap)[0]


def _closed_form(lib, rate):
    closed = C.c_int(-1)
    r = lib.wmi_selftest_resample_plan(5000, rate, 16000, 2, None, None, C.byref(closed), 0, None, None)
    assert r == 0, (rate, r)
    return closed.value


CANDIDATE_RATES = [48000, 44100, 32000, 96000, 8000, 192000, 24000, 64000, 12000, 4000, 128000, 22050, 11025, 47999, 16001, 88200]


def _capture_plan(lib, n_old, n_new, rate, converter):
    fd, a, b = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    r = lib.wmi_selftest_capture_plan(n_old, n_new, rate, converter, C.byref(fd), C.byref(a), C.byref(b))
    return r, fd.value, a.value, b.value


@pytest.mark.parametrize("converter", [1, 2, 3, 4])
def test_outputs_below_first_dirty_do_not_change_when_frames_are_appended(lib, dsp, converter):
    closed = [r for r in CANDIDATE_RATES if _closed_form(lib, r) == 1]
    assert {48000, 44100, 32000, 96000, 8000} <= set(closed), closed
    rng = np.random.default_rng(100 + converter)
    for rate in closed:
        for _ in range(2):
            n_old = int(rng.integers(4096, 5200))
            n_new = n_old + int(rng.integers(1, 2500))
            x = rng.uniform(-1.0, 1.0, n_new).astype(np.float32)
            r, fd, n_out_old, n_out_new = _capture_plan(lib, n_old, n_new, rate, converter)
            assert r == 0, (rate, converter, n_old, n_new, r)
            old, new = _sequential(dsp, x[:n_old], rate, converter), _sequential(dsp, x, rate, converter)
            assert (n_out_old, n_out_new) == (old.size, new.size), (rate, converter, n_old, n_new)
            assert 0 <= fd <= min(n_out_old, n_out_new)
            assert old[:fd].tobytes() == new[:fd].tobytes(), (rate, converter, n_old, n_new, fd)
            # loose on purpose: the longest half-filter here is about 274 input frames, or 46 outputs at 96 kHz
            assert fd > n_out_old / 2, (rate, converter, n_old, n_new, fd, n_out_old)
    for rate in [r for r in CANDIDATE_RATES if r not in closed]:          # positions from the host's table: everything is recomputed
        r, fd, n_out_old, n_out_new = _capture_plan(lib, 4096, 6000, rate, converter)
        assert r == 0 and fd == 0 and 0 < n_out_old < n_out_new, (rate, converter, r, fd)


def test_capture_plan_argument_errors(lib):
    for args in [(-1, 10, 48000, 2), (10, 9, 48000, 2), (10, 20, 0, 2), (10, 20, 16000, 2), (10, 20, 48000, 0), (10, 20, 48000, 5)]:
        assert lib.wmi_selftest_capture_plan(*args, None, None, None) == -1, args
    assert lib.wmi_selftest_capture_plan(0, 0, 48000, 2, None, None, None) == 0
    r, fd, a, b = _capture_plan(lib, 0, 4800, 48000, 2)
    assert (r, fd, a) == (0, 0, 0) and b == 1600
    r, fd, a, b = _capture_plan(lib, 5000, 5000, 48000, 2)                 # nothing appended: nothing past the old outputs to compute
    assert r == 0 and a == b and fd <= a


# ------------------------------------------------------------------------------------------------ the VAD filter in blocks
BLOCK, WARM_DEFAULT = 64, 32


def _alpha(cutoff, sample_rate):
    rc = np.float32(1.0 / (2.0 * math.pi * float(np.float32(cutoff))))
    dt = np.float32(1.0) / np.float32(sample_rate)
    return np.float32(dt / np.float32(rc + dt))


def _chain(alpha, y, xs, out=None):
    """y_i = alpha * ((y_{i-1} + x_i) - y_{i-1}) in f32, sample by sample (one lane's re-run)."""
    for j in range(xs.size):
        y = np.float32(alpha * np.float32(np.float32(y + xs[j]) - y))
        if out is not None:
            out[j] = y
    return y


def blocked_filter(x, alpha, warm):
    """csrc/k_mel.hip k_vad_blocks + the hand-over part of k_vad_finish, vectorised over the blocks: -> (y, blocks, blocks re-run)."""
    n = x.size
    nb = (n + BLOCK - 1) // BLOCK
    xp = np.concatenate([np.zeros(BLOCK, np.float32), x, np.zeros(nb * BLOCK - n, np.float32)]).reshape(nb + 1, BLOCK)
    prev, own = xp[:-1], xp[1:]                              # row b: the block in front of block b, block b itself
    y = np.zeros(nb, np.float32)                             # every lane's guess
    for j in range(BLOCK - warm, BLOCK):
        y = (alpha * ((y + prev[:, j]) - y)).astype(np.float32)
    entry = y.copy()
    ys = np.zeros((nb, BLOCK), np.float32)
    for j in range(BLOCK):
        y = (alpha * ((y + own[:, j]) - y)).astype(np.float32)
        if j == 0:
            y[0] = own[0, 0]                                  # block 0 starts as the reference does
        ys[:, j] = y
    cnt = np.minimum(BLOCK, n - BLOCK * np.arange(nb))
    exit_ = ys[np.arange(nb), cnt - 1].copy()
    rerun = 0
    state = exit_[0]
    for b in range(1, nb):                                    # compared as integers: the BITS of the two states
        if entry[b].view(np.uint32) == state.view(np.uint32):
            state = exit_[b]
            continue
        state = _chain(alpha, state, own[b, :cnt[b]], ys[b])
        rerun += 1
    return ys.reshape(-1)[:n].copy(), nb, rerun


def _signals():
    sr, n = 16000, 48000
    rng = np.random.default_rng(2024)
    t = np.arange(n) / sr
    env = 0.5 * (1 + np.sin(2 * np.pi * 1.7 * t)) * (np.sin(2 * np.pi * 0.4 * t) > -0.3)
    out = {
        "gaussian": 0.1 * rng.standard_normal(n),
        "tones": env * (0.3 * np.sin(2 * np.pi * 180 * t) + 0.2 * np.sin(2 * np.pi * 1230 * t + 1.0) + 0.1 * np.sin(2 * np.pi * 3100 * t)),
        "gated": 0.05 * rng.standard_normal(n) * (np.floor(t * 4) % 2),
        "tiny": 1e-6 * rng.standard_normal(n),
        "decades": rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 0, n),
        "dc": 0.5 + 0.01 * rng.standard_normal(n),
        "int16": np.round(3000 * rng.standard_normal(n)).clip(-32768, 32767) / 32768.0,
        "constant": np.full(n, 0.25),
        "silence": np.zeros(n),
    }
    return {k: v.astype(np.float32) for k, v in out.items()}


SIGNALS = _signals()


@pytest.fixture(scope="module")
def filtered_200():
    """host.high_pass_filter (the reference's loop) of every signal at 200 Hz, computed once."""
    out = {}
    for kind, x in SIGNALS.items():
        y = x.copy()
        host.high_pass_filter(y, 200.0, 16000.0)
        out[kind] = y
    return out


@pytest.mark.parametrize("kind", list(SIGNALS))
def test_block_scheme_equals_the_sequential_filter(filtered_200, kind):
    x, want = SIGNALS[kind], filtered_200[kind]
    alpha = _alpha(200.0, 16000)
    with np.errstate(all="ignore"):
        got, nb, rerun = blocked_filter(x, alpha, WARM_DEFAULT)
        assert nb == 750 and got.tobytes() == want.tobytes(), kind
        assert rerun == 0, (kind, rerun)
        m = 16000 + 37                                           # (the re-run is a Python loop: a shorter, ragged window for these)
        for warm in (0, 1):
            got, nb, rerun = blocked_filter(x[:m], alpha, warm)
            assert nb == 251 and got.tobytes() == want[:m].tobytes(), (kind, warm)
            assert warm != 0 or kind == "silence" or rerun > 0, (kind, warm, rerun)      # (a silent stretch hands over 0.0 = the guess)


@pytest.mark.parametrize("cutoff", [100.0, 200.0, 1000.0])
def test_no_block_is_run_again_at_the_default_warm_up(cutoff):
    alpha = _alpha(cutoff, 16000)
    for kind, x in SIGNALS.items():
        with np.errstate(all="ignore"):
            got, nb, rerun = blocked_filter(x, alpha, WARM_DEFAULT)
            assert rerun == 0, (cutoff, kind, rerun)
            m = 4096 + 5                                         # and the answer is the sequential one (warm 0 = every block from its predecessor)
            seq = x[:m].copy()
            host.high_pass_filter(seq, cutoff, 16000.0)
            assert got[:m].tobytes() == seq.tobytes(), (cutoff, kind)


def test_hand_over_check_compares_bits():
    """A NaN state never equals itself as a float: compared as integers, a window that has gone NaN hands over without a re-run per block
    only where the bits agree, and the answer stays the sequential one."""
    x = SIGNALS["gaussian"][:1000].copy()
    x[300] = np.nan
    alpha = _alpha(200.0, 16000)
    with np.errstate(all="ignore"):
        got, nb, rerun = blocked_filter(x, alpha, WARM_DEFAULT)
        want = x.copy()
        host.high_pass_filter(want, 200.0, 16000.0)
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    assert np.all(np.isnan(got[300:])) and 0 < rerun <= nb


# ------------------------------------------------------------------------------------------------ arguments, NULL safety (no device)
def test_new_entry_points_refuse_bad_arguments_without_a_device(lib):
    m = synth.make_model("micro.en", seed=1)
    buf = C.create_string_buffer(m, len(m))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(m))
    assert ctx
    try:
        # a session needs a context that can compute
        assert not lib.wmi_capture_init(ctx, 44100, 2, 0)
        assert not lib.wmi_capture_init(None, 44100, 2, 0)
        x = np.zeros(128, np.float32)
        en = np.zeros(2, np.float32); st = np.zeros(2, np.int32)
        for form in (0, 1):
            assert lib.wmi_selftest_vad(ctx, x.ctypes.data, 128, 1000, 20, 2.0, 200.0, form, -1, en.ctypes.data, st.ctypes.data) == -1
        assert lib.wmi_selftest_vad(None, x.ctypes.data, 128, 1000, 20, 2.0, 200.0, 1, -1, None, None) == -1
    finally:
        lib.whisper_free(ctx)
    # NULL sessions: every call answers an error (or nothing), none touches memory
    lib.wmi_capture_free(None)
    n = C.c_int(123)
    stats = (C.c_int64 * 4)()
    assert lib.wmi_capture_push(None, x.ctypes.data, 4, 0) == -1
    assert lib.wmi_capture_keep_last(None, 4) == -1
    assert lib.wmi_capture_resample(None, C.byref(n)) == -1
    assert lib.wmi_capture_pcm(None, C.byref(n)) is None and n.value == 0
    assert lib.wmi_capture_pcm(None, None) is None
    assert lib.wmi_capture_read_pcm(None, x.ctypes.data, 128) == -1
    assert lib.wmi_capture_vad(None, 2.0, 200.0, None) == -1
    p = lib.whisper_full_default_params(0)
    assert lib.wmi_capture_full(None, p) == -1
    assert lib.wmi_capture_stats(None, stats) == -1

"""The judge of the IMA-ADPCM decode (tests/adpcm_ref.py) on the CPU: it agrees with audioop on mono streams, REFUSES the wrong decoders
a port could write, csrc/adpcm_map.h's composed maps (wmi_selftest_adpcm_maps) give the sequential decoder's state at every chunk edge —
through both clamps and through an additive term that wraps 32 bits twice —, and the mode's error codes and counts are answered without a
device."""
import ctypes as C

import numpy as np
import pytest

import adpcm_ref as ar
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


# ------------------------------------------------------------------------------------------------ the judge

def test_the_judge_equals_audioop_on_mono_streams():
    audioop = pytest.importorskip("audioop")
    for kind in ar.CONTENTS:
        for n in (2, 64, 1026, 4000):
            data = ar.pack([ar.content(kind, n, seed=n)])
            swapped = bytes(((b & 15) << 4) | (b >> 4) for b in data)        # audioop reads the high nibble first
            lin, _ = audioop.adpcm2lin(swapped, 2, None)
            ar.hold(ar.decode(data, 0), np.frombuffer(lin, "<i2"))
    sat = ar.pack([ar.saturation_nibbles()])
    lin, _ = audioop.adpcm2lin(bytes(((b & 15) << 4) | (b >> 4) for b in sat), 2, None)
    ar.hold(ar.decode(sat, 0), np.frombuffer(lin, "<i2"))


def test_the_definition_by_hand():
    # nibble 7 from (0, 0): step 7, diff 0 + 1 + 3 + 7 = 11, index 8; then step 16: diff 2 + 4 + 8 + 16 = 30
    assert ar.decode(bytes([0x77]), 0).tolist() == [11, 41]
    # nibble 15: the same magnitudes, negative; low nibble first: 0xF7 = 7, then 15
    assert ar.decode(bytes([0xF7]), 0).tolist() == [11, 11 - 30]
    # stereo: byte 0 is the left channel's two frames, byte 1 the right's; an odd trailing byte adds nothing
    assert ar.decode(bytes([0x77, 0xFF]), 1).tolist() == [11, -11, 41, -41]
    assert ar.decode(bytes([0x77, 0xFF, 0x12]), 1).tolist() == [11, -11, 41, -41] and ar.frames_of(3, 1) == 2
    # both clamps
    up = ar.decode(ar.pack([[7] * 200]), 0)
    assert up[-1] == 32767 and ar.decode_nibbles([7] * 200)[1][-1] == (32767, 88)
    assert ar.decode(ar.pack([[15] * 200]), 0)[-1] == -32768
    assert ar.decode_nibbles([0] * 50)[1][-1][1] == 0
    # the builder round-trips, the encoder tracks a sine within its step
    x = (np.sin(np.arange(4000) * 0.05) * 12000).astype(np.int64)
    y = np.array(ar.decode_nibbles(ar.encode(x))[0])
    assert np.max(np.abs(y[200:] - x[200:])) < 3000
    assert ar.channel_nibbles(ar.pack([[1, 2, 3, 4], [5, 6, 7, 8]]), 1, 1) == [5, 6, 7, 8]


def _decode_variant(data, stereo, high_first=False, per_nibble_stereo=False, step_after=False, no_clamp=False, idx_max=88, no_shr3=False,
                    sign_first=False, reset_every=0):
    """A decoder with one mistake switched on."""
    data = bytes(data)
    nch = 2 if stereo else 1
    if stereo:
        data = data[:len(data) & ~1]
    nib = []
    for b in data:
        nib += [b >> 4, b & 15] if high_first else [b & 15, b >> 4]
    if stereo:
        chans = [nib[c::2] for c in range(2)] if per_nibble_stereo else [[n for k in range(c, len(data), 2) for n in nib[2 * k:2 * k + 2]] for c in range(2)]
    else:
        chans = [nib]
    step_tab = ar.STEP + [32767]
    out = np.zeros(len(chans[0]) * nch, np.int64)
    for c, l in enumerate(chans):
        pred, idx = 0, 0
        for i, n in enumerate(l):
            if reset_every and i % (2 * reset_every) == 0:
                pred, idx = 0, 0
            if step_after:
                idx = ar.clamp(idx + ar.INDEX[n], 0, idx_max)
                step = step_tab[idx]
            else:
                step = step_tab[idx]
                idx = ar.clamp(idx + ar.INDEX[n], 0, idx_max)
            if sign_first:
                d = -(step >> 3) if n & 8 else step >> 3
                d += (step >> 2 if n & 1 else 0) + (step >> 1 if n & 2 else 0) + (step if n & 4 else 0)
            else:
                d = ar.diff_of(step, n)
                if no_shr3:
                    d -= -(step >> 3) if n & 8 else step >> 3
            pred = pred + d if no_clamp else ar.clamp(pred + d, -32768, 32767)
            out[i * nch + c] = pred
    return (out & 0xffff).astype(np.uint16).view(np.int16)


def test_the_judge_refuses_wrong_decoders():
    # 1200 bytes of mixed content: random codes, then a run that saturates both clamps
    mono = ar.pack([ar.content("random", 1200, 1) + [7] * 300 + [15] * 300 + ar.content("small", 600, 2)])
    left = ar.content("random", 1200, 3) + [7] * 300 + [15] * 300 + ar.content("small", 600, 4)
    right = ar.content("small", 1200, 6) + [15] * 300 + [7] * 300 + ar.content("random", 600, 7)
    stereo = ar.pack([left, right])
    want_m, want_s = ar.decode(mono, 0), ar.decode(stereo, 1)
    ar.hold(_decode_variant(mono, 0), want_m)                                # the variant machine itself, no mistake on
    ar.hold(_decode_variant(stereo, 1), want_s)
    ar.hold(_decode_variant(stereo + b"\x5a", 1), want_s)

    def refused(got, want):
        with pytest.raises(AssertionError):
            ar.hold(got, want)
    refused(_decode_variant(mono, 0, high_first=True), want_m)
    refused(_decode_variant(stereo, 1, per_nibble_stereo=True), want_s)
    refused(_decode_variant(stereo, 0), want_s)                              # stereo read as mono: the same sample count, other samples
    assert _decode_variant(stereo, 0).size == want_s.size
    refused(_decode_variant(mono, 0, step_after=True), want_m)
    refused(_decode_variant(mono, 0, no_clamp=True), want_m)
    refused(_decode_variant(mono, 0, idx_max=89), want_m)
    refused(_decode_variant(mono, 0, no_shr3=True), want_m)
    refused(_decode_variant(mono, 0, sign_first=True), want_m)
    refused(_decode_variant(mono, 0, reset_every=512), want_m)
    refused(np.zeros(want_m.size, np.int16), want_m)
    refused(want_m[:-1], want_m)
    refused(want_m.astype(np.int32), want_m)


# ------------------------------------------------------------------------------------------------ the map algebra of the library

def _lib_maps(lib, nibbles, chunk):
    nb = np.asarray(nibbles, np.uint8)
    chunks = (nb.size + chunk - 1) // chunk
    pred, idx = np.full(chunks + 1, -99999, np.int32), np.full(chunks + 1, -99999, np.int32)
    r = lib.wmi_selftest_adpcm_maps(nb.ctypes.data_as(C.c_void_p), nb.size, chunk, pred.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                    chunks + 1)
    assert r == chunks, (r, chunks)
    return list(zip(pred.tolist(), idx.tolist()))


def _alternating(n, chunk):
    """7s and 15s swapping one nibble off every chunk edge, so that runs end just in front of, on and behind the edges."""
    out, v = [], 7
    for i in range(n):
        if i % chunk in (chunk - 1, 0, 1) and i % 3 == 0:
            v = 22 - v
        out.append(v)
    return out


def test_composed_maps_give_the_sequential_states_at_every_chunk_edge(lib):
    for chunk in (1, 2, 8, 64):
        for n in sorted({1, 2, max(chunk - 1, 1), chunk, chunk + 1, 513, 4000}):
            streams = [ar.content(kind, n, seed=n + chunk) for kind in ("random", "sevens", "fifteens", "zeros", "runs", "small")]
            streams.append(_alternating(n, chunk))
            for nibbles in streams:
                _, states = ar.decode_nibbles(nibbles)
                want = [states[min(j * chunk, n)] for j in range((n + chunk - 1) // chunk + 1)]
                got = _lib_maps(lib, nibbles, chunk)
                assert got == want, (chunk, n, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:4])
                assert ar.plan_entry_states(nibbles, chunk) == want          # the restated plan, for the GPU tests' sake


def test_an_additive_term_beyond_32_bits(lib):
    nibbles = ar.saturation_nibbles()
    _, states = ar.decode_nibbles(nibbles)
    n = len(nibbles)
    # the sum of the diffs alone, unclamped, leaves 32 bits on the way up and comes all the way down again
    idx, s, peak = 0, 0, 0
    for x in nibbles:
        s += ar.diff_of(ar.STEP[idx], x)
        idx = ar.clamp(idx + ar.INDEX[x], 0, 88)
        peak = max(peak, s)
    assert peak > 2 ** 32 and peak - s > 2 ** 32
    for chunk in (64, 35000, 70000, n):
        want = [states[min(j * chunk, n)] for j in range((n + chunk - 1) // chunk + 1)]
        assert _lib_maps(lib, nibbles, chunk) == want, chunk
    assert states[70000] == (32767, 88) and states[n] == (-32768, 88)
    # a map composed over a whole half and applied to the far end of the domain
    m = ar.PRED_ID
    for x in nibbles[:70000]:
        m = ar.compose(m, (ar.diff_of(ar.STEP[88], x), -32768, 32767))
    assert m[0] > 2 ** 31 and ar.apply_map(m, -32768) == 32767


def test_maps_hook_argument_errors(lib):
    nb = np.array([1, 2, 3], np.uint8)
    out = np.zeros(8, np.int32)
    p, o = nb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.wmi_selftest_adpcm_maps(p, 3, 0, o, o, 8) == -1 and lib.wmi_selftest_adpcm_maps(p, -1, 2, o, o, 8) == -1
    assert lib.wmi_selftest_adpcm_maps(p, 3, 2, o, o, 2) == -4 and lib.wmi_selftest_adpcm_maps(None, 3, 2, o, o, 8) == -1
    bad = np.array([1, 16, 3], np.uint8)
    assert lib.wmi_selftest_adpcm_maps(bad.ctypes.data_as(C.c_void_p), 3, 2, o, o, 8) == -1
    assert lib.wmi_selftest_adpcm_maps(None, 0, 4, o, o, 1) == 0 and out[0] == 0


def test_the_host_decoder_is_the_judge(lib):
    for stereo in (0, 1):
        for n_bytes in (0, 1, 2, 3, 33, 1000):
            data = bytes(np.random.default_rng(n_bytes + stereo).integers(0, 256, n_bytes, dtype=np.uint8))
            want = ar.decode(data, stereo)
            frames = ar.frames_of(n_bytes, stereo)
            got = np.full(want.size + 4, 12345, np.int16)
            buf = C.create_string_buffer(data, max(n_bytes, 1))
            assert lib.wmi_selftest_adpcm_host(buf, n_bytes, stereo, got.ctypes.data_as(C.c_void_p), frames) == frames
            ar.hold(got[:want.size], want)
            assert np.all(got[want.size:] == 12345)
            if frames:
                assert lib.wmi_selftest_adpcm_host(buf, n_bytes, stereo, got.ctypes.data_as(C.c_void_p), frames - 1) == -4
    sat = ar.pack([ar.saturation_nibbles()])
    got = np.zeros(140000, np.int16)
    assert lib.wmi_selftest_adpcm_host(sat, len(sat), 0, got.ctypes.data_as(C.c_void_p), 140000) == 140000
    ar.hold(got, ar.decode(sat, 0))


# ------------------------------------------------------------------------------------------------ the mode, without a device

def test_symbols_and_shape(lib):
    import pathlib
    text = (pathlib.Path(__file__).resolve().parent.parent / "include" / "wmi_device.h").read_text()
    for name in ("wmi_set_wav_adpcm", "wmi_selftest_adpcm_plan", "wmi_selftest_adpcm_shape", "wmi_selftest_adpcm_decode", "wmi_selftest_adpcm_host",
                 "wmi_selftest_adpcm_maps", "wmi_bench_adpcm_decode"):
        assert name + "(" in text and hasattr(lib, name)
    assert abi.WMI_WAV_IMA_ADPCM == ar.ADPCM == 2
    shape = (C.c_int * 5)()
    assert lib.wmi_selftest_adpcm_shape(shape) == 0 and lib.wmi_selftest_adpcm_shape(None) == -1
    chunk, lanes, wg, tile, launches = list(shape)
    assert chunk >= 2 and chunk % 2 == 0 and lanes == 64 and wg % lanes == 0 and tile >= lanes and launches >= 3


def test_plan_counts_against_the_judge(lib):
    frames, n_out = C.c_longlong(-1), C.c_longlong(-1)
    for stereo in (0, 1):
        for n_bytes in (0, 1, 2, 3, 16, 17, 4801, 66150):
            for rate, conv in ((16000, 2), (44100, 2), (22050, 4), (48000, 3), (8000, 1)):
                w = _wav(bytes(n_bytes), ar.ADPCM, stereo, rate)
                assert lib.wmi_selftest_adpcm_plan(C.byref(w), conv, C.byref(frames), C.byref(n_out)) == 0, (stereo, n_bytes, rate, conv)
                n = ar.frames_of(n_bytes, stereo)
                assert frames.value == n == ar.decode(bytes(n_bytes), stereo).size // (2 if stereo else 1)
                # behind the decode the clip IS an s16 clip of that many frames: the same plan
                ws = _wav(bytes(n * (4 if stereo else 2)), wr.S16, stereo, rate)
                f2, o2 = C.c_longlong(-1), C.c_longlong(-1)
                assert lib.wmi_selftest_wav_plan(C.byref(ws), conv, C.byref(f2), C.byref(o2)) == 0
                assert (frames.value, n_out.value) == (f2.value, o2.value)
                if n and not (conv == 4 and n == 1 and rate < 16000):
                    wr.hold_count(n_out.value, n, rate, conv)
    # the PCM formats plan as they do without the mode
    w = _wav(bytes(9600), wr.S16, 1, 48000)
    assert lib.wmi_selftest_adpcm_plan(C.byref(w), 2, C.byref(frames), C.byref(n_out)) == 0 and (frames.value, n_out.value) == (2400, 800)


def test_error_codes_in_both_modes_without_a_device(lib):
    mb = synth.make_model("micro.en", seed=1)
    buf = C.create_string_buffer(mb, len(mb))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(mb))
    p = lib.whisper_full_default_params(0)
    data = ar.pack([ar.content("random", 4800, 1), ar.content("small", 4800, 2)])
    dst = np.full(4800, np.nan, np.float32)
    dp = dst.ctypes.data_as(C.c_void_p)
    t = (C.c_int64 * 1)(0)
    spk = (abi.wmi_speaker * 1)()

    def codes(w, conv=2):
        wp = C.byref(w)
        return (lib.wmi_wav_to_pcm(ctx, wp, conv, dp, 4800, 0), lib.wmi_wav_to_pcm_channels(ctx, wp, conv, dp, dp, 2400, 0),
                lib.wmi_full_wav(ctx, p, wp, conv), lib.wmi_full_long_wav(ctx, p, wp, conv, None), lib.wmi_full_batch_wav(ctx, p, wp, 1, conv),
                lib.wmi_full_wav_channels(ctx, p, wp, conv), lib.wmi_wav_speaker(ctx, wp, t, t, 1, 1.1, spk))
    try:
        assert lib.wmi_set_wav_adpcm(None, 1) == -2
        ad_s, ad_m, qoa = _wav(data, ar.ADPCM, 1, 48000), _wav(data, ar.ADPCM, 0, 48000), _wav(data, 3, 1, 48000)
        # mode 0, the default: -11 everywhere, as without the interface
        for w in (ad_s, ad_m, qoa):
            assert codes(w) == (-11, -11, -111, -111, -111, -111, -11)
        assert lib.wmi_selftest_wav_plan(C.byref(ad_s), 2, None, None) == -11
        assert lib.wmi_selftest_adpcm_plan(C.byref(ad_s), 2, None, None) == 0 and lib.wmi_selftest_adpcm_plan(C.byref(qoa), 2, None, None) == -11
        # mode 1: the format is planned; this context cannot compute, so every call stops at -2 — behind the argument checks, before a device
        assert lib.wmi_set_wav_adpcm(ctx, 1) == 0 and lib.wmi_set_wav_adpcm(ctx, 7) == 1 and lib.wmi_set_wav_adpcm(ctx, 1) == 1
        assert codes(ad_s) == (-2, -2, -102, -102, -102, -102, -2)
        assert codes(ad_m) == (-2, -12, -102, -102, -102, -112, -12)                # a mono clip: -12, decided as for the PCM formats
        assert codes(qoa) == (-11, -11, -111, -111, -111, -111, -11)                # QOA stays refused
        assert lib.wmi_selftest_wav_plan(C.byref(ad_s), 2, None, None) == -11       # no context, no mode
        # the argument errors of a format-2 clip
        for kw, e in ((dict(stereo=2), -1), (dict(stereo=-1), -1), (dict(rate=0), -1), (dict(n_bytes=-2), -1), (dict(conv=0), -10), (dict(conv=5), -1),
                      (dict(n_bytes=2 ** 30, stereo=0), -1),                         # 2 * n_bytes = 2^31 frames: one more than an int holds
                      (dict(n_bytes=2 ** 31 + 2, stereo=1), -1)):
            kw = dict(kw)
            conv = kw.pop("conv", 2)
            a = dict(stereo=1, rate=48000, n_bytes=None)
            a.update(kw)
            w = _wav(data, ar.ADPCM, a["stereo"], a["rate"], 0, a["n_bytes"])
            got = codes(w, conv)
            assert got[0] == e and got[2:5] == (-100 + e,) * 3 and lib.wmi_selftest_adpcm_plan(C.byref(w), conv, None, None) == e, (kw, got)
        w = _wav(data, ar.ADPCM, 0, 48000, 0, 2 ** 30 - 1)                           # 2^31 - 2 frames: planned
        frames = C.c_longlong(0)
        assert lib.wmi_selftest_adpcm_plan(C.byref(w), 2, C.byref(frames), None) == 0 and frames.value == 2 ** 31 - 2
        w = _wav(data, ar.ADPCM, 1, 48000); w.data = None
        assert codes(w)[0] == -1
        # a device source at an odd address is planned (nothing is read); an s16 one is refused as before
        w = abi.wmi_wav(C.c_void_p(0x7f0000001001), 9600, ar.ADPCM, 1, 48000, 1)
        assert lib.wmi_selftest_adpcm_plan(C.byref(w), 2, None, None) == 0 and lib.wmi_wav_to_pcm(ctx, C.byref(w), 2, dp, 4800, 0) == -2
        w = abi.wmi_wav(C.c_void_p(0x7f0000001001), 9600, wr.S16, 1, 48000, 1)
        assert lib.wmi_selftest_adpcm_plan(C.byref(w), 2, None, None) == -1
        # capacity: 4800 stereo bytes are 4800 frames, 1600 samples at 48 kHz
        assert lib.wmi_wav_to_pcm(ctx, C.byref(ad_s), 2, dp, 1599, 0) == -4
        assert np.all(np.isnan(dst))
        st = (C.c_int64 * 5)(7, 7, 7, 7, 7)
        assert lib.wmi_wav_stats(ctx, st) == 0 and list(st) == [0, 0, 0, 0, 0]       # no work set was ever made
        assert lib.wmi_set_wav_adpcm(ctx, 0) == 1
        assert codes(ad_s) == (-11, -11, -111, -111, -111, -111, -11)
    finally:
        lib.whisper_free(ctx)

"""The judge of the IMA-ADPCM decode (include/wmi_device.h wmi_set_wav_adpcm): the definition in plain Python integers.

    tables   STEP[89] = 7 .. 32767, INDEX[16] = {-1, -1, -1, -1, 2, 4, 6, 8} twice
    state    per channel (predictor, step_index) = (0, 0) in front of the clip; no block headers
    nibble   step = STEP[index]; index = clamp(index + INDEX[n], 0, 88); diff = step >> 3 (+ step >> 2, + step >> 1, + step by bits 0, 1, 2),
             negated by bit 3; predictor = clamp(predictor + diff, -32768, 32767)
    layout   the low nibble of a byte first; mono byte k = frames 2k, 2k + 1; stereo byte 2k + c = frames 2k, 2k + 1 of channel c; a trailing
             odd byte of a stereo clip is ignored; the decoded clip is interleaved s16

Also here: an encoder (for making clips that sound like something; its quality does not matter), the contents the tests share, and the
chunked-scan plan of csrc/k_adpcm.hip restated with the map algebra in Python (maps as tuples (a, lo, hi))."""
import numpy as np

ADPCM = 2                                                                   # AudioStreamWAV.FORMAT_IMA_ADPCM

STEP = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,
        173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878,
        2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289,
        16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767]
INDEX = [-1, -1, -1, -1, 2, 4, 6, 8] * 2
assert len(STEP) == 89


def clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def diff_of(step, n):
    d = step >> 3
    if n & 1:
        d += step >> 2
    if n & 2:
        d += step >> 1
    if n & 4:
        d += step
    return -d if n & 8 else d


def decode_nibbles(nibbles, state=(0, 0), keep_states=True):
    """The sequential decoder over one channel's nibbles: (samples, states) — states[i] = (predictor, index) in front of nibble i, and
    states[len] the state behind the last (keep_states=False: the last one only)."""
    pred, idx = state
    out, states = [], [(pred, idx)]
    for n in nibbles:
        step = STEP[idx]
        idx = clamp(idx + INDEX[n], 0, 88)
        pred = clamp(pred + diff_of(step, n), -32768, 32767)
        out.append(pred)
        if keep_states:
            states.append((pred, idx))
    return out, states if keep_states else [(pred, idx)]


def frames_of(n_bytes, stereo):
    return 2 * (n_bytes // 2) if stereo else 2 * n_bytes


def channel_nibbles(data, stereo, c):
    """Channel c's nibbles in stream order."""
    data = bytes(data)
    if stereo:
        data = data[:len(data) & ~1][c::2]
    out = []
    for b in data:
        out.append(b & 15)
        out.append(b >> 4)
    return out


def decode(data, stereo):
    """The clip as interleaved int16 (L R L R .. in stereo)."""
    nch = 2 if stereo else 1
    n = frames_of(len(data), stereo)
    out = np.zeros(n * nch, np.int16)
    for c in range(nch):
        s, _ = decode_nibbles(channel_nibbles(data, stereo, c), keep_states=False)
        assert len(s) == n
        out[c::nch] = np.array(s, np.int64).astype(np.int16)
    return out


def pack(nibble_lists):
    """One list of nibbles (mono) or two of equal length (stereo), each of even length, as AudioStreamWAV bytes."""
    nch = len(nibble_lists)
    n = len(nibble_lists[0])
    assert nch in (1, 2) and n % 2 == 0 and all(len(l) == n for l in nibble_lists)
    out = bytearray(n // 2 * nch)
    for c, l in enumerate(nibble_lists):
        for k in range(n // 2):
            out[k * nch + c] = l[2 * k] | (l[2 * k + 1] << 4)
    return bytes(out)


def encode(samples):
    """int16-range samples of one channel -> nibbles, by the usual successive approximation against the decoder's own state."""
    pred, idx = 0, 0
    out = []
    for x in np.asarray(samples).astype(np.int64).tolist():
        step = STEP[idx]
        d = x - pred
        n = 0
        if d < 0:
            n, d = 8, -d
        if d >= step:
            n |= 4; d -= step
        if d >= step >> 1:
            n |= 2; d -= step >> 1
        if d >= step >> 2:
            n |= 1
        idx = clamp(idx + INDEX[n], 0, 88)
        pred = clamp(pred + diff_of(step, n), -32768, 32767)
        out.append(n)
    return out


def encode_clip(pcm, stereo):
    """f32 samples in [-1, 1] (stereo: interleaved) -> AudioStreamWAV ADPCM bytes; an odd frame is dropped."""
    v = np.clip(np.rint(np.asarray(pcm, np.float64) * 32767.0), -32768, 32767).astype(np.int64)
    nch = 2 if stereo else 1
    n = v.size // nch // 2 * 2
    return pack([encode(v[c:n * nch:nch]) for c in range(nch)])


# ------------------------------------------------------------------------------------------------ contents the tests share

def content(kind, n, seed=0):
    """n nibbles of one channel."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 16, n).tolist()
    if kind == "sevens":                                                    # index to 88, predictor to 32767
        return [7] * n
    if kind == "fifteens":                                                  # index to 88, predictor to -32768
        return [15] * n
    if kind == "zeros":                                                     # index pinned at 0
        return [0] * n
    if kind == "runs":                                                      # 7s and 15s in runs of 37: the runs' edges walk across every chunk edge
        return [7 if (i // 37) % 2 == 0 else 15 for i in range(n)]
    if kind == "small":                                                     # mostly low codes: the index stays in the low steps, no clamp for long
        return (np.random.default_rng(seed).integers(0, 4, n) + 8 * np.random.default_rng(seed + 1).integers(0, 2, n)).tolist()
    raise KeyError(kind)


CONTENTS = ("random", "sevens", "fifteens", "zeros", "runs", "small")


def saturation_nibbles():
    """70 000 nibbles of 7, then 70 000 of 15: the predictor map's additive term passes 2^31 upwards and then 2^31 back down — a 32-bit sum
    wraps twice."""
    return [7] * 70000 + [15] * 70000


# ------------------------------------------------------------------------------------------------ the map algebra and the chunked plan

IDX_ID, PRED_ID = (0, 0, 88), (0, -32768, 32767)


def compose(f, g):
    """The map 'f, then g' of maps x -> min(max(x + a, lo), hi)."""
    return (f[0] + g[0], clamp(f[1] + g[0], g[1], g[2]), clamp(f[2] + g[0], g[1], g[2]))


def apply_map(m, x):
    return clamp(x + m[0], m[1], m[2])


def plan_entry_states(nibbles, chunk):
    """The plan of k_adpcm.hip on one channel: [(predictor, index)] in front of every chunk and, last, behind the stream."""
    chunks = [nibbles[i:i + chunk] for i in range(0, len(nibbles), chunk)]
    imaps = []
    for ch in chunks:
        m = IDX_ID
        for n in ch:
            m = compose(m, (INDEX[n], 0, 88))
        imaps.append(m)
    entry_idx, pre = [], IDX_ID
    for m in imaps + [None]:
        entry_idx.append(apply_map(pre, 0))
        if m is not None:
            pre = compose(pre, m)
    entry_pred, pre = [], PRED_ID
    for j in range(len(chunks) + 1):
        entry_pred.append(apply_map(pre, 0))
        if j == len(chunks):
            break
        idx, m = entry_idx[j], PRED_ID
        for n in chunks[j]:
            m = compose(m, (diff_of(STEP[idx], n), -32768, 32767))
            idx = clamp(idx + INDEX[n], 0, 88)
        pre = compose(pre, m)
    return list(zip(entry_pred, entry_idx))


def hold(got, want):
    """Strict equality of two int16 clips."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.int16 and want.dtype == np.int16, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"first difference at sample {i} of {want.size}: got {got[i]}, want {want[i]}")

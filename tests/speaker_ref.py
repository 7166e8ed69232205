"""The judge of the speaker labels (include/wmi_device.h wmi_speaker): whisper.cpp's --diarize restated in NumPy and Python integers,
from examples/main/main.cpp:41-43 (timestamp_to_sample) and :237-268 (estimate_diarization_speaker), at any rate.

    is(t)   = max(0, min(n - 1, (t * rate) // 100))           t >= 0 in centiseconds; Python integers, so nothing overflows
    E_c     = sum_{j = is(t0)}^{is(t1) - 1} |x_c[j]|          a literal sequential loop in a double over the channel's f32 samples
    label   = 0 if E_0 > ratio * E_1 else 1 if E_1 > ratio * E_0 else -1

The clamp keeps is(t) <= n - 1 and the end is exclusive: no range counts frame n - 1.  The table the device writes says the same: bin b
holds the channel sums over frames [B(b), min(B(b + 1), n - 1)), B(b) = (b * rate) // 100, for b < nb = the smallest b with B(b) >= n,
and the magnitudes of frame n - 1 stand apart (last2).  `variant` restates the definition with one mistake each, for the tests that show
the judge refuses it."""

import numpy as np

S8, S16, F32 = 0, 1, 32
SAMPLE_BYTES = {S8: 1, S16: 2, F32: 4}
SCALE = {S8: 128, S16: 32768}
RATIO = 1.1


def frames_of(n_bytes, fmt):
    return n_bytes // SAMPLE_BYTES[fmt] // 2


def ints(data, fmt):
    """the whole frames of an integer clip as Python-int-safe int64 [n][2] (signed samples)"""
    data = bytes(data)
    n = frames_of(len(data), fmt)
    dt = "<i2" if fmt == S16 else "i1"
    return np.frombuffer(data, dt, 2 * n).astype(np.int64).reshape(n, 2)


def channels(data, fmt):
    """the two channels as the f32 samples the reference holds (pcmf32s): [n][2] float32; trailing incomplete samples and frames ignored"""
    data = bytes(data)
    n = frames_of(len(data), fmt)
    if fmt == F32:
        return np.frombuffer(data, "<f4", 2 * n).reshape(n, 2).copy()
    return (ints(data, fmt).astype(np.float64) / float(SCALE[fmt])).astype(np.float32)       # exact in f32


def sample_of(t, n, rate):
    return max(0, min(n - 1, (int(t) * int(rate)) // 100)) if t >= 0 else 0


def seq_abs_sum(x):
    """main.cpp:247-250: energy += fabs(x[j]) in a double, left to right"""
    e = 0.0
    for v in np.abs(np.asarray(x, np.float32)).astype(np.float64).tolist():
        e += v
    return e


def label(e0, e1, ratio=RATIO):
    return 0 if e0 > ratio * e1 else 1 if e1 > ratio * e0 else -1


def speaker(x, rate, t0, t1, ratio=RATIO):
    """x: [n][2] float32 -> dict(speaker, is0, is1, e0, e1)"""
    n = int(x.shape[0])
    if n == 0:
        return dict(speaker=-1, is0=0, is1=0, e0=0.0, e1=0.0)
    is0, is1 = sample_of(t0, n, rate), sample_of(t1, n, rate)
    e0 = seq_abs_sum(x[is0:is1, 0]) if is1 > is0 else 0.0
    e1 = seq_abs_sum(x[is0:is1, 1]) if is1 > is0 else 0.0
    return dict(speaker=label(e0, e1, ratio), is0=is0, is1=is1, e0=e0, e1=e1)


def speaker_of_clip(data, fmt, rate, t0, t1, ratio=RATIO):
    return speaker(channels(data, fmt), rate, t0, t1, ratio)


# ---- the table

def n_bins(n, rate):
    """the smallest b with (b * rate) // 100 >= n"""
    return 0 if n <= 0 else -((-100 * n) // rate)


def bin_edges(n, rate):
    nb = n_bins(n, rate)
    return [min((b * rate) // 100, n - 1) for b in range(nb + 1)] if nb else [0]


def table(data, fmt, rate):
    """-> (bins [nb][2], last2 [2]): uint64 sums of |v| from Python integers for the integer formats; float64 for f32, every bin by the
    sequential double loop"""
    n = frames_of(len(bytes(data)), fmt)
    nb = n_bins(n, rate)
    edges = bin_edges(n, rate)
    if fmt == F32:
        x = channels(data, fmt)
        bins = np.zeros((nb, 2), np.float64)
        for b in range(nb):
            for c in range(2):
                bins[b, c] = seq_abs_sum(x[edges[b]:edges[b + 1], c])
        last = np.abs(x[n - 1]).astype(np.float64) if n else np.zeros(2, np.float64)
        return bins, last
    v = ints(data, fmt)
    bins = np.zeros((nb, 2), np.uint64)
    for b in range(nb):
        for c in range(2):
            bins[b, c] = sum(abs(int(s)) for s in v[edges[b]:edges[b + 1], c].tolist())
    last = np.array([abs(int(s)) for s in v[n - 1].tolist()] if n else [0, 0], np.uint64)
    return bins, last


def speaker_from_table(bins, fmt, n, rate, t0, t1, ratio=RATIO):
    """the header's order: bins [t0, min(t1, nb)) added left to right (integers for the integer formats, then ONE division)"""
    nb = n_bins(n, rate)
    if n == 0:
        return dict(speaker=-1, is0=0, is1=0, e0=0.0, e1=0.0)
    t0, t1 = max(int(t0), 0), max(int(t1), 0)
    is0, is1 = sample_of(t0, n, rate), sample_of(t1, n, rate)
    lo, hi = t0, min(t1, nb)
    e = [0.0, 0.0]
    if is1 > is0:
        for c in range(2):
            if fmt == F32:
                acc = 0.0
                for v in bins[lo:hi, c].tolist():
                    acc += v
                e[c] = acc
            else:
                e[c] = float(sum(int(v) for v in bins[lo:hi, c].tolist())) / float(SCALE[fmt])
    return dict(speaker=label(e[0], e[1], ratio), is0=is0, is1=is1, e0=e[0], e1=e[1])


def f32_bound(m, e):
    """|E_device - E_judge| <= 2 m 2^-53 E_judge: m non-negative terms added in two different orders"""
    return 2.0 * m * 2.0 ** -53 * e


def f32_label_safe(r, ratio=RATIO):
    """the judge's inequality holds with the bound's margin on both sides: the label may be compared"""
    m = r["is1"] - r["is0"]
    if m <= 0:
        return True
    d0, d1 = f32_bound(m, r["e0"]), f32_bound(m, r["e1"])

    def clear(a, da, b, db):                                   # a > ratio * b, or not, whichever way the errors fall
        return (a - da > ratio * (b + db) * (1 + 2.0 ** -52)) or (a + da < ratio * (b - db) * (1 - 2.0 ** -52)) or (a + da <= 0 and b == 0)
    return clear(r["e0"], d0, r["e1"], d1) and clear(r["e1"], d1, r["e0"], d0)


# ---- wrong answers the judge must refuse

VARIANTS = ["swapped", "squares", "inclusive_end", "no_clamp", "clamp_is1_only", "ratio_wrong_side", "ge", "s8_unsigned", "abs_narrow",
            "f32_accumulators", "folded_mono", "rate_16000"]


def variant(name, data, fmt, rate, t0, t1, ratio=RATIO):
    """the definition with one mistake; same result form as speaker_of_clip"""
    x = channels(data, fmt)
    n = int(x.shape[0])
    if n == 0:
        return dict(speaker=-1, is0=0, is1=0, e0=0.0, e1=0.0)
    if name == "s8_unsigned":
        x = (np.frombuffer(bytes(data), "u1", 2 * n).astype(np.float64) / 128.0).astype(np.float32).reshape(n, 2)
    use_rate = 16000 if name == "rate_16000" else rate
    raw = lambda t: max(0, (int(t) * int(use_rate)) // 100)
    if name == "no_clamp":
        is0, is1 = min(raw(t0), n), min(raw(t1), n)            # (slicing stops at n)
    elif name == "clamp_is1_only":
        is0, is1 = min(raw(t0), n), min(raw(t1), n - 1)
    else:
        is0, is1 = sample_of(t0, n, use_rate), sample_of(t1, n, use_rate)
    if name == "inclusive_end":
        is1 = min(is1 + 1, n)
    seg = x[is0:is1] if is1 > is0 else x[:0]
    if name == "squares":
        e = [float(np.sum(seg[:, c].astype(np.float64) ** 2)) for c in range(2)]
    elif name == "abs_narrow":                                  # abs in the sample's own width: the most negative value stays negative
        v = ints(data, fmt)[is0:is1] if is1 > is0 else ints(data, fmt)[:0]
        lo = -SCALE[fmt]
        a = np.where(v == lo, lo, np.abs(v)).astype(np.float64) / float(SCALE[fmt])
        e = [float(np.sum(a[:, c])) for c in range(2)]
    elif name == "f32_accumulators":
        e = []
        for c in range(2):
            acc = np.float32(0.0)
            for v in np.abs(seg[:, c]):
                acc = np.float32(acc + v)
            e.append(float(acc))
    elif name == "folded_mono":
        m = ((seg[:, 0] + seg[:, 1]).astype(np.float64) / 2.0).astype(np.float32)
        e = [seq_abs_sum(m), seq_abs_sum(m)]
    else:
        e = [seq_abs_sum(seg[:, 0]), seq_abs_sum(seg[:, 1])]
    if name == "swapped":
        e = e[::-1]
    if name == "ratio_wrong_side":
        lab = 0 if ratio * e[0] > e[1] else 1 if ratio * e[1] > e[0] else -1
    elif name == "ge":
        lab = 0 if e[0] >= ratio * e[1] else 1 if e[1] >= ratio * e[0] else -1
    else:
        lab = label(e[0], e[1], ratio)
    return dict(speaker=lab, is0=is0, is1=is1, e0=e[0], e1=e[1])


# ---- clips

def pack(x, fmt):
    """interleaved values -> bytes: integers as they are for the integer formats, float32 for f32"""
    if fmt == F32:
        return np.asarray(x, "<f4").tobytes()
    return np.asarray(x, "<i2" if fmt == S16 else "i1").tobytes()


def crafted(fmt, n, seed):
    """n stereo frames with asymmetric channels and the format's edge values near the front and the back"""
    rng = np.random.default_rng(seed)
    if fmt == F32:
        x = rng.standard_normal((n, 2)).astype(np.float32) * np.array([0.3, 0.05], np.float32)
        edge = [(-0.0, 1e-40), (1e30, 1e-30), (-1e30, -1e-30), (1e-38, -1e-45), (0.0, -0.0)]
    else:
        hi = SCALE[fmt]
        x = np.stack([rng.integers(-hi, hi, n), rng.integers(-hi // 8, hi // 8, n)], axis=1)
        edge = [(-hi, hi - 1), (hi - 1, -hi), (-hi, -hi), (0, -1), (-1, 0)]
    if fmt == F32 and n > 40:
        x[n // 2] = (2.0 ** 60, 2.0 ** 40)                      # beside terms near 1: an order of addition that loses them shows, within the bound
    for i, ev in enumerate(edge):
        if i < n:
            x[i] = ev
        if n - 1 - i > len(edge):
            x[n - 1 - i] = ev if fmt == F32 else ev[::-1]        # (f32: the loud channel stays the loud one, so no label is a near tie)
    return pack(x.reshape(-1), fmt)

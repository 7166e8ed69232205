"""The judge of the long-recording front (include/wmi_device.h wmi_full_long): NumPy restatements of the frame energies and of the plan,
the input families the kernel is held to, and the crafted energy arrays that hit every rule of the plan.

Energies.  For 16 kHz f32 PCM x[0 .. n) and every 10 ms frame f < F = ceil(n / 160):
    e[f] = sum over i in [160 f, min(160 f + 160, n)) of | x[i] - x[i-1] |,   x[-1] := 0
subtraction and |.| in f32, the sum the left-to-right f32 sum from 0.0f (np.cumsum(dtype=float32) accumulates sequentially, as in
host.vad_simple; np.add.reduce would pair).  Equality with the kernel is bit for bit: there is no tolerance to derive.

Plan.  Written from the rules of DESIGN.md section 5 ("Long recordings"), not from csrc/segment.cpp; all quantities in frames.
 1  E = (sum of e[f] in double, ascending f) / n.  quiet[f] = e[f] < thold E len_f  or  e[f] < floor len_f, evaluated in double,
    len_f the frame's sample count.
 2  A gap is a maximal run of quiet frames of at least G = min_silence_ms / 10 frames; islands are the maximal runs of frames in no gap.
 3  Island [a, b) is widened to [max(a - P, m_prev), min(b + P, m_next)), P = pad_ms / 10, m = floor((gap_start + gap_end) / 2) of the gap
    to the neighbouring ISLAND; an island without a neighbour on a side is bounded by 0 / F there (also when the signal begins or ends
    with a gap: no other island claims it).
 4  Left to right: a piece starts at the widened start of the first unassigned island and absorbs the next island while the gap in front
    of that island (its unwidened length) is shorter than max_gap_ms / 10 frames and (that island's widened end) - (piece start) <= Lmax =
    max_piece_ms / 10.
 5  A first unassigned island longer than Lmax is cut at c = the frame of smallest e in [start + Lmax - Lmax / 3, start + Lmax], earliest
    on ties; [start, c) is a piece, the rest a new island at c without padding there.
 6  After all pieces stand, in order: a piece below 100 frames moves its end to min(start + 100, next piece's start or F); if still below,
    its start to max(end - 100, previous piece's end or 0); a piece still below is kept.
 7  audio_ctx = min(n_audio_ctx, (frames + 1) / 2 + 128) with fit_audio_ctx, else 0 (the call then takes params.audio_ctx).
    offset_ms / duration_ms: the plan sees the frames [min(offset_ms / 10, F), min(that + duration_ms / 10, F)) (duration 0: to F) as a
    signal of their own (e restricted, n = the samples they hold); frame numbers are shifted back afterwards.
`wrong` selects one of the mistakes the tests make sure this judge refuses."""
import ctypes as C

import numpy as np

from godot_whisper_amd import abi

FRAME = 160
WRONG_PLANS = ("gap_start", "tie_latest", "pad_after_packing", "mean_over_F")


# ------------------------------------------------------------------------------------------------ energies
def terms(x, edge_zero=False):
    """| x[i] - x[i-1] | in f32; edge_zero: the mistake of reading x[160 f - 1] as 0 at every frame edge"""
    x = np.ascontiguousarray(x, np.float32)
    prev = np.concatenate([np.zeros(1, np.float32), x[:-1]])
    if edge_zero:
        prev[::FRAME] = 0.0
    return np.abs(x - prev)


def energies(x, edge_zero=False):
    t = terms(x, edge_zero)
    n = t.size
    F = (n + FRAME - 1) // FRAME
    e = np.empty(F, np.float32)
    full = n // FRAME
    if full:
        e[:full] = np.cumsum(t[:full * FRAME].reshape(full, FRAME), axis=1, dtype=np.float32)[:, -1]
    if F > full:
        e[full] = np.cumsum(t[full * FRAME:], dtype=np.float32)[-1]
    return e


def energies_tree(x, butterfly=False):
    """what a tree (adjacent pairs) or a butterfly (lane i with lane i + half) reduction of a frame's terms would give"""
    t = terms(x)
    F = (t.size + FRAME - 1) // FRAME
    a = np.zeros((F, 256), np.float32)
    for f in range(F):
        seg = t[f * FRAME:(f + 1) * FRAME]
        a[f, :seg.size] = seg
    while a.shape[1] > 1:
        h = a.shape[1] // 2
        a = (a[:, :h] + a[:, h:]) if butterfly else (a[:, 0::2] + a[:, 1::2])
    return a[:, 0].copy()


def sizes(stage):
    return [1, 2, 159, 160, 161, 319, 320, 321, stage - 1, stage, stage + 1, 3 * stage + 7, 480007]


def make_input(family, n, seed):
    rng = np.random.default_rng(seed)
    if family == "noise":
        return (0.1 * rng.standard_normal(n)).astype(np.float32)
    if family == "special":          # denormals, signed zeros, unit steps
        vals = np.array([1e-42, -1e-42, 3e-39, -0.0, 0.0, 1.0, -1.0, 1e-38], np.float32)
        x = vals[rng.integers(0, vals.size, n)]
        x[FRAME - 1::FRAME] = 1.0            # a unit step at every frame edge (a kernel that takes the sample in front of a frame for 0 shows)
        return x
    if family == "seqsum":
        # every frame ends on 4096 and the next begins near 0: its first term is ~4096 (ulp 2^-11 = 4.9e-4), the ~1e-4 terms behind it are
        # each below half an ulp and vanish one by one in the sequential sum, while a pairwise sum adds them up first.  The same jump makes
        # a kernel that takes x[160 f - 1] for 0 lose the whole first term.  (From 159 samples on; below that there is too little to sum.)
        x = (1e-4 * rng.standard_normal(n)).astype(np.float32)
        x[FRAME - 1::FRAME] = 4096.0
        x[0] = 4096.0                        # the first frame too: two terms of 4096 (the step up and back), then the small ones
        return x
    raise KeyError(family)


FAMILIES = ("noise", "special", "seqsum")


# ------------------------------------------------------------------------------------------------ plan
def params(**kw):
    p = abi.wmi_long_params(0.25, 1e-4, 300, 100, 2000, 30000, 0)
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def window(n, offset_ms, duration_ms):
    F = (n + FRAME - 1) // FRAME
    f0 = min(offset_ms // 10, F)
    f1 = F if duration_ms == 0 else min(f0 + duration_ms // 10, F)
    f1 = max(f0, f1)
    return f0, f1, (min(FRAME * f1, n) - FRAME * f0 if f1 > f0 else 0)


def plan(e, n, lp, n_audio_ctx, wrong=None, offset_ms=0, duration_ms=0):
    """-> [(frame0, frame1, audio_ctx)]"""
    if offset_ms or duration_ms:
        f0, f1, n_sub = window(n, offset_ms, duration_ms)
        if f1 <= f0:
            return []
        return [(a + f0, b + f0, c) for a, b, c in plan(e[f0:f1], n_sub, lp, n_audio_ctx, wrong)]
    e = np.asarray(e, np.float32)
    F = e.size
    assert F == (n + FRAME - 1) // FRAME
    G, P, Gmax, Lmax = lp.min_silence_ms // 10, lp.pad_ms // 10, lp.max_gap_ms // 10, lp.max_piece_ms // 10
    thold, floor = float(lp.thold), float(lp.floor)          # the f32 values, widened
    # rule 1
    total = 0.0
    for v in e:
        total += float(v)
    E = total / (F if wrong == "mean_over_F" else n)
    quiet = []
    for f in range(F):
        ln = float(min(FRAME, n - FRAME * f))
        quiet.append(float(e[f]) < thold * E * ln or float(e[f]) < floor * ln)
    # rule 2
    gaps, f = [], 0
    while f < F:
        if not quiet[f]:
            f += 1
            continue
        r = f
        while r < F and quiet[r]:
            r += 1
        if r - f >= G:
            gaps.append((f, r))
        f = r
    islands, pos = [], 0          # (a, b, the gap in front or None)
    last_gap = None
    for g in gaps:
        if g[0] > pos:
            islands.append((pos, g[0], last_gap))
        pos, last_gap = g[1], g
    if pos < F:
        islands.append((pos, F, last_gap))
    if not islands:
        return []

    def bound(g):
        return g[0] if wrong == "gap_start" else (g[0] + g[1]) // 2

    # rule 3
    wide = []
    for i, (a, b, g) in enumerate(islands):
        lo = 0 if i == 0 else bound(g)
        hi = F if i == len(islands) - 1 else bound(islands[i + 1][2])
        if wrong == "pad_after_packing":
            wide.append([a, b, 0 if i == 0 else g[1] - g[0], lo, hi])
        else:
            wide.append([max(a - P, lo), min(b + P, hi), 0 if i == 0 else g[1] - g[0], lo, hi])
    # rules 4 and 5
    pieces, i = [], 0
    while i < len(wide):
        s, b = wide[i][0], wide[i][1]
        if b - s > Lmax:
            lo_c, hi_c = s + Lmax - Lmax // 3, s + Lmax
            rng = e[lo_c:hi_c + 1]
            k = int(np.flatnonzero(rng == rng.min())[-1 if wrong == "tie_latest" else 0])
            c = lo_c + k
            pieces.append([s, c, wide[i][3], c])
            wide[i] = [c, b, 0, c, wide[i][4]]
            continue
        end, lo, hi = b, wide[i][3], wide[i][4]
        i += 1
        while i < len(wide) and wide[i][2] < Gmax and wide[i][1] - s <= Lmax:
            end, hi = wide[i][1], wide[i][4]
            i += 1
        pieces.append([s, end, lo, hi])
    if wrong == "pad_after_packing":
        pieces = [[max(s - P, lo), min(b + P, hi), lo, hi] for s, b, lo, hi in pieces]
    # rule 6
    for i, pc in enumerate(pieces):
        if pc[1] - pc[0] >= 100:
            continue
        pc[1] = min(pc[0] + 100, pieces[i + 1][0] if i + 1 < len(pieces) else F)
        if pc[1] - pc[0] >= 100:
            continue
        pc[0] = max(pc[1] - 100, pieces[i - 1][1] if i > 0 else 0)
    # rule 7
    return [(s, b, min(n_audio_ctx, (b - s + 1) // 2 + 128) if lp.fit_audio_ctx else 0) for s, b, _, _ in pieces]


def lib_window(lib, n, offset_ms, duration_ms):
    f0, f1, ns = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.wmi_selftest_long_window(n, offset_ms, duration_ms, C.byref(f0), C.byref(f1), C.byref(ns)) == 0
    return f0.value, f1.value, ns.value


def lib_plan(lib, e, n, lp, n_audio_ctx, offset_ms=0, duration_ms=0, cap=256):
    """the library's plan through its hooks, as wmi_full_long composes them -> [(frame0, frame1, audio_ctx)]"""
    e = np.ascontiguousarray(e, np.float32)
    f0, f1, ns = lib_window(lib, n, offset_ms, duration_ms) if (offset_ms or duration_ms) else (0, e.size, n)
    if f1 <= f0:
        return []
    sub = np.ascontiguousarray(e[f0:f1])
    out = (abi.wmi_long_piece * cap)()
    got = lib.wmi_selftest_long_plan(sub.ctypes.data, sub.size, ns, C.byref(lp) if lp is not None else None, n_audio_ctx, out, cap)
    assert 0 <= got <= cap, got
    for i in range(got):
        assert (out[i].mode, out[i].i_segment, out[i].n_segments) == (0, 0, 0)
    return [(out[i].frame0 + f0, out[i].frame1 + f0, out[i].audio_ctx) for i in range(got)]


def hold_plan(got, case, wrong=None):
    """`got` must be the restatement's plan of `case`, piece for piece"""
    want = plan(case["e"], case["n"], case["lp"], case["n_audio_ctx"], None, case.get("offset_ms", 0), case.get("duration_ms", 0))
    assert [tuple(p) for p in got] == want, (case["name"], wrong, got, want)
    return want


# energy arrays: "speech" frames carry 16.0 (0.1 per sample), quiet frames 0; runs = [(frames, level)]
def _e(runs, tail=FRAME):
    e = np.concatenate([np.full(k, v, np.float32) for k, v in runs])
    n = FRAME * (e.size - 1) + tail
    return e, n


def cases():
    S, Q = 16.0, 0.0
    out = []

    def add(name, runs, lp=None, n_audio_ctx=1500, tail=FRAME, edit=None, **kw):
        e, n = _e(runs, tail)
        if edit:
            edit(e)
        out.append(dict(name=name, e=e, n=n, lp=lp if lp is not None else params(), n_audio_ctx=n_audio_ctx, **kw))

    add("no island", [(400, Q)])
    add("one island fills the signal", [(500, S)])
    add("gap of G and of G - 1", [(200, S), (30, Q), (200, S), (29, Q), (200, S)])
    add("pad clipped at a midpoint and at both ends", [(35, Q), (150, S), (40, Q), (150, S), (32, Q)], params(pad_ms=500, max_gap_ms=300))
    add("pad clipped at the ends, no gap there", [(5, Q), (150, S), (40, Q), (150, S), (3, Q)], params(pad_ms=300))
    add("absorption stopped by max_gap", [(150, S), (150, Q), (150, S), (200, Q), (150, S), (199, Q), (150, S)])
    add("absorption stopped by Lmax", [(100, Q), (200, S), (50, Q), (245, S), (50, Q), (100, S), (100, Q)], params(max_piece_ms=5000))
    add("absorption just fits Lmax", [(100, Q), (200, S), (50, Q), (230, S), (100, Q)], params(max_piece_ms=5000))

    def unique(e):
        e[50 + 400] = 8.0; e[50 + 470] = 9.0                                   # first cut at the unique minimum
        e[50 + 400 + 350] = 9.0; e[50 + 400 + 420] = 7.5                       # second cut: the later frame is the lower one
    add("island of 2.5 Lmax, unique minima", [(50, Q), (1250, S), (60, Q)], params(max_piece_ms=5000), edit=unique)

    def tie(e):
        e[50 + 380] = 8.0; e[50 + 455] = 8.0; e[50 + 490] = 8.0                # a three-way tie: the earliest
    add("island of 2.5 Lmax, ties", [(50, Q), (1250, S), (60, Q)], params(max_piece_ms=5000), edit=tie)
    add("island of 2.5 Lmax, flat", [(1250, S)], params(max_piece_ms=5000))
    add("40-frame island between long gaps", [(300, S), (250, Q), (40, S), (250, Q), (300, S)])
    add("40-frame island squeezed on both sides", [(300, S), (30, Q), (40, S), (30, Q), (300, S)], params(max_gap_ms=300))
    add("40-frame island at the end", [(300, S), (250, Q), (40, S), (35, Q)])
    add("shorter than 1 s", [(60, S)], tail=77)
    add("fit_audio_ctx against a small n_audio_ctx", [(300, S), (250, Q), (100, S), (250, Q), (40, S), (250, Q)], params(fit_audio_ctx=1), n_audio_ctx=200)
    add("fit_audio_ctx", [(300, S), (250, Q), (101, S), (250, Q)], params(fit_audio_ctx=1))
    add("offset and duration", [(200, S), (100, Q), (200, S), (100, Q), (200, S), (100, Q), (200, S)], offset_ms=2530, duration_ms=6000)
    add("offset only, partial last frame", [(200, S), (100, Q), (200, S), (100, Q), (200, S)], tail=31, offset_ms=1000)
    add("offset behind the signal", [(200, S)], offset_ms=5000)
    add("low speech level beside a loud burst", [(200, 2.0), (100, Q), (200, 200.0)])          # 2.0 < 0.25 E 160: the soft run is quiet
    return out


# the case on which each wrong plan must part from the right one
WRONG_ON = {"gap_start": "pad clipped at a midpoint and at both ends", "tie_latest": "island of 2.5 Lmax, ties",
            "pad_after_packing": "absorption stopped by Lmax", "mean_over_F": "one island fills the signal"}

"""The encoder self-attention restated in NumPy, and the crafted operands its kernels are held to (tests/test_attn_f64.py proves the
conditions on the CPU, tests/test_gpu_attn_encoder.py runs the kernels on them through wmi_selftest_attn_encoder).

    attend_f64(q, k, v, T)          float64 soft-max of q.k / 8 over exactly T keys per 64-wide head, times v: the yardstick
    attend_ref_points(q, k, v, T)   the same with the reference's rounding points (W/whisper.cpp:1877-1950, the soft-max of W/ggml.c): what the
                                    reference computes, NOT what the kernels do — its distance from attend_f64 is the unit they are measured in
    vt_pos(t)                       where time step t sits in a row of the q|k|v projection's V^T image (written here independently)

A Case holds the operands of one launch in the hook's layouts: q, k [B][qk_rows][S], v [B][Tpad][S] (time-major), f16.  Whatever must never
be read as a query or a key is poisoned: rows [T_chunk, qk_rows) of q and k and time rows [T_chunk, Tpad) of v alternate +60000 / -60000 —
finite, because the product promises only finite junk there (0 x inf would be a NaN of the test's own making) — and large enough that ONE
such key in a sum is gross.  Three families:

    selector   k[j] = 4 code(j), q[i] = 4 code(pi(i)), code(j) in {+1, -1}^64 per head: the matching score leads every other by >= 40 after
               the 1/8 scale, every other numerator is 0 in f16 (or is scaled by e^-40 in the one-sweep form): out[i] == v[pi(i)], and a
               wrong row names the key that was read
    uniform    q = 0: every numerator is 1, the sum is T exactly, sum(v) is exact in f32: out = sum(v[:T]) / T; one key more or less
               moves it by about 1 / T
    random     standard normal operands at a score spread: compared with attend_f64 in units of attend_ref_points' own error

hold_case() is the ONE judge of a launch's result: the GPU test passes it what the kernels wrote, the CPU test what deliberately wrong
restatements (restate()) write, which it must refuse.  Nothing here reads the reference checkout."""
from __future__ import annotations

import dataclasses

import numpy as np

POISON = 60000.0
SENTINEL16 = 0x7E5A                  # an f16 NaN pattern no kernel produces
SENTINEL32 = 0x7FC5A5A5              # an f32 NaN pattern
SELECTOR_MARGIN = 40.0
# a kernel's distance from float64 on the random family, as a multiple of attend_ref_points' on the same operands: rms at most
# decoder_f64.SWEEP_LIMIT (the project's margin for this kind of comparison: the kernels make the same number of f16 roundings per element
# as the reference; what differs is the f32 summation order and rounding the unnormalised numerator instead of the normalised one), the
# largest |d| at most twice (a maximum over ~10^5 elements scatters more than an rms)
RMS_LIMIT = 1.5
MAX_LIMIT = 2.0


def vt_pos(t):
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def _heads(a, T):
    """[rows][S] -> [H][T][64] float64 of the first T rows"""
    a = np.asarray(a)[:T].astype(np.float64)
    return a.reshape(T, -1, 64).transpose(1, 0, 2)


def attend_f64(q, k, v, T):
    """[T][S] float64"""
    qh, kh, vh = _heads(q, T), _heads(k, T), _heads(v, T)
    s = qh @ kh.transpose(0, 2, 1) / 8.0
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return (p @ vh).transpose(1, 0, 2).reshape(T, -1)


def attend_ref_points(q, k, v, T, f16_result=False):
    """The reference's rounding points: f32 scores, scaled by 1/8; the argument s - max rounded to f16; exp rounded to f16 (its table);
    the sum in double; the probability scaled in f32 and rounded to f16 for the P.V product (an f16 x f16 mul_mat accumulated in f32);
    the result f32, or rounded to f16 as the kernels store it.  Returns float64 values."""
    f32 = np.float32
    qh, kh, vh = (_heads(a, T).astype(f32) for a in (q, k, v))
    s = (qh @ kh.transpose(0, 2, 1)) * f32(0.125)
    arg = (s - s.max(-1, keepdims=True)).astype(np.float16)
    e = np.exp(arg.astype(f32)).astype(np.float16)
    inv = (1.0 / e.astype(np.float64).sum(-1, keepdims=True)).astype(f32)
    p = (e.astype(f32) * inv).astype(np.float16)
    o = (p.astype(f32) @ vh).transpose(1, 0, 2).reshape(T, -1)
    if f16_result:
        o = o.astype(np.float16)
    return o.astype(np.float64)


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    family: str
    name: str
    B: int
    T: int                       # the launch's (largest) length
    Tpad: int
    S: int
    H: int
    qk_rows: int
    out_rows: int
    lens: list                   # length of every chunk
    ragged: bool                 # pass the lengths as row_T
    q: np.ndarray                # [B][qk_rows][S] f16
    k: np.ndarray
    v: np.ndarray                # [B][Tpad][S] f16
    pi: list                     # selector: per chunk the key of every query
    _memo: dict = dataclasses.field(default_factory=dict)

    def expected(self, b):
        """[T_b][S] float64: what chunk b's rows must hold"""
        if ("exp", b) not in self._memo:
            Tb = self.lens[b]
            if self.family == "selector":
                e = self.v[b][self.pi[b]].astype(np.float64)
            elif self.family == "uniform":
                e = np.broadcast_to(self.v[b][:Tb].astype(np.float64).sum(0) / Tb, (Tb, self.S)).copy()
            else:
                e = attend_f64(self.q[b], self.k[b], self.v[b], Tb)
            self._memo[("exp", b)] = e
        return self._memo[("exp", b)]

    def ref_error(self, b, want_f32):
        """(rms, max) of attend_ref_points' distance from float64 on chunk b's operands, with the result type of the launch"""
        key = ("ref", b, bool(want_f32))
        if key not in self._memo:
            d = attend_ref_points(self.q[b], self.k[b], self.v[b], self.lens[b], f16_result=not want_f32) - self.expected(b)
            self._memo[key] = (float(np.sqrt(np.mean(d * d))), float(np.abs(d).max()))
        return self._memo[key]

    def one_chunk(self, b):
        """chunk b's operands as a launch of its own at its own length (same row counts and Tpad: the same images)"""
        return Case(self.family, f"{self.name}[{b}]", 1, self.lens[b], self.Tpad, self.S, self.H, self.qk_rows, self.out_rows, [self.lens[b]],
                    False, self.q[b:b + 1], self.k[b:b + 1], self.v[b:b + 1], [self.pi[b]] if self.pi else [])


def _poison(rows, S):
    r, c = np.meshgrid(np.arange(rows), np.arange(S), indexing="ij")
    return np.where((r + c) & 1, -POISON, POISON).astype(np.float16)


def v_formula(b, T, S):
    j, c = np.meshgrid(np.arange(T), np.arange(S), indexing="ij")
    return (((7 * j + 3 * c + 11 * b) % 255 - 127) / 16.0).astype(np.float16)


def boundary_keys(T):
    """keys on both sides of every 32- and 64-key boundary and of every key-group boundary (four and two groups of whole 64-key tiles)"""
    ks = {0, T - 1}
    for e in range(32, T + 32, 32):
        ks |= {e - 1, e}
    nt = (T + 63) // 64
    for groups in (2, 4):
        per = (nt + groups - 1) // groups
        for g in range(1, groups):
            ks |= {g * per * 64 - 1, g * per * 64}
    return sorted(x for x in ks if 0 <= x < T)


def selector_margin(q, k, T):
    """smallest lead of the matching score over the best other one, after the 1/8 scale, given q[i] matches key pi(i) — returned with pi"""
    qh, kh = _heads(q, T), _heads(k, T)
    s = qh @ kh.transpose(0, 2, 1) / 8.0
    pi = s[0].argmax(-1)
    if T == 1:
        return float("inf"), pi
    top2 = np.sort(s, -1)[..., -2:]
    assert all((s[h].argmax(-1) == pi).all() for h in range(s.shape[0]))
    return float((top2[..., 1] - top2[..., 0]).min()), pi


def make_case(family, lens, Tpad=None, H=2, qk_rows=None, out_rows=None, ragged=None, spread=1.0, seed=0):
    """lens: one length, or one per chunk.  Defaults: Tpad = the largest length rounded up to 64, qk_rows = Tpad (so that poisoned query
    / key rows exist wherever T is no multiple of 64), out_rows = the largest length + 3 (sentinel rows behind every chunk)."""
    lens = [int(lens)] if np.isscalar(lens) else [int(x) for x in lens]
    B, T, S = len(lens), max(lens), 64 * H
    Tpad = Tpad or (T + 63) // 64 * 64
    qk_rows = qk_rows or Tpad
    out_rows = out_rows or T + 3
    ragged = (len(set(lens)) > 1) if ragged is None else ragged
    rng = np.random.default_rng([seed, T, B, H, {"selector": 1, "uniform": 2, "random": 3}[family], int(spread * 4)])
    q = np.empty((B, qk_rows, S), np.float16); k = np.empty_like(q); v = np.empty((B, Tpad, S), np.float16)
    pis = []
    for b, Tb in enumerate(lens):
        q[b] = _poison(qk_rows, S); k[b] = _poison(qk_rows, S); v[b] = _poison(Tpad, S)
        if family == "selector":
            code = rng.integers(0, 2, (Tb, S)) * 2 - 1
            pi = rng.permutation(Tb)
            k[b, :Tb] = 4 * code; q[b, :Tb] = 4 * code[pi]; v[b, :Tb] = v_formula(b, Tb, S)
            margin, got = selector_margin(q[b], k[b], Tb)
            assert margin >= SELECTOR_MARGIN and (got == pi).all(), (Tb, margin)
            assert set(boundary_keys(Tb)) <= set(pi.tolist())
            pis.append(pi)
        elif family == "uniform":
            q[b, :Tb] = 0; k[b, :Tb] = rng.standard_normal((Tb, S)); v[b, :Tb] = v_formula(b, Tb, S)
        else:
            q[b, :Tb] = (rng.standard_normal((Tb, S)).astype(np.float16).astype(np.float32) * spread)
            k[b, :Tb] = rng.standard_normal((Tb, S)); v[b, :Tb] = rng.standard_normal((Tb, S))
    name = f"{family}{'' if family != 'random' else f'x{spread:g}'} T={lens if B > 1 else T} H={H}"
    return Case(family, name, B, T, Tpad, S, H, qk_rows, out_rows, lens, ragged, q, k, v, pis)


def ulp16(x):
    return np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)


def _assert_hold(kind, measured, limit, what=None):
    assert measured <= limit, (kind, what, measured, limit)


def hold_case(case: Case, raw: np.ndarray, want_f32: bool, label: str = "", hold=_assert_hold):
    """raw: everything the launch left in `out`, [B][out_rows][S] as uint16 (f16 result) or uint32 (f32) bit patterns.  Asserts, per
    chunk at the chunk's own length, the family's expectation, and that rows [T_chunk, out_rows) still hold the sentinel.  `hold`
    (stage_compare.hold on the GPU) records the random family's ratios under `label`."""
    sent = SENTINEL32 if want_f32 else SENTINEL16
    assert raw.shape == (case.B, case.out_rows, case.S) and raw.dtype == (np.uint32 if want_f32 else np.uint16)
    for b, Tb in enumerate(case.lens):
        what = f"{label} {case.name} chunk {b} {'f32' if want_f32 else 'f16'}"
        tail = raw[b, Tb:]
        bad = np.argwhere(tail != sent)
        assert bad.size == 0, (what, "rows behind the chunk's length were written; first (row, column):", (Tb + int(bad[0][0]), int(bad[0][1])))
        got = raw[b, :Tb].view(np.float32 if want_f32 else np.float16).astype(np.float64)
        assert np.isfinite(got).all(), (what, "not finite (or never written) at (row, column)", tuple(np.argwhere(~np.isfinite(got))[0]))
        exp = case.expected(b)
        d = np.abs(got - exp)
        if case.family == "selector":
            # f16: the value of v[pi(i)] exactly (a zero of either sign: what the one-sweep form's e^-40-scaled remainders round to)
            lim = 2.0 ** -30 if want_f32 else 0.0
            if d.max() > lim:
                i, c = np.unravel_index(d.argmax(), d.shape)
                h = c // 64
                looks = np.flatnonzero((case.v[b, :, h * 64:h * 64 + 64].astype(np.float64) == got[i, h * 64:h * 64 + 64]).all(1))
                over = d > lim
                raise AssertionError((what, f"query {i} head {h}: expected key {case.pi[b][i]}, the row equals key(s) {looks.tolist()[:4]}",
                                      f"max |d| {d.max():.3e} (bound {lim:.3e}), {int(over.sum())} of {d.size} elements over it, "
                                      f"largest |d| / |v| among them {float((d / np.maximum(np.abs(exp), 1e-30))[over].max()):.3e}"))
        elif case.family == "uniform":
            lim = 2.0 ** -22 * np.abs(exp) if want_f32 else ulp16(exp)
            over = d > lim
            if over.any():
                i, c = np.argwhere(over)[0]
                raise AssertionError((what, f"row {i} column {c}: {got[i, c]!r} for {exp[i, c]!r}: off by {d[i, c] / max(abs(exp[i, c]), 1e-30):.3e} relative (1/T = {1 / Tb:.3e})"))
        else:
            ref_rms, ref_max = case.ref_error(b, want_f32)
            rms = float(np.sqrt(np.mean(d * d)))
            # (one key: p = 1 and the result is v[0] in every arithmetic — the reference points are exact, and so must the kernel be)
            ratio = lambda mine, ref: mine / ref if ref > 0 else 0.0 if mine == 0 else float("inf")
            hold(f"encoder attention {label}: rms vs float64 / the reference points' rms", ratio(rms, ref_rms), RMS_LIMIT, what)
            hold(f"encoder attention {label}: max |d| vs float64 / the reference points' max", ratio(float(d.max()), ref_max), MAX_LIMIT, what)


# ------------------------------------------------------------------------------------------------ restatements (negative controls)
def restate(case: Case, want_f32: bool, fault: str = ""):
    """What a kernel with the product's rounding points writes for `case` (the reference's f16 argument and f16 numerator; the P.V product on
    the UNNORMALISED numerators in f32, then one multiplication by 1 / sum) — and, with `fault`, what one with a classic mistake writes:
      extra_key    the first padded key counted            missing_key   the last valid key dropped
      vt_no_swap   the V^T time order read without vt_pos' bit swap
      next_head    head h reads head h + 1's value columns  next_chunk    chunk b reads chunk b + 1's rows
      row_at_T     a result row written at T_chunk
    Returns the raw `out` image hold_case() takes."""
    out = np.full((case.B, case.out_rows, case.S), SENTINEL32 if want_f32 else SENTINEL16, np.uint32 if want_f32 else np.uint16)
    for b, Tb in enumerate(case.lens):
        src = (b + 1) % case.B if fault == "next_chunk" else b
        q, k, v = case.q[src][:Tb], case.k[src], case.v[src]
        nk = Tb + 1 if fault == "extra_key" else Tb - 1 if fault == "missing_key" else Tb
        assert 1 <= nk <= min(case.qk_rows, case.Tpad), "the case has no such key"
        if fault == "vt_no_swap":
            v = v[vt_pos(np.arange(case.Tpad))]
        if fault == "next_head":
            v = np.roll(v, -64, axis=1)
        # nk keys, Tb queries
        f32 = np.float32
        qh = q.astype(f32).reshape(Tb, -1, 64).transpose(1, 0, 2)
        kh = k[:nk].astype(f32).reshape(nk, -1, 64).transpose(1, 0, 2)
        vh = v[:nk].astype(f32).reshape(nk, -1, 64).transpose(1, 0, 2)
        s = (qh @ kh.transpose(0, 2, 1)) * f32(0.125)
        with np.errstate(over="ignore"):                     # a poisoned key's score: -inf as an f16 argument
            e = np.exp((s - s.max(-1, keepdims=True)).astype(np.float16).astype(f32)).astype(np.float16)
        inv = (1.0 / e.astype(np.float64).sum(-1, keepdims=True)).astype(f32)
        o = ((e.astype(f32) @ vh) * inv).transpose(1, 0, 2).reshape(Tb, -1)
        rows = Tb + 1 if fault == "row_at_T" else Tb
        o = np.concatenate([o, o[-1:]])[:rows]
        out[b, :rows] = o.view(np.uint32) if want_f32 else o.astype(np.float16).view(np.uint16)
    return out


# ------------------------------------------------------------------------------------------------ the q|k|v projection
@dataclasses.dataclass
class QkvCase:
    name: str
    M: int
    S: int
    T: int
    Tpad: int
    rows_per_chunk: int
    xn: np.ndarray               # [M][S] f16
    W: np.ndarray                # [3 S][S] f16
    bias: np.ndarray             # [3 S] f32
    exact: bool

    @property
    def chunks(self):
        return self.M // self.rows_per_chunk if self.rows_per_chunk else 1

    def product(self):
        """[M][3 S] float64"""
        return self.xn.astype(np.float64) @ self.W.astype(np.float64).T + self.bias.astype(np.float64)

    def abs_product(self):
        return np.abs(self.xn.astype(np.float64)) @ np.abs(self.W.astype(np.float64)).T


def make_qkv_case(chunks, S=128, T=563, Tpad=576, rpc=576, exact=True, seed=0):
    """chunks = 0: one chunk of M = T rows (rows_per_chunk = 0); else M = chunks x rpc rows, rpc rows per chunk (T valid ones).
    exact: xn integers in [-8, 8], two entries from {+1, -1, +0.5} per row of W, bias integers / 8 — every result is a multiple of 1/8
    below 32, exact in f32 whatever the summation order and exact in f16."""
    rng = np.random.default_rng([seed, chunks, S, T, int(exact)])
    rpc = 0 if chunks == 0 else rpc
    assert T <= (rpc or T) <= Tpad
    M = T if chunks == 0 else chunks * rpc
    if exact:
        xn = rng.integers(-8, 9, (M, S)).astype(np.float16)
        W = np.zeros((3 * S, S), np.float16)
        for n in range(3 * S):
            W[n, rng.choice(S, 2, replace=False)] = rng.choice([1.0, -1.0, 0.5], 2)
        bias = (rng.integers(-8, 9, 3 * S) / 8.0).astype(np.float32)
    else:
        xn = rng.standard_normal((M, S)).astype(np.float16)
        W = (rng.standard_normal((3 * S, S)) / np.sqrt(S)).astype(np.float16)
        bias = rng.standard_normal(3 * S).astype(np.float32)
    return QkvCase(f"{'exact' if exact else 'normal'} chunks={chunks} M={M} Tpad={Tpad}", M, S, T, Tpad, rpc, xn, W, bias, exact)


def hold_qkv(case: QkvCase, q, k, vt, out_rows):
    """q, k [out_rows][S], vt [chunks][S][Tpad] as uint16 bit patterns, prefilled with SENTINEL16 by the hook."""
    M, S, T, Tpad = case.M, case.S, case.T, case.Tpad
    full = case.product()
    tol = None if case.exact else ulp16(full) / 2 + S * 2.0 ** -24 * case.abs_product()       # f32 accumulation, then one f16 rounding
    def close(got, exp, lim, what):
        got = got.view(np.float16).astype(np.float64)
        assert np.isfinite(got).all(), (case.name, what, "not finite (or never written) at", tuple(np.argwhere(~np.isfinite(got))[0]))
        over = np.abs(got - exp) > (0.0 if lim is None else lim)
        assert not over.any(), (case.name, what, "first wrong (row, column)", tuple(np.argwhere(over)[0]), int(over.sum()))
    for name, img, third in (("q", q, 0), ("k", k, 1)):
        close(img[:M], full[:, third * S:(third + 1) * S], None if tol is None else tol[:, third * S:(third + 1) * S], name)
        assert (img[M:] == SENTINEL16).all(), (case.name, name, "rows past M were written")
    rpc = case.rows_per_chunk or M
    T16 = (T + 15) // 16 * 16
    pos = vt_pos(np.arange(Tpad))
    for b in range(case.chunks):
        img = vt[b][:, pos]                                  # [S][t]: time order restored
        rows = slice(b * rpc, b * rpc + T)
        close(img[:, :T], full[rows, 2 * S:].T, None if tol is None else tol[rows, 2 * S:].T, f"V^T chunk {b}")
        assert np.isfinite(img[:, T:T16].view(np.float16).astype(np.float64)).all(), (case.name, f"V^T chunk {b}: padding columns up to {T16} not finite")
        assert (img[:, T16:] == SENTINEL16).all(), (case.name, f"V^T chunk {b}: columns past {T16} were written")

"""The decoder's attention restated in NumPy, and the crafted operands its kernels are held to (tests/test_dec_attn_f64.py proves the
conditions on the CPU, tests/test_gpu_attn_decoder.py runs the kernels on them through wmi_selftest_attn_decoder / wmi_selftest_attn_cross).
Same structure as tests/attn_f64.py, whose constants, poison and value formula are imported.

    attend_f64(q, k, v, visible)          float64 soft-max of q.k over the keys row i sees, per 64-wide head, times v: the yardstick.  No 1/8
                                          factor: the decoder's q and k arrive pre-scaled (d^-1/4 each)
    attend_ref_points(q, k, v, visible)   the same with the reference's rounding points (attn_f64.attend_ref_points): f32 scores, the argument
                                          s - max rounded to f16, the exponential rounded to f16, the sum in double, the probability scaled in
                                          f32 and rounded to f16, P.V in f32, the result f32 or f16.  Its distance from attend_f64 is the unit
                                          the random family is measured in

A Case holds the operands of one launch in the hooks' layouts: q [n][S] f16, the caches k, v [rows][cells][S] f16 (rows = 1: one cache for
every query row, else a cache per row; cells = the cache's capacity `cap` for the self-attention, T for the cross-attention).  Row i sees the
first vis[i] cells of cache crow[i]; every cell behind what ANY row of that cache sees is poisoned +-60000 — finite, as the product promises
only finite junk there — so ONE such cell in a sum is gross.  Three kinds: "self" (one token per row against its own cache: self_attn_rows,
the sa_* prologue of gemv), "dec" (k_attn_dec: n rows against one cache under an additive mask, row i sees n_past + i + 1 cells) and "cross".

Three families:

    selector   k[j] = code(j) in {+1, -1}^64 per head, q[i] = a code(pi(i)), a the power of two at which the generator itself asserts that
               the match leads every other visible score by >= SELECTOR_MARGIN: every other numerator is 0 in f16 (or belongs to another
               key slice, whose weight is e^-40 or less): out[i] == v[pi(i)], and a wrong row names the key that was read
    uniform    q = 0: every numerator is 1 and the sum is the key count n exactly.  The forms that round the normalised probability (every
               self-attention form, k_attn_dec) multiply by p = f16(f32(1 / n)), the cross-attention normalises after P.V: p = 1 / n.
               out = p sum(v[:n]).  THE BOUND: the values are multiples of 1/16 below 8 and p has 11 significant bits, so every product
               p v is exact in f32 and the result is an f32 sum of n exact terms in some order: at most (n - 1) roundings of at most
               2^-24 sum|p v| each (the cross-attention: exact partial sums, then f32(1 / n) and one product: two roundings).  So
               |out - p sum v| <= (n + 1) 2^-24 sum|p v|, plus the result's own rounding: 2^-24 |out| as f32, half an f16 ulp (taken at
               |out| + the bound, so that a value pushed over a binade edge is covered) as f16.  One key more or less moves the result by
               about |v| / n: at n = 1500 the bound is ~1e-4 |v| against 7e-4 |v|, at n = 448 3e-5 |v| against 2e-3 |v|
    random     standard normal operands at a score spread; the distance from attend_f64 in units of attend_ref_points' own, pooled over the
               launch's rows (>= 8 rows x 2 heads: the maximum is over 1000 elements or more).  Limits: attn_f64.RMS_LIMIT / MAX_LIMIT.
               One key: the reference points are exact, and so must the kernel be

hold_case() is the ONE judge of a launch's result: the GPU test passes it what the kernels wrote, the CPU test what restate() writes — the
product's rounding points, and with `fault` one classic mistake, which it must refuse.  Nothing here reads the reference checkout."""
from __future__ import annotations

import dataclasses

import numpy as np

from attn_f64 import MAX_LIMIT, POISON, RMS_LIMIT, SELECTOR_MARGIN, SENTINEL16, SENTINEL32, _poison, ulp16, v_formula

XS_MAX_SLICES = 16                       # csrc/k_attn.hip
F32 = np.float32


def values(b, cells, S):
    """attn_f64.v_formula for the first 255 cells; behind them the column slope grows with the block of 255, so that no two cells of a cache
    hold the same 64 values in any head (v_formula alone repeats every 255 cells: a key read 255 cells off would pass the selector).
    Multiples of 1/16 below 8, like v_formula's."""
    j, c = np.meshgrid(np.arange(cells), np.arange(S), indexing="ij")
    out = (((7 * j + (3 + 2 * (j // 255)) * c + 11 * b) % 255 - 127) / 16.0).astype(np.float16)
    assert np.array_equal(out[:255], v_formula(b, min(cells, 255), S))
    return out


def _keys(visible, i):
    v = visible[i]
    return np.arange(int(v)) if np.ndim(v) == 0 else np.asarray(v, np.int64)


def _cache(a, crow, i):
    return a if a.ndim == 2 else a[crow[i] if crow is not None else i]


def attend_f64(q, k, v, visible, crow=None):
    """q [n][S]; k, v [cells][S] (one cache) or [rows][cells][S] with crow[i] the cache of row i (default: row i's own); visible[i] = the count
    of leading cells row i sees, or their indices.  Returns [n][S] float64."""
    q = np.asarray(q)
    n, S = q.shape
    out = np.empty((n, S))
    for i in range(n):
        idx = _keys(visible, i)
        qh = q[i].astype(np.float64).reshape(-1, 64)
        kh = _cache(k, crow, i)[idx].astype(np.float64).reshape(len(idx), -1, 64)
        vh = _cache(v, crow, i)[idx].astype(np.float64).reshape(len(idx), -1, 64)
        s = np.einsum("jhc,hc->hj", kh, qh)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out[i] = np.einsum("hj,jhc->hc", p, vh).reshape(S)
    return out


def _row_f32(q, k, v, crow, i, idx, next_head=False):
    qh = q[i].astype(F32).reshape(-1, 64)
    kh = _cache(k, crow, i)[idx].astype(F32).reshape(len(idx), -1, 64)
    vr = _cache(v, crow, i)[idx]
    if next_head:
        vr = np.roll(vr, -64, axis=1)
    return qh, kh, vr.astype(F32).reshape(len(idx), -1, 64)


def _exp16(arg):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(arg.astype(np.float16).astype(F32)).astype(np.float16)


def attend_ref_points(q, k, v, visible, crow=None, f16_result=False):
    """The reference's rounding points (see the module docstring).  Returns float64 values."""
    q = np.asarray(q)
    n, S = q.shape
    out = np.empty((n, S), F32)
    for i in range(n):
        qh, kh, vh = _row_f32(q, k, v, crow, i, _keys(visible, i))
        s = np.einsum("jhc,hc->hj", kh, qh)
        e = _exp16(s - s.max(-1, keepdims=True))
        inv = (1.0 / e.astype(np.float64).sum(-1, keepdims=True)).astype(F32)
        p = (e.astype(F32) * inv).astype(np.float16)
        out[i] = np.einsum("hj,jhc->hc", p.astype(F32), vh).reshape(S)
    if f16_result:
        out = out.astype(np.float16)
    return out.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the launch plans the kernels follow
def xattn_plan(T):
    """xattn_layout (csrc/k_attn.hip): the number of key slices and the keys per slice at T keys"""
    ns = min(max((T + 191) // 192, 1), XS_MAX_SLICES)
    return ns, (T + ns - 1) // ns


def groups_of(kind, vis, long_form=False):
    """The contiguous key groups a form cuts row's keys into: the cross-attention's slices; the long self-attention's quarters; for the other
    self-attention forms the first 32 cells and the rest (self_attn_wave's two load batches, <= 64 cells) or blocks of 64 (the barrier form's
    lane stride); k_attn_dec's blocks of 256 (its thread stride).  [(start, end)], none empty."""
    if kind == "cross":
        ns, ks = xattn_plan(vis)
        g = [(s * ks, min((s + 1) * ks, vis)) for s in range(ns)]
    elif kind == "self" and long_form:
        per = (vis + 3) // 4
        g = [(w * per, min((w + 1) * per, vis)) for w in range(4)]
    elif kind == "self":
        g = [(0, min(vis, 32)), (32, vis)] if vis <= 64 else [(b, min(b + 64, vis)) for b in range(0, vis, 64)]
    else:
        g = [(b, min(b + 256, vis)) for b in range(0, vis, 256)]
    return [(a, b) for a, b in g if a < b]


def boundary_keys(kind, vis, long_form=False):
    """cell 0, the last one, both sides of every group boundary of groups_of(), and of what the form does inside a group: the self-attention takes
    its keys 8 at a time (every multiple of 8: the passes of the wave routine, the P.V batches of the barrier and the long form — there from each
    quarter's start); k_attn_dec's P.V walks 32 cells per trip; a cross-attention slice is cut into four wavefronts of roundup8(ceil(ks / 4))
    keys.  The first entries are 0, vis - 1 and the first group boundary."""
    first = [0, vis - 1]
    ks = set()
    gs = groups_of(kind, vis, long_form)
    for a, b in gs[1:]:
        first += [a - 1, a]
    for a, b in gs:
        if kind == "cross":
            kpw = ((xattn_plan(vis)[1] + 3) // 4 + 7) & ~7
            ks |= {a + w * kpw + d for w in range(1, 4) for d in (-1, 0)}
        elif kind == "self" and long_form:
            ks |= {a + m + d for m in range(8, b - a, 8) for d in (-1, 0)}
    if kind == "self":
        ks |= {m + d for m in range(8, vis, 8) for d in (-1, 0)}
    if kind == "dec":
        ks |= {m + d for m in range(32, vis, 32) for d in (-1, 0)}
    out = []
    for x in first + sorted(ks):
        if 0 <= x < vis and x not in out:
            out.append(x)
    return out


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    kind: str                    # "self" | "dec" | "cross"
    family: str
    name: str
    n: int
    S: int
    H: int
    cells: int                   # the caches' second extent: cap (self, dec) or T (cross)
    vis: list                    # cells row i sees: [0, vis[i])
    crow: list                   # cache of row i
    out_rows: int
    q: np.ndarray                # [n][S] f16
    k: np.ndarray                # [rows][cells][S] f16
    v: np.ndarray
    pi: list                     # selector: the key of every row
    long_form: bool = False      # self: the four-wavefront form
    n_past: int = 0              # dec
    ragged: bool = False         # cross: pass vis as row_lens
    p_rounded: bool = True       # uniform: the form rounds the normalised probability to f16
    _memo: dict = dataclasses.field(default_factory=dict)

    @property
    def rows(self):
        return self.k.shape[0]

    def expected(self):
        """[n][S] float64"""
        if "exp" not in self._memo:
            if self.family == "selector":
                e = np.stack([self.v[self.crow[i], self.pi[i]] for i in range(self.n)]).astype(np.float64)
            elif self.family == "uniform":
                e = np.stack([self.uniform_p(i) * self.v[self.crow[i], :self.vis[i]].astype(np.float64).sum(0) for i in range(self.n)])
            else:
                e = attend_f64(self.q, self.k, self.v, self.vis, self.crow)
            self._memo["exp"] = e
        return self._memo["exp"]

    def uniform_p(self, i):
        return float(np.float16(F32(1.0 / self.vis[i]))) if self.p_rounded else 1.0 / self.vis[i]

    def uniform_bound(self, want_f32):
        """[n][S]: the module docstring's bound"""
        exp = self.expected()
        lim = np.stack([(self.vis[i] + 1) * 2.0 ** -24 * self.uniform_p(i) * np.abs(self.v[self.crow[i], :self.vis[i]].astype(np.float64)).sum(0)
                        for i in range(self.n)])
        return lim + (2.0 ** -24 * np.abs(exp) if want_f32 else ulp16(np.minimum(np.abs(exp) + lim, 65000.0)) / 2)

    def ref_error(self, want_f32):
        """(rms, max) of attend_ref_points' distance from float64 over the launch's rows, with the launch's result type"""
        key = ("ref", bool(want_f32))
        if key not in self._memo:
            d = attend_ref_points(self.q, self.k, self.v, self.vis, self.crow, f16_result=not want_f32) - self.expected()
            self._memo[key] = (float(np.sqrt(np.mean(d * d))), float(np.abs(d).max()))
        return self._memo[key]

    def mask(self):
        """dec: [n][n_kv] f32, 0 where row i sees the cell, -inf elsewhere"""
        n_kv = self.n_past + self.n
        j = np.arange(n_kv)[None, :]
        return np.where(j < np.asarray(self.vis)[:, None], 0.0, -np.inf).astype(F32)

    def one_row(self, i):
        """row i as a launch of its own at its own length (cross: T = vis[i]; self: the same cache and capacity)"""
        cells = self.vis[i] if self.kind == "cross" else self.cells
        r = self.crow[i]
        return Case(self.kind, self.family, f"{self.name}[{i}]", 1, self.S, self.H, cells, [self.vis[i]], [0], 4, self.q[i:i + 1],
                    np.ascontiguousarray(self.k[r:r + 1, :cells]), np.ascontiguousarray(self.v[r:r + 1, :cells]),
                    [self.pi[i]] if len(self.pi) else [], self.long_form, self.n_past, False, self.p_rounded)


def selector_lead(case):
    """the smallest lead of the matching score over the best other VISIBLE one, over rows and heads"""
    lead = np.inf
    for i in range(case.n):
        vis = case.vis[i]
        if vis == 1:
            continue
        qh = case.q[i].astype(np.float64).reshape(-1, 64)
        kh = case.k[case.crow[i], :vis].astype(np.float64).reshape(vis, -1, 64)
        s = np.einsum("jhc,hc->hj", kh, qh)
        match = s[:, case.pi[i]].copy()
        s[:, case.pi[i]] = -np.inf
        lead = min(lead, float((match - s.max(-1)).min()))
    return lead


def _make(kind, family, name, n, H, cells, vis, crow, rows, out_rows, pis, spread, seed, same_q=False, **kw):
    S = 64 * H
    vis = [int(x) for x in vis]
    assert all(1 <= x <= cells for x in vis) and len(vis) == n and len(crow) == n
    rng = np.random.default_rng([seed, n, H, cells, sum(vis), {"selector": 1, "uniform": 2, "random": 3}[family], int(spread * 4), len(kind)])
    seen = [max([vis[i] for i in range(n) if crow[i] == r], default=0) for r in range(rows)]      # cells of cache r any row sees
    q = np.zeros((n, S), np.float16)
    k = np.stack([_poison(cells, S) for _ in range(rows)])
    v = k.copy()
    pi = []
    for r in range(rows):
        m = seen[r]
        k[r, :m] = rng.integers(0, 2, (m, S)) * 2 - 1 if family == "selector" else rng.standard_normal((m, S))
        v[r, :m] = rng.standard_normal((m, S)) if family == "random" else values(r, m, S)
    if family == "selector":
        pi = [int(x) for x in (pis if pis is not None else [rng.integers(0, vis[i]) for i in range(n)])]
        assert all(0 <= pi[i] < vis[i] for i in range(n)), (name, pi, vis)
        if same_q:                                            # one query for every row (the projection's bias): row i's cache holds its code at pi(i)
            assert rows == n
            code0 = rng.integers(0, 2, S) * 2 - 1
            for i in range(n):
                k[i, pi[i]] = code0
        if kind == "dec":
            # a row that picks its own cell (the mask's edge): the cell behind it, which the row must NOT see, gets the same code wherever no
            # other row's match is either of the two — a mask off by one then ties the scores and returns the mean of two value rows
            for i in range(n):
                j = pi[i]
                if j == vis[i] - 1 and j + 1 < seen[0] and not any(pi[o] in (j, j + 1) for o in range(n) if o != i):
                    k[0, j + 1] = k[0, j]
        for i in range(n):
            q[i] = k[crow[i], pi[i]]
    elif family == "random":
        q[:] = rng.standard_normal((1 if same_q else n, S)).astype(np.float16).astype(F32) * spread
    c = Case(kind, family, name, n, S, H, cells, vis, list(crow), out_rows, q, k, v, pi, **kw)
    if family == "selector" and max(vis) > 1:
        lead1 = selector_lead(c)
        assert lead1 >= 2, (name, "two visible keys share a head's code", lead1)
        a = 1
        while a * lead1 < SELECTOR_MARGIN:
            a *= 2
        assert a <= 32
        c.q = (c.q.astype(F32) * a).astype(np.float16)
        assert selector_lead(c) >= SELECTOR_MARGIN
    return c


def make_self(family, lens, H=2, cap=448, long_form=False, pis=None, spread=1.0, seed=0):
    """one token per row, row i against its own cache of `cap` cells, lens[i] of them valid"""
    n = len(lens)
    name = f"self {family}{'' if family != 'random' else f'x{spread:g}'} cells={lens if len(set(lens)) > 1 else lens[0]} n={n} cap={cap} H={H}{' long' if long_form else ''}"
    return _make("self", family, name, n, H, cap, lens, list(range(n)), n, n + 3, pis, spread, seed, long_form=long_form)


def make_dec(family, n, n_past, H=2, cap=None, all_visible=False, pis=None, spread=1.0, seed=0):
    """k_attn_dec: n rows against ONE cache of n_past + n cells (capacity cap), row i sees n_past + i + 1 of them (all_visible: a mask of zeros)"""
    n_kv = n_past + n
    cap = cap or n_kv
    vis = [n_kv if all_visible else n_past + i + 1 for i in range(n)]
    name = f"dec {family}{'' if family != 'random' else f'x{spread:g}'} n={n} n_past={n_past} cap={cap} H={H}{' all visible' if all_visible else ''}"
    return _make("dec", family, name, n, H, cap, vis, [0] * n, 1, n + 3, pis, spread, seed, n_past=n_past)


def make_cross(family, T, n, H=2, lens=None, per_row=False, same_q=False, pis=None, spread=1.0, seed=0):
    """n rows against a cross cache of T keys (per_row: a cache each, kv_row_stride = T S); lens: a length per row, passed as row_lens"""
    vis = list(lens) if lens is not None else [T] * n
    rows = n if per_row or lens is not None else 1
    name = f"cross {family}{'' if family != 'random' else f'x{spread:g}'} T={T} n={n} H={H}{f' lens={vis}' if lens is not None else ''}{' cache per row' if rows > 1 else ''}{' one query' if same_q else ''}"
    return _make("cross", family, name, n, H, T, vis, list(range(n)) if rows > 1 else [0] * n, rows, n + 3, pis, spread, seed, same_q=same_q,
                 ragged=lens is not None, p_rounded=False)


def chunks(keys, n, limit=None):
    """keys in launches of n rows (the last one filled up from the front)"""
    out = [list(keys[a:a + n]) for a in range(0, len(keys), n)]
    out[-1] += list(keys[:n - len(out[-1])]) if len(keys) >= n else [keys[0]] * (n - len(out[-1]))
    return out[:limit]


# ------------------------------------------------------------------------------------------------ the judge
def _assert_hold(kind, measured, limit, what=None):
    assert measured <= limit, (kind, what, measured, limit)


def hold_case(case: Case, raw: np.ndarray, want_f32: bool, label: str = "", hold=_assert_hold, partials=None):
    """raw: everything the launch left in `out`, [out_rows][S] as uint16 (f16 result) or uint32 (f32) bit patterns.  Asserts the family's
    expectation per row at the row's own key count, and that rows [n, out_rows) still hold the sentinel.  partials = (pmax, part_l, part_o,
    ns) of a cross-attention launch with per-row lengths ([n][H][ns], [n][H][ns], [n][H][ns][64], as float32): every slice a row does not have
    must hold the neutral partial exactly.  `hold` (stage_compare.hold on the GPU) records the random family's ratios under `label`."""
    sent = SENTINEL32 if want_f32 else SENTINEL16
    assert raw.shape == (case.out_rows, case.S) and raw.dtype == (np.uint32 if want_f32 else np.uint16), (raw.shape, raw.dtype)
    what = f"{label} {case.name} {'f32' if want_f32 else 'f16'}"
    bad = np.argwhere(raw[case.n:] != sent)
    assert bad.size == 0, (what, "rows behind the launch's rows were written; first (row, column):", (case.n + int(bad[0][0]), int(bad[0][1])))
    got = raw[:case.n].view(F32 if want_f32 else np.float16).astype(np.float64)
    assert np.isfinite(got).all(), (what, "not finite (or never written) at (row, column)", tuple(np.argwhere(~np.isfinite(got))[0]))
    if partials is not None:
        pmax, part_l, part_o, ns = partials
        assert case.kind == "cross" and pmax.shape == (case.n, case.H, ns) and part_o.shape == (case.n, case.H, ns, 64)
        for i in range(case.n):
            nsr = xattn_plan(case.vis[i])[0] if case.ragged else ns
            assert nsr <= ns
            assert (pmax[i, :, nsr:] == -np.inf).all() and (part_l[i, :, nsr:].view(np.uint32) == 0).all() and \
                (part_o[i, :, nsr:].view(np.uint32) == 0).all(), (what, f"row {i} has {nsr} slices: the partials of slices {nsr}..{ns - 1} are not neutral")
            assert np.isfinite(pmax[i, :, :nsr]).all() and (part_l[i, :, :nsr] >= 1).all(), (what, f"row {i}: a slice it has holds no partial")
    exp = case.expected()
    d = np.abs(got - exp)
    if case.family == "selector":
        # f16: the value of v[pi(i)] exactly (a zero of either sign); f32: the slice-maximum form carries e^-40-scaled remainders of the other slices
        lim = 2.0 ** -30 if want_f32 else 0.0
        if d.max() > lim:
            i, c = np.unravel_index(d.argmax(), d.shape)
            h = c // 64
            vr = case.v[case.crow[i], :, h * 64:h * 64 + 64].astype(np.float64)
            looks = np.flatnonzero((vr == got[i, h * 64:h * 64 + 64]).all(1))
            over = d > lim
            raise AssertionError((what, f"row {i} head {h}: expected key {case.pi[i]} of {case.vis[i]}, the row equals key(s) {looks.tolist()[:4]}",
                                  f"max |d| {d.max():.3e} (bound {lim:.3e}), {int(over.sum())} of {d.size} elements over it, rows {sorted(set(np.argwhere(over)[:, 0].tolist()))[:8]}"))
    elif case.family == "uniform":
        over = d > case.uniform_bound(want_f32)
        if over.any():
            i, c = np.argwhere(over)[0]
            raise AssertionError((what, f"row {i} column {c}: {got[i, c]!r} for {exp[i, c]!r}: off by {d[i, c]:.3e}, bound {case.uniform_bound(want_f32)[i, c]:.3e} "
                                        f"(one key is about {1 / case.vis[i]:.3e} of a value), {int(over.sum())} of {d.size} elements, rows {sorted(set(np.argwhere(over)[:, 0].tolist()))[:8]}"))
    else:
        ref_rms, ref_max = case.ref_error(want_f32)
        rms = float(np.sqrt(np.mean(d * d)))
        ratio = lambda mine, ref: mine / ref if ref > 0 else 0.0 if mine == 0 else float("inf")      # (one key: the reference points are exact)
        hold(f"decoder attention {label}: rms vs float64 / the reference points' rms", ratio(rms, ref_rms), RMS_LIMIT, what)
        hold(f"decoder attention {label}: max |d| vs float64 / the reference points' max", ratio(float(d.max()), ref_max), MAX_LIMIT, what)


# ------------------------------------------------------------------------------------------------ restatements (negative controls)
FAULTS = {
    "drop_last":      "the last valid cell dropped",
    "extra_cell":     "the cell behind the last valid one counted (self, dec: cell n_kv, poisoned; cross with lengths: key len)",
    "slice_first":    "the first key of every key slice but the first dropped",
    "slice_overlap":  "the last key of a key slice counted in the next slice too",
    "quarter_twice":  "the long self-attention form: the last key of a quarter counted by the next quarter too",
    "weight_one":     "slices combined with weight 1 instead of exp(m_s - M)",
    "stale_partial":  "a slice the row does not have counted with a stale l (that of the launch's longest row)",
    "next_head":      "head h reads head h + 1's value columns",
    "row_stride":     "every row reads the first row's cache (the row stride ignored)",
    "mask_off_by_one": "the causal mask off by one: row i sees cell n_past + i + 1",
}
# what a family cannot see by arithmetic: q = 0 makes every slice maximum 0, so weight 1 IS exp(m_s - M); a key counted twice is counted twice
# in the soft-max sum too, so the selector's match still returns its value
BLIND = {("weight_one", "uniform"), ("slice_overlap", "selector"), ("quarter_twice", "selector")}
FAULTS_OF = {"self": ("drop_last", "extra_cell", "next_head", "row_stride"),
             "self long": ("drop_last", "extra_cell", "next_head", "row_stride", "quarter_twice"),
             "dec": ("drop_last", "extra_cell", "next_head", "mask_off_by_one"),
             "cross": ("drop_last", "slice_first", "slice_overlap", "weight_one", "next_head", "row_stride"),
             "cross lens": ("drop_last", "extra_cell", "slice_first", "slice_overlap", "weight_one", "stale_partial", "next_head", "row_stride")}


class NoSuchKey(Exception):
    """the case has no key or slice the fault could touch"""


def fault_kind(case):
    return "self long" if case.long_form else "cross lens" if case.ragged else case.kind


def _fault_groups(case, i, fault):
    vis = case.vis[i]
    gs = [np.arange(a, b) for a, b in groups_of(case.kind, vis, case.long_form)]
    if fault == "drop_last":
        if vis < 2: return None
        gs[-1] = gs[-1][:-1]
        gs = [g for g in gs if len(g)]
    elif fault == "extra_cell":
        cell = case.n_past + case.n if case.kind == "dec" else vis
        if cell >= case.cells: return None
        gs[-1] = np.append(gs[-1], cell)
    elif fault == "mask_off_by_one":
        if vis >= case.cells: return None
        gs[-1] = np.append(gs[-1], vis)
    elif fault == "slice_first":
        if len(gs) < 2: return None
        gs = [gs[0]] + [g[1:] for g in gs[1:]]
        gs = [g for g in gs if len(g)]
    elif fault in ("slice_overlap", "quarter_twice"):
        if len(gs) < 2: return None
        gs = [gs[0]] + [np.append(gs[s - 1][-1], gs[s]) for s in range(1, len(gs))]
    return gs


def restate(case: Case, want_f32: bool, fault: str = "", variant: str = ""):
    """What a kernel with the product's rounding points writes for `case`, and with `fault` (FAULTS) what one with that mistake writes.
    variant "points": the reference's points (every self-attention form, k_attn_dec); "slices": the one-launch cross form — per key slice
    the maximum m_s, e = f16(exp(f16(s - m_s))), l_s = sum e and o_s = e.V in f32, combined as o = sum o_s w_s, l = sum l_s w_s (double) with
    w_s = exp(m_s - M) in f32, out = o f32(1 / l); "global": the two-launch cross form — the exact maximum, e as in the reference, P.V on the
    unnormalised numerators, one multiplication by f32(1 / l).  Default: "slices" for cross cases, else "points".
    Returns (raw, partials): the `out` image hold_case() takes and, for "slices", (pmax, part_l, part_o, ns) (else None).
    Raises NoSuchKey when no row of the case has the key or slice the fault touches."""
    variant = variant or ("slices" if case.kind == "cross" else "points")
    assert not fault or fault in FAULTS
    n, S, H = case.n, case.S, case.H
    out = np.zeros((n, S), F32)
    ns = xattn_plan(max(case.vis))[0] if case.kind == "cross" else 1
    pmax = np.full((n, H, ns), -np.inf, F32); part_l = np.zeros((n, H, ns), F32); part_o = np.zeros((n, H, ns, 64), F32)
    touched = not fault or fault in ("next_head",)
    if fault == "weight_one":
        if variant != "slices": raise NoSuchKey(fault)
    if fault == "row_stride" and case.rows < 2: raise NoSuchKey(fault)
    crow = [0] * n if fault == "row_stride" else case.crow
    for i in range(n):
        gs = _fault_groups(case, i, fault) if fault in ("drop_last", "extra_cell", "mask_off_by_one", "slice_first", "slice_overlap", "quarter_twice") else None
        if gs is None:
            gs = [np.arange(a, b) for a, b in groups_of(case.kind, case.vis[i], case.long_form)]
        else:
            touched = True
        if fault == "row_stride" and case.crow[i] != 0: touched = True
        if fault == "weight_one" and len(gs) > 1: touched = True
        idx = np.concatenate(gs)
        qh, kh, vh = _row_f32(case.q, case.k, case.v, crow, i, idx, next_head=fault == "next_head")
        s = np.einsum("jhc,hc->hj", kh, qh)                  # [H][keys]
        if variant == "slices":
            o = np.zeros((H, 64), F32); l = np.zeros(H); at = 0
            starts = np.cumsum([0] + [len(g) for g in gs[:-1]])
            ms = np.stack([s[:, a:a + len(g)].max(-1) for a, g in zip(starts, gs)], -1)      # [H][slices]
            M = ms.max(-1)
            for sl, g in enumerate(gs):
                e = _exp16(s[:, at:at + len(g)] - ms[:, sl:sl + 1]).astype(F32)
                ls = e.sum(-1, dtype=F32); os_ = np.einsum("hj,jhc->hc", e, vh[at:at + len(g)]).astype(F32)
                w = np.ones(H, F32) if fault == "weight_one" else np.exp((ms[:, sl] - M).astype(F32)).astype(F32)
                o += os_ * w[:, None]; l += ls.astype(np.float64) * w.astype(np.float64)
                pmax[i, :, sl] = ms[:, sl]; part_l[i, :, sl] = ls; part_o[i, :, sl] = os_
                at += len(g)
            if fault == "stale_partial" and len(gs) < ns:
                touched = True
                stale = float(xattn_plan(max(case.vis))[1])
                l += stale * (ns - len(gs))
                pmax[i, :, len(gs):] = ms[:, :1]; part_l[i, :, len(gs):] = stale
            out[i] = (o * (1.0 / l).astype(F32)[:, None]).reshape(S)
        else:
            e = _exp16(s - s.max(-1, keepdims=True))
            inv = (1.0 / e.astype(np.float64).sum(-1, keepdims=True)).astype(F32)
            if variant == "points":
                p = (e.astype(F32) * inv).astype(np.float16).astype(F32)
                out[i] = np.einsum("hj,jhc->hc", p, vh).reshape(S)
            else:
                out[i] = (np.einsum("hj,jhc->hc", e.astype(F32), vh).astype(F32) * inv).reshape(S)
    if not touched:
        raise NoSuchKey(fault)
    raw = np.full((case.out_rows, S), SENTINEL32 if want_f32 else SENTINEL16, np.uint32 if want_f32 else np.uint16)
    with np.errstate(over="ignore"):
        raw[:n] = out.view(np.uint32) if want_f32 else out.astype(np.float16).view(np.uint16)
    return raw, ((pmax, part_l, part_o, ns) if variant == "slices" else None)


# ------------------------------------------------------------------------------------------------ the shapes both test modules walk
SELF_CELLS = (1, 2, 8, 9, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 447, 448)
LOCKSTEP_SELF = (1, 32, 33, 64, 65, 200)
HEADS = (6, 8, 12, 16, 20)
HEAD_CELLS = (5, 40, 100)
DEC_PROMPTS = ((5, 59), (5, 60), (5, 61), (200, 0), (448, 0))           # (n, n_past)
CROSS_T = (1, 2, 191, 192, 193, 384, 385, 768, 777, 1152, 1344, 1345, 1499, 1500)         # ns = 1 .. 8 (768: 4 slices, 1152: 6)
LOCKSTEP_CROSS = (1500, 777, 193, 1)
SPREADS = (0.25, 1.0, 4.0)
SELF_ROWS = 16                           # rows of a self-attention launch (lock-step rows: at most 16)
CROSS_ROWS = 8


def _families(family, make, sel_keys=None, rows=8, limit=None):
    if family == "selector":
        return [make("selector", n=rows, pis=ch) for ch in chunks(sel_keys, rows, limit)]
    if family == "uniform":
        return [make("uniform", n=rows)]
    return [make("random", n=max(rows, 8), spread=s) for s in SPREADS]


def self_cases(family, cells, H=2, cap=448, long_form=False, rows=SELF_ROWS, limit=None):
    """launches of `rows` rows (random: 8) with `cells` valid cells each; the selector's launches cover boundary_keys()"""
    mk = lambda fam, n, **kw: make_self(fam, [cells] * (min(n, 8) if fam != "selector" else n), H=H, cap=cap, long_form=long_form, **kw)
    return _families(family, mk, boundary_keys("self", cells, long_form), rows, limit)


def dec_row_cases(family, cells, H=2, cap=448):
    """k_attn_dec at n = 1 with n_past = cells - 1: the selector one launch per boundary key; the random family 8 rows under a mask of zeros"""
    if family == "selector":
        return [make_dec("selector", 1, cells - 1, H=H, cap=cap, pis=[key]) for key in boundary_keys("dec", cells)]
    if family == "uniform":
        return [make_dec("uniform", 1, cells - 1, H=H, cap=cap)]
    # at least 1024 elements for the ratios: fewer cells than 8 rows take more heads (k_attn_dec is one workgroup per (row, head))
    n = min(8, cells)
    return [make_dec("random", n, cells - n, H=max(H, -(-16 // n)), cap=cap, all_visible=True, spread=s) for s in SPREADS]


def dec_prompt_cases(family, n, n_past, cap=None):
    """n rows from n_past: the selector's row i picks its own cell n_past + i (the mask's edge), cell 0, or a cell on either side of a boundary"""
    if family == "selector":
        keys = boundary_keys("dec", n_past + n)
        def pick(i):
            top = n_past + i
            if i % 3 == 0: return top
            if i % 3 == 2: return (i * 7919) % (top + 1)
            below = sorted(x for x in keys if x <= top)
            return below[-1 - (i // 3) % min(4, len(below))]
        pis = [pick(i) for i in range(n)]
        return [make_dec("selector", n, n_past, cap=cap, pis=pis)]
    if family == "uniform":
        return [make_dec("uniform", n, n_past, cap=cap)]
    return [make_dec("random", n, n_past, H=max(2, -(-16 // n)), cap=cap, spread=s) for s in SPREADS]      # at least 1024 elements: 5 rows take 4 heads


def cross_cases(family, T, n=CROSS_ROWS, H=2, per_row=False, same_q=False, limit=None):
    mk = lambda fam, n, **kw: make_cross(fam, T, n, H=H, per_row=per_row or same_q, same_q=same_q, **kw)
    if family == "selector":
        return [mk("selector", n, pis=ch) for ch in chunks(boundary_keys("cross", T), n, limit)]
    if family == "uniform":
        return [mk("uniform", n)]
    return [mk("random", max(n, 8), spread=s) for s in SPREADS]


def cross_lockstep_cases(family, lens=LOCKSTEP_CROSS, H=2, same_q=False):
    T = max(lens)
    if family == "selector":
        per = [boundary_keys("cross", L) for L in lens]
        launches = max(len(p) for p in per)
        return [make_cross("selector", T, len(lens), H=H, lens=lens, same_q=same_q, pis=[p[j % len(p)] for p in per]) for j in range(launches)]
    if family == "uniform":
        return [make_cross("uniform", T, len(lens), H=H, lens=lens, same_q=same_q)]
    return [make_cross("random", T, 2 * len(lens), H=H, lens=list(lens) * 2, same_q=same_q, spread=s) for s in SPREADS]      # 8 rows


def self_lockstep_cases(family, lens=LOCKSTEP_SELF, H=2, cap=448, long_form=False):
    if family == "selector":
        per = [boundary_keys("self", L, long_form) for L in lens]
        return [make_self("selector", list(lens), H=H, cap=cap, long_form=long_form, pis=[p[j % len(p)] for p in per]) for j in range(max(len(p) for p in per))]
    if family == "uniform":
        return [make_self("uniform", list(lens), H=H, cap=cap, long_form=long_form)]
    return [make_self("random", list(lens) * 2, H=H, cap=cap, long_form=long_form, spread=s) for s in SPREADS]      # 12 rows

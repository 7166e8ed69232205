"""Token alignment restated in NumPy: the float64 judge of the alignment matrix, the f32 DTW as a loop, and the crafted operands the
kernels are held to (tests/test_dtw_f64.py proves the conditions on the CPU, tests/test_gpu_token_dtw.py runs the kernels).

The definition (include/wmi_device.h).  A pass has n rows and M key frames; a pair p has a query [n][64] and keys
[M][64], f16.  s = q . k^T (no further scale), w = soft-max over exactly the M keys, z = (w - mean) / sigma per (pair, frame) over all n
rows with the population sigma (sigma == 0 gives 0), a median of 7 along the frames with reflect padding (none for M <= 3),
A[r][t] = mean over the pairs of z[n_sot + r][t], r < R = n - n_sot - 1.  The path is the DTW of -A in f32 with OpenAI's tie rule.

    matrix_f64(qp, kp, n_sot)         A in float64 and its per-element bound for an f32 implementation
    matrix_f32(qp, kp, n_sot, wrong)  the same arithmetic in f32 (one summation order of many); `wrong` names a deliberate mistake
    dtw_f32(A)                        (jumps, path): the f32 recurrence swept over anti-diagonals — a cell depends on three finished cells
                                      only, so every order that respects the dependencies gives the same bits; dtw_scalar(A) is the literal
                                      j-outer, i-inner loop, dtw_f32(A, wrong=...) the deliberately wrong ones
    hold_matrix / hold_path           the ONE judge of a result: the GPU tests pass what the kernels wrote, the CPU test what the wrong
                                      restatements write, which it must refuse

The bound of A, per element, first order with the float64 quantities of the same operands (u = 2^-24):
    scores     f16 x f16 products are exact in f32; a 64-term f32 sum in any order: |ds| <= 64 u sum_c |q_c k_c|
    argument   a = s - max(s): the soft-max does not depend on the shift, so only the subtraction's rounding counts: |da| <= |ds| + u |a|
    exp        expf within EXP_ULP ulp: relative error theta_t = |da_t| + 2 EXP_ULP u (+ one denormal, 2^-126, absolute)
    soft-max   the denominator is a sum of M positive terms in any order, (M - 1) u relative, plus the terms' own errors weighted by
               w; the division u:  |dw_t| <= w_t (theta_t + sum_j w_j theta_j + M u) + 2^-126
    mean       |dmu| <= mean_i |dw_i| + (n + 1) u mean_i |w_i|           (a sum of n terms and a division)
    deviation  d_i = w_i - mu: |dd_i| <= |dw_i| + |dmu| + u |d_i|
    sigma      the root-mean-square is a norm: |dsigma| <= rms_i |dd_i| + sigma (n + 4) u   (the sum of squares, the division, the root)
    z          |dz_i| <= (|dd_i| + |z_i| |dsigma|) / sigma + u |z_i|, times 1 / (1 - |dsigma| / sigma) for the second order;
               a column whose float64 sigma is 0 must give exactly 0 (M = 1: every weight is 1.0 in f32 too)
    median     1-Lipschitz in the sup norm: the largest |dz| of the seven taps
    mean       over P pairs, a sequential f32 sum and one division: mean_p(bound_p) + (P + 1) u mean_p |med_p|
Measured on the random family of cases() (test_dtw_f64.py::test_f32_restatement_within_bound prints it): the f32 restatement's distance
from float64 is 0.0025 of this bound at the most — the bound is a worst case over summation orders, the restatement takes one.  The kernels are
held to the bound itself, not to twice a measured value: every term is derived.

Crafted families (cases()):
    bands    keys of frame t carry 4 code(band(t)), row n_sot + r carries 4 code(r), the start rows and the last row are 0; the codes are
             rows of the 64 x 64 Hadamard matrix (the matching score is 1024, every other 0), the bands are >= 7 frames wide and monotone:
             z is constant on a band for every row, the median changes nothing, A is a staircase and jump[r] is the start of band r
    ties     integer-valued A (all zeros among them): the tie rule decides the path
    random   standard normal operands scaled to a score spread of SPREAD; every column's sigma stays above SIGMA_FLOOR times its mean
             weight (asserted when the case is built), so that the bound stays far below the distance of every wrong restatement"""
from __future__ import annotations

import dataclasses

import numpy as np

U = 2.0 ** -24
EXP_ULP = 2.0
TINY = 2.0 ** -126
SPREAD = 3.0
SIGMA_FLOOR = 0.05
POISON = 60000.0
SENTINEL32 = 0x7FC5A5A5


# ------------------------------------------------------------------------------------------------ the matrix
def _median7(z, wrong=None):
    """[..][M] -> the median of 7 along the last axis, reflect padding"""
    M = z.shape[-1]
    width = 5 if wrong == "median5" else 7
    pad = width // 2
    if M <= 3:
        return z
    zp = np.pad(z, [(0, 0)] * (z.ndim - 1) + [(pad, pad)], mode="edge" if wrong == "edge_pad" else "reflect")
    win = np.lib.stride_tricks.sliding_window_view(zp, width, axis=-1)
    return np.sort(win, axis=-1)[..., width // 2]


def _max7(e):
    M = e.shape[-1]
    if M <= 3:
        return e
    ep = np.pad(e, [(0, 0)] * (e.ndim - 1) + [(3, 3)], mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(ep, 7, axis=-1).max(-1)


def pair_f64(q, k):
    """one pair: q [n][64], k [M][64] f16 -> (filtered z [n][M], its bound [n][M]) in float64"""
    q = np.asarray(q).astype(np.float64); k = np.asarray(k).astype(np.float64)
    n, M = q.shape[0], k.shape[0]
    s = q @ k.T
    ds = 64 * U * (np.abs(q) @ np.abs(k).T)
    a = s - s.max(-1, keepdims=True)
    e = np.exp(a)
    w = e / e.sum(-1, keepdims=True)
    theta = ds + U * np.abs(a) + 2 * EXP_ULP * U
    dw = w * (theta + (w * theta).sum(-1, keepdims=True) + M * U) + TINY
    mu = w.mean(0)
    d = w - mu
    sigma = np.sqrt((d * d).mean(0))
    dmu = dw.mean(0) + (n + 1) * U * np.abs(w).mean(0)
    dd = dw + dmu + U * np.abs(d)
    dsig = np.sqrt((dd * dd).mean(0)) + sigma * (n + 4) * U
    ok = sigma > 0
    sg = np.where(ok, sigma, 1.0)
    z = np.where(ok, d / sg, 0.0)
    rel = np.where(ok, dsig / sg, 0.0)
    second = np.where(rel < 0.5, 1.0 / (1.0 - np.minimum(rel, 0.5)), np.inf)
    dz = np.where(ok, ((dd + np.abs(z) * dsig) / sg + U * np.abs(z)) * second, 0.0)
    return _median7(z), _max7(dz)


def matrix_f64(qp, kp, n_sot):
    """qp [P][n][64], kp [P][M][64] (f16) -> (A [R][M], bound [R][M]) float64"""
    P, n = len(qp), np.asarray(qp[0]).shape[0]
    R = n - n_sot - 1
    acc = bnd = mag = 0.0
    for p in range(P):
        med, dz = pair_f64(qp[p], kp[p])
        acc = acc + med[n_sot:n_sot + R]; bnd = bnd + dz[n_sot:n_sot + R]; mag = mag + np.abs(med[n_sot:n_sot + R])
    return acc / P, bnd / P + (P + 1) * U * mag / P


def matrix_f32(qp, kp, n_sot, wrong=None, k_all=None):
    """The kernels' arithmetic in NumPy f32.  wrong: 'softmax_T' (k_all [P][T][64]: the soft-max runs over all T keys), 'sample_sigma',
    'edge_pad', 'median5', 'no_shift' (rows 0 .. R-1 instead of n_sot ..).  ('wrong_layer' is a matter of which operands are passed.)"""
    f32 = np.float32
    P, n = len(qp), np.asarray(qp[0]).shape[0]
    M = np.asarray(kp[0]).shape[0]
    R = n - n_sot - 1
    acc = np.zeros((R, M), f32)
    for p in range(P):
        q = np.asarray(qp[p]).astype(f32)
        k = np.asarray(k_all[p] if wrong == "softmax_T" else kp[p]).astype(f32)
        s = (q @ k.T).astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.exp((s - s.max(-1, keepdims=True)).astype(f32)).astype(f32)
            w = (e / e.sum(-1, keepdims=True, dtype=f32)).astype(f32)[:, :M]
            mu = (w.sum(0, dtype=f32) / f32(n)).astype(f32)
            d = (w - mu).astype(f32)
            var = ((d * d).sum(0, dtype=f32) / f32(n - 1 if wrong == "sample_sigma" else n)).astype(f32)
            sigma = np.sqrt(var).astype(f32)
            z = np.where(sigma == 0, f32(0), d / np.where(sigma == 0, f32(1), sigma)).astype(f32)
        med = _median7(z, wrong)
        r0 = 0 if wrong == "no_shift" else n_sot
        acc = (acc + med[r0:r0 + R]).astype(f32)
    return (acc / f32(P)).astype(f32)


def hold_matrix(A, A64, bound, what=None, hold=None):
    """A is what an implementation wrote ([R][M] f32): every element finite and within `bound` of A64.  Returns the largest
    |d| / bound (elements with bound 0 must be exact).  hold: stage_compare.hold, so that a GPU run's log shows the margin."""
    A = np.asarray(A)
    assert A.shape == A64.shape, (what, A.shape, A64.shape)
    assert np.isfinite(A).all(), (what, "not finite", int((~np.isfinite(A)).sum()))
    d = np.abs(A.astype(np.float64) - A64)
    exact = bound == 0
    assert (d[exact] == 0).all(), (what, "an element that must be exact is not")
    ratio = float((d[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    if hold is not None:
        hold("dtw matrix |d| / bound", ratio, 1.0, what)
    assert ratio <= 1.0, (what, ratio, int(np.argmax(np.where(exact, 0, d / np.where(exact, 1, bound)))))
    return ratio


# ------------------------------------------------------------------------------------------------ the path
def _backtrace(trace, R, M, transposed=False):
    trace[0, :] = 2; trace[:, 0] = 1
    i, j, rev = R, M, []
    while i > 0 or j > 0:
        rev.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0: i -= 1; j -= 1
        elif t == 1: i -= 1
        else: j -= 1
    path = np.array(rev[::-1], np.int32).reshape(-1, 2)
    if transposed:
        path = path[:, ::-1].copy()
    jumps = np.full(R, -1, np.int32)
    for r, t in path:
        if 0 <= r < R and jumps[r] < 0:
            jumps[r] = t
    return jumps, path


def dtw_scalar(A):
    """the literal loop: j outer, i inner, f32"""
    A = np.asarray(A, np.float32)
    R, M = A.shape
    f32 = np.float32
    D = np.full((R + 1, M + 1), np.inf, f32); D[0, 0] = 0
    trace = np.zeros((R + 1, M + 1), np.int8)
    for j in range(1, M + 1):
        for i in range(1, R + 1):
            c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
            if c0 < c1 and c0 < c2: c, t = c0, 0
            elif c1 < c0 and c1 < c2: c, t = c1, 1
            else: c, t = c2, 2
            D[i, j] = f32(-A[i - 1, j - 1]) + c
            trace[i, j] = t
    return _backtrace(trace, R, M)


def dtw_f32(A, wrong=None):
    """the same recurrence swept over anti-diagonals (vector operations over the cells of a diagonal, every one an f32 operation).
    wrong: 'tie_le' (<= in place of < in the tie rule), 'transposed' (the path's columns swapped)"""
    A = np.asarray(A, np.float32)
    R, M = A.shape
    D = np.full((R + 1, M + 1), np.inf, np.float32); D[0, 0] = 0
    trace = np.zeros((R + 1, M + 1), np.int8)
    C = -A
    for d in range(2, R + M + 1):
        i = np.arange(max(1, d - M), min(R, d - 1) + 1)
        j = d - i
        c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
        if wrong == "tie_le":
            s0 = (c0 <= c1) & (c0 <= c2); s1 = ~s0 & (c1 <= c0) & (c1 <= c2)
        else:
            s0 = (c0 < c1) & (c0 < c2); s1 = ~s0 & (c1 < c0) & (c1 < c2)
        best = np.where(s0, c0, np.where(s1, c1, c2))
        D[i, j] = C[i - 1, j - 1] + best
        trace[i, j] = np.where(s0, 0, np.where(s1, 1, 2))
    return _backtrace(trace, R, M, transposed=wrong == "transposed")


def hold_path(A, jumps, path, what=None):
    """exact: the jumps and the whole path an implementation wrote for A are dtw_f32's"""
    ej, ep = dtw_f32(A)
    path = np.asarray(path).reshape(-1, 2)
    assert path.shape == ep.shape and (path == ep).all(), (what, "path", path.shape, ep.shape)
    assert (np.asarray(jumps) == ej).all(), (what, "jumps")


# ------------------------------------------------------------------------------------------------ operands
def hadamard64():
    h = np.array([[1.0]])
    while h.shape[0] < 64:
        h = np.block([[h, h], [h, -h]])
    return h


@dataclasses.dataclass
class Case:
    """the operands of one wmi_selftest_dtw_matrix call: q [L][n][S], k [L][T][S] f16, the keys [M, T) poisoned"""
    family: str
    name: str
    L: int
    S: int
    H: int
    n: int
    n_sot: int
    M: int
    T: int
    q: np.ndarray
    k: np.ndarray
    pairs: list
    starts: list = None          # bands: the first frame of every band
    _memo: dict = dataclasses.field(default_factory=dict)

    @property
    def R(self):
        return self.n - self.n_sot - 1

    def operands(self, pairs=None, keys=None):
        """per pair: (q [n][64], k [keys][64])"""
        pairs = self.pairs if pairs is None else pairs
        keys = self.M if keys is None else keys
        return ([self.q[l][:, 64 * h:64 * h + 64] for l, h in pairs], [self.k[l][:keys, 64 * h:64 * h + 64] for l, h in pairs])

    def expected(self):
        if "A" not in self._memo:
            self._memo["A"] = matrix_f64(*self.operands(), self.n_sot)
        return self._memo["A"]


def _poison(rows, S):
    r, c = np.meshgrid(np.arange(rows), np.arange(S), indexing="ij")
    return np.where((r + c) & 1, -POISON, POISON).astype(np.float16)


def random_case(name, S, H, n, n_sot, M, T, pairs, seed, L=None):
    L = L if L is not None else max(l for l, _ in pairs) + 1
    rng = np.random.default_rng(seed)
    # q . k over 64 standard normal products has deviation 8: scale both by sqrt(SPREAD / 8)
    g = np.sqrt(SPREAD / 8.0)
    q = (rng.standard_normal((L, n, S)) * g).astype(np.float16)
    k = (rng.standard_normal((L, T, S)) * g).astype(np.float16)
    k[:, M:] = _poison(T - M, S)
    c = Case("random", name, L, S, H, n, n_sot, M, T, q, k, list(pairs))
    if M > 1:                                                 # the floor the family promises (M = 1: sigma is exactly 0, z exactly 0)
        for qq, kk in zip(*c.operands()):
            s = qq.astype(np.float64) @ kk.astype(np.float64).T
            w = np.exp(s - s.max(-1, keepdims=True)); w /= w.sum(-1, keepdims=True)
            assert (w.std(0) > SIGMA_FLOOR * w.mean(0)).all(), (name, "a column's sigma is below the floor")
    return c


def band_case(name, S, H, n, n_sot, M, T, pairs, seed, L=None):
    """R bands of >= 7 frames, monotone, covering [0, M); needs R <= 63 and M >= 7 R"""
    L = L if L is not None else max(l for l, _ in pairs) + 1
    R = n - n_sot - 1
    assert R <= 63 and M >= 7 * R
    rng = np.random.default_rng(seed)
    extra = np.sort(rng.integers(0, R, M - 7 * R))
    widths = 7 + np.bincount(extra, minlength=R)
    starts = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(int)
    band = np.repeat(np.arange(R), widths)
    code = hadamard64()[1:]                                   # (row 0 is all ones: left to nobody)
    q = np.zeros((L, n, S), np.float16); k = np.zeros((L, T, S), np.float16)
    for l in range(L):
        for h in range(H):
            k[l, :M, 64 * h:64 * h + 64] = 4 * code[band]
            q[l, n_sot:n_sot + R, 64 * h:64 * h + 64] = 4 * code[np.arange(R)]
    k[:, M:] = _poison(T - M, S)
    return Case("bands", name, L, S, H, n, n_sot, M, T, q, k, list(pairs), starts=list(starts))


def tie_matrices():
    """integer-valued matrices: (name, A)"""
    rng = np.random.default_rng(7)
    out = []
    for R, M in ((1, 1), (1, 5), (5, 1), (4, 9), (9, 4), (12, 12), (30, 50)):
        out.append((f"zeros {R}x{M}", np.zeros((R, M), np.float32)))
        out.append((f"ints {R}x{M}", rng.integers(-2, 3, (R, M)).astype(np.float32)))
        out.append((f"two-valued {R}x{M}", rng.integers(0, 2, (R, M)).astype(np.float32)))
    return out


def path_matrix(family, R, M, seed=0):
    """an A [R][M] of the family for the path tests (bands: a staircase where it fits, i.e. M >= R; otherwise the transposed staircase)"""
    rng = np.random.default_rng(seed + 1000 * R + M)
    if family == "ties":
        return rng.integers(-1, 2, (R, M)).astype(np.float32)
    if family == "random":
        return rng.standard_normal((R, M)).astype(np.float32)
    A = np.full((R, M), -0.25, np.float32)
    if M >= R:
        edges = np.linspace(0, M, R + 1).astype(int)
        for r in range(R):
            A[r, edges[r]:edges[r + 1]] = 2.0
    else:
        edges = np.linspace(0, R, M + 1).astype(int)
        for t in range(M):
            A[edges[t]:edges[t + 1], t] = 2.0
    return A


def staircase_jumps(R, M):
    """path_matrix('bands', R, M)'s closed form where M >= R: the band starts"""
    return np.linspace(0, M, R + 1).astype(int)[:-1]

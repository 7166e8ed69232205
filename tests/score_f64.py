"""The text scorer in float64: the judge of wmi_score_texts (no device, no library).

Definition (include/wmi_device.h).  A scored row has RAW f32 logits l and a target t.  The vocabulary is cut into
blocks of BLOCK entries; a block keeps m_b = max l and s_b = sum exp(l - m_b), the DIFFERENCE in f32, exp and sums in float64, an entry of
-inf adding 0 (the block pass of the no-speech head, tests/no_speech_f64.py); the blocks are combined in ascending order, M = max m_b,
S = sum_b s_b exp(f32(m_b - M)); lp = f32(f64(f32(l[t] - M)) - log(S)), rounded to f32 once; l[t] = -inf gives -inf.  `spec_lp` restates it
with numpy and returns the float64 value in front of that one rounding.

Bound A (per value).  What the restatement leaves free is what the definition leaves free: the order of the float64 additions inside a
block's 64 lanes and the last bit of a float64 exp / log.  Those move the float64 value by ~1e-13 at most (some hundred terms of relative
2^-53 each), far below an f32 ulp of any |lp| >= 1e-3 — the crafted cases keep |lp| there or make it exactly 0.  So a correct kernel's
result is the float64 value rounded once (half an ulp, counted as one), give or take one f32 ulp for a double exp / log that is not
correctly rounded: the judge holds ULPS = 2 f32 ulp at the value, exactly -inf where the target is -inf, exactly 0 where the value is 0.

Bound B (the defined form against the plain float64 log-soft-max `exact_lp`).  The definition takes l[t] - M in f32: relative 2^-24, i.e.
2^-24 |l[t] - M| of lp.  The same rounding of the differences inside the denominator moves log S by at most 2^-24 E|d| under the soft-max
(first order: d log S = sum p_i d_i eps_i), once for l - m_b and once for m_b - M, and E|d| = E[M - l] <= ln n for a soft-max over n entries.
bound_b = 2^-24 (|l[t] - M| + 2 ln n + 1); the leading term is the one the target contributes.

Per text: sum_logprob = the sum of its lp in float64 in ascending row order (exact here: a Python float loop), avg = sum / count,
posterior = exp(v_c - max v) / sum_c exp(v_c - max v) in float64 over the texts in ascending order, rounded to f32; v = sum or (length_norm)
sum / count; v = -inf gives 0; all -inf gives 0 everywhere, never NaN.

The plan (csrc/score.cpp: score_plan) and the cache's mask rule are restated at the bottom.
"""
import math

import numpy as np

BLOCK = 128
ULPS = 2


def describe_bounds() -> str:
    return (f"bound A: {ULPS} f32 ulp at the float64 value (one rounding by the definition + one ulp for a double exp / log that is not "
            f"correctly rounded); bound B: 2^-24 (|l[t] - M| + 2 ln n + 1) between the defined form and the plain float64 log-soft-max")


print(describe_bounds())


# ---------------------------------------------------------------------------------------------- one row
def spec_parts(l, block: int = BLOCK):
    """(M f32, S float64) of the definition"""
    l = np.asarray(l, np.float32)
    ms, ss = [], []
    for b0 in range(0, l.size, block):
        v = l[b0:b0 + block]
        m = np.float32(v.max())
        fin = v[v != -np.inf]
        with np.errstate(invalid="ignore"):
            d = (fin - m).astype(np.float32)
        ss.append(math.fsum(np.exp(d.astype(np.float64))) if fin.size else 0.0)
        ms.append(m)
    M = np.float32(max(ms))
    S = 0.0
    for m, s in zip(ms, ss):                                  # ascending block order
        if s > 0.0:
            S += s * math.exp(float(np.float32(m - M)))
    return M, S


def spec_lp(l, t: int, block: int = BLOCK) -> float:
    l = np.asarray(l, np.float32)
    if l[t] == -np.inf:
        return -math.inf
    M, S = spec_parts(l, block)
    return float(np.float32(l[t] - M)) - math.log(S)


def exact_lp(l, t: int) -> float:
    """the log-soft-max with every difference in float64 (not the definition: bound B)"""
    l = np.asarray(l, np.float32).astype(np.float64)
    if l[t] == -np.inf:
        return -math.inf
    fin = l[l != -np.inf]
    m = fin.max()
    return (l[t] - m) - math.log(math.fsum(np.exp(fin - m)))


def bound_b(l, t: int) -> float:
    l = np.asarray(l, np.float32).astype(np.float64)
    fin = l[l != -np.inf]
    return 2.0 ** -24 * (abs(l[t] - fin.max()) + 2.0 * math.log(l.size) + 1.0)


def ulps_off(got, want: float) -> float:
    """distance of an f32 result from the float64 value in f32 ulp at that value (inf for a NaN or a wrong infinity)"""
    g = float(np.float32(got))
    if g != g:
        return math.inf
    if math.isinf(want) or math.isinf(g):
        return 0.0 if g == want else math.inf
    if want == 0.0:
        return 0.0 if g == 0.0 else math.inf
    return abs(g - want) / float(np.spacing(np.float32(abs(want))))


def judge_lp(got, l, t: int) -> bool:
    return ulps_off(got, spec_lp(l, t)) <= ULPS


# ---------------------------------------------------------------------------------------------- the texts of a call
def text_scores(lp, first, length_norm: bool = False):
    """lp: the per-token values as returned (f32); first [n_texts + 1].  -> [(sum float64, avg f32, posterior f32, n_scored, first)]"""
    lp = np.asarray(lp, np.float32)
    sums, vs = [], []
    for c in range(len(first) - 1):
        s = 0.0
        for x in lp[first[c]:first[c + 1]]:
            s += float(x)
        sums.append(s)
        vs.append(s / (first[c + 1] - first[c]) if length_norm else s)
    vmax = max(vs)
    den = 0.0
    for v in vs:
        if v != -math.inf:
            den += math.exp(v - vmax)
    out = []
    for c, (s, v) in enumerate(zip(sums, vs)):
        post = np.float32(math.exp(v - vmax) / den) if (v != -math.inf and den > 0.0) else np.float32(0.0)
        out.append((s, np.float32(s / (first[c + 1] - first[c])), post, first[c + 1] - first[c], first[c]))
    return out


def judge_texts(recs, lp, first, length_norm: bool = False) -> bool:
    """recs: [(sum, avg, posterior, n_scored, first)] as the call returned them — exactly the recomputation from the returned lp"""
    want = text_scores(lp, first, length_norm)
    if len(recs) != len(want):
        return False
    for g, w in zip(recs, want):
        same_sum = (g[0] == w[0]) or (math.isinf(w[0]) and g[0] == w[0])
        if not same_sum or g[0] != g[0]:
            return False
        for a, b in ((g[1], w[1]), (g[2], w[2])):
            if np.float32(a) != np.float32(a) or np.float32(a).view(np.uint32) != np.float32(b).view(np.uint32):
                if not (float(a) == 0.0 and float(b) == 0.0):
                    return False
        if (int(g[3]), int(g[4])) != (int(w[3]), int(w[4])):
            return False
    return True


# ---------------------------------------------------------------------------------------------- the plan
def special_ids(n_vocab: int) -> dict:
    """the loader's special tokens (W/whisper.cpp:365-394 and the shifts for multilingual / 100-language files)"""
    ml = n_vocab >= 51865
    dt = (n_vocab - 51765 - 1) - 98 if ml else 0
    return dict(eot=50256 + ml, sot=50257 + ml, translate=50357 + dt, transcribe=50358 + dt, prev=50360 + dt, notimestamps=50362 + dt, multilingual=ml,
                n_lang=(n_vocab - 51765 - 1) if ml else 99)


def plan(n_vocab: int, n_text_ctx: int, texts, prompt=(), lang_id: int = 0, translate: bool = False, with_eot: bool = True, kv_cells=None):
    """-> None for a refused call, else dict(prefix, first, prefix_target, rows=[(pass, token, pos, seq, flag, target, place)], pass_text0)"""
    ids = special_ids(n_vocab)
    kv_cells = 3 * n_text_ctx if kv_cells is None else kv_cells
    if len(texts) < 1 or len(texts) > 4096:
        return None
    prefix = []
    if len(prompt) > 0:
        take = list(prompt)[-min(n_text_ctx // 2 - 1, len(prompt)):]
        if any(t < 0 or t >= n_vocab for t in take):
            return None
        prefix += [ids["prev"]] + take
    prefix.append(ids["sot"])
    if ids["multilingual"]:
        if lang_id < 0 or lang_id >= ids["n_lang"]:
            return None
        prefix += [ids["sot"] + 1 + lang_id, ids["translate"] if translate else ids["transcribe"]]
    prefix.append(ids["notimestamps"])
    P = len(prefix)
    for y in texts:
        if (len(y) == 0 and not with_eot) or len(y) > n_text_ctx - P or any(t < 0 or t >= ids["eot"] for t in y):
            return None
    cap = min(n_text_ctx, kv_cells - P)
    first, prefix_target, rows, pass_text0 = [0], [], [], [0]
    in_pass = 0
    for c, y in enumerate(texts):
        n_rows = len(y) if with_eot else len(y) - 1
        if n_rows > cap:
            return None
        if in_pass + n_rows > cap:
            pass_text0.append(c); in_pass = 0
        f = first[-1]
        prefix_target.append(y[0] if len(y) else ids["eot"])
        for i in range(n_rows):
            rows.append((len(pass_text0) - 1, y[i], P + i, c + 1, 1, y[i + 1] if i + 1 < len(y) else ids["eot"], f + 1 + i))
        in_pass += n_rows
        first.append(f + 1 + n_rows)
    pass_text0.append(len(texts))
    return dict(prefix=prefix, first=first, prefix_target=prefix_target, rows=rows, pass_text0=pass_text0)


def sees(cell_seqs, cell_pos: int, seq: int, pos: int) -> bool:
    """the unified self cache's mask rule (csrc/device.cpp decode()): a row of sequence `seq` at position `pos` attends a cell iff
    has(seq) && cell position <= pos"""
    return seq in cell_seqs and cell_pos <= pos


def plan_cells(pl, i_pass: int):
    """the cache cells a pass's rows can meet: the prefix (sequence 0 copied to the pass's texts) and the pass's own rows.
    -> [(seqs, pos, owner text or -1)]"""
    P = len(pl["prefix"])
    c0, c1 = pl["pass_text0"][i_pass], pl["pass_text0"][i_pass + 1]
    cells = [({0} | {c + 1 for c in range(c0, c1)}, p, -1) for p in range(P)]
    cells += [({r[3]}, r[2], r[3] - 1) for r in pl["rows"] if r[0] == i_pass]
    return cells

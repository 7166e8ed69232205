"""The judge of the draft verifier: a plain restatement of the rule of DESIGN.md §5 ("Verify a draft in one decoder pass"), independent of
the product's code.  Given the model's constants, the call's parameters, the prompt length P, the draft and — where an outcome is judged —
the filtered greedy pick of every logits row, it says what a drafted window must look like:

  clip        n = min(n_offered, n_max - 1, max_tokens + 1 if max_tokens > 0, n_text_ctx - P - 1), n_max = n_text_ctx / 2 - 4; n <= 0: nothing
  rows        logits row j (j = 0 .. n) is batch row P - 1 + j and predicts token j
  records     row j is filtered as the step of a decoder whose tokens so far are draft[0 .. j): the blank ban on row 0 only, the two
              timestamp-history flags from draft[j - 1] and draft[j - 2], ts_floor_end from the state machine's has_ts / seek_delta after
              draft[0 .. j), ts_initial_start on row 0 only
  accept      a = the largest a <= n with pick_j == draft[j] for all j < a
  tokens      pick_0 .. pick_a (a accepted tokens and the one the pass gives for free), replayed through the per-token state machine as
              if each had just been sampled at iteration i; the replay stops at the first token that completes or fails the decoder

judge() compares an answer with that and returns the list of its complaints (empty: the answer is right)."""
import math
from dataclasses import dataclass, field

import numpy as np

CHUNK = 3000                                     # a window's seek_delta without timestamps: 100 * WHISPER_CHUNK_SIZE


@dataclass(frozen=True)
class Model:
    n_vocab: int
    eot: int
    beg: int
    n_text_ctx: int
    n_audio_ctx: int
    space_id: int = -1


@dataclass(frozen=True)
class Params:
    suppress_blank: bool = True
    max_initial_ts: float = 1.0
    max_tokens: int = 0
    single_segment: bool = False


@dataclass
class Dec:
    tokens: list = field(default_factory=list)
    has_ts: bool = False
    seek_delta: int = CHUNK
    result_len: int = 0
    completed: bool = False
    failed: bool = False


def n_max(m: Model) -> int:
    return m.n_text_ctx // 2 - 4


def clip(m: Model, p: Params, P: int, n_offered: int) -> int:
    n = min(n_offered, n_max(m) - 1, m.n_text_ctx - P - 1)
    if p.max_tokens > 0:
        n = min(n, p.max_tokens + 1)
    return max(0, n)


def advance(m: Model, p: Params, d: Dec, i: int, seek: int, seek_end: int):
    """the state machine on d.tokens[-1], sampled at iteration i"""
    tok = d.tokens[-1]
    if tok > m.beg:
        sd = 2 * (tok - m.beg)
        if d.has_ts and d.seek_delta > sd and d.result_len < i:
            d.failed = True
            return
        d.seek_delta, d.result_len, d.has_ts = sd, i + 1, True
    if tok == m.eot or (p.max_tokens > 0 and i >= p.max_tokens) or (d.has_ts and seek + d.seek_delta + 100 >= seek_end):
        if d.result_len == 0:
            if seek + d.seek_delta + 100 >= seek_end:
                d.result_len = i + 1
            else:
                d.failed = True
                return
        if p.single_segment:
            d.result_len, d.seek_delta = i + 1, CHUNK
        d.completed = True
        return
    if i == n_max(m) - 1 and (d.result_len == 0 or d.seek_delta < CHUNK // 2):
        d.failed = True


def record(m: Model, p: Params, d: Dec) -> dict:
    """the step record of the token a decoder in state d samples next"""
    h = d.tokens
    initial = len(h) == 0
    flags = (1 if (p.suppress_blank and initial) else 0) | (2 if (h and h[-1] >= m.beg) else 0) | (4 if (len(h) < 2 or h[-2] >= m.beg) else 0)
    ts_initial_start = m.n_vocab
    if initial and p.max_initial_ts > 0.0:
        precision = np.float32(30.0) / np.float32(m.n_audio_ctx)
        q = float(np.float32(p.max_initial_ts) / precision)
        ts_initial_start = m.beg + int(math.floor(q + 0.5)) + 1
    return {"flags": flags, "space_id": m.space_id, "eot": m.eot, "beg": m.beg, "n_vocab": m.n_vocab,
            "ts_floor_end": m.beg + d.seek_delta // 2 if d.has_ts else m.beg, "ts_initial_start": ts_initial_start}


@dataclass
class Plan:
    n: int
    logit_rows: list
    records: list
    states: list                                  # per row: (history, has_ts, seek_delta) — what wmi_selftest_filters builds a record from


def plan(m: Model, p: Params, P: int, draft, seek=0, seek_end=CHUNK) -> Plan:
    n = clip(m, p, P, len(draft))
    d = Dec()
    recs, states = [], []
    for j in range(n + 1):
        recs.append(record(m, p, d))
        states.append((list(d.tokens), d.has_ts, d.seek_delta))
        if j == n:
            break
        d.tokens.append(int(draft[j]))
        if not d.completed and not d.failed:
            advance(m, p, d, j, seek, seek_end)
    return Plan(n, [P - 1 + j for j in range(n + 1)], recs, states)


def accept_len(picks, draft, n) -> int:
    a = 0
    while a < n and int(picks[a]) == int(draft[a]):
        a += 1
    return a


def replay(m: Model, p: Params, picks, a: int, seek=0, seek_end=CHUNK):
    """tokens 0 .. a through the state machine -> (the tokens consumed, the decoder behind them)"""
    d = Dec()
    for i in range(a + 1):
        d.tokens.append(int(picks[i]))
        advance(m, p, d, i, seek, seek_end)
        if d.completed or d.failed:
            break
    return list(d.tokens), d


def answer(m: Model, p: Params, P: int, draft, picks, seek=0, seek_end=CHUNK) -> dict:
    """the right answer, in the form judge() takes"""
    pl = plan(m, p, P, draft, seek, seek_end)
    if pl.n <= 0:
        return {"n": 0, "logit_rows": [], "records": [], "a": 0, "tokens": []}
    a = accept_len(picks, draft, pl.n)
    toks, _ = replay(m, p, picks, a, seek, seek_end)
    return {"n": pl.n, "logit_rows": pl.logit_rows, "records": pl.records, "a": a, "tokens": toks}


def judge(m: Model, p: Params, P: int, draft, picks, ans: dict, seek=0, seek_end=CHUNK) -> list:
    want = answer(m, p, P, draft, picks, seek, seek_end)
    bad = []
    if ans["n"] != want["n"]:
        bad.append(f"n = {ans['n']}, the clip gives {want['n']}")
        return bad
    if list(ans["logit_rows"]) != want["logit_rows"]:
        bad.append("logits rows")
    if len(ans["records"]) != len(want["records"]):
        bad.append(f"{len(ans['records'])} records for {len(want['records'])} rows")
    else:
        for j, (g, w) in enumerate(zip(ans["records"], want["records"])):
            for k in w:
                if g[k] != w[k]:
                    bad.append(f"row {j}: {k} = {g[k]}, its history gives {w[k]}")
    if ans["a"] != want["a"]:
        bad.append(f"accepted {ans['a']}, the longest matching prefix is {want['a']}")
    if list(ans["tokens"]) != want["tokens"]:
        bad.append(f"tokens {list(ans['tokens'])}, the pass gives {want['tokens']}")
    return bad


STEP_WORDS = {"flags": 4, "space_id": 5, "eot": 6, "beg": 7, "n_vocab": 8, "ts_floor_end": 9, "ts_initial_start": 10}


def record_of_words(w) -> dict:
    """a DecStep as 16 int32 words -> the fields the filters read"""
    return {k: int(w[i]) for k, i in STEP_WORDS.items()}


def words_of_record(r: dict, seq=1) -> np.ndarray:
    w = np.zeros(16, np.int32)
    for k, i in STEP_WORDS.items():
        w[i] = r[k]
    w[11] = seq
    return w

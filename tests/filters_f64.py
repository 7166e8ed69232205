"""The logit filters, the greedy pick and the draws restated in float64 (plain numpy), and the crafted cases the filter tests run.

What is restated: whisper_process_logits (W/whisper.cpp:4493-4775) and the statistics of whisper_sample_token / _topk (:4777-4909) as
csrc/host_logic.cpp defines them for the product — from the raw logits, the static ban set (derived here from the vocabulary's token
strings, not from the product's byte mask) and the step-filter fields (derived here from parameters and history):

    allowed set . log-probabilities and probabilities . "the timestamp mass beats every text token" . the greedy id with the
    first-index tie-break . tid, pt, ptsum . the CDF over the probabilities and the id of a draw u = first i with cdf(i) >= u * total

tests/test_filters_f64.py proves it against the host definition (wmi_process_logits) on every case below, without a GPU;
tests/test_gpu_filters.py holds the three device copies of the predicate (csrc/k_sample.hip, csrc/k_dec.hip) to both.

The case generator works in the domain BEHIND the temperature division: a pattern states its offsets there and the raw logits are the
design times the temperature, so a case keeps its decision at every temperature.  Every case has a name and its decision gaps
(Ref.gaps); the conditions the GPU tests rely on are asserted by check_conditions():

    greedy winner exactly tied with the runner-up or ahead by >= WIN_GAP (1e-2) . |timestamp log-mass - best text log-prob| >= MASS_GAP
    (5e-2) . top timestamp exactly tied or ahead by >= WIN_GAP . a probability that must be positive is >= e^-60 (POS), one that must
    be zero sits >= 150 below the maximum (ZERO); f32 denormals lie between and are not pinned."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

# geometry of the device passes: where positions are placed, never what the yardstick computes
NB = 64                      # workgroups of k_filter_stats / k_prob_blocks; block b covers [b * per, (b + 1) * per)
NT = 256                     # their threads: element e of thread t in block b is b * per + e * NT + t (waves of 64 threads)
FUSED_ROWS = 32              # rows a workgroup of the fused vocabulary projection produces per tile (4 wavefronts x 8 rows)
FUSED_PARTS = 768            # its workgroup cap: the tiles of a workgroup are FUSED_PARTS * FUSED_ROWS rows apart

WIN_GAP, MASS_GAP, POS, ZERO = 1e-2, 5e-2, -60.0, -150.0

NON_SPEECH = ["\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
              "「", "」", "『", "』", "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))", "[[", "]]",
              "{{", "}}", "♪♪", "♪♪♪", "♩", "♪", "♫", "♬", "♭", "♮", "♯"]


def per_block(nv):
    return -(-nv // NB)


def lane_run(nv):
    return -(-per_block(nv) // 64)


@dataclass
class Vocab:
    n_vocab: int
    eot: int
    sot: int
    translate: int
    transcribe: int
    solm: int
    prev: int
    nosp: int
    not_: int
    beg: int
    n_langs: int
    n_audio_ctx: int
    token_to_id: dict = field(repr=False, default_factory=dict)

    @property
    def space_id(self):
        return self.token_to_id.get(b" ", -1)


def vocab_of(lib, ctx) -> Vocab:
    nv = lib.whisper_n_vocab(ctx)
    t2i = {}
    for i in range(nv):
        t2i[lib.whisper_token_to_str(ctx, i)] = i          # a later id replaces an earlier one, as in the loader's map
    g = lambda n: int(getattr(lib, "whisper_token_" + n)(ctx))
    return Vocab(nv, g("eot"), g("sot"), g("translate"), g("transcribe"), g("solm"), g("prev"), g("nosp"), g("not"), g("beg"),
                 lib.whisper_lang_max_id() + 1, lib.whisper_n_audio_ctx(ctx), t2i)


# ------------------------------------------------------------------------------------------------ filter states
@dataclass(frozen=True)
class State:
    """A filter state, reached through parameters and history.  hist: "x" a text token, "t" a timestamp (beg + 10)."""
    name: str
    hist: str = "xx"
    has_ts: bool = False
    seek_delta: int = 0
    suppress_blank: bool = True
    max_initial_ts: float = 1.0
    no_timestamps: bool = False
    non_speech: bool = False
    tdrz: bool = False

    def history(self, v: Vocab):
        return [1000 + 1000 * i if c == "x" else v.beg + 10 for i, c in enumerate(self.hist)]

    def params(self, lib, strategy=0):
        p = lib.whisper_full_default_params(strategy)
        p.suppress_blank = self.suppress_blank; p.max_initial_ts = self.max_initial_ts; p.no_timestamps = self.no_timestamps
        p.suppress_non_speech_tokens = self.non_speech; p.tdrz_enable = self.tdrz
        return p


STATES = [
    State("initial", hist=""),
    State("initial max_initial_ts=0", hist="", max_initial_ts=0.0),
    State("initial no suppress_blank", hist="", suppress_blank=False),
    State("[ts]", hist="t"),
    State("[text,ts]", hist="xt"),
    State("[ts,ts]", hist="tt"),
    State("[ts,text]", hist="tx"),
    State("[text,text]", hist="xx"),
    State("has_ts seek 0", has_ts=True, seek_delta=0),
    State("has_ts seek 2", has_ts=True, seek_delta=2),
    State("has_ts seek 1500", has_ts=True, seek_delta=1500),
    State("has_ts seek 3000", has_ts=True, seek_delta=3000),
    State("[text,ts] has_ts seek 0", hist="xt", has_ts=True, seek_delta=0),
    State("[text,ts] has_ts seek 2", hist="xt", has_ts=True, seek_delta=2),
    State("[text,ts] has_ts seek 1500", hist="xt", has_ts=True, seek_delta=1500),
    State("[text,ts] has_ts seek 3000", hist="xt", has_ts=True, seek_delta=3000),
    State("no_timestamps", no_timestamps=True),
    State("non-speech suppressed", non_speech=True),
    State("tdrz", tdrz=True),
    State("tdrz non-speech initial", hist="", tdrz=True, non_speech=True),
]
STATE = {s.name: s for s in STATES}
# the states the wider vocabularies and the wider projections repeat
REDUCED_STATES = ["initial", "[text,ts]", "[text,text]", "has_ts seek 1500", "no_timestamps", "tdrz non-speech initial"]
WIDE_STATES = ["initial", "[text,ts]", "has_ts seek 1500"]


def static_ban(v: Vocab, st: State) -> np.ndarray:
    ban = np.zeros(v.n_vocab, bool)

    def B(i):
        if 0 <= i < v.n_vocab:
            ban[i] = True
    for i in (v.not_, v.sot, v.nosp, v.translate, v.transcribe, v.prev):
        B(i)
    if not st.tdrz:
        B(v.solm)
    for i in range(v.n_langs):
        B(v.sot + 1 + i)
    if st.no_timestamps:
        ban[v.beg:] = True
    if st.non_speech:
        for t in NON_SPEECH:
            for f in (t, " " + t):
                B(v.token_to_id.get(f.encode("utf-8"), -1))
        for f in (" -", " '"):
            B(v.token_to_id.get(f.encode("utf-8"), -1))
    return ban


def rule_allowed(v: Vocab, st: State) -> np.ndarray:
    """the entries the rules leave (static ban and step fields), before a look at the logits"""
    a = ~static_ban(v, st)
    h = st.history(v)
    if st.suppress_blank and not h:
        a[v.eot] = False
        if v.space_id >= 0:
            a[v.space_id] = False
    last_ts = bool(h) and h[-1] >= v.beg
    penult_ts = len(h) < 2 or h[-2] >= v.beg
    if last_ts:
        if penult_ts:
            a[v.beg:] = False
        else:
            a[:v.eot] = False
    if not h and st.max_initial_ts > 0:
        precision = np.float32(30.0) / np.float32(v.n_audio_ctx)
        tid0 = int(np.round(np.float32(st.max_initial_ts) / precision))
        a[v.beg + tid0 + 1:] = False
    if st.has_ts:
        a[v.beg:v.beg + st.seek_delta // 2] = False
    return a


# ------------------------------------------------------------------------------------------------ the yardstick
@dataclass
class Ref:
    allowed: np.ndarray          # bool [n_vocab]: what the filters leave
    cand: np.ndarray             # ... and what is left to pick from: the allowed timestamps when one is forced (the host clears the text)
    logprobs: np.ndarray         # float64, -inf outside the allowed set (text NOT cleared when a timestamp is forced: see probs)
    probs: np.ndarray            # float64, text cleared when a timestamp is forced
    force_ts: bool
    id: int
    tid: int                     # with tid_default 0 (the greedy pick and the single draw); draws(): tid_default
    ts_positive: bool            # the top timestamp's probability counts as > 0
    pt: float
    ptsum: float
    gaps: dict

    @property
    def p(self):
        return float(self.probs[self.id])

    @property
    def plog(self):
        return float(self.logprobs[self.id])

    def pick(self, tid_default=0):
        return self.token(self.id, tid_default)

    def token(self, i, tid_default=0):
        """(id, tid, p, plog, pt, ptsum) of token i as sample_token / sample_token_topk report it"""
        tid = self.tid if self.ts_positive else tid_default
        pt = self.pt
        if i >= self._beg:
            tid, pt = i, float(self.probs[i])
        return int(i), int(tid), float(self.probs[i]), float(self.logprobs[i]), float(pt), float(self.ptsum)

    def cdf(self):
        """indices with p > 0 and the running sum of their probabilities"""
        idx = np.flatnonzero(self.probs > 0)
        return idx, np.cumsum(self.probs[idx])

    def draw(self, u):
        idx, c = self.cdf()
        j = int(np.searchsorted(c, u * c[-1], side="left"))
        return int(idx[min(j, idx.size - 1)])

    def cell_mid(self, i):
        """the uniform number in the middle of token i's cell of the CDF"""
        idx, c = self.cdf()
        j = int(np.searchsorted(idx, i)); assert idx[j] == i
        lo = c[j - 1] if j > 0 else 0.0
        return float(0.5 * (lo + c[j]) / c[-1])


def _lse(x):
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def evaluate(raw: np.ndarray, v: Vocab, st: State, temperature: float) -> Ref:
    l = raw.astype(np.float64)
    if temperature > 0:
        l = l / np.float64(np.float32(temperature))
    allowed = rule_allowed(v, st) & (l > -np.inf)
    assert allowed.any()
    lf = np.where(allowed, l, -np.inf)
    lse = _lse(lf[allowed])
    logprobs = lf - lse
    ts, tx = allowed.copy(), allowed.copy()
    ts[:v.beg] = False; tx[v.beg:] = False
    ts_mass = _lse(logprobs[ts]) if ts.any() else -np.inf
    max_text = float(logprobs[tx].max()) if tx.any() else -np.inf
    force = ts_mass > max_text
    cand = ts if force else allowed
    probs = np.where(cand, np.exp(logprobs), 0.0)
    cl = np.where(cand, lf, -np.inf)
    i = int(np.argmax(cl))                                   # first index of the maximum
    srt = np.sort(cl[cand])
    gaps = {"winner": float(srt[-1] - srt[-2]) if srt.size > 1 else np.inf,
            "mass": abs(ts_mass - max_text) if np.isfinite(ts_mass) and np.isfinite(max_text) else np.inf,
            "p": float(logprobs[i]), "ts_top": np.inf, "ts_p": None}
    tid, pt, ptsum, ts_pos = 0, 0.0, 0.0, False
    if ts.any():
        tl = np.where(ts, lf, -np.inf)
        j = int(np.argmax(tl))
        s = np.sort(tl[ts])
        gaps["ts_top"] = float(s[-1] - s[-2]) if s.size > 1 else np.inf
        gaps["ts_p"] = float(logprobs[j])
        ptsum = float(np.exp(logprobs[ts]).sum())
        if logprobs[j] > 0.5 * (POS + ZERO):
            ts_pos, tid, pt = True, j, float(np.exp(logprobs[j]) / (ptsum + 1e-10))
    r = Ref(allowed, cand, logprobs, probs, bool(force), i, tid, ts_pos, pt, ptsum, gaps)
    r._beg = v.beg
    return r


def check_conditions(r: Ref, name):
    """the conditions on the inputs (module docstring): with them no comparison needs an escape hatch"""
    g = r.gaps
    assert g["winner"] == 0.0 or g["winner"] >= WIN_GAP, (name, g)
    assert g["mass"] >= MASS_GAP, (name, g)
    assert g["ts_top"] == 0.0 or g["ts_top"] >= WIN_GAP, (name, g)
    assert g["p"] >= POS, (name, g)
    assert g["ts_p"] is None or g["ts_p"] >= POS or g["ts_p"] <= ZERO, (name, g)


# ------------------------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    name: str
    state: State
    pattern: str
    temperature: float
    raw: np.ndarray              # float32 [n_vocab]
    expect: dict = field(default_factory=dict)     # what the pattern is about: {"id": ..} / {"force_ts": ..} / {"tid0": True} / {"p": ..}
    targets: list = field(default_factory=list)    # draw cases: tokens whose CDF cell a uniform number is placed in


def _near(idx, pos, side):
    """the allowed index nearest to the boundary `pos`: the last one below it (side 0) or the first one at / above it (side 1)"""
    j = int(np.searchsorted(idx, pos))
    if side == 0:
        return int(idx[j - 1]) if j > 0 else None
    return int(idx[j]) if j < idx.size else None


def boundaries(v: Vocab):
    """(label, first index of the upper side) of the boundaries of the device passes, text region then timestamp region"""
    per = per_block(v.n_vocab)
    ts_block = (v.beg // per + 1) * per
    tail = v.n_vocab // FUSED_ROWS * FUSED_ROWS if v.n_vocab % FUSED_ROWS else v.n_vocab - FUSED_ROWS
    return [("wave 0|1 of block 2", 2 * per + 64), ("element 0|1 of block 2", 2 * per + NT), ("block 0|1", per), ("block 30|31", 31 * per),
            ("fused rows 32", 20 * FUSED_ROWS), ("fused tile", FUSED_PARTS * FUSED_ROWS), ("fused tile 2", 2 * FUSED_PARTS * FUSED_ROWS),
            ("lane run", 5 * per + 7 * lane_run(v.n_vocab)),
            ("text|timestamps", v.beg), ("ts block", ts_block), ("ts wave", ts_block + 64), ("ts fused rows 32", (v.beg // 32 + 3) * 32),
            ("ragged tail", tail), ("last row", v.n_vocab - 1)]


def boundary_pairs(v: Vocab, allowed: np.ndarray):
    """per boundary the allowed indices on both sides (dropped where a side is empty or both fall on the same side of text|timestamps
    for no reason of the boundary), without duplicates"""
    idx = np.flatnonzero(allowed)
    out, seen = [], set()
    for label, pos in boundaries(v):
        a, b = _near(idx, pos, 0), _near(idx, pos, 1)
        if a is None or b is None or (a, b) in seen:
            continue
        seen.add((a, b))
        out.append((label, a, b))
    return out


TEMPS = (0.0, 0.2, 1.0)
HI = 12.0                    # a crafted winner over N(0, 1) noise: ahead by ~8, the noise still carries probabilities >= e^-20


def _settle(d, *groups):
    """random noise may leave the two largest entries of a group closer than the conditions allow: the larger one is raised (an exact tie
    is a design and stays)"""
    for g in groups:
        if g.size >= 2:
            o = g[np.argsort(d[g])[-2:]]
            if 0.0 < d[o[1]] - d[o[0]] < 0.05:
                d[o[1]] += 0.25
    return d


def _raw(design, T):
    return (design * (T if T > 0 else 1.0)).astype(np.float32)


def make_cases(v: Vocab, st: State, seed=0, temps=TEMPS, patterns=None):
    """Every (pattern, temperature) case of one state.  The tie and single-winner families do not depend on the temperature (a division
    keeps order and equality) and take the temperatures in rotation; the others take each.  A pattern that is meaningless in a state is
    left out here, by name (DROPPED lists them), never skipped at run time."""
    rule = rule_allowed(v, st)
    idx = np.flatnonzero(rule)
    txt, tss = idx[idx < v.beg], idx[idx >= v.beg]
    rng = np.random.default_rng([seed, v.n_vocab, STATES.index(st) if st in STATES else 99])
    cases, dropped = [], []
    rot = [0]

    def add(pattern, design, T=None, expect=None, targets=None):
        if patterns is not None and pattern.split(":")[0] not in patterns:
            return
        if T is None:
            T = temps[rot[0] % len(temps)]; rot[0] += 1
        cases.append(Case(f"{st.name} / {pattern} / t={T:g}", st, pattern, T, _raw(_settle(design, tss, idx), T), expect or {}, targets or []))

    noise = lambda: rng.standard_normal(v.n_vocab)
    # 1. N(0, 3^2)
    for T in temps:
        add("gauss", 3.0 * noise(), T)
    # 2. timestamp mass wins / loses: ~50 allowed timestamps 1.0 (6.0) below the best text token
    if tss.size >= 20 and txt.size >= 2:
        for T in temps:
            for nm, below, forced in (("ts-mass wins", 1.0, True), ("ts-mass loses", 6.0, False)):
                d = noise()
                d[txt[txt.size // 3]] = HI
                pick = tss[:: max(1, tss.size // 50)][:50]
                d[pick] = HI - below - 0.02 * np.arange(pick.size)       # the first one clearly the top timestamp
                d[pick[0]] += 0.02
                add(nm, d, T, {"force_ts": forced and pick.size >= 20})
    else:
        dropped.append("ts-mass wins"); dropped.append("ts-mass loses")
    # 3. exact ties of the maximum across each boundary: the first index wins
    pairs = boundary_pairs(v, rule)
    for label, a, b in pairs:
        if (a < v.beg) != (b < v.beg):
            continue                                   # a text / timestamp tie of two is not decidable: the three-way case below
        d = noise(); d[[a, b]] = HI
        add(f"tie: {label} {a}|{b}", d, None, {"id": a})
    if txt.size >= 3:
        t3 = [int(txt[1]), int(txt[txt.size // 2]), int(txt[-1])]
        d = noise(); d[t3] = HI
        add(f"tie: three text {t3}", d, None, {"id": t3[0]})
    else:
        dropped.append("tie: three text")
    if tss.size >= 3 and txt.size >= 1:
        z = [int(tss[0]), int(tss[tss.size // 2]), int(tss[-1])]
        d = noise(); d[z] = HI; d[int(txt[-1])] = HI
        add(f"tie: text {int(txt[-1])} and timestamps {z}", d, None, {"id": z[0], "force_ts": True})
    else:
        dropped.append("tie: text and timestamps")
    # 4. single winners at the edges and on both sides of each boundary
    edges = {int(idx[0]): "first allowed", int(idx[-1]): "last allowed"}
    if txt.size:
        edges.setdefault(int(txt[-1]), "last allowed text")
    if tss.size:
        edges.setdefault(int(tss[0]), "first allowed timestamp")
    for label, a, b in pairs:
        edges.setdefault(a, f"below {label}"); edges.setdefault(b, f"above {label}")
    for i, label in edges.items():
        d = noise(); d[i] = HI
        add(f"winner: {label} {i}", d, None, {"id": i})
    # 5. wide range: uniform in +-80, a few raw -inf and -1e30 entries (never the winner, never the top timestamp)
    for T in temps:
        d = rng.uniform(-80.0, 80.0, v.n_vocab)
        w = int(idx[np.argmax(d[idx])]); d[w] = 81.0
        z = None
        if tss.size:                                   # the top timestamp clear, and its probability out of the denormal range
            z = int(tss[tss.size // 2])
            if z == w and tss.size > 1:
                z = int(tss[0])
            d[tss] = np.minimum(d[tss], 60.0)
            d[z] = 61.0; d[w] = 81.0
        c = _raw(d, T)
        keep = idx[(idx != w) & (idx != (z if z is not None else -1))]
        for n, h in enumerate(rng.choice(keep, size=min(8, keep.size), replace=False) if keep.size else []):
            c[h] = -np.inf if n % 2 == 0 else np.float32(-1e30)
        if patterns is None or "wide" in patterns:
            cases.append(Case(f"{st.name} / wide / t={T:g}", st, "wide", T, c, {"id": w}))
    # 6. every timestamp 200 below the maximum: p_ts_max underflows, tid = 0 (tid_default for draws), pt = ptsum = 0
    if tss.size and txt.size:
        for T in temps:
            d = noise(); d[tss] -= 200.0; d[txt[txt.size // 2]] = HI
            add("ts underflow", d, T, {"tid0": True})
    else:
        dropped.append("ts underflow")
    # 7. all logits equal: the first allowed index, p = 1 / |allowed| (two or more timestamps: their mass beats the one best text token
    #    and a timestamp is forced; exactly one timestamp beside text: mass and best text are EQUAL, not decidable by a margin)
    if tss.size == 1 and txt.size:
        dropped.append("all equal")
    else:
        for T in temps:
            add("all equal", np.full(v.n_vocab, 1.5), T, {"flat": True})
    return cases, dropped


def make_draw_case(v: Vocab, st: State, T: float, forced=False, seed=0):
    """N(0, 1) logits (the timestamps 6 lower and one text token at 8, so that text keeps its probability; forced = True raises them by 3 instead: their mass wins and
    every text block of the CDF search is empty) with the draw targets set to 3 (p >= 1e-5 with room): the first and last token with
    p > 0, both sides of block and lane-run boundaries of the CDF search, the first positive token behind >= 2 wholly empty blocks"""
    rng = np.random.default_rng([seed, v.n_vocab, 7, int(T * 10), int(forced)])
    d = rng.standard_normal(v.n_vocab)
    if forced:
        d[v.beg:] += 3.0
    else:
        d[v.beg:] -= 6.0
        txt = np.flatnonzero(rule_allowed(v, st)[:v.beg])
        anchor = int(txt[txt.size // 2]) if txt.size else None      # one text token well above the timestamp mass, the raised targets included
        if anchor is not None:
            d[anchor] = 8.0
    r0 = evaluate(_raw(d, T), v, st, T)                       # which entries carry probability (a forced timestamp clears the text)
    idx = np.flatnonzero(r0.probs > 0)
    per, run = per_block(v.n_vocab), lane_run(v.n_vocab)
    t = {int(idx[0]), int(idx[-1])}
    blocks = np.unique(idx // per)
    for b in blocks[:-1][:3].tolist() + blocks[-3:-1].tolist():      # block boundaries with probability on both sides
        lo, hi = _near(idx, (b + 1) * per, 0), _near(idx, (b + 1) * per, 1)
        if lo is not None and hi is not None and lo // per == b:
            t.update((lo, hi))
    b = int(blocks[len(blocks) // 2])
    for L in (1, 7, 40):                                              # lane-run boundaries inside a block
        lo, hi = _near(idx, b * per + L * run, 0), _near(idx, b * per + L * run, 1)
        if lo is not None and hi is not None:
            t.update((lo, hi))
    empty_stretch = None
    full = np.zeros(NB, bool); full[blocks] = True
    for b in range(2, NB):
        if full[b] and not full[b - 1] and not full[b - 2]:
            empty_stretch = int(idx[np.searchsorted(idx, b * per)]); t.add(empty_stretch)
            break
    t = sorted(t)
    d[t] = 3.0
    if not forced and anchor is not None:
        d[anchor] = 8.0
    _settle(d, idx[idx >= v.beg], idx)
    name = f"{st.name} / draws{' forced' if forced else ''} / t={T:g}"
    return Case(name, st, "draws", T, _raw(d, T), {"empty_stretch": empty_stretch, **({"force_ts": True} if forced else {})}, t)


# ------------------------------------------------------------------------------------------------ what the tests run
VOCABS = ["micro.en", "micro", "v3-slice"]                 # 51 864, 51 865 and 51 866 tokens (another beg)
# default parameters, so that rows of one launch (one static ban, one suppress_blank / max_initial_ts) can mix them
ROW_STATES = [s.name for s in STATES if s.suppress_blank and s.max_initial_ts == 1.0 and not (s.no_timestamps or s.non_speech or s.tdrz)]
# (state, forced): with level timestamps (forced) the monotone floor and the initial cap carry half of the mass of the draw
DRAW_STATES = [("initial", False), ("initial", True), ("[text,ts]", False), ("[text,text]", False), ("[text,text]", True),
               ("has_ts seek 1500", False), ("has_ts seek 1500", True), ("[text,ts] has_ts seek 1500", True),
               ("no_timestamps", False), ("tdrz non-speech initial", False)]


def states_of(label):
    return [s.name for s in STATES] if label == VOCABS[0] else REDUCED_STATES


class HostSide:
    """The host definition (csrc/host_logic.cpp: process_logits, sample_token, sample_token_topk) on a host-only context."""

    def __init__(self, lib, model: bytes):
        self.lib = lib
        self.buf = C.create_string_buffer(model, len(model))
        self.ctx = lib.wmi_init_host_only(C.cast(self.buf, C.c_void_p), len(model))
        assert self.ctx
        self.v = vocab_of(lib, self.ctx)

    def close(self):
        self.lib.whisper_free(self.ctx); self.ctx = None

    def filters(self, raw, st: State, T):
        nv = self.v.n_vocab
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        lo, lp, pr = (np.empty(nv, np.float32) for _ in range(3))
        h = np.asarray(st.history(self.v), np.int32)
        raw = np.ascontiguousarray(raw, np.float32)
        self.lib.wmi_process_logits(self.ctx, st.params(self.lib), fp(raw), h.ctypes.data_as(C.POINTER(C.c_int32)), h.size,
                                    int(st.has_ts), st.seek_delta, C.c_float(T), fp(lo), fp(lp), fp(pr))
        return lo, lp, pr

    def token(self, lp, pr, i, tid_default=0):
        """what sample_token / sample_token_topk report for token i of these arrays"""
        beg = self.v.beg
        ts = pr[beg:].astype(np.float64)
        tid = beg + int(np.argmax(ts)) if ts.max() > 0 else tid_default
        ptsum = float(ts.sum()); pt = float(np.float32(ts.max() / (ptsum + 1e-10)))
        if i >= beg:
            tid, pt = i, float(pr[i])
        return int(i), int(tid), float(pr[i]), float(lp[i]), pt, float(np.float32(ptsum))

    def pick(self, raw, st, T, tid_default=0):
        lo, lp, pr = self.filters(raw, st, T)
        return lo, self.token(lp, pr, int(np.argmax(pr)), tid_default)        # the first index of the largest probability, as sample_token(best)

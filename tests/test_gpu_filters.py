"""-m gpu: the device logit filters, the greedy pick and the draws on crafted logits, through wmi_selftest_filters.

What token a decode step emits is decided by three device copies of one predicate: the statistics pass (csrc/k_sample.hip: k_filter_stats
+ k_filter_pick; the block-quantised step, every lock-step row), the fused epilogue of the vocabulary projection (csrc/k_dec.hip: the FS
branch of k_gemv1 feeding k_filter_pick<XU, 12>; the headline greedy step) and the draw predicate (k_prob_blocks / k_draw; beam search and
temperature > 0).  The hook runs each on caller logits; the step records are built from parameters and history by the product's own
builder (make_step_filter), never from a raw record.  Every case comes from tests/filters_f64.py, whose float64 restatement and whose
conditions on the inputs tests/test_filters_f64.py proves on the CPU; here no case is left uncompared:

  mode 0, one row   id and tid equal the host's (wmi_process_logits on a host-only context) and the float64 values; p, plog, pt, ptsum
                    within PICK_TOL of both
  mode 0, rows      2 / 8 / 16 rows of different states and patterns in one launch: every row bit for bit what it gives alone
  mode 1            the fused form at K = 128 over the whole state x pattern matrix, a reduced set at K = 512 / 768 / 1280 (the other chunk
                    counts of the projection kernel): the same bounds on the logits the launch returned, those logits within LOGIT_ABS of a
                    float64 W . LN(x), id and tid equal to mode 0's on the same logits
  mode 2            uniform numbers placed in the middle of chosen CDF cells (first / last positive token, both sides of block and lane-run
                    boundaries, behind empty blocks), u = 0 and u = 1 - 2^-53: the id is exactly the target; the statistics within PICK_TOL;
                    8 rows x 8 draws in one launch bit for bit the one-row, one-draw launches; a uniform number EXACTLY on a cell's upper
                    edge takes that cell (cdf >= target, not >)

A raw -inf logit is out of the allowed set, as in process_logits: before these tests both statistics kernels let it in, and where it was
the only (k_filter_stats: a block whose other entries are banned) or the first (fused epilogue: a lane's first row) allowed entry the
sums became exp(-inf + inf) = NaN — the "wide" pattern found it.

No test reads the reference checkout or oracle/_ref."""
import ctypes as C

import numpy as np
import pytest

import filters_f64 as ff
import stage_compare as sc
from godot_whisper_amd import abi, synth
from test_gpu_decode_lengths import PICK_TOL
from test_gpu_parity import LOGIT_ABS

pytestmark = pytest.mark.gpu

# device vs the host filters / vs float64 on the same logits, held to PICK_TOL (1e-4).  Measured worst |d| per field over every case
# below (MI355X); the host's own distance from float64 on these cases is p 2.5e-5, plog 7.6e-5, pt 3.1e-6, ptsum 3.2e-6
# (tests/test_filters_f64.py): the device sums in trees and sits next to float64, the left-to-right f32 sums of the host do not.
#   mode 0            vs host: p 2.5e-5, plog 7.5e-5, pt 2.8e-6, ptsum 3.2e-6     vs float64: p 3.1e-6, plog 6.0e-6, pt 3.1e-6, ptsum 3.1e-6
#   mode 1, K = 128   vs host: p 1.4e-5, plog 7.5e-5, pt 2.5e-6, ptsum 3.2e-6     vs float64: p 2.9e-6, plog 4.1e-6, pt 2.9e-6, ptsum 2.9e-6
#   mode 1, K >= 512  vs host: p 7.6e-6, plog 1.5e-5, pt 1.9e-6, ptsum 2.0e-6     vs float64: p 5.7e-7, plog 7.3e-7, pt 5.7e-7, ptsum 6.9e-7
#   mode 2            vs host: p 6.9e-6, plog 1.3e-5, pt 1.2e-7, ptsum 1.7e-6     vs float64: p 3.7e-7, plog 8.7e-7, pt 1.4e-7, ptsum 4.4e-7
# mode 1's returned logits are within 6.0e-5 of the float64 W . LN(x) (LOGIT_ABS 3e-2).
FIELDS = ("p", "plog", "pt", "ptsum")
MODE1_TEMPS = (0.0, 0.5)         # the epilogue reads the record's temperature although the product passes 0
WORST = {}


class Side:
    """a compute context and a host-only context of one vocabulary"""

    def __init__(self, lib, label):
        model = synth.make_model(label, seed=1234)
        self.lib, self.label = lib, label
        self.buf = C.create_string_buffer(model, len(model))
        self.ctx = lib.whisper_init_from_buffer_with_params(C.cast(self.buf, C.c_void_p), len(model), abi.whisper_context_params(True))
        assert self.ctx
        self.host = ff.HostSide(lib, model)
        self.v = self.host.v
        self.W = {}

    def close(self):
        self.lib.whisper_free(self.ctx); self.host.close()

    # ---- the hook
    def run(self, mode, st, rows, T, u=None, k=1, tid_default=0, W=None, x=None):
        """rows: [(raw, state)] (mode 1: one state, the logits come from W and x).  Returns (tokens [n_rows][k] as tuples, logits)"""
        n = len(rows)
        hist = [t for _, s in rows for t in s.history(self.v)]
        h = np.asarray(hist if hist else [0], np.int32)
        nh = np.asarray([len(s.hist) for _, s in rows], np.int32)
        hs = np.asarray([int(s.has_ts) for _, s in rows], np.int32); sd = np.asarray([s.seek_delta for _, s in rows], np.int32)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        out = (abi.whisper_token_data * (n * k))()
        lg = lo = None
        if mode == 1:
            lo = np.empty(self.v.n_vocab, np.float32)
        else:
            lg = np.ascontiguousarray(np.stack([r for r, _ in rows]), np.float32)
        uu = None if u is None else np.ascontiguousarray(u, np.float64)
        rc = self.lib.wmi_selftest_filters(self.ctx, st.params(self.lib), mode, n, vp(lg), vp(h), vp(nh), vp(hs), vp(sd), C.c_float(T),
                                           vp(W), vp(x), 0 if W is None else W.shape[1], vp(lo), vp(uu), k, tid_default, out)
        assert rc == 0, (rc, mode, st.name)
        return [[(o.id, o.tid, o.p, o.plog, o.pt, o.ptsum) for o in out[r * k:(r + 1) * k]] for r in range(n)], lo

    # ---- a projection that puts a chosen logit on every vocabulary entry: x alternates +-1 (LayerNorm(x) = x / sqrt(1 + eps)), the value
    # rides on three columns of W with x = +1 as an f16 head and two f16 corrections (columns 8, 10, 12: a lane past K re-reads columns 0..7
    # against an activation of exactly 0, so those stay 0 and an infinite entry cannot turn into a NaN there)
    def projection(self, K, want):
        W = self.W.get(K)
        if W is None:
            W = self.W[K] = np.zeros((self.v.n_vocab, K), np.float16)
        w = want.astype(np.float64)
        for c in (8, 10, 12):
            with np.errstate(over="ignore", invalid="ignore"):
                h = w.astype(np.float16)
                W[:, c] = h
                w = np.where(np.isfinite(h), w - h.astype(np.float64), 0.0)
        x = np.where(np.arange(K) % 2 == 0, 1.0, -1.0).astype(np.float32)
        return W, x

    def projection_f64(self, W, x):
        xd = x.astype(np.float64)
        ln = (xd - xd.mean()) / np.sqrt(xd.var() + 1e-5)
        with np.errstate(invalid="ignore"):
            return W[:, [8, 10, 12]].astype(np.float64) @ ln[[8, 10, 12]]


_sides = {}


@pytest.fixture(scope="module")
def sides(product_lib):
    def get(label):
        if label not in _sides:
            _sides[label] = Side(product_lib, label)
        return _sides[label]
    yield get
    for s in _sides.values():
        s.close()
    _sides.clear()
    for mode in sorted(WORST):
        print(f"\n{mode}: worst |d| " + "; ".join(f"{k} {v:.2e}" for k, v in sorted(WORST[mode].items())))


def hold_token(mode, got, host, ref, what):
    """a device token against the host's and the float64 one: ids exact, the four statistics within PICK_TOL of both"""
    assert got[0] == host[0] == ref[0], (what, got, host, ref)
    assert got[1] == host[1] == ref[1], (what, got, host, ref)
    w = WORST.setdefault(mode, {})
    for j, k in enumerate(FIELDS):
        for side, other in (("the host filters", host), ("float64", ref)):
            d = abs(got[2 + j] - other[2 + j])
            assert d == d, (what, k, got, other)               # not a NaN
            w[f"{k} vs {side}"] = max(w.get(f"{k} vs {side}", 0.0), d)
            sc.hold(f"filters {mode}: {k} vs {side}", d, PICK_TOL, what)


def bits(tok):
    return (tok[0], tok[1]) + tuple(np.asarray(tok[2:], np.float32).view(np.uint32).tolist())


STATE_IDS = [(lb, sn) for lb in ff.VOCABS for sn in ff.states_of(lb)]


@pytest.mark.parametrize("label,sn", STATE_IDS, ids=[f"{a}-{b}" for a, b in STATE_IDS])
def test_statistics_pass_and_pick_on_every_case(sides, label, sn):
    s = sides(label); st = ff.STATE[sn]
    cases, _ = ff.make_cases(s.v, st)
    assert cases
    for c in cases:
        got, _ = s.run(0, st, [(c.raw, st)], c.temperature)
        _, host = s.host.pick(c.raw, st, c.temperature)
        hold_token("mode 0", got[0][0], host, ff.evaluate(c.raw, s.v, st, c.temperature).pick(), c.name)


@pytest.mark.parametrize("n_rows", [2, 8, 16])
@pytest.mark.parametrize("label", ff.VOCABS)
def test_rows_of_one_launch_equal_the_rows_alone(sides, label, n_rows):
    s = sides(label)
    for T in ff.TEMPS:
        rows = []
        for r in range(n_rows):                               # a different state and a different pattern per row
            st = ff.STATE[ff.ROW_STATES[(r * 5 + n_rows) % len(ff.ROW_STATES)]]
            cases, _ = ff.make_cases(s.v, st, temps=(T,))
            rows.append((cases[(7 * r + 3) % len(cases)].raw, st))
        assert len({st.name for _, st in rows}) == min(n_rows, len(ff.ROW_STATES))
        got, _ = s.run(0, rows[0][1], rows, T)
        for r, (raw, st) in enumerate(rows):
            alone, _ = s.run(0, st, [(raw, st)], T)
            assert bits(got[r][0]) == bits(alone[0][0]), (label, n_rows, T, r, st.name, got[r][0], alone[0][0])


def fused_case(s, st, c, K, mode):
    W, x = s.projection(K, c.raw)
    got, lo = s.run(1, st, [(None, st)], c.temperature, W=W, x=x)
    want = s.projection_f64(W, x)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(lo), fin) and not np.isnan(lo).any(), c.name
    sc.hold(f"filters {mode}: returned logits vs float64 W . LN(x), max |d|", float(np.abs(lo[fin] - want[fin]).max()), LOGIT_ABS, c.name)
    # the yardsticks on the logits the launch wrote
    r = ff.evaluate(lo, s.v, st, c.temperature)
    ff.check_conditions(r, c.name)
    _, host = s.host.pick(lo, st, c.temperature)
    hold_token(mode, got[0][0], host, r.pick(), c.name)
    unfused, _ = s.run(0, st, [(lo, st)], c.temperature)
    assert got[0][0][:2] == unfused[0][0][:2], (c.name, got[0][0], unfused[0][0])
    if "id" in c.expect:
        assert got[0][0][0] == c.expect["id"], (c.name, got[0][0])


@pytest.mark.parametrize("label,sn", STATE_IDS, ids=[f"{a}-{b}" for a, b in STATE_IDS])
def test_fused_epilogue_on_every_case(sides, label, sn):
    s = sides(label); st = ff.STATE[sn]
    cases, _ = ff.make_cases(s.v, st, temps=MODE1_TEMPS)
    assert cases
    for c in cases:
        fused_case(s, st, c, 128, "mode 1, K = 128")


WIDE = [(K, lb, sn) for K, lb in ((512, "micro.en"), (768, "micro"), (1280, "v3-slice")) for sn in ff.WIDE_STATES]


@pytest.mark.parametrize("K,label,sn", WIDE, ids=[f"K{a}-{b}-{c}" for a, b, c in WIDE])
def test_fused_epilogue_at_the_wider_projections(sides, K, label, sn):
    s = sides(label); st = ff.STATE[sn]
    cases, _ = ff.make_cases(s.v, st, temps=MODE1_TEMPS, patterns=("ts-mass wins", "ts-mass loses", "tie", "winner"))
    assert len(cases) >= 10
    for c in cases:
        fused_case(s, st, c, K, f"mode 1, K = {K}")


@pytest.mark.parametrize("label", ff.VOCABS)
def test_draws_land_in_the_chosen_cells(sides, label):
    s = sides(label); v = s.v
    for sn, forced in ff.DRAW_STATES:
        st = ff.STATE[sn]
        for T in ff.TEMPS:
            c = ff.make_draw_case(v, st, T, forced)
            r = ff.evaluate(c.raw, v, st, T)
            idx, _ = r.cdf()
            lo, lp, pr = s.host.filters(c.raw, st, T)
            want = list(c.targets) + [int(idx[0]), int(idx[-1])]
            us = [r.cell_mid(t) for t in c.targets] + [0.0, 1.0 - 2.0 ** -53]
            for tid_default in (v.beg, 0):
                for j in range(0, len(us), 8):
                    u = us[j:j + 8]
                    got, _ = s.run(2, st, [(c.raw, st)], T, u=np.asarray([u]), k=len(u), tid_default=tid_default)
                    for n, tok in enumerate(got[0]):
                        t = want[j + n]
                        assert tok[0] == t, (c.name, u[n], tok, t)
                        hold_token("mode 2", tok, s.host.token(lp, pr, t, tid_default), r.token(t, tid_default), (c.name, t))


@pytest.mark.parametrize("label", ff.VOCABS)
def test_a_draw_exactly_on_a_cell_boundary_takes_the_lower_token(sides, label):
    """first i with cdf(i) >= u * total, with equality: 2^15 allowed tokens of equal logit (every other entry a raw -inf) have bit-equal
    probabilities p, so every block sum, prefix and the total 2^15 p are exact multiples of p in double and u = j / 2^15 puts the target
    exactly on the upper edge of the j-th token's cell — at the end of a block, of a lane run and inside a run"""
    s = sides(label); v = s.v
    st = ff.STATE["[text,text]"]
    keep = np.flatnonzero(ff.rule_allowed(v, st)[:v.beg])[:1 << 15]
    raw = np.full(v.n_vocab, -np.inf, np.float32); raw[keep] = 1.5
    per, run = ff.per_block(v.n_vocab), ff.lane_run(v.n_vocab)
    js = [int(np.searchsorted(keep, edge)) for edge in (per, 7 * per, 3 * per + 5 * run, 3 * per + 5 * run + 4, 40 * per)] + [1, 1 << 15]
    assert all(0 < j <= 1 << 15 for j in js)
    u = np.asarray([[j / float(1 << 15) for j in js] + [0.0]])
    got, _ = s.run(2, st, [(raw, st)], 0.0, u=u, k=8, tid_default=v.beg)
    assert [t[0] for t in got[0]] == [int(keep[j - 1]) for j in js] + [int(keep[0])], (label, js, got[0])
    assert all(abs(t[2] - 2.0 ** -15) < 1e-9 for t in got[0])


@pytest.mark.parametrize("label", ff.VOCABS)
def test_timestamp_underflow_reports_the_default_tid_in_draws(sides, label):
    s = sides(label); v = s.v
    st = ff.STATE["[text,text]"]
    for T in ff.TEMPS:
        c = [c for c in ff.make_cases(v, st, temps=(T,), patterns=("ts underflow",))[0]][0]
        r = ff.evaluate(c.raw, v, st, T)
        lo, lp, pr = s.host.filters(c.raw, st, T)
        for tid_default in (v.beg, 0):
            got, _ = s.run(2, st, [(c.raw, st)], T, u=np.asarray([[0.5]]), k=1, tid_default=tid_default)
            tok = got[0][0]
            assert tok[0] == r.draw(0.5) and tok[1] == tid_default and tok[4] == 0.0 and tok[5] == 0.0, (c.name, tok)
            hold_token("mode 2", tok, s.host.token(lp, pr, tok[0], tid_default), r.token(tok[0], tid_default), c.name)


@pytest.mark.parametrize("label", ff.VOCABS)
def test_draws_of_one_launch_equal_the_draws_alone(sides, label):
    s = sides(label); v = s.v
    rng = np.random.default_rng(11)
    for T in (0.0, 0.2):
        rows = []
        for r in range(8):
            st = ff.STATE[ff.ROW_STATES[(3 * r + 1) % len(ff.ROW_STATES)]]
            rows.append((ff.make_draw_case(v, st, T, forced=r % 3 == 0, seed=r).raw, st))
        u = rng.uniform(0.0, 1.0, (8, 8))
        got, _ = s.run(2, rows[0][1], rows, T, u=u, k=8, tid_default=v.beg)
        for r, (raw, st) in enumerate(rows):
            for j in range(8):
                alone, _ = s.run(2, st, [(raw, st)], T, u=u[r:r + 1, j:j + 1], k=1, tid_default=v.beg)
                assert bits(got[r][j]) == bits(alone[0][0]), (label, T, r, j, st.name, got[r][j], alone[0][0])


def test_hook_answers_bad_arguments_on_a_compute_context(sides):
    s = sides("micro.en"); nv = s.v.n_vocab
    z = np.zeros(nv, np.float32); td = (abi.whisper_token_data * 64)(); i16 = (C.c_int * 16)()
    x = np.ones(12, np.float32); W = np.zeros((8, 12), np.float16); u = np.zeros(64, np.float64)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    f = lambda mode, n, lg, W_, x_, K, lo, u_, k: s.lib.wmi_selftest_filters(
        s.ctx, s.lib.whisper_full_default_params(0), mode, n, vp(lg), None, i16, i16, i16, C.c_float(0.0), vp(W_), vp(x_), K, vp(lo), vp(u_), k, 0, td)
    assert f(3, 1, z, None, None, 0, None, None, 1) == -1 and f(0, 17, z, None, None, 0, None, None, 1) == -1
    assert f(0, 1, None, None, None, 0, None, None, 1) == -1 and f(2, 9, z, None, None, 0, None, u, 1) == -1
    assert f(2, 1, z, None, None, 0, None, u, 9) == -1 and f(2, 1, z, None, None, 0, None, None, 1) == -1
    assert f(1, 1, None, W, x, 12, z, None, 1) == -4 and f(1, 1, None, W, x, 2048, z, None, 1) == -4
    assert f(1, 1, None, None, x, 128, z, None, 1) == -1

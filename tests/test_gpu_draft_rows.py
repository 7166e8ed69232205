"""-m gpu: the draft verifier's device side on crafted logits, through wmi_selftest_draft_rows — filter_stats + k_draft_pick per group of 8
rows + k_draft_finish, as decode() queues them behind the vocabulary projection of a drafted batch.

  records    every out[r] is BYTE-equal to what the row form of wmi_selftest_filters (k_filter_stats + k_filter_pick<.., 1>) returns for the
             same logits and the same step record — the record of a decoder whose history is draft[0 .. r) (tests/draft_ref.py), which the
             filters hook builds with make_step_filter from that history; both halves carry the call's tag
  accepted   equals the judge's accept length over those picks
  shapes     1, 7, 8, 9, 16, 17 rows (the groups of 8 and their edges), the micro and the tiny vocabulary
  cases      a mismatch at row 0, in the middle, at a group edge, at the last row, nowhere; an exact tie on the target that the first index
             wins, and one it loses; a row where the timestamp mass forces a timestamp; -inf logits; a row whose every entry is out;
             sentinels behind every output array

No test reads the reference checkout or oracle/_ref."""
import ctypes as C

import numpy as np
import pytest

import draft_ref as dr
import filters_f64 as ff
from godot_whisper_amd import abi, synth

pytestmark = pytest.mark.gpu

TAG = 0x1234567
SENT = np.int32(0x5A5A5A5A)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Side:
    def __init__(self, lib, label):
        model = synth.make_model(label, seed=1234)
        self.lib = lib
        self.buf = C.create_string_buffer(model, len(model))
        self.ctx = lib.whisper_init_from_buffer_with_params(C.cast(self.buf, C.c_void_p), len(model), abi.whisper_context_params(True))
        assert self.ctx
        self.v = ff.vocab_of(lib, self.ctx)
        self.m = dr.Model(self.v.n_vocab, self.v.eot, self.v.beg, lib.whisper_n_text_ctx(self.ctx), self.v.n_audio_ctx, self.v.space_id)
        self.ban = ff.static_ban(self.v, ff.State("default")).astype(np.uint8)

    def close(self):
        self.lib.whisper_free(self.ctx)

    def reference(self, logits, states):
        """the existing row form on the same logits, the records built from the rows' histories: [(id, tid, p, plog, pt, ptsum)] as words"""
        out = []
        p = self.lib.whisper_full_default_params(0)
        for r0 in range(0, len(states), 16):
            st = states[r0:r0 + 16]
            n = len(st)
            hist = np.asarray([t for h, _, _ in st for t in h] or [0], np.int32)
            nh = np.asarray([len(h) for h, _, _ in st], np.int32)
            hs = np.asarray([int(b) for _, b, _ in st], np.int32); sd = np.asarray([d for _, _, d in st], np.int32)
            res = (abi.whisper_token_data * n)()
            lg = np.ascontiguousarray(logits[r0:r0 + n], np.float32)
            rc = self.lib.wmi_selftest_filters(self.ctx, p, 0, n, vp(lg), vp(hist), vp(nh), vp(hs), vp(sd), C.c_float(0.0), None, None, 0, None,
                                               None, 1, 0, res)
            assert rc == 0
            for o in res:
                out.append((np.int32(o.id), np.int32(o.tid)) + tuple(np.float32(x).view(np.int32) for x in (o.p, o.plog, o.pt, o.ptsum)))
        return out

    def draft_rows(self, logits, records, targets):
        n_rows = len(records)
        steps = np.stack([dr.words_of_record(r, TAG) for r in records]).astype(np.int32)
        out = np.full((n_rows + 1, 8), SENT, np.int32)
        acc = (C.c_int32 * 2)(-77, int(SENT))
        tg = np.asarray(list(targets) + [int(SENT)], np.int32)
        rc = self.lib.wmi_selftest_draft_rows(0, n_rows, self.m.n_vocab, vp(np.ascontiguousarray(logits, np.float32)), vp(self.ban), vp(steps),
                                              vp(tg) if n_rows > 1 else None, vp(out), C.cast(acc, C.POINTER(C.c_int32)))
        assert rc == 0, rc
        assert (out[n_rows] == SENT).all() and acc[1] == int(SENT) and tg[-1] == SENT, "a store behind an output array"
        return out[:n_rows], acc[0]


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


def make_draft(m, n, rng):
    """<|0.00|> x x x <|t|><|t|> x x x <|t'|><|t'|> ..: legal under the filters at every row"""
    d, t = [m.beg], 0
    while len(d) < n:
        d += rng.integers(1000, m.eot - 1, 3).tolist()
        t += 20
        d += [m.beg + t, m.beg + t]
    return d[:n]


def craft(side, n_rows, k, rng, special=True):
    """logits whose filtered greedy decode follows the draft up to row k (None: to its end) -> (logits, draft, plan)"""
    m = side.m
    n = n_rows - 1
    draft = make_draft(m, n, rng)
    pl = dr.plan(m, dr.Params(), 1, draft)
    assert pl.n == n
    lg = rng.normal(0.0, 2.0, (n_rows, m.n_vocab)).astype(np.float32)
    lg[rng.random(lg.shape) < 0.03] = -np.inf                              # raw -inf entries are out, wherever they lie
    for j in range(n):
        lg[j, draft[j]] = 25.0
    if special and n >= 3 and k != 2:                                       # an exact tie on the target: the first index wins
        lg[2, draft[2] + 1] = 25.0
    if special and n >= 5 and k != 4:                                       # the timestamp mass forces a timestamp although a text token leads
        lg[4] = np.where(np.isfinite(lg[4]), lg[4], -9.0)
        lg[4, m.beg:m.beg + 400] = 10.0
        lg[4, draft[4]] = 10.5
        lg[4, 5000] = 12.0
    if k is not None and k < n:
        if k == 2 and special:
            lg[2, draft[2] - 1] = 25.0                                      # the tie lost: an equal logit at a smaller index
        elif k % 3 == 1:
            lg[k, :] = -np.inf                                              # a row whose every entry is out
        else:
            lg[k, draft[k]] = -5.0
    return lg, draft, pl


CASES = [(1, None), (7, None), (7, 0), (7, 3), (8, 6), (8, None), (9, 7), (9, 8), (9, None), (16, 2), (16, 7), (16, 8), (16, 14),
         (17, 8), (17, 15), (17, 16), (17, None)]


@pytest.mark.parametrize("label", ["micro", "tiny.en"])
@pytest.mark.parametrize("n_rows,k", CASES)
def test_rows_equal_the_row_form_and_the_judge(sides, label, n_rows, k):
    s = sides(label)
    rng = np.random.default_rng(1000 * n_rows + (99 if k is None else k))
    lg, draft, pl = craft(s, n_rows, None if k == n_rows - 1 else k, rng)
    ref = s.reference(lg, pl.states)
    picks = [int(r[0]) for r in ref]
    want_a = dr.accept_len(picks, draft, pl.n)
    assert want_a == (pl.n if k is None or k >= pl.n else k), ("the case is not what it claims", want_a, k)
    out, acc = s.draft_rows(lg, pl.records, draft)
    for r in range(n_rows):
        got = (out[r, 0], out[r, 1], out[r, 2], out[r, 4], out[r, 5], out[r, 6])
        assert tuple(int(x) for x in got) == tuple(int(x) for x in ref[r]), (label, n_rows, k, "row", r)
        assert out[r, 3] == TAG and out[r, 7] == TAG
    assert acc == want_a
    if pl.n >= 5 and k != 4:
        assert picks[4] == draft[4] and lg[4].argmax() == 5000, "the forced timestamp did not happen"
    if pl.n >= 3 and k == 2:
        assert picks[2] == draft[2] - 1


def test_a_row_without_a_target_never_matches(sides):
    """the last row has no target: even when its pick equals the word behind the targets, accepted stays n"""
    s = sides("micro.en")
    rng = np.random.default_rng(3)
    lg, draft, pl = craft(s, 9, None, rng, special=False)
    out, acc = s.draft_rows(lg, pl.records, draft)
    assert acc == 8 and len(out) == 9

"""No GPU: the judge of the draft verifier (tests/draft_ref.py) refuses wrong answers, the product's plan (wmi_selftest_draft_plan on a
host-only context) equals the judge's, and wmi_set_draft's argument checks and arm / consume / clear bookkeeping hold without a device."""
import ctypes as C

import numpy as np
import pytest

import draft_ref as dr
import filters_f64 as ff
from godot_whisper_amd import abi, runtime, synth


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------- the judge refuses wrong answers
M = dr.Model(n_vocab=51864, eot=50256, beg=50363, n_text_ctx=448, n_audio_ctx=1500, space_id=220)
TS = lambda k: M.beg + k


def right(p, P, draft, picks, **kw):
    a = dr.answer(M, p, P, draft, picks, **kw)
    assert dr.judge(M, p, P, draft, picks, a, **kw) == []
    return a


def refused(p, P, draft, picks, wrong, **kw):
    bad = dr.judge(M, p, P, draft, picks, wrong, **kw)
    assert bad, "the judge let a wrong answer through"
    return bad


def test_the_judge_refuses_wrong_accept_lengths_and_missing_bonus():
    p = dr.Params()
    draft = [TS(0), 1000, 2000, 3000, 4000, TS(50)]
    picks = [TS(0), 1000, 2000, 3333, 4000, TS(50), M.eot]            # the greedy decode leaves the draft at token 3
    a = right(p, 3, draft, picks)
    assert a["a"] == 3 and a["tokens"] == [TS(0), 1000, 2000, 3333]
    refused(p, 3, draft, picks, dict(a, a=2, tokens=a["tokens"][:3]))                        # one short
    refused(p, 3, draft, picks, dict(a, a=4, tokens=a["tokens"] + [4000]))                   # one long
    refused(p, 3, draft, picks, dict(a, a=6, tokens=picks))                                  # accepting past the mismatch
    refused(p, 3, draft, picks, dict(a, tokens=a["tokens"][:3]))                             # no bonus token
    refused(p, 3, draft, picks, dict(a, tokens=[TS(0), 1000, 2000, 3000]))                   # the draft's token where the pick differs
    # the whole draft accepted: the bonus token is the row behind it
    full = right(p, 3, draft, [TS(0), 1000, 2000, 3000, 4000, TS(50), 777])
    assert full["a"] == 6 and full["tokens"][-1] == 777


def test_the_judge_refuses_wrong_histories():
    p = dr.Params()
    draft = [TS(0), 1000, TS(20), TS(20), 2000, 3000]
    picks = draft + [M.eot]
    a = right(p, 1, draft, picks)
    recs = a["records"]
    assert recs[0]["flags"] & 1 and not any(r["flags"] & 1 for r in recs[1:])
    # row j filtered with row j - 1's history
    for j in (1, 3, 4):
        wrong = [dict(r) for r in recs]; wrong[j] = dict(recs[j - 1])
        refused(p, 1, draft, picks, dict(a, records=wrong))
    # the blank ban on a row other than 0
    wrong = [dict(r) for r in recs]; wrong[2]["flags"] |= 1
    refused(p, 1, draft, picks, dict(a, records=wrong))
    # a stale ts_floor_end: row 4 sits behind the pair <|0.40|><|0.40|>, the floor of row 1 (behind <|0.00|>) is too low
    assert recs[4]["ts_floor_end"] == TS(20) and recs[1]["ts_floor_end"] == TS(0)
    wrong = [dict(r) for r in recs]; wrong[4]["ts_floor_end"] = recs[1]["ts_floor_end"]
    refused(p, 1, draft, picks, dict(a, records=wrong))
    # max_initial_ts on a later row
    wrong = [dict(r) for r in recs]; wrong[1]["ts_initial_start"] = recs[0]["ts_initial_start"]
    assert recs[0]["ts_initial_start"] == TS(50) + 1 and recs[1]["ts_initial_start"] == M.n_vocab
    refused(p, 1, draft, picks, dict(a, records=wrong))


def test_the_judge_refuses_ignored_completion_and_wrong_clips():
    p = dr.Params()
    draft = [TS(0), 1000, TS(30), M.eot, 2000, 3000]
    picks = draft + [4000]
    a = right(p, 2, draft, picks)
    assert a["a"] == 6 and a["tokens"] == draft[:4]                                          # <eot> completes the decoder at token 3
    refused(p, 2, draft, picks, dict(a, tokens=picks))                                       # completion inside the accepted run ignored
    # a timestamp that goes back in time fails the decoder: the replay stops there
    back = [TS(0), 1000, TS(30), 2000, TS(10), 3000]
    ab = right(p, 2, back, back + [M.eot])
    assert ab["tokens"] == back[:5]
    refused(p, 2, back, back + [M.eot], dict(ab, tokens=back + [M.eot]))
    # max_tokens: at most max_tokens + 1 draft rows, and the token at iteration max_tokens completes
    pm = dr.Params(max_tokens=3)
    long_draft = [TS(0), 1000, 2000, 3000, 4000, 5000, 6000]
    am = right(pm, 2, long_draft, long_draft + [M.eot])
    assert am["n"] == 4 and len(am["records"]) == 5 and am["tokens"] == long_draft[:4]
    over = dr.plan(M, dr.Params(), 2, long_draft)
    refused(pm, 2, long_draft, long_draft + [M.eot], dict(am, n=5))                          # clip past max_tokens + 1
    refused(pm, 2, long_draft, long_draft + [M.eot], dict(am, records=over.records[:6], logit_rows=over.logit_rows[:6]))
    # the other clips
    assert dr.clip(M, dr.Params(), 3, 1000) == dr.n_max(M) - 1 and dr.clip(M, dr.Params(), 300, 1000) == 448 - 300 - 1
    assert dr.clip(M, dr.Params(), 447, 5) == 0 and dr.clip(M, dr.Params(), 3, 0) == 0
    assert dr.answer(M, dr.Params(), 447, [1000], [1000, 2000])["n"] == 0


def test_single_segment_and_the_end_of_the_audio():
    # a timestamp that reaches the end of the audio completes the decoder; single_segment resets seek_delta
    p = dr.Params(single_segment=True)
    draft = [TS(0), 1000, TS(100), 2000]
    a = right(p, 1, draft, draft + [M.eot], seek=0, seek_end=300)
    assert a["tokens"] == draft[:3]
    _, d = dr.replay(M, p, draft + [M.eot], 4, 0, 300)
    assert d.completed and d.seek_delta == dr.CHUNK and d.result_len == 3


# ---------------------------------------------------------------------------------------------- the product's plan equals the judge's
@pytest.fixture(scope="module")
def host_ctx():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    out = {}
    for name in ("micro.en", "micro"):
        mb = synth.make_model(name, seed=1)
        buf = C.create_string_buffer(mb, len(mb))
        ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(mb))
        assert ctx
        out[name] = (ctx, buf)
    yield lib, out
    for ctx, _ in out.values():
        lib.whisper_free(ctx)


def model_of(lib, ctx) -> dr.Model:
    v = ff.vocab_of(lib, ctx)
    return dr.Model(v.n_vocab, v.eot, v.beg, lib.whisper_n_text_ctx(ctx), v.n_audio_ctx, v.space_id)


def hook_plan(lib, ctx, m, prompt, draft, **kw):
    p = lib.whisper_full_default_params(0)
    for k, val in kw.items():
        setattr(p, k, val)
    cap = dr.n_max(m) + 8
    n_rows = C.c_int32(-7)
    rows = np.full(cap, -9, np.int32); steps = np.full((cap, 16), -9, np.int32)
    pr = np.asarray(prompt, np.int32); d = np.asarray(draft, np.int32)
    rc = lib.wmi_selftest_draft_plan(ctx, p, vp(pr), pr.size, vp(d) if d.size else None, d.size, C.byref(n_rows), vp(rows), vp(steps))
    if rc != 0:
        return rc
    n = n_rows.value
    assert (rows[n:] == -9).all() and (steps[n:] == -9).all(), "the hook wrote behind its rows"
    return dict(n=n - 1, logit_rows=rows[:n].tolist(), records=[dr.record_of_words(w) for w in steps[:n]])


def prompts_of(lib, ctx, m):
    sot = lib.whisper_token_sot(ctx)
    init = [sot] + ([sot + 1, lib.whisper_token_transcribe(ctx)] if lib.whisper_is_multilingual(ctx) else [])
    prev = [lib.whisper_token_prev(ctx)] + list(range(300, 340))
    return [init, prev + init]


@pytest.mark.parametrize("name", ["micro.en", "micro"])
def test_the_plan_equals_the_judge(host_ctx, name):
    lib, ctxs = host_ctx
    ctx = ctxs[name][0]
    m = model_of(lib, ctx)
    ts = lambda k: m.beg + k
    nm = dr.n_max(m)
    rng = np.random.default_rng(5)
    text = lambda n: rng.integers(100, m.eot - 1, n).tolist()
    drafts = {
        "empty": [], "one": text(1), "n_max + 5": text(nm + 5),
        "timestamps": [ts(0)] + text(4) + [ts(40), ts(40)] + text(3) + [ts(90)],
        "non-monotone pair": [ts(0)] + text(2) + [ts(60), ts(20)] + text(3),
        "eot inside": [ts(0)] + text(3) + [ts(30), m.eot] + text(4),
        "leading text": text(6),
    }
    checked = 0
    for prompt in prompts_of(lib, ctx, m):
        for what, draft in drafts.items():
            for kw in ({}, {"max_tokens": 4}, {"suppress_blank": False, "max_initial_ts": 0.0}, {"single_segment": True, "duration_ms": 3000}):
                got = hook_plan(lib, ctx, m, prompt, draft, **kw)
                p = dr.Params(suppress_blank=kw.get("suppress_blank", True), max_initial_ts=kw.get("max_initial_ts", 1.0),
                              max_tokens=kw.get("max_tokens", 0), single_segment=kw.get("single_segment", False))
                seek_end = kw.get("duration_ms", 0) // 10 or dr.CHUNK
                want = dr.plan(m, p, len(prompt), draft, 0, seek_end)
                assert got["n"] == want.n, (what, kw, got["n"], want.n)
                assert got["logit_rows"] == want.logit_rows and got["records"] == want.records, (what, kw, len(prompt))
                checked += 1
    assert checked == 2 * 7 * 4
    assert dr.plan(m, dr.Params(), 1, drafts["n_max + 5"]).n == nm - 1
    # a prompt that leaves no room: clipped to nothing — one row, the prompt's last
    full_prompt = [lib.whisper_token_prev(ctx)] + list(range(300, 300 + m.n_text_ctx - 2))
    got = hook_plan(lib, ctx, m, full_prompt, drafts["one"])
    assert got["n"] == 0 and got["logit_rows"] == [len(full_prompt) - 1]


def test_the_plan_hook_refuses_bad_arguments(host_ctx):
    lib, ctxs = host_ctx
    ctx = ctxs["micro.en"][0]
    m = model_of(lib, ctx)
    assert hook_plan(lib, ctx, m, [], [100]) == -1
    assert hook_plan(lib, ctx, m, [m.n_vocab], [100]) == -1
    assert hook_plan(lib, ctx, m, [lib.whisper_token_sot(ctx)], [-1]) == -1
    assert hook_plan(lib, ctx, m, [lib.whisper_token_sot(ctx)], [m.n_vocab]) == -1


# ---------------------------------------------------------------------------------------------- arming, without a device
def status(lib, ctx):
    s = abi.wmi_draft_status()
    assert lib.wmi_draft_status(ctx, C.byref(s)) == 0
    return (s.n_offered, s.n_rows, s.n_accepted, s.n_emitted_from_draft, s.reason)


def test_set_draft_errors_and_bookkeeping(host_ctx):
    lib, ctxs = host_ctx
    ctx = ctxs["micro"][0]
    nv = lib.whisper_n_vocab(ctx)
    arm = lambda t, n=None: lib.wmi_set_draft(ctx, vp(np.asarray(t, np.int32)) if len(t) else None, len(t) if n is None else n)
    assert status(lib, ctx) == (0, 0, 0, 0, abi.DRAFT_NONE)
    # every error return: nothing is armed
    assert lib.wmi_set_draft(None, None, 0) == -1
    assert arm([1, 2], -1) == -1 and arm([], 3) == -1 and arm([5, -1]) == -1 and arm([5, nv]) == -1
    assert lib.wmi_draft_status(ctx, None) == -1 and lib.wmi_draft_status(None, C.byref(abi.wmi_draft_status())) == -1
    pcm = np.zeros(16000 * 2, np.float32)
    lock_step = lambda: lib.wmi_full_batch(ctx, lib.whisper_full_default_params(0), (C.c_void_p * 1)(pcm.ctypes.data), (C.c_int * 1)(pcm.size), 1, 0)
    lock_step()                                              # (a host-only context: the call fails, the bookkeeping is the same)
    assert status(lib, ctx) == (0, 0, 0, 0, abi.DRAFT_NONE), "a refused draft was armed"
    # arm -> a call that cannot carry it consumes it and says so
    assert arm([10, 20, nv - 1]) == 0
    lock_step()
    assert status(lib, ctx) == (3, 0, 0, 0, abi.DRAFT_NOT_ELIGIBLE)
    lock_step()
    assert status(lib, ctx) == (0, 0, 0, 0, abi.DRAFT_NONE), "the draft outlived the call that consumed it"
    # n = 0 clears; a bad list leaves the armed one alone
    assert arm([10, 20]) == 0 and arm([]) == 0
    lock_step()
    assert status(lib, ctx)[0] == 0
    assert arm([10, 20]) == 0 and arm([5, nv]) == -1
    lock_step()
    assert status(lib, ctx) == (2, 0, 0, 0, abi.DRAFT_NOT_ELIGIBLE)
    # whisper_full on a host-only context fails before its first window: armed, consumed, not used
    assert arm([10]) == 0
    lib.whisper_full(ctx, lib.whisper_full_default_params(0), pcm.ctypes.data_as(C.POINTER(C.c_float)), pcm.size)
    assert status(lib, ctx) == (1, 0, 0, 0, abi.DRAFT_NOT_ELIGIBLE)
    lib.whisper_full(ctx, lib.whisper_full_default_params(0), pcm.ctypes.data_as(C.POINTER(C.c_float)), pcm.size)
    assert status(lib, ctx) == (0, 0, 0, 0, abi.DRAFT_NONE)
    # the rows hook judges its arguments before it touches a device
    z = np.zeros((2, 8), np.float32); st = np.zeros((2, 16), np.int32); st[:, 8] = 8
    out = np.zeros((2, 8), np.int32); acc = C.c_int32(-5)
    ban = np.zeros(8, np.uint8)
    rows = lambda n, nv_, lg=z, b=ban, s=st, t=np.zeros(1, np.int32): lib.wmi_selftest_draft_rows(0, n, nv_, vp(lg), vp(b), vp(s), vp(t), vp(out), C.byref(acc))
    assert rows(0, 8) == -1 and rows(2, 0) == -1 and rows(2, 70000) == -1 and rows(2, 8, lg=None) == -1 and rows(2, 8, b=None) == -1
    assert rows(2, 8, t=np.asarray([8], np.int32)) == -1 and rows(2, 9) == -1 and acc.value == -5

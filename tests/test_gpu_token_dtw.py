"""-m gpu: token times by DTW over the alignment heads' cross-attention (wmi_set_token_dtw).

  kernels   wmi_selftest_dtw_matrix on crafted operands against the float64 judge (tests/dtw_f64.py: per-element bound, keys [M, T)
            poisoned, the output sentinel-filled and checked whole) at the smallest shapes where they can go wrong: M 1 / 3 (no median) /
            4 / 7 / 50 / 77 / 1500, T = M, M + 37, 1500, n from n_sot + 2 to 230, 6 and 20 heads, one pair / all heads of two layers / a
            list with gaps; wmi_selftest_dtw_path: the device equals the host form and the NumPy loop exactly, R 1 .. 448 (one row up to
            eight wavefronts, R > M included), ties / staircases / random
  driver    tiny.en, tiny, tiny q5_1; 11 s and 65 s of gated noise, the host's parameters and single_segment = False with max_len = 16,
            audio_ctx 0 and 256: mode 1 changes no token field, segment, text or counter of wmi_get_timings; for the last window the jumps
            are the NumPy DTW of the device's own matrix, the matrix is within the judge's bound of float64 on the query rows the pass used
            and the cross keys, the query rows of the f16 models are whisper_decode's of the same tokens bit for bit, and
            t_dtw = seek + 2 jump per text token; three windows each with its own seek; explicit pairs; wmi_full_batch (chunk mode 1);
            the node; beam search; mode 0 answers -1 and counts nothing"""
import ctypes as C

import numpy as np
import pytest

import dtw_f64 as dj
import golden_util as gu
import stage_compare as sc
from godot_whisper_amd import abi, host, runtime, synth

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ kernels
def _two_layers(H):
    return [(l, h) for l in (0, 1) for h in range(H)]


MATRIX_CASES = [
    # family, S, H, n, n_sot, M, T, pairs
    ("random", 384, 6, 3, 1, 1, 1, [(0, 3)]),
    ("random", 1280, 20, 9, 3, 1, 38, [(0, 0), (0, 19), (2, 7)]),
    ("random", 384, 6, 5, 3, 3, 3, _two_layers(6)),
    ("random", 384, 6, 9, 1, 3, 1500, [(1, 5)]),
    ("random", 1280, 20, 65, 3, 4, 41, [(0, 2), (0, 11), (1, 19)]),
    ("random", 384, 6, 9, 1, 7, 44, _two_layers(6)),
    ("random", 384, 6, 230, 3, 50, 87, [(0, 0), (0, 2), (2, 5)]),
    ("random", 384, 6, 65, 3, 50, 50, [(0, 4)]),
    ("random", 1280, 20, 65, 1, 77, 114, _two_layers(20)),
    ("random", 384, 6, 3, 1, 77, 1500, [(0, 0)]),
    ("random", 1280, 20, 230, 3, 1500, 1500, [(0, 1), (1, 0), (1, 18)]),
    ("random", 384, 6, 9, 1, 1500, 1500, [(0, 5)]),
    ("bands", 384, 6, 15, 3, 77, 114, [(0, 0), (0, 5), (1, 3)]),
    ("bands", 1280, 20, 62, 1, 1500, 1500, [(0, 13)]),
]


def device_path(lib, A, device=0):
    A = np.ascontiguousarray(A, np.float32)
    R, M = A.shape
    jumps = np.full(R, -7, np.int32); path = np.full((R + M, 2), -7, np.int32); n_path = C.c_int(-1)
    assert lib.wmi_selftest_dtw_path(device, R, M, A.ctypes.data, jumps.ctypes.data, path.ctypes.data, C.byref(n_path)) == 0
    assert 1 <= n_path.value <= R + M and (path[n_path.value:] == -7).all()
    return jumps, path[:n_path.value]


@pytest.mark.parametrize("i", range(len(MATRIX_CASES)), ids=[f"{c[0]}-S{c[1]}-n{c[3]}-M{c[5]}-T{c[6]}-P{len(c[7])}" for c in MATRIX_CASES])
def test_matrix_kernels_against_the_judge(product_lib, i):
    family, S, H, n, n_sot, M, T, pairs = MATRIX_CASES[i]
    make = dj.random_case if family == "random" else dj.band_case
    c = make(f"case{i}", S, H, n, n_sot, M, T, pairs, seed=100 + i)
    lh = np.asarray(pairs, np.int32).ravel()
    out = np.full((c.R, M), dj.SENTINEL32, np.uint32).view(np.float32)
    rc = product_lib.wmi_selftest_dtw_matrix(0, c.L, S, H, n, n_sot, M, T, c.q.ctypes.data, c.k.ctypes.data, lh.ctypes.data, len(pairs),
                                             out.ctypes.data)
    assert rc == 0, rc
    A64, bound = c.expected()
    ratio = dj.hold_matrix(out, A64, bound, c.name, hold=sc.hold)
    print(f"{c.name}: largest |d| / bound = {ratio:.4f}, largest bound = {bound.max():.3g}")
    if family == "bands":                                     # the closed form, end to end through the path kernel
        j, _ = device_path(product_lib, out)
        assert list(j) == list(c.starts)


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 225, 448])
@pytest.mark.parametrize("family", ["ties", "bands", "random"])
def test_path_kernel_is_the_host_form_and_the_numpy_loop(product_lib, family, R):
    for M in (1, 2, 50, 1500):
        A = dj.path_matrix(family, R, M)
        j, p = device_path(product_lib, A)
        dj.hold_path(A, j, p, (family, R, M))
        hj, hp = device_path(product_lib, A, device=-1)
        assert (hj == j).all() and hp.shape == p.shape and (hp == p).all(), (family, R, M)
        if family == "bands" and M >= R:
            assert list(j) == list(dj.staircase_jumps(R, M))
    if family == "ties" and R == 1:
        for name, T in dj.tie_matrices():
            dj.hold_path(T, *device_path(product_lib, T), name)


# ------------------------------------------------------------------------------------------------ driver
_models, _pcm = {}, {}
MODELS = ["tiny.en", "tiny", "tiny-q5_1"]


def model_of(name):
    if name not in _models:
        m = synth.make_model(name.split("-")[0], seed=4321)
        _models[name] = synth.quantize_model(m, "q5_1") if name.endswith("q5_1") else m
    return _models[name]


def pcm_of(seconds, seed=31):
    if (seconds, seed) not in _pcm:
        _pcm[(seconds, seed)] = synth.make_pcm(seconds, seed=seed, gate=True)
    return _pcm[(seconds, seed)]


def new_node(lib, name, token_dtw=False):
    node = host.SpeechToText(lib, token_dtw=token_dtw)
    node.set_language_model(model_of(name))
    assert node.ctx
    return node


@pytest.fixture(scope="module")
def nodes(product_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = new_node(product_lib, name)
        return made[name]
    yield get
    for n in made.values():
        n.close()


def params(node, audio_ctx=0, multi=False, **kw):
    """the host's parameters with n_max_text_ctx = 0 and temperature_inc = 0; multi: single_segment = False, max_len = 16"""
    p = node.full_params("", audio_ctx)
    p.n_max_text_ctx = 0
    p.temperature_inc = 0.0
    if multi:
        p.single_segment = False
        p.max_len = 16
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def counters(node):
    t6 = (C.c_int64 * 6)(); n5 = (C.c_int32 * 5)()
    node.lib.wmi_get_timings(node.ctx, t6, n5)
    return list(n5)


def dtw_timings(node):
    us, nw = C.c_int64(-1), C.c_int32(-1)
    node.lib.wmi_get_token_dtw_timings(node.ctx, C.byref(us), C.byref(nw))
    return us.value, nw.value


def run(node, token_dtw, p, pcm):
    """-> dict of whisper_full's result with the alignment mode `token_dtw`"""
    lib = node.lib
    assert node.set_token_dtw(token_dtw) >= 0
    c0, w0 = counters(node), dtw_timings(node)[1]
    r = node.transcribe(pcm, params=p)
    assert node.last_ret == 0, node.last_ret
    segs = [(lib.whisper_full_get_segment_t0(node.ctx, i), lib.whisper_full_get_segment_t1(node.ctx, i), lib.whisper_full_n_tokens(node.ctx, i))
            for i in range(lib.whisper_full_n_segments(node.ctx))]
    return {"tokens": gu.tokens_array(r), "text": bytes(r[0]), "segs": segs, "raw": r, "t_dtw": [d.get("t_dtw") for d in r[1:]],
            "counters": [a - b for a, b in zip(counters(node), c0)], "windows": dtw_timings(node)[1] - w0}


def frames_of(node):
    n_len_org = C.c_int()
    node.lib.wmi_mel_dims(node.ctx, None, C.byref(n_len_org), None)
    return n_len_org.value


def same_result(a, b):
    assert np.array_equal(a["tokens"], b["tokens"]) and a["text"] == b["text"] and a["segs"] == b["segs"] and len(a["tokens"]) > 0
    assert a["counters"] == b["counters"], (a["counters"], b["counters"])


def last_window(node):
    """dims, A, jumps, the query rows and the pairs of the last aligned window"""
    lib, ctx = node.lib, node.ctx
    v = [C.c_int() for _ in range(5)]
    assert lib.wmi_token_dtw_dims(ctx, *[C.byref(x) for x in v]) == 0
    n, n_sot, R, M, P = (x.value for x in v)
    assert R == n - n_sot - 1 and R >= 2 and M >= 1
    A = runtime.get_tensor(lib, ctx, "dtw_matrix").reshape(R, M)
    jumps = runtime.get_tensor(lib, ctx, "dtw_jumps").astype(np.int64)
    q = runtime.get_tensor(lib, ctx, "dtw_q").reshape(P, n, 64)
    lh = (C.c_int32 * (2 * P))()
    assert lib.wmi_token_dtw_heads(ctx, lh, P) == P
    return n, n_sot, R, M, A, jumps, q, [(lh[2 * i], lh[2 * i + 1]) for i in range(P)]


def check_last_window(node, res, seek, audio_ctx, f16_model):
    """the statements about the last window of the call that produced `res` (see the module docstring)"""
    lib, ctx = node.lib, node.ctx
    n, n_sot, R, M, A, jumps, q, pairs = last_window(node)
    eot = lib.whisper_token_eot(ctx)
    assert n_sot == (3 if lib.whisper_is_multilingual(ctx) else 1)
    # the path is defined bit for bit by the matrix
    ej, _ = dj.dtw_f32(A)
    assert jumps.shape == (R,) and (jumps == ej).all()
    assert (np.diff(jumps) >= 0).all() and jumps.min() >= 0 and jumps.max() < M
    # the matrix against float64 on the operands the pass used
    Lt = lib.whisper_model_n_text_layer(ctx); S = lib.whisper_model_n_text_state(ctx)
    ck = runtime.get_tensor(lib, ctx, "cross_k").reshape(Lt, -1, S)
    assert ck.shape[1] == (audio_ctx or 1500) and M <= ck.shape[1]
    q16 = q.astype(np.float16)
    assert np.array_equal(q16.astype(np.float32), q)
    kp = [ck[l][:M, 64 * h:64 * h + 64].astype(np.float16) for l, h in pairs]
    A64, bound = dj.matrix_f64(list(q16), kp, n_sot)
    ratio = dj.hold_matrix(A, A64, bound, "dtw_matrix", hold=sc.hold)
    print(f"last window: n = {n}, M = {M}, {len(pairs)} pairs, largest |d| / bound = {ratio:.4f}, bounded elements {np.isfinite(bound).mean():.3f}")
    # t_dtw: the last window's text tokens are the call's last R - 1 text tokens
    ids = res["tokens"][:, 0].astype(np.int64)
    t_dtw = np.asarray(res["t_dtw"], np.int64)
    assert (t_dtw[ids >= eot] == -1).all() and (t_dtw[ids < eot] >= 0).all()
    text = np.flatnonzero(ids < eot)[-(R - 1):]
    assert len(text) == R - 1
    if seek is None:                                          # (several segments: the last window starts where its times say, at or before its first segment)
        seek = int(t_dtw[text][0] - 2 * jumps[0])
        assert 0 <= seek <= max(s[0] for s in res["segs"]) and seek % 2 == 0
    assert (t_dtw[text] == seek + 2 * jumps[:R - 1]).all()
    assert (t_dtw[text] >= seek).all() and (t_dtw[text] < seek + 2 * M).all()
    if f16_model:                                            # the pass's query rows are whisper_decode's of the same tokens
        x = [lib.whisper_token_sot(ctx)]
        if n_sot == 3:
            x += [lib.whisper_token_lang(ctx, lib.whisper_full_lang_id(ctx)), lib.whisper_token_transcribe(ctx)]
        x += [lib.whisper_token_not(ctx)] + [int(i) for i in ids[text]] + [eot]
        assert len(x) == n
        xa = np.asarray(x, np.int32)
        assert lib.whisper_decode(ctx, xa.ctypes.data_as(C.POINTER(C.c_int32)), n, 0, 1) == 0
        dq = runtime.get_tensor(lib, ctx, "dec_cross_q").reshape(n, S)
        top = [(i, h) for i, (l, h) in enumerate(pairs) if l == Lt - 1]
        assert top
        for i, h in top:
            assert np.array_equal(q[i], dq[:, 64 * h:64 * h + 64]), (i, h)
    return M


@pytest.mark.parametrize("audio_ctx", [0, 256])
@pytest.mark.parametrize("multi", [False, True], ids=["host", "multi"])
@pytest.mark.parametrize("name", MODELS)
def test_short_clip_mode_1_against_mode_0(nodes, name, multi, audio_ctx):
    node = nodes(name)
    pcm = pcm_of(11.0)
    r0 = run(node, False, params(node, audio_ctx, multi), pcm)
    r1 = run(node, True, params(node, audio_ctx, multi), pcm)
    same_result(r0, r1)
    assert r0["windows"] == 0 and all(t is None for t in r0["t_dtw"])
    assert r1["windows"] >= 1 if multi else r1["windows"] == 1          # (multi: a window ends at its last timestamp token, the clip takes several)
    M = check_last_window(node, r1, None if multi else 0, audio_ctx, not name.endswith("q5_1"))
    full = min(audio_ctx or 1500, frames_of(node) // 2)       # seek_end = the frames of the 11 s
    assert M <= full if multi else M == full                  # (multi: the window's own seek and seek_delta decide)
    assert node.set_token_dtw(False) == 1


@pytest.mark.parametrize("name", MODELS)
def test_three_windows_each_with_its_own_seek(nodes, name):
    node = nodes(name)
    pcm = pcm_of(65.0)
    r0 = run(node, False, params(node), pcm)
    r1 = run(node, True, params(node), pcm)
    same_result(r0, r1)
    assert r1["windows"] == 3 and len(r1["segs"]) == 3                    # single_segment: a segment per window
    M = check_last_window(node, r1, 6000, 0, not name.endswith("q5_1"))
    assert M == (frames_of(node) - 6000) // 2 and 240 <= M <= 250         # min(3000, seek_end - 6000, 3000) / 2
    eot = node.lib.whisper_token_eot(node.ctx)
    first = 0
    for w, (_, _, cnt) in enumerate(r1["segs"]):
        ids = r1["tokens"][first:first + cnt, 0]; t = np.asarray(r1["t_dtw"][first:first + cnt], np.int64)[ids < eot]
        span = 3000 if w < 2 else 500
        assert len(t) > 0 and (np.diff(t) >= 0).all() and t.min() >= 3000 * w and t.max() < 3000 * w + span, (w, t)
        first += cnt
    node.set_token_dtw(False)


def test_explicit_pairs(nodes):
    node = nodes("tiny")
    pcm = pcm_of(11.0)
    r_def = run(node, True, params(node), pcm)
    A_def = last_window(node)[4]
    want = [(0, 1), (2, 3), (3, 0)]
    r_exp = run(node, want, params(node), pcm)
    same_result(r_def, r_exp)
    n, n_sot, R, M, A, jumps, q, pairs = last_window(node)
    assert pairs == want and A.shape == A_def.shape and not np.array_equal(A, A_def)
    check_last_window(node, r_exp, 0, 0, True)
    assert node.set_token_dtw([(4, 0)]) == -1 and node.set_token_dtw([(0, 6)]) == -1       # tiny: 4 layers of 6 heads; nothing changed
    node.set_token_dtw(False)


def test_full_batch_takes_the_general_driver(nodes):
    node = nodes("tiny.en"); lib = node.lib
    pcms = [pcm_of(11.0), pcm_of(9.0, seed=5), pcm_of(35.0, seed=9)]
    alone = [run(node, True, params(node), x) for x in pcms]
    assert node.set_token_dtw(True) == 1
    got = node.transcribe_batch(pcms, params=params(node))
    assert node.last_ret == 0 and node.last_modes == [1, 1, 1]
    for a, g in zip(alone, got):
        assert np.array_equal(gu.tokens_array(g), a["tokens"]) and bytes(g[0]) == a["text"]
        assert [d["t_dtw"] for d in g[1:]] == a["t_dtw"] and any(t >= 0 for t in a["t_dtw"])
    node.set_token_dtw(False)
    got0 = node.transcribe_batch(pcms, params=params(node))                # mode 0: lock-step again, no times
    assert node.last_modes == [0, 0, 0] and all("t_dtw" not in d for g in got0 for d in g[1:])
    assert lib.wmi_full_get_token_dtw(node.ctx, 0, 0) == -1


def test_node_delivers_t_dtw(product_lib):
    node = new_node(product_lib, "tiny.en", token_dtw=True)
    try:
        r = node.transcribe(pcm_of(11.0), params=params(node))
        assert node.last_ret == 0 and len(r) > 2 and all("t_dtw" in d for d in r[1:])
        eot = product_lib.whisper_token_eot(node.ctx)
        assert all((d["t_dtw"] >= 0) == (d["id"] < eot) for d in r[1:])
        assert dtw_timings(node)[1] == 1 and dtw_timings(node)[0] > 0
    finally:
        node.close()


def test_beam_search(product_lib):
    """a context per leg: the beams draw from the decoders' generators, which carry their state from call to call"""
    res = []
    for token_dtw in (False, True):
        node = new_node(product_lib, "tiny")
        try:
            p = params(node)
            p.strategy = abi.WHISPER_SAMPLING_BEAM_SEARCH
            p.beam_search.beam_size = 2
            res.append(run(node, token_dtw, p, pcm_of(11.0)))
            if token_dtw:
                check_last_window(node, res[-1], 0, 0, True)
        finally:
            node.close()
    same_result(res[0], res[1])


def test_mode_0_answers_nothing(product_lib):
    node = new_node(product_lib, "tiny.en")
    try:
        r = node.transcribe(pcm_of(11.0), params=params(node))
        lib, ctx = node.lib, node.ctx
        assert node.last_ret == 0 and len(r) > 2 and all("t_dtw" not in d for d in r[1:])
        assert all(lib.wmi_full_get_token_dtw(ctx, 0, j) == -1 for j in range(lib.whisper_full_n_tokens(ctx, 0)))
        assert lib.wmi_full_get_token_dtw(ctx, 5, 0) == -1 and lib.wmi_full_get_token_dtw(ctx, 0, -1) == -1
        assert lib.wmi_token_dtw_dims(ctx, None, None, None, None, None) == -1
        assert runtime_count(lib, ctx, "dtw_jumps") == 0 and runtime_count(lib, ctx, "dtw_matrix") == 0
        assert dtw_timings(node) == (0, 0)
    finally:
        node.close()


def runtime_count(lib, ctx, name):
    return lib.wmi_get_tensor(ctx, name.encode(), None, 0)

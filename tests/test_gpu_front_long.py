"""-m gpu: the front of a decoder layer as ONE launch (csrc/k_dec.hip: k_front) at every self-cache length.

Up to 64 cells the launch attends on one wavefront per head; beyond, its long-cache form runs k_self_attn_rows_long's arithmetic on
the head workgroup's four wavefronts.  Both are a launch structure over the arithmetic of the plain launches (q|k|v, self-attention,
out projection), so every result must be the same bits:

  1. the form is taken: a shape that fronts its short-cache steps fronts every longer one, eager, replayed and chained;
  2. the step's raw logits at every position up to the last cell, and again after a rewind, equal WMI_NO_FRONT=1's bit for bit;
  3. whisper_full through host.SpeechToText, uncapped and behind an initial_prompt that starts past cell 64, gives WMI_NO_FRONT=1's
     token records;
  4. a hand-off that does not complete inside the long form is reported, the step re-run, the stream unchanged.

A slow hand-off is the device being shared, and test 1 excuses at most 3 such steps per shape.  Seen on a shared device: 0 / 0 / 2 / 2 /
0 / 0 over the six shapes in one run of the file, 4 on base.en in another (three of the four on short-cache steps, whose kernels this
form does not touch) — that run fails test 1, as it should on a device that busy.

No checker decode here: the comparison with the compiled reference at every length is tests/test_gpu_decode_lengths.py's."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import stage_compare as sc
from godot_whisper_amd import abi, synth
from test_gpu_parity import sot_prompt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# forms of the greedy step (include/wmi_device.h: wmi_selftest_greedy_step)
LONG, CHAINED, GRAPH, PAIRED, FRONTED, BACKED, RERUN, SLOW, QUANT = 1, 2, 4, 8, 16, 32, 64, 128, 256
MAX_EXCUSED = 3          # steps per shape that may report a slow hand-off (a device shared with someone else's work)

T_FILE = time.time()


@pytest.fixture(scope="module", autouse=True)
def _file_duration():
    yield
    print(f"\ntest_gpu_front_long.py: {time.time() - T_FILE:.1f} s")


def _step(lib, ctx, tok, pos, nv):
    lg = np.empty(nv, np.float32); td = abi.whisper_token_data(); fm = C.c_int(0)
    rc = lib.wmi_selftest_greedy_step(ctx, int(tok), int(pos), sc._fptr(lg), C.byref(td), C.byref(fm))
    assert rc == 0, (tok, pos, rc)
    return lg, td, fm.value


# ------------------------------------------------------------------------------------------------ 1. the form is taken
FORM_SHAPES = ["base.en", "tiny.en", "small", "medium-slice", "v3-slice", "micro.en"]
MUST_FRONT = {"base.en", "tiny.en", "small"}          # (v3-slice: S = 1280, micro.en: odd layer count — neither fronts)


@pytest.mark.parametrize("shape", FORM_SHAPES)
def test_long_caches_take_the_one_launch_front(product_lib, shape):
    t0 = time.time()
    lib = product_lib
    prod = sc.ProductSide(lib, synth.make_model(shape, seed=1234))
    try:
        ctx = prod.ctx
        prod.mel(synth.make_pcm(30.0, seed=1234)); prod.encode(0, 0)
        n_ctx = lib.whisper_n_text_ctx(ctx); nv = prod.NV; eot = lib.whisper_token_eot(ctx)
        rng = np.random.default_rng(4321)
        prompt = sot_prompt(None, prod)
        seen, excused = [], 0                           # (n_kv, forms) of every step that was not excused
        for sweep in range(2):                           # the second one after a rewind through whisper_decode
            prod.decode(prompt, 0)
            tok = int(rng.integers(0, eot))
            for pos in range(len(prompt), n_ctx):
                _, td, fm = _step(lib, ctx, tok, pos, nv)
                assert not fm & RERUN, (shape, pos, hex(fm))
                if fm & SLOW:                            # correct, but the hand-off waited: re-arm the one-launch forms and go on
                    excused += 1
                    st = (C.c_int32 * 3)()
                    assert lib.wmi_pair_status(ctx, st, 1) == 0
                else:
                    seen.append((pos + 1, fm))
                tok = td.id if td.id < eot else int(rng.integers(0, eot))       # the step's own pick: the next step is chained
        count = {}
        for n_kv, fm in seen:
            count[hex(fm)] = count.get(hex(fm), 0) + 1
        print(f"\n{shape}: forms {dict(sorted(count.items()))}, excused {excused}, {time.time() - t0:.1f} s")
        assert excused <= MAX_EXCUSED, (shape, excused, count)
        short = [fm for n_kv, fm in seen if n_kv <= 64]
        long_ = [(n_kv, fm) for n_kv, fm in seen if n_kv > 64]
        assert short and len(long_) > 2 * (n_ctx - 64) - 16, (shape, len(short), len(long_))
        assert not any(fm & LONG for fm in short) and all(fm & LONG for _, fm in long_), (shape, count)
        fronts_short = all((fm & (PAIRED | FRONTED)) == (PAIRED | FRONTED) for fm in short)
        if shape in MUST_FRONT:
            assert fronts_short, (shape, count)
        if fronts_short:
            bad = [(n_kv, hex(fm)) for n_kv, fm in long_ if (fm & (LONG | PAIRED | FRONTED)) != (LONG | PAIRED | FRONTED)]
            assert not bad, (shape, bad[:8], count)
            has = lambda want, mask: any((fm & mask) == want for _, fm in long_)
            assert has(0, GRAPH) and has(GRAPH, GRAPH), (shape, count)          # an eager and a replayed long fronted step
            assert has(CHAINED, CHAINED), (shape, count)
        else:
            assert not any(fm & FRONTED for fm in short), (shape, count)       # (fronted on some short steps only: not a shape's property)
            assert not any(fm & FRONTED for _, fm in long_), (shape, count)
    finally:
        prod.close()


# ------------------------------------------------------------------------------------------------ 2. the same bits at every length
_SWEEP_SCRIPT = r"""
import ctypes as C, json, sys
sys.path.insert(0, ROOT_PLACEHOLDER); sys.path.insert(0, ROOT_PLACEHOLDER + "/tests")
import numpy as np
import __graft_entry__ as entry
entry.load_package()
from godot_whisper_amd import abi, runtime, synth
import stage_compare as sc
from test_gpu_parity import sot_prompt
lib = runtime.require_gpu(); runtime.silence_logs(lib)
shape, path = sys.argv[1], sys.argv[2]
prod = sc.ProductSide(lib, synth.make_model(shape, seed=1234)); ctx = prod.ctx
prod.mel(synth.make_pcm(30.0, seed=1234)); prod.encode(0, 0)
n_ctx = lib.whisper_n_text_ctx(ctx); nv = prod.NV; eot = lib.whisper_token_eot(ctx)
rng = np.random.default_rng(4321)
prompt = sot_prompt(None, prod)
positions = list(range(len(prompt), n_ctx))
def step(tok, pos):
    lg = np.empty(nv, np.float32); td = abi.whisper_token_data(); fm = C.c_int(0)
    assert lib.wmi_selftest_greedy_step(ctx, int(tok), int(pos), sc._fptr(lg), C.byref(td), C.byref(fm)) == 0, (tok, pos)
    if fm.value & 128:                                   # a slow hand-off: allow the one-launch forms again instead of 512 plain steps
        assert lib.wmi_pair_status(ctx, None, 1) == 0
    return lg, td.id, fm.value
logits = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(2, len(positions), nv))
picks = [[], []]; forms = [[], []]; fed = []
# sweep 0 feeds the step its own picks; sweep 1, after a rewind through whisper_decode, the same tokens
prod.decode(prompt, 0)
tok = int(rng.integers(0, eot))
for i, pos in enumerate(positions):
    lg, pick, fm = step(tok, pos)
    logits[0, i] = lg; picks[0].append(pick); forms[0].append(fm); fed.append(tok)
    tok = pick if pick < eot else int(rng.integers(0, eot))
prod.decode(prompt, 0)
for i, pos in enumerate(positions):
    lg, pick, fm = step(fed[i], pos)
    logits[1, i] = lg; picks[1].append(pick); forms[1].append(fm)
logits.flush(); del logits
prod.close()
print("RESULT" + json.dumps({"positions": positions, "picks": picks, "forms": forms, "fed": fed}))
""".replace("ROOT_PLACEHOLDER", repr(ROOT))


def _run_sweep(shape, path, env_extra):
    env = dict(os.environ); env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _SWEEP_SCRIPT, shape, str(path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")][-1]
    return json.loads(line[len("RESULT"):])


@pytest.mark.parametrize("shape", ["base.en", "tiny.en", "small", "medium-slice"])
def test_fronted_steps_equal_the_plain_launches_at_every_length(tmp_path, shape):
    t0 = time.time()
    pa, pb = tmp_path / "front.npy", tmp_path / "plain.npy"
    try:
        a = _run_sweep(shape, pa, {}); b = _run_sweep(shape, pb, {"WMI_NO_FRONT": "1"})
        positions = a["positions"]
        assert positions == b["positions"] and a["fed"] == b["fed"], shape
        # the ragged quarters of P.V (65 .. 68 cells: the last quarter is the short one) and the last cell of the text context
        cells = {pos + 1 for pos in positions}
        assert {65, 66, 67, 68, 448} <= cells and cells >= set(range(8, 449)), (shape, min(cells), max(cells))
        assert not any(fm & FRONTED for sw in b["forms"] for fm in sw), shape
        la, lb = np.load(pa, mmap_mode="r"), np.load(pb, mmap_mode="r")
        assert la.shape == lb.shape == (2, len(positions), la.shape[2])
        for sweep in range(2):
            for i, pos in enumerate(positions):
                if not np.array_equal(la[sweep, i], lb[sweep, i]):
                    d = np.abs(np.asarray(la[sweep, i], np.float64) - np.asarray(lb[sweep, i], np.float64))
                    pytest.fail(f"{shape}: sweep {sweep}, first differing position {pos} ({pos + 1} cells): forms {hex(a['forms'][sweep][i])} "
                                f"against {hex(b['forms'][sweep][i])}, max |d| {d.max():.3e} in {int((d > 0).sum())} logits")
            assert a["picks"][sweep] == b["picks"][sweep], (shape, sweep)
        fa = [fm for sw in a["forms"] for fm in sw]
        n_long_fronted = sum(1 for fm in fa if (fm & (LONG | FRONTED)) == (LONG | FRONTED))
        print(f"\n{shape}: {2 * len(positions)} steps, {n_long_fronted} long fronted, {sum(1 for fm in fa if fm & SLOW)} slow, {time.time() - t0:.1f} s")
        assert not any(fm & RERUN for fm in fa), shape
        # the comparison must cover the kernel: most long steps of each sweep of the default run took the long fronted form
        for sweep in range(2):
            n_long = sum(1 for fm in a["forms"][sweep] if fm & LONG)
            n_lf = sum(1 for fm in a["forms"][sweep] if (fm & (LONG | FRONTED)) == (LONG | FRONTED))
            assert n_long == 448 - 64 and 2 * n_lf > n_long, (shape, sweep, n_long, n_lf)
    finally:
        for p in (pa, pb):
            if p.exists():
                p.unlink()


# ------------------------------------------------------------------------------------------------ 3. / 4. the host's pattern
SENTENCE = " The quick brown fox jumps over the lazy dog near the river bank."
PROMPT = SENTENCE * 8

_HOST_SCRIPT = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, ROOT_PLACEHOLDER)
import __graft_entry__ as entry
entry.load_package()
from godot_whisper_amd import host, runtime, synth
lib = runtime.require_gpu(); runtime.silence_logs(lib)
prompt = sys.argv[1]
out = {}
for shape in ("base.en", "small"):
    node = host.SpeechToText(lib); node.set_language_model(synth.make_model(shape, seed=4242))
    if not shape.endswith(".en"): node.language = "de"
    for case in ("uncapped", "prompt"):
        res = []; status = []
        assert lib.wmi_pair_status(node.ctx, None, 1) == 0                             # each case starts with the one-launch forms allowed
        for rep in range(6):                               # enough steps for the long form's graphs to be captured and replayed
            p = node.full_params(prompt if case == "prompt" else "", 0); p.max_tokens = 0; p.temperature_inc = 0.0
            r = node.transcribe(synth.make_pcm(30.0, seed=900 + rep % 2), params=p)
            res.append([[int(t["id"]), int(t["tid"]), float(t["p"]), float(t["plog"]), int(t["t0"]), int(t["t1"])] for t in r[1:]])
            st = (C.c_int32 * 3)()
            assert lib.wmi_pair_status(node.ctx, st, 1 if rep % 2 == 0 else 0) == 0      # (re-armed after every other transcription)
            status.append(list(st))
        out["%s/%s" % (shape, case)] = res; out["status:%s/%s" % (shape, case)] = status
        # the launches of the call's last step (in-kernel stamps of a replay; the plain self-attention launch carries none)
        # (not in the run that withholds a granule: the replay would leave its report in the status word)
        buf = (C.c_double * (6 * 256))(); n = lib.wmi_step_stamps(node.ctx, buf, 256, 1) if not os.environ.get("WMI_FRONT_WITHHOLD") else -1
        out["launches:%s/%s" % (shape, case)] = [sum(1 for i in range(max(n, 0)) if buf[6 * i + 3] > 0), int(lib.whisper_model_n_text_layer(node.ctx))]
    node.close()
print("RESULT" + json.dumps(out))
""".replace("ROOT_PLACEHOLDER", repr(ROOT))


def _run_host(env_extra):
    env = dict(os.environ); env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _HOST_SCRIPT, PROMPT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")][-1]
    return json.loads(line[len("RESULT"):])


@pytest.fixture(scope="module")
def host_default_run():
    return _run_host({})


def test_the_prompt_starts_the_call_past_cell_64(product_lib):
    """CPU side: whisper_full decodes [prev] + the prompt's tokens (at most n_text_ctx / 2) + the SOT sequence before its first pick,
    so a prompt of 64 .. 200 tokens puts every greedy step of the call on a cache of more than 64 cells and leaves room to decode."""
    lib = product_lib
    for shape in ("micro.en", "micro"):                 # the two vocabularies (base.en's, small's)
        m = synth.make_model(shape, seed=4242)
        buf = C.create_string_buffer(m, len(m))
        ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(m))
        assert ctx
        try:
            toks = (C.c_int32 * 1024)()
            n = lib.whisper_tokenize(ctx, PROMPT.encode("utf-8"), toks, 1024)
            assert 64 <= n <= 200, (shape, n)
        finally:
            lib.whisper_free(ctx)


def test_whisper_full_uncapped_and_with_a_prompt_is_bit_identical(host_default_run):
    other = _run_host({"WMI_NO_FRONT": "1"})
    for key, runs in host_default_run.items():
        if key.startswith("status:"):
            assert all(s[0] == 0 for s in runs), (key, runs)                       # nothing re-run
            continue
        if key.startswith("launches:"):
            # behind the prompt every step is on a long cache: its last one took one stamped launch per layer (k_front) where the plain
            # form takes two (q|k|v, out projection) — whisper_full did run the long fronted form
            if key.endswith("/prompt"):
                assert runs[0] > 0 and other[key][0] - runs[0] == runs[1], (key, runs, other[key])
            continue
        assert len(runs[0]) > 0, key
        for a, b in zip(runs, other[key]):
            assert a == b, key                          # ids, tids, probabilities (exact f32 values) and token times
    assert max(len(r) for r in host_default_run["base.en/uncapped"]) > 64          # (the uncapped call does reach long caches)


def test_a_failed_hand_off_inside_the_long_front_launch_is_reported_and_the_step_rerun(host_default_run):
    """WMI_FRONT_WITHHOLD=6: wavefront 5 of k_front's phase 1 never publishes (rows 20 .. 23 of q: head 0's gather waits in vain, and
    with it every consumer of the attention row); WMI_PAIR_SPIN_CAP: give up after 3000 polls.  Behind the prompt every greedy step of a
    call is on a long cache, so there the launch that reports is the long form's.  Reported through the status word, the step re-run
    in the plain launches, the stream unchanged."""
    got = _run_host({"WMI_FRONT_WITHHOLD": "6", "WMI_PAIR_SPIN_CAP": "3000"})
    for key, runs in got.items():
        if key.startswith("status:"):
            fallbacks = [s[0] for s in runs]
            assert fallbacks[0] >= 1 and fallbacks[-1] >= fallbacks[0] + 2, (key, runs)         # one per armed transcription (the count runs on across a node's cases)
            assert all(s[2] & 1 for s in runs), (key, runs)                        # ... and the one-launch form stays off behind each
            continue
        if key.startswith("launches:"):
            continue
        for a, b in zip(host_default_run[key], runs):
            assert a == b, key

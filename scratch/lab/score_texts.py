"""Lab: "which of my N commands was said?" three ways on base.en (synthetic weights), N = 4, 16 and 64 command texts of 1 - 6 tokens
(the style of the reference's examples/command/commands.txt), 4 s of bench.py's noise, one encoded window.

  (a) wmi_score_texts on the encoded window: the prefix batch, one candidate pass, one wait
  (b) the same numbers by what the library offered before: per text whisper_decode of the prefix, then one whisper_decode step per token
      (whisper_decode hands out its last row's logits only), every row's 207 KB of logits to the host and a numpy float64 log-soft-max there
  (c) the grammar-device greedy call (wmi_set_grammar_device 1) with the list as a grammar: whisper_full, its decode + sample timers
      beside the wall clock (the wall clock includes log-mel and encoder, which (a) and (b) do not)

The routes take turns inside every repetition, the first --warm repetitions dropped; medians (min - max) of --reps, milliseconds.
Then the headline, `bench.py --gpus 1`, from fresh child processes, this tree and --parent (a built tree of the parent commit) taking turns.

    python scratch/lab/score_texts.py [--root DIR] [--parent DIR] [--reps 20] [--warm 3] [--bench-runs 3]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(pathlib.Path(__file__).resolve().parents[2]))
ap.add_argument("--parent", default=None)
ap.add_argument("--shape", default="base.en")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, args.root)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
import numpy as np  # noqa: E402
from godot_whisper_amd import abi, host, runtime, synth  # noqa: E402

VERBS = ["turn", "go", "open", "close", "stop", "start", "play", "pause", "enable", "disable", "select", "drop", "take", "use", "show", "hide"]
TAILS = ["", " left", " right", " the door", " the map", " all units", " now", " the next one", " music", " the red flag please"]


def summary(ts):
    return "%.3f (%.3f - %.3f)" % (statistics.median(ts), min(ts), max(ts))


def timers(lib, ctx):
    t6 = (C.c_int64 * 6)(); n5 = (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return list(t6)


def list_grammar(texts):
    """root ::= " text_0" | " text_1" | ..."""
    rule = []
    for i, t in enumerate(texts):
        if i:
            rule.append((abi.GRETYPE_ALT, 0))
        rule += [(abi.GRETYPE_CHAR, ord(ch)) for ch in " " + t]
    return [rule]


def headline(root):
    root = str(pathlib.Path(root).resolve())
    cmd = [sys.executable, str(pathlib.Path(root) / "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=280)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


lib = runtime.require_gpu()
runtime.silence_logs(lib)
node = host.SpeechToText(lib)
node.language = "en"
node.set_language_model(synth.make_model(args.shape, seed=1234))
ctx = node.ctx
pcm = synth.make_pcm(4.0, seed=1234)
fp = pcm.ctypes.data_as(C.POINTER(C.c_float))
nv = lib.whisper_n_vocab(ctx)
pool = []
for v in VERBS:
    for t in TAILS:
        y = node.tokenize(" " + v + t)
        if 1 <= len(y) <= 6:
            pool.append((v + t, y))
prefix = [lib.whisper_token_sot(ctx), lib.whisper_token_not(ctx)]
eot = lib.whisper_token_eot(ctx)


def encode():
    assert lib.whisper_pcm_to_mel(ctx, fp, pcm.size, 4) == 0 and lib.whisper_encode(ctx, 0, 4) == 0


def route_a(toks):
    flat = np.asarray([t for y in toks for t in y], np.int32); nt = np.asarray([len(y) for y in toks], np.int32)
    out = (abi.wmi_text_score * len(toks))(); lp = np.zeros(int(nt.sum()) + len(toks), np.float32)
    p = lib.wmi_score_default_params()
    t0 = time.perf_counter()
    rc = lib.wmi_score_texts(ctx, p, flat.ctypes.data_as(C.c_void_p), nt.ctypes.data_as(C.c_void_p), len(toks), out, lp.ctypes.data_as(C.c_void_p))
    dt = 1e3 * (time.perf_counter() - t0)
    assert rc == 0
    return dt, [o.sum_logprob for o in out]


def last_logits(tokens, n_past):
    t = np.asarray(tokens, np.int32)
    assert lib.whisper_decode(ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, n_past, 4) == 0
    return np.ctypeslib.as_array(lib.whisper_get_logits(ctx), shape=(t.size * nv,))[-nv:].astype(np.float64)


def lsm(l, t):
    m = l.max()
    return float(l[t] - m - np.log(np.exp(l - m).sum()))


def route_b(toks):
    t0 = time.perf_counter()
    sums = []
    for y in toks:
        l = last_logits(prefix, 0)
        s = 0.0
        for i, t in enumerate(list(y) + [eot]):
            s += lsm(l, t)
            if i < len(y):
                l = last_logits([y[i]], len(prefix) + i)
        sums.append(s)
    return 1e3 * (time.perf_counter() - t0), sums


def route_c(texts):
    p = lib.whisper_full_default_params(abi.WHISPER_SAMPLING_GREEDY)
    p.language = b"en"; p.temperature_inc = 0.0; p.print_progress = False
    p.no_timestamps = True; p.single_segment = True; p.max_tokens = 8
    ptrs, n_rules, keep = abi.make_grammar(list_grammar(texts))
    p.grammar_rules = C.cast(ptrs, C.c_void_p); p.n_grammar_rules = n_rules; p.i_start_rule = 0; p.grammar_penalty = 100.0
    node.set_grammar_device(True)
    ta = timers(lib, ctx)
    t0 = time.perf_counter()
    r = node.transcribe(pcm, params=p)
    dt = 1e3 * (time.perf_counter() - t0)
    tb = timers(lib, ctx)
    assert node.last_ret == 0
    del keep
    return dt, 1e-3 * sum(tb[i] - ta[i] for i in (2, 3, 4, 5)), r[0].decode(errors="replace") if r else ""


for N in (4, 16, 64):
    rng = np.random.default_rng(N)
    pick = [pool[i] for i in rng.choice(len(pool), N, replace=False)]
    texts, toks = [t for t, _ in pick], [y for _, y in pick]
    ta, tb, tc, tcd = [], [], [], []
    us0, nc0, nl0 = C.c_int64(), C.c_int32(), C.c_int32()
    lib.wmi_get_score_timings(ctx, C.byref(us0), C.byref(nc0), C.byref(nl0))
    worst = 0.0
    for it in range(args.reps + args.warm):
        order = "abc" if it % 2 == 0 else "cba"
        for r in order:
            if r == "a":
                encode(); dt, sa = route_a(toks)
                if it >= args.warm:
                    ta.append(dt)
            elif r == "b":
                encode(); dt, sb = route_b(toks)
                if it >= args.warm:
                    tb.append(dt)
            else:
                dt, dec, text = route_c(texts)
                if it >= args.warm:
                    tc.append(dt); tcd.append(dec)
        worst = max(worst, max(abs(a - b) for a, b in zip(sa, sb)))
    us, nc, nl = C.c_int64(), C.c_int32(), C.c_int32()
    lib.wmi_get_score_timings(ctx, C.byref(us), C.byref(nc), C.byref(nl))
    print(json.dumps({"N": N, "tokens per text": [len(y) for y in toks][:16], "rows scored": int(sum(len(y) + 1 for y in toks)),
                      "(a) wmi_score_texts ms": summary(ta), "(b) whisper_decode per row + host log-soft-max ms": summary(tb),
                      "(c) grammar-device whisper_full ms": summary(tc), "(c) its prompt + decode + sample timers ms": summary(tcd),
                      "(b) / (a)": round(statistics.median(tb) / statistics.median(ta), 1), "(c) picked": text,
                      "(a) best": texts[int(np.argmax(sa))], "max |sum_logprob (a) - (b)|": worst,
                      "score kernels' launches per call": (nl.value - nl0.value) // max(1, nc.value - nc0.value)}), flush=True)
node.close()
if args.bench_runs > 0:
    trees = [("this tree", args.root)] + ([("parent", args.parent)] if args.parent else [])
    got = {name: [] for name, _ in trees}
    for _ in range(args.bench_runs):
        for name, root in trees:
            got[name].append(headline(root))
    keys = [k for k, v in got["this tree"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
    out = {"leg": "headline: bench.py --gpus 1 --steps %d --warmup %d" % (args.bench_steps, args.bench_warmup), "runs": args.bench_runs}
    for name, _ in trees:
        out[name] = {k: [r.get(k) for r in got[name]] for k in keys}
    print(json.dumps(out), flush=True)

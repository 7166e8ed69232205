"""Lab: what token alignment (wmi_set_token_dtw) adds to a window, and the headline beside the parent commit's.

Per shape (default base.en and small; 30 s chunks of bench.py's noise, the host's parameters with temperature_inc = 0), whisper_full is timed
with the mode off and on, alternating inside every repetition, the first --warm repetitions dropped; medians, minima and maxima.  Then the
added time is split two ways, each figure a median of its own:

  total        wmi_get_token_dtw_timings / windows: the pass, the matrix launches, the path and the window's one wait (the product's own timer)
  pass         whisper_decode of the same n tokens on the same context: the teacher-forced batch alone, host clock (it ends in a wait of its own)
  matrix+path  total - pass: the score / statistics / accumulate launches of every layer with pairs, the finish launch and the path kernel

(The path kernel alone is not split off: wmi_selftest_dtw_path allocates, copies and frees around it — 4 to 250 ms of host time when tried —
and says nothing about the kernel.)

--large adds large-v3 q5_1 with its default 320 pairs (synthesising and quantising that model takes minutes of host time).  Then the headline
figure — `bench.py --gpus 1`, which runs in mode 0 — from a fresh child process, --bench-runs times; with --parent DIR (a built tree of the
parent commit) the same from that tree, the two alternating.  Prints one JSON line per shape and one for the headline.

    python scratch/lab/token_dtw.py [--root DIR] [--parent DIR] [--shapes base.en,small] [--large] [--reps 20] [--warm 5] [--bench-runs 3]
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
ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its headline beside this tree's")
ap.add_argument("--shapes", default="base.en,small")
ap.add_argument("--large", action="store_true", help="also large-v3 q5_1 (320 default pairs)")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, args.root)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
import numpy as np  # noqa: E402
from godot_whisper_amd import host, runtime, synth  # noqa: E402


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def dtw_timer(lib, ctx):
    us, nw = C.c_int64(), C.c_int32()
    lib.wmi_get_token_dtw_timings(ctx, C.byref(us), C.byref(nw))
    return us.value, nw.value


def shape_legs(lib, shape, quant=None):
    model = synth.make_model(shape, seed=1234)
    if quant:
        model = synth.quantize_model(model, quant)
    node = host.SpeechToText(lib)
    node.language = "en"
    node.set_language_model(model)
    del model
    ctx = node.ctx
    pcm = synth.make_pcm(30.0, seed=1234)
    times = {"off": [], "on": []}
    per_window = []
    for it in range(args.reps + args.warm):
        for name in (("off", "on") if it % 2 == 0 else ("on", "off")):
            p = node.full_params("", 0)
            p.temperature_inc = 0.0
            node.set_token_dtw(name == "on")
            us0, n0 = dtw_timer(lib, ctx)
            t0 = time.perf_counter()
            r = node.transcribe(pcm, params=p)
            dt = 1e3 * (time.perf_counter() - t0)
            assert node.last_ret == 0
            us1, n1 = dtw_timer(lib, ctx)
            if it >= args.warm:
                times[name].append(dt)
                if name == "on" and n1 > n0:
                    per_window.append(1e-3 * (us1 - us0) / (n1 - n0))
    # the last aligned window's own dimensions and matrix, for the split
    v = [C.c_int() for _ in range(5)]
    assert lib.wmi_token_dtw_dims(ctx, *[C.byref(x) for x in v]) == 0
    n, n_sot, R, M, P = (x.value for x in v)
    ids = [d["id"] for d in r[1:] if d["id"] < lib.whisper_token_eot(ctx)][-(R - 1):]
    x = [lib.whisper_token_sot(ctx)]
    if n_sot == 3:
        x += [lib.whisper_token_lang(ctx, lib.whisper_full_lang_id(ctx)), lib.whisper_token_transcribe(ctx)]
    x = np.asarray(x + [lib.whisper_token_not(ctx)] + ids + [lib.whisper_token_eot(ctx)], np.int32)
    t_pass = []
    for it in range(args.reps + args.warm):
        t0 = time.perf_counter()
        assert lib.whisper_decode(ctx, x.ctypes.data_as(C.POINTER(C.c_int32)), len(x), 0, 1) == 0
        if it >= args.warm:
            t_pass.append(1e3 * (time.perf_counter() - t0))
    node.close()
    total = statistics.median(per_window)
    out = {"shape": shape + ("-" + quant if quant else ""), "n": n, "R": R, "M": M, "pairs": P, "reps": args.reps,
           "whisper_full off": summary(times["off"]), "whisper_full on": summary(times["on"]),
           "added_per_window_ms": summary(per_window), "pass_ms": summary(t_pass),
           "matrix_and_path_ms (total - pass)": round(total - statistics.median(t_pass), 3)}
    print(json.dumps(out), flush=True)


def headline(root):
    """one `bench.py --gpus 1` in a fresh child process; its JSON result line"""
    root = str(pathlib.Path(root).resolve())
    cmd = [sys.executable, str(pathlib.Path(root) / "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=280)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


lib = runtime.require_gpu()
runtime.silence_logs(lib)
for shape in [s for s in args.shapes.split(",") if s]:
    shape_legs(lib, shape)
if args.large:
    shape_legs(lib, "large-v3", "q5_1")
if args.bench_runs > 0:
    trees = [("this tree", args.root)] + ([("parent", args.parent)] if args.parent else [])
    got = {name: [] for name, _ in trees}
    for _ in range(args.bench_runs):
        for name, root in trees:
            got[name].append(headline(root))
    keys = [k for k, v in got["this tree"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
    out = {"headline": "bench.py --gpus 1 --steps %d --warmup %d, mode 0" % (args.bench_steps, args.bench_warmup), "runs": args.bench_runs}
    for name, _ in trees:
        out[name] = {k: [r.get(k) for r in got[name]] for k in keys}
    print(json.dumps(out), flush=True)

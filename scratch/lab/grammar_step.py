"""Lab: what a grammar-constrained sampling step costs on the host route (wmi_set_grammar_device 0) and on the device route (1).

base.en (synthetic weights), 20 s of bench.py's noise, the colour-list grammar of tests/golden_util.py, max_tokens = 24, no timestamps,
greedy and beam search 3.  whisper_full is timed with the mode 0 and 1 in the same sitting, taking turns inside every repetition, the
first --warm repetitions dropped; medians, minima and maxima of --reps.  Per call: the wall clock around whisper_full.  Per step: the
product's own timers of the decode and sampling phases (wmi_get_timings: decode + batched decode + sample) over the call's sampling
steps, and the sampling phase alone — what the mode moves.

Then k_grammar_reject on its own, by events around the launch (wmi_selftest_grammar where = 1, wmi_grammar_status.reject_us): one row at
the initial state and at a mid-word state (behind " red, gre"), and 3 rows (a beam step).

Then the headline — `bench.py --gpus 1`, which sets no grammar — from a fresh child process, --bench-runs times; with --parent DIR (a
built tree of the parent commit) the same from that tree, the two taking turns.  One JSON line per leg.

    python scratch/lab/grammar_step.py [--root DIR] [--parent DIR] [--reps 20] [--warm 3] [--bench-runs 3]
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
ap.add_argument("--shape", default="base.en")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, args.root)
sys.path.insert(0, str(pathlib.Path(args.root) / "tests"))
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
import numpy as np  # noqa: E402
from godot_whisper_amd import abi, host, runtime, synth  # noqa: E402
import golden_util as gu  # noqa: E402


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def timers(lib, ctx):
    t6 = (C.c_int64 * 6)(); n5 = (C.c_int32 * 5)()
    lib.wmi_get_timings(ctx, t6, n5)
    return list(t6), list(n5)


def call_legs(lib, node, pcm, beam):
    times = {0: [], 1: []}; step = {0: [], 1: []}; samp = {0: [], 1: []}
    status = {}
    for it in range(args.reps + args.warm):
        for mode in ((0, 1) if it % 2 == 0 else (1, 0)):
            p = node.lib.whisper_full_default_params(abi.WHISPER_SAMPLING_BEAM_SEARCH if beam else abi.WHISPER_SAMPLING_GREEDY)
            p.language = b"en"; p.temperature_inc = 0.0; p.print_progress = False
            p.no_timestamps = True; p.single_segment = True; p.max_tokens = 24
            if beam:
                p.beam_search.beam_size = 3; p.greedy.best_of = 1
            ptrs, n_rules, keep = abi.make_grammar(gu.colour_list_grammar())
            p.grammar_rules = C.cast(ptrs, C.c_void_p); p.n_grammar_rules = n_rules; p.i_start_rule = 0; p.grammar_penalty = 100.0
            node.set_grammar_device(mode == 1)
            ta, _ = timers(lib, node.ctx)
            t0 = time.perf_counter()
            r = node.transcribe(pcm, params=p)
            dt = 1e3 * (time.perf_counter() - t0)
            assert node.last_ret == 0
            tb, _ = timers(lib, node.ctx)
            steps = max(1, len(r) - 1)
            if it >= args.warm:
                times[mode].append(dt)
                step[mode].append(1e-3 * ((tb[2] - ta[2]) + (tb[3] - ta[3]) + (tb[5] - ta[5])) / steps)
                samp[mode].append(1e-3 * (tb[5] - ta[5]) / steps)
            status[mode] = (node.grammar_status(), steps, r[0])
            del keep
    out = {"leg": "beam 3" if beam else "greedy", "shape": args.shape, "reps": args.reps, "steps": status[1][1], "text mode 1": status[1][2].decode(errors="replace"),
           "device steps / host rows (mode 1)": [status[1][0]["steps_device"], status[1][0]["rows_host"]]}
    for mode in (0, 1):
        out[f"mode {mode}"] = {"call_ms": summary(times[mode]), "step_ms (decode + sample timers / steps)": summary(step[mode]),
                               "sample_ms per step": summary(samp[mode])}
    out["mode 0 / mode 1, per step"] = round(statistics.median(step[0]) / statistics.median(step[1]), 3)
    out["mode 0 / mode 1, sampling per step"] = round(statistics.median(samp[0]) / statistics.median(samp[1]), 3)
    out["mode 0 / mode 1, per call"] = round(statistics.median(times[0]) / statistics.median(times[1]), 3)
    print(json.dumps(out), flush=True)


def reject_legs(lib, node):
    ctx = node.ctx
    p = node.lib.whisper_full_default_params(abi.WHISPER_SAMPLING_GREEDY)
    ptrs, n_rules, keep = abi.make_grammar(gu.colour_list_grammar())
    p.grammar_rules = C.cast(ptrs, C.c_void_p); p.n_grammar_rules = n_rules; p.i_start_rule = 0
    nv = lib.whisper_n_vocab(ctx)
    buf = (C.c_int32 * 64)()
    n = lib.whisper_tokenize(ctx, b" red, gre", buf, 64)
    mid = np.asarray(list(buf[:n]), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = {"leg": "k_grammar_reject alone, microseconds by events", "reps": args.reps}
    for name, hists in (("initial state, 1 row", [np.zeros(0, np.int32)]), ("mid-word state, 1 row", [mid]),
                        ("3 rows (initial, mid-word, initial)", [np.zeros(0, np.int32), mid, np.zeros(0, np.int32)])):
        flat = np.concatenate(hists + [np.zeros(1, np.int32)]).astype(np.int32)
        nh = np.asarray([h.size for h in hists], np.int32)
        mask = np.zeros((len(hists), nv), np.uint8); over = np.zeros(8, np.uint32)
        us = []
        for it in range(args.reps + args.warm):
            assert lib.wmi_selftest_grammar(ctx, p, 1, len(hists), vp(flat), vp(nh), vp(mask), vp(over)) == 0 and not over.any()
            if it >= args.warm:
                us.append(node.grammar_status()["reject_us"])
        out[name] = dict(summary(us), rejected=[int(m.sum()) for m in mask])
    del keep
    print(json.dumps(out), flush=True)


def headline(root):
    """one `bench.py --gpus 1` in a fresh child process; its JSON result line"""
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
pcm = synth.make_pcm(20.0, seed=1234)
for beam in (False, True):
    call_legs(lib, node, pcm, beam)
reject_legs(lib, node)
node.close()
if args.bench_runs > 0:
    trees = [("this tree", args.root)] + ([("parent", args.parent)] if args.parent else [])
    got = {name: [] for name, _ in trees}
    for _ in range(args.bench_runs):
        for name, root in trees:
            got[name].append(headline(root))
    keys = [k for k, v in got["this tree"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
    out = {"leg": "headline: bench.py --gpus 1 --steps %d --warmup %d (no grammar)" % (args.bench_steps, args.bench_warmup), "runs": args.bench_runs}
    for name, _ in trees:
        out[name] = {k: [r.get(k) for r in got[name]] for k in keys}
    print(json.dumps(out), flush=True)

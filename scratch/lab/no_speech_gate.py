"""Lab: what the no-speech head costs and what a gated step saves, on the streaming node's step (`small` shape, the host's parameters).

A node step transcribes the whole accumulation with audio_ctx = total_time * 50 + 128.  At 3, 9 and 15 s of accumulation the same step is
timed in three no-speech modes (wmi_set_no_speech):

  0        off: the step as it is without the interface
  1        report: the step plus the head (its <sot> row's probability computed and stored)
  3 gated  gate with no_speech_thold = 0: the window ends behind its <sot> step (every p is > 0), no sampling step

Host clock around whisper_full (it returns with the results on the host), the modes alternating inside every repetition, the first --warm
repetitions dropped; medians, minima and maxima.  Then the headline figure — `bench.py --gpus 1`, which runs in mode 0 — from a fresh child
process, --bench-runs times: its own run-to-run spread; with --parent DIR (a built tree of the parent commit) the same from that tree, the
two alternating.  Prints one JSON line per accumulation and one for the headline.

    python scratch/lab/no_speech_gate.py [--root DIR] [--parent DIR] [--shape small] [--reps 20] [--warm 5] [--bench-runs 3] [--headline-only]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(pathlib.Path(__file__).resolve().parents[2]))
ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its headline beside this tree's")
ap.add_argument("--shape", default="small")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--headline-only", action="store_true", help="skip the node steps")
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, args.root)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from godot_whisper_amd import host, runtime, synth  # noqa: E402


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def node_steps():
    lib = runtime.require_gpu()
    runtime.silence_logs(lib)
    node = host.SpeechToText(lib)
    node.language = "en"
    node.set_language_model(synth.make_model(args.shape, seed=1234))
    pcm = synth.make_pcm(15.0, seed=77, gate=True)
    legs = (("mode 0", 0, None), ("mode 1", 1, None), ("mode 3 gated", 3, 0.0))
    for seconds in (3.0, 9.0, 15.0):
        acc = pcm[:int(seconds * 16000)]
        audio_ctx = min(int(seconds * 50 + 128), 1500)
        times = {name: [] for name, _, _ in legs}
        tokens, windows = {}, {}
        for it in range(args.reps + args.warm):
            order = legs[it % 3:] + legs[:it % 3]
            for name, mode, thold in order:
                p = node.full_params("", audio_ctx)
                p.temperature_inc = 0.0                       # (a fallback's draws would make the repetitions differ)
                if thold is not None:
                    p.no_speech_thold = thold
                node.set_no_speech(mode)
                t0 = time.perf_counter()
                r = node.transcribe(acc, params=p)
                dt = 1e3 * (time.perf_counter() - t0)
                assert node.last_ret == 0
                if it >= args.warm:
                    times[name].append(dt)
                tokens[name] = len(r) - 1
                windows[name] = node.last_windows
        node.set_no_speech(0)
        out = {"shape": args.shape, "accumulated_s": seconds, "audio_ctx": audio_ctx, "reps": args.reps}
        for name, _, _ in legs:
            out[name] = dict(summary(times[name]), tokens=tokens[name])
        out["no_speech_prob"] = windows["mode 1"][0]["no_speech_prob"] if windows["mode 1"] else None
        out["gated_outcomes"] = [w["outcome"] for w in windows["mode 3 gated"]]
        out["head_cost_ms_median"] = round(out["mode 1"]["median_ms"] - out["mode 0"]["median_ms"], 3)
        out["gate_saves_ms_median"] = round(out["mode 0"]["median_ms"] - out["mode 3 gated"]["median_ms"], 3)
        print(json.dumps(out), flush=True)
    node.close()


def headline(root):
    """one `bench.py --gpus 1` in a fresh child process; its JSON result line"""
    root = str(pathlib.Path(root).resolve())
    cmd = [sys.executable, str(pathlib.Path(root) / "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=280)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


if not args.headline_only:
    node_steps()
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

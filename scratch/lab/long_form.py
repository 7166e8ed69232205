"""Lab: a ten-minute recording through whisper_full (window by window) and through wmi_full_long (cut at silences, lock-step), the cost
of the detector on its own, and the headline beside the parent commit's.

Input: synth.make_pcm(600 s, gate=True) — BASELINE's gated generator, 9 600 000 samples, 2 s on / 1 s off.  Per shape (default base.en and
small), with the host's parameters and temperature_inc = 0, the two calls alternate inside every repetition, the first --warm repetitions
dropped; medians, minima and maxima, the number of pieces and of groups of 16.  The detector's figures come from the product's own timer
(wmi_get_long_timings: the launch, the copy of the energies and the one wait, host clock) on the ten minutes and on a 30 s chunk, with
the bytes of PCM the kernel read per second of that time beside them.

Then the headline figure — `bench.py --gpus 1` — from a fresh child process, --bench-runs times; with --parent DIR (a built tree of the
parent commit) the same from that tree, the two taking turns.  Prints one JSON line per shape, one for the detector and one for the headline.

    python scratch/lab/long_form.py [--root DIR] [--parent DIR] [--shapes base.en,small] [--reps 20] [--warm 3] [--bench-runs 3]
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
ap.add_argument("--seconds", type=float, default=600.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, args.root)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from godot_whisper_amd import host, runtime, synth  # noqa: E402


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def long_timer(lib, ctx):
    us, n2 = (C.c_int64 * 3)(), (C.c_int32 * 2)()
    lib.wmi_get_long_timings(ctx, us, n2)
    return list(us), list(n2)


def shape_legs(lib, shape, pcm, pcm30):
    node = host.SpeechToText(lib)
    node.language = "en"
    node.set_language_model(synth.make_model(shape, seed=1234))
    ctx = node.ctx
    times = {"whisper_full": [], "wmi_full_long": []}
    front = {"upload": [], "energies": [], "plan": []}
    n_tok = {}
    for it in range(args.reps + args.warm):
        for name in (("whisper_full", "wmi_full_long") if it % 2 == 0 else ("wmi_full_long", "whisper_full")):
            p = node.full_params("", 0)
            p.temperature_inc = 0.0
            t0 = time.perf_counter()
            r = node.transcribe(pcm, params=p) if name == "whisper_full" else node.transcribe_long(pcm, params=p)
            dt = 1e3 * (time.perf_counter() - t0)
            assert node.last_ret == 0
            n_tok[name] = len(r) - 1
            if it >= args.warm:
                times[name].append(dt)
                if name == "wmi_full_long":
                    us, _ = long_timer(lib, ctx)
                    for k, v in zip(("upload", "energies", "plan"), us):
                        front[k].append(1e-3 * v)
    pieces, modes = list(node.last_pieces), sorted(set(node.last_modes))
    det30 = []
    for it in range(args.reps + args.warm):
        p = node.full_params("", 0)
        p.temperature_inc = 0.0
        node.transcribe_long(pcm30, params=p)
        assert node.last_ret == 0
        if it >= args.warm:
            det30.append(1e-3 * long_timer(lib, ctx)[0][1])
    node.close()
    out = {"shape": shape, "seconds": args.seconds, "reps": args.reps, "whisper_full": summary(times["whisper_full"]),
           "wmi_full_long": summary(times["wmi_full_long"]), "tokens": n_tok, "pieces": len(pieces), "groups_of_16": (len(pieces) + 15) // 16,
           "piece_frames": [q["frame1"] - q["frame0"] for q in pieces], "modes": modes,
           "front_ms": {k: summary(v) for k, v in front.items()}}
    print(json.dumps(out), flush=True)
    e_ms, e30_ms = statistics.median(front["energies"]), statistics.median(det30)
    print(json.dumps({"detector (kernel + copy + wait, host clock)": shape,
                      "ten_minutes": {"ms": summary(front["energies"]), "GB_per_s": round(4e-9 * pcm.size / (1e-3 * e_ms), 1)},
                      "thirty_seconds": {"ms": summary(det30), "GB_per_s": round(4e-9 * pcm30.size / (1e-3 * e30_ms), 1)}}), flush=True)


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
shapes = [s for s in args.shapes.split(",") if s]
if shapes:
    pcm = synth.make_pcm(args.seconds, seed=1234, gate=True)
    pcm30 = synth.make_pcm(30.0, seed=1234, gate=True)
    for shape in shapes:
        shape_legs(lib, shape, pcm, pcm30)
if args.bench_runs > 0:
    trees = [("this tree", args.root)] + ([("parent", args.parent)] if args.parent else [])
    got = {name: [] for name, _ in trees}
    for _ in range(args.bench_runs):
        for name, root in trees:
            got[name].append(headline(root))
    keys = [k for k, v in got["this tree"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
    out = {"headline": "bench.py --gpus 1 --steps %d --warmup %d" % (args.bench_steps, args.bench_warmup), "runs": args.bench_runs}
    for name, _ in trees:
        out[name] = {k: [r.get(k) for r in got[name]] for k in keys}
    print(json.dumps(out), flush=True)

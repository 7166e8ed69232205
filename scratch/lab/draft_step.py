"""Lab: what a draft (wmi_set_draft) saves, and what a wrong one costs.  Synthetic weights, bench.py's kind of noise.

  (a) one node step on `small`: whisper_full with the streaming node's parameters on 3 / 9 / 15 s of accumulation at the node's audio_ctx,
      plain against drafted with the call's own result (what draft_reuse offers when the text did not change)
  (b) base.en, the uncapped 30 s chunk (max_tokens = 0, temperature_inc = 0: with the fallback on, the uncapped window of these synthetic
      weights fails at t = 0 and ends as a sampled decode, which no draft can follow — measured so first: 1.3 s a call, 0 accepted):
      plain, its own result as the draft, and that draft wrong at token 0 (the price of a bad guess: one batch of P + n rows on top of
      the plain call)
  (c) the same chunk with the first k tokens of its own result as the draft, k = 1, 2, 4, 8, 16, 32, ..: the accepted length at which the
      drafted call breaks even with the plain one

The routes take turns inside every repetition, the first --warm repetitions dropped; medians (min - max) of --reps, milliseconds, wall clock
of the whole call (log-mel and encoder included, equal in every route).  Then the headline, `bench.py --gpus 1`, which arms nothing, from
fresh child processes — this tree and --parent (a built tree of the parent commit) taking turns.

    python scratch/lab/draft_step.py [--root DIR] [--parent DIR] [--reps 20] [--warm 3] [--bench-runs 3]
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
ap.add_argument("--parent", default=None)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-warmup", type=int, default=5)
ap.add_argument("--bench-timeout", type=float, default=240.0)
ap.add_argument("--parts", default="a,b,c,bench", help="which parts to run")
args = ap.parse_args()
sys.path.insert(0, args.root)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
import numpy as np  # noqa: E402
from godot_whisper_amd import host, runtime, synth  # noqa: E402


def summary(ts):
    return "%.3f (%.3f - %.3f)" % (statistics.median(ts), min(ts), max(ts))


def take_turns(routes):
    """routes: {name: callable} -> {name: [ms]}"""
    out = {k: [] for k in routes}
    for rep in range(args.warm + args.reps):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= args.warm:
                out[name].append(dt)
    return out


def ids_of(res):
    return [t["id"] for t in res[1:]]


lib = runtime.require_gpu()
runtime.silence_logs(lib)

parts = set(args.parts.split(","))
print("(a) node step on small")
node = host.SpeechToText(lib)
if "a" in parts:
    node.set_language_model(synth.make_model("small", seed=1234))
for seconds in (3.0, 9.0, 15.0) if "a" in parts else ():
    pcm = synth.make_pcm(seconds, seed=77)
    actx = min(int(seconds * 1500 / 30 + 128), 1500)
    p = node.full_params("", actx)
    own = ids_of(node.transcribe(pcm, params=p))
    drafted = node.transcribe(pcm, params=p, draft=own)
    st = dict(node.last_draft_status)
    r = take_turns({"plain": lambda: node.transcribe(pcm, params=p), "drafted": lambda: node.transcribe(pcm, params=p, draft=own)})
    print(f"  {seconds:4.0f} s, audio_ctx {actx}, {len(own)} tokens, accepted {st['n_accepted']} of {st['n_rows']}, same ids {ids_of(drafted) == own}: "
          f"plain {summary(r['plain'])}  drafted {summary(r['drafted'])}")
node.close()

print("(b) base.en, uncapped 30 s chunk")
node = host.SpeechToText(lib); node.set_language_model(synth.make_model("base.en", seed=1234))
pcm = synth.make_pcm(30.0, seed=78)
p = node.full_params("", 0); p.max_tokens = 0; p.temperature_inc = 0.0
own = ids_of(node.transcribe(pcm, params=p))
wrong = [own[0] + 1] + own[1:]
node.transcribe(pcm, params=p, draft=own); st_own = dict(node.last_draft_status)
node.transcribe(pcm, params=p, draft=wrong); st_wrong = dict(node.last_draft_status)
r = take_turns({"plain": lambda: node.transcribe(pcm, params=p), "own": lambda: node.transcribe(pcm, params=p, draft=own),
                "wrong at 0": lambda: node.transcribe(pcm, params=p, draft=wrong)}) if "b" in parts else {}
print(f"  {len(own)} tokens; own: accepted {st_own['n_accepted']} of {st_own['n_rows']}; wrong at 0: accepted {st_wrong['n_accepted']} of {st_wrong['n_rows']}")
for k, v in r.items():
    print(f"  {k:12s} {summary(v)}")

print("(c) break-even: the first k tokens of the own result as the draft")
ks = [k for k in (1, 2, 4, 8, 16, 32, 64, 128, 216) if k <= len(own)]
routes = {"plain": lambda: node.transcribe(pcm, params=p)}
for k in ks:
    routes[f"k = {k}"] = (lambda kk: lambda: node.transcribe(pcm, params=p, draft=own[:kk]))(k)
r = take_turns(routes) if "c" in parts else {}
for k, v in r.items():
    print(f"  {k:12s} {summary(v)}")
node.close()

print("headline: bench.py --gpus 1 --steps %d --warmup %d, fresh processes taking turns" % (args.bench_steps, args.bench_warmup))
trees = [("this tree", args.root)] + ([("parent", args.parent)] if args.parent else [])
vals = {n: [] for n, _ in trees}
for run in range(args.bench_runs if "bench" in parts else 0):
    for name, root in (trees if run % 2 == 0 else trees[::-1]):      # (the first child of a sitting starts cold: the trees swap places every run)
        # (a time limit per child, and the sitting ends at the first child that fails or runs into it)
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                             cwd=root, capture_output=True, text=True, check=True, timeout=args.bench_timeout).stdout.strip().splitlines()[-1]
        vals[name].append(json.loads(out))
for name, rs in vals.items() if "bench" in parts else ():
    key = next((k for k in ("value", "ms_per_chunk", "ms") if k in rs[0]), None)
    print(f"  {name}: " + ("; ".join(json.dumps(x) for x in rs) if key is None else ", ".join("%.4f" % x[key] for x in rs)))

"""Lab: what the two-channel WAV call (include/wmi_device.h wmi_full_wav_channels) costs beside the routes it replaces, and the headline
beside the parent commit's.

Routes take turns inside every repetition, the first --warm repetitions dropped; medians, minima and maxima of --reps.  Call times are a
host clock around calls that end in a device wait; a conversion alone is the device-event time of wmi_wav_stats (whole microseconds).
  (1) conversion alone, device-resident s16 stereo, 30 s at 48 kHz with converter 2 and 30 s at 16 kHz: ONE split launch
      (wmi_wav_to_pcm_channels, device -> device) | the parent commit's route: two single-channel conversions (wmi_wav_to_pcm) of two
      de-interleaved mono s16 clips, their two event times added.  The outputs are compared bit for bit first.
  (2) whole call, --shape (base.en), 30 s of s16 stereo 48 kHz, converter 2, host bytes: wmi_full_wav_channels | NumPy de-interleave into
      two mono clips + wmi_full_batch_wav (the parent commit's route; NumPy's strided copy is a much kinder baseline than the node's
      GDScript loop per sample) | wmi_full_wav (folded, one chunk: for scale, another transcription)
Then `bench.py --gpus 1` from a fresh child process, --bench-runs times; with --parent DIR (a built tree of the parent commit) the same
from that tree, the two taking turns.  One JSON line per leg.

    python scratch/lab/wav_channels.py [--root DIR] [--parent DIR] [--shape base.en] [--reps 20] [--warm 3] [--bench-runs 3]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

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
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from godot_whisper_amd import abi, host, runtime, synth  # noqa: E402

S16 = abi.WMI_WAV_S16


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def stereo_s16(rate, seconds, seed):
    """the 16 kHz generator's samples played at `rate`, a different voice per channel -> int16 [n][2]"""
    n = int(seconds * rate)
    xy = np.stack([synth.make_pcm(n / 16000, seed=seed + c)[:n] for c in range(2)], axis=1)
    return np.clip(np.rint(xy.astype(np.float64) * 32767), -32768, 32767).astype("<i2")


def turns(routes, check=None):
    names = list(routes)
    times = {n: [] for n in names}
    last = {}
    for it in range(args.reps + args.warm):
        order = names[it % len(names):] + names[:it % len(names)]
        for name in order:
            t0 = time.perf_counter()
            last[name] = routes[name]()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= args.warm:
                times[name].append(dt)
    if check:
        check(last)
    return {n: {k + "_ms": v for k, v in summary(t).items()} for n, t in times.items()}


def headline(root):
    root = str(pathlib.Path(root).resolve())
    cmd = [sys.executable, str(pathlib.Path(root) / "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=280)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


lib = runtime.require_gpu()
runtime.silence_logs(lib)
hip = C.CDLL("libamdhip64.so")

if args.reps > 0:
    node = host.SpeechToText(lib)
    node.set_language_model(synth.make_model(args.shape, seed=1234))
    ctx = node.ctx

    def stats():
        s = (C.c_int64 * 5)()
        assert lib.wmi_wav_stats(ctx, s) == 0
        return list(s)

    def dev(raw):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(max(len(raw), 16))) == 0 and hip.hipMemcpy(d, raw, C.c_size_t(len(raw)), 1) == 0
        return d

    # ---- (1) the conversion alone, by device events
    out1 = {"leg": 1, "unit": "us by device events (wmi_wav_stats[4])", "cases": {}}
    for name, rate in (("30 s s16 stereo 48 kHz, converter 2", 48000), ("30 s s16 stereo 16 kHz", 16000)):
        xy = stereo_s16(rate, 30.0, 77)
        n_frames = xy.shape[0]
        d_st, d_l, d_r = dev(xy.tobytes()), dev(np.ascontiguousarray(xy[:, 0]).tobytes()), dev(np.ascontiguousarray(xy[:, 1]).tobytes())
        cap = n_frames + 64
        outs = [C.c_void_p() for _ in range(4)]
        for o in outs:
            assert hip.hipMalloc(C.byref(o), C.c_size_t(4 * cap)) == 0
        w_st = abi.wmi_wav(d_st, 4 * n_frames, S16, 1, rate, 1)
        w_l, w_r = abi.wmi_wav(d_l, 2 * n_frames, S16, 0, rate, 1), abi.wmi_wav(d_r, 2 * n_frames, S16, 0, rate, 1)

        def split():
            n = lib.wmi_wav_to_pcm_channels(ctx, C.byref(w_st), 2, outs[0], outs[1], cap, 1)
            assert n > 0
            return n, stats()[4]

        def two():
            n = lib.wmi_wav_to_pcm(ctx, C.byref(w_l), 2, outs[2], cap, 1)
            t = stats()[4]
            assert n > 0 and lib.wmi_wav_to_pcm(ctx, C.byref(w_r), 2, outs[3], cap, 1) == n
            return n, t + stats()[4]
        n_out = split()[0]
        assert two()[0] == n_out
        back = [np.zeros(n_out, np.float32) for _ in range(4)]
        for b, o in zip(back, outs):
            assert hip.hipMemcpy(b.ctypes.data_as(C.c_void_p), o, C.c_size_t(4 * n_out), 2) == 0
        assert back[0].tobytes() == back[2].tobytes() and back[1].tobytes() == back[3].tobytes(), "the split launch and the two launches differ"
        us = {"one split launch": [], "two single-channel launches (parent route)": []}
        for it in range(args.reps + args.warm):
            for key, fn in ((("one split launch", split), ("two single-channel launches (parent route)", two)) if it % 2 == 0 else
                            (("two single-channel launches (parent route)", two), ("one split launch", split))):
                t = fn()[1]
                if it >= args.warm:
                    us[key].append(t)
        out1["cases"][name] = {"frames": n_frames, "samples_per_channel": n_out, **{k: {kk + "_us": vv for kk, vv in summary(v).items()} for k, v in us.items()}}
        for p in [d_st, d_l, d_r] + outs:
            hip.hipFree(p)
    print(json.dumps(out1), flush=True)

    # ---- (2) the whole call
    xy = stereo_s16(48000, 30.0, 77)
    data = xy.tobytes()

    def params():
        p = node.full_params("", 0)
        p.temperature_inc = 0.0
        return p

    def channels_route():
        node.transcribe_wav_channels(data, S16, 48000, params=params())
        assert node.last_ret == 0
        return [list(r) for r in node.last_channels]

    def numpy_route():
        v = np.frombuffer(data, "<i2").reshape(-1, 2)                              # the de-interleave on the host
        clips = [(np.ascontiguousarray(v[:, c]).tobytes(), S16, 0, 48000) for c in range(2)]
        r = node.transcribe_wav_batch(clips, params=params())
        assert node.last_ret == 0
        return [list(x) for x in r]

    def folded_route():
        r = node.transcribe_wav(data, S16, 1, 48000, params=params())
        assert node.last_ret == 0
        return r

    def same(last):
        assert last["wmi_full_wav_channels"] == last["NumPy de-interleave + wmi_full_batch_wav"], "the two channel routes disagree"
        assert all(len(r) > 1 for r in last["wmi_full_wav_channels"])
    res = turns({"wmi_full_wav_channels": channels_route, "NumPy de-interleave + wmi_full_batch_wav": numpy_route,
                 "wmi_full_wav (folded, one chunk)": folded_route}, same)
    channels_route()
    print(json.dumps({"leg": 2, "shape": args.shape, "clip": "30 s s16 stereo 48 kHz, converter 2, host bytes", "wav_stats_channels": stats(), **res}), flush=True)
    node.close()

if args.bench_runs > 0:
    trees = [("this tree", args.root)] + ([("parent", args.parent)] if args.parent else [])
    got = {name: [] for name, _ in trees}
    for _ in range(args.bench_runs):
        for name, root in trees:
            got[name].append(headline(root))
            print("headline run done:", name, file=sys.stderr, flush=True)
    keys = [k for k, v in got["this tree"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
    out = {"headline": "bench.py --gpus 1 --steps %d --warmup %d" % (args.bench_steps, args.bench_warmup), "runs": args.bench_runs}
    for name, _ in trees:
        out[name] = {k: [r.get(k) for r in got[name]] for k in keys}
    print(json.dumps(out), flush=True)

"""Lab: what the AudioStreamWAV calls (include/wmi_device.h wmi_full_wav & co.) cost beside the routes they replace, and the headline
beside the parent commit's.

Routes take turns inside every repetition, the first --warm repetitions dropped; medians, minima and maxima of --reps.  Call times are a
host clock around calls that end in a device wait; the conversion alone is the device-event time of wmi_wav_stats.
  (a) --shape (base.en), 30 s: wmi_full_wav from s16 mono 16 kHz bytes | whisper_full from host f32 (half the upload, one launch more)
  (b) 30 s of s16 stereo 48 kHz, converter 2: wmi_full_wav | NumPy decode + wmi_downmix_stereo + wmi_resample + whisper_full.  NumPy's
      vectorised decode is a much kinder baseline than the node's GDScript loop (one append per sample), which cannot be run here.
  (c) the conversion alone, device sources, by device events: s16 stereo 48 kHz through the packed-frame reader | the same samples as f32
      stereo frames through the f32-stereo reader
  (d) eight clips of mixed formats and rates: one wmi_full_batch_wav | eight wmi_full_wav calls
Then `bench.py --gpus 1` from a fresh child process, --bench-runs times; with --parent DIR (a built tree of the parent commit) the same
from that tree, the two taking turns.  One JSON line per leg.

    python scratch/lab/wav_ingest.py [--root DIR] [--parent DIR] [--shape base.en] [--reps 20] [--warm 3] [--bench-runs 3]
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

S8, S16, F32 = abi.WMI_WAV_S8, abi.WMI_WAV_S16, abi.WMI_WAV_F32


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def pack(x, fmt):
    if fmt == F32:
        return np.ascontiguousarray(x, "<f4").tobytes()
    hi, dt = (32767, "<i2") if fmt == S16 else (127, "i1")
    return np.clip(np.rint(np.asarray(x, np.float64) * hi), -hi - 1, hi).astype(dt).tobytes()


def clip(fmt, stereo, rate, seconds, seed):
    """the 16 kHz generator's samples played at `rate`, two different channels when stereo"""
    n = int(seconds * rate)
    chans = [synth.make_pcm(n / 16000, seed=seed + c)[:n] for c in range(2 if stereo else 1)]
    return pack(np.stack(chans, axis=1).reshape(-1), fmt)


def wav_of(data, fmt, stereo, rate, on_device=0, ptr=None):
    buf = None if ptr is not None else C.create_string_buffer(data, max(len(data), 1))
    w = abi.wmi_wav(ptr if ptr is not None else C.cast(buf, C.c_void_p), len(data), fmt, stereo, rate, on_device)
    w._keep = buf
    return w


def turns(routes, check=None):
    """routes: name -> callable returning the result; they alternate, the first --warm repetitions are dropped"""
    names = list(routes)
    times = {n: [] for n in names}
    last = {}
    for it in range(args.reps + args.warm):
        for name in (names if it % 2 == 0 else names[::-1]):
            t0 = time.perf_counter()
            last[name] = routes[name]()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= args.warm:
                times[name].append(dt)
    if check:
        check(last)
    return {n: summary(t) for n, t in times.items()}


def stats(lib, ctx):
    s = (C.c_int64 * 5)()
    assert lib.wmi_wav_stats(ctx, s) == 0
    return list(s)


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

    def params():
        p = node.full_params("", 0)
        p.temperature_inc = 0.0
        return p

    def same(last):
        vals = list(last.values())
        assert all(v == vals[0] for v in vals[1:]) and len(vals[0]) > 1, "the routes disagree"

    # (a) s16 mono 16 kHz, 30 s
    data_a = clip(S16, 0, 16000, 30.0, 1234)
    pcm_a = (np.frombuffer(data_a, "<i2").astype(np.float32) / np.float32(32768.0))
    wav_a = wav_of(data_a, S16, 0, 16000)

    def full_wav(w, conv=2):
        assert lib.wmi_full_wav(ctx, params(), C.byref(w), conv) == 0
        return node.collect()
    res = turns({"wmi_full_wav (s16 bytes)": lambda: full_wav(wav_a), "whisper_full (host f32)": lambda: node.transcribe(pcm_a, params=params())}, same)
    print(json.dumps({"leg": "a", "shape": args.shape, "seconds": 30, "bytes_uploaded": {"wav": len(data_a), "f32": pcm_a.nbytes}, **res}), flush=True)

    # (b) s16 stereo 48 kHz, 30 s, converter 2
    data_b = clip(S16, 1, 48000, 30.0, 77)
    wav_b = wav_of(data_b, S16, 1, 48000)

    def numpy_route():
        xy = (np.frombuffer(data_b, "<i2").astype(np.float32) / np.float32(32768.0)).reshape(-1, 2)
        return node.transcribe(node.resample(xy, 2, mix_rate=48000), params=params())
    res = turns({"wmi_full_wav (s16 stereo 48 kHz bytes)": lambda: full_wav(wav_b), "numpy decode + downmix + resample + whisper_full": numpy_route}, same)
    print(json.dumps({"leg": "b", "shape": args.shape, "seconds": 30, "bytes_uploaded": {"wav": len(data_b), "f32 frames": 2 * len(data_b)},
                      "note": "NumPy's vectorised decode stands in for the node's per-sample GDScript loop, which cannot be run here", **res}), flush=True)

    # (c) the conversion alone on device sources, by device events
    f32_b = (np.frombuffer(data_b, "<i2").astype(np.float32) / np.float32(32768.0))
    n_out = 480000
    d_s16, d_f32, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_s16), C.c_size_t(len(data_b))) == 0 and hip.hipMalloc(C.byref(d_f32), C.c_size_t(f32_b.nbytes)) == 0
    assert hip.hipMalloc(C.byref(d_out), C.c_size_t(4 * n_out)) == 0
    assert hip.hipMemcpy(d_s16, data_b, C.c_size_t(len(data_b)), 1) == 0 and hip.hipMemcpy(d_f32, f32_b.ctypes.data_as(C.c_void_p), C.c_size_t(f32_b.nbytes), 1) == 0
    w_s16 = wav_of(data_b, S16, 1, 48000, 1, d_s16)
    w_f32 = abi.wmi_wav(d_f32, f32_b.nbytes, F32, 1, 48000, 1)
    ev = {"packed s16 stereo reader": [], "f32 stereo reader": []}
    outs = {}
    for it in range(args.reps + args.warm):
        for name, w in ((("packed s16 stereo reader", w_s16), ("f32 stereo reader", w_f32)) if it % 2 == 0 else (("f32 stereo reader", w_f32), ("packed s16 stereo reader", w_s16))):
            assert lib.wmi_wav_to_pcm(ctx, C.byref(w), 2, d_out, n_out, 1) == n_out
            us = stats(lib, ctx)[4]
            if it >= args.warm:
                ev[name].append(1e-3 * us)
            back = np.zeros(n_out, np.float32)
            assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), d_out, C.c_size_t(back.nbytes), 2) == 0
            outs[name] = back.tobytes()
    assert outs["packed s16 stereo reader"] == outs["f32 stereo reader"], "the readers disagree"
    print(json.dumps({"leg": "c", "frames": len(data_b) // 4, "outputs": n_out, "converter": 2, "device_event_ms": {k: summary(v) for k, v in ev.items()},
                      "bytes_read_per_frame": {"packed": 4, "f32": 8}}), flush=True)
    for d in (d_s16, d_f32, d_out):
        hip.hipFree(d)

    # (d) eight clips of mixed formats and rates
    specs = [(S16, 0, 16000, 6.0), (S16, 1, 44100, 9.0), (S8, 0, 22050, 4.0), (S16, 1, 48000, 12.0), (S8, 1, 48000, 5.0), (S16, 0, 44100, 8.0),
             (F32, 1, 16000, 7.0), (S16, 0, 8000, 10.0)]
    clips = [(clip(f, st, r, sec, 300 + i), f, st, r) for i, (f, st, r, sec) in enumerate(specs)]
    wavs8 = [wav_of(*c) for c in clips]
    arr8 = (abi.wmi_wav * 8)(*wavs8)

    def batch_route():
        assert lib.wmi_full_batch_wav(ctx, params(), arr8, 8, 2) == 0
        return node.collect_batch(8)

    def eight_route():
        return [full_wav(w) for w in wavs8]
    res = turns({"wmi_full_batch_wav (8 clips)": batch_route, "8 x wmi_full_wav": eight_route})
    print(json.dumps({"leg": "d", "shape": args.shape, "clips": [(f, st, r, sec) for f, st, r, sec in specs], **res}), flush=True)
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

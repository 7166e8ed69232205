"""Lab: what the speaker labels (include/wmi_device.h wmi_set_speaker) cost, and the headline beside the parent commit's.

Routes take turns inside every repetition, the first --warm repetitions dropped; medians, minima and maxima of --reps.  Call times are a
host clock around calls that end in a device wait; the kernel alone is timed by device events (wmi_bench_channel_bins).
  (1) --shape (base.en), 30 s of s16 stereo 48 kHz, converter 2: wmi_full_wav in mode 0 | mode 1 | mode 2 (records read through the
      accessors inside the timed call) | mode 0 plus the host route the mode replaces: an f32 copy of both channels and main.cpp's loop
      per segment in NumPy (vectorised: a kinder baseline than the loop itself)
  (2) k_channel_bins alone, device-resident sources, by device events: 30 s and ten minutes of s16 stereo 48 kHz, 30 s and ten minutes of
      f32 stereo 48 kHz, beside the bytes read over 6.29 TB/s
  (3) one wmi_capture_full step on --capture-shape (small) at 3 / 9 / 15 s of accumulation, 44.1 kHz: mode 0 | mode 1
Then `bench.py --gpus 1` from a fresh child process, --bench-runs times; with --parent DIR (a built tree of the parent commit) the same
from that tree, the two taking turns.  One JSON line per leg.

    python scratch/lab/speaker_bins.py [--root DIR] [--parent DIR] [--shape base.en] [--reps 20] [--warm 3] [--bench-runs 3]
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
ap.add_argument("--capture-shape", default="small")
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

S16, F32 = abi.WMI_WAV_S16, abi.WMI_WAV_F32
HBM_TBS = 6.29


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def stereo_clip(rate, seconds, seed, gains=(1.0, 0.3)):
    """the 16 kHz generator's samples played at `rate`, two different channels; long clips repeat a 30 s stretch"""
    n = int(seconds * rate)
    base = [g * synth.make_pcm(min(n, 30 * rate) / 16000, seed=seed + c)[:min(n, 30 * rate)] for c, g in enumerate(gains)]
    xy = np.stack([np.resize(b, n) for b in base], axis=1).astype(np.float32)
    return xy


def s16_bytes(xy):
    return np.clip(np.rint(xy.astype(np.float64) * 32767), -32768, 32767).astype("<i2").tobytes()


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
    return {n: summary(t) for n, t in times.items()}


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
    # ---- (1) wmi_full_wav, modes 0 / 1 / 2 and the host route
    node = host.SpeechToText(lib)
    node.set_language_model(synth.make_model(args.shape, seed=1234))
    ctx = node.ctx
    xy = stereo_clip(48000, 30.0, 77)
    data = s16_bytes(xy)
    keep = C.create_string_buffer(data, len(data))
    wav = abi.wmi_wav(C.cast(keep, C.c_void_p), len(data), S16, 1, 48000, 0)

    def params():
        p = node.full_params("", 0)
        p.temperature_inc = 0.0
        return p

    def records(tokens):
        out, rec = [], abi.wmi_speaker()
        for i in range(lib.whisper_full_n_segments(ctx)):
            assert lib.wmi_full_get_segment_speaker(ctx, i, C.byref(rec)) == 0
            out.append((rec.speaker, rec.e0, rec.e1))
            for j in range(lib.whisper_full_n_tokens(ctx, i) if tokens else 0):
                if lib.wmi_full_get_token_speaker(ctx, i, j, C.byref(rec)) == 0:
                    out.append((rec.speaker, rec.e0, rec.e1))
        return out

    def run(mode):
        lib.wmi_set_speaker(ctx, mode, 0.0)
        assert lib.wmi_full_wav(ctx, params(), C.byref(wav), 2) == 0
        segs = node.segments()
        return segs, (records(mode == 2) if mode else None)

    def host_route():
        segs, _ = run(0)
        ch = (np.frombuffer(data, "<i2").astype(np.float32) / np.float32(32768.0)).reshape(-1, 2)       # the f32 copy of both channels
        n, labels = ch.shape[0], []
        for t0, t1, _ in segs:
            is0, is1 = max(0, min(n - 1, t0 * 48000 // 100)), max(0, min(n - 1, t1 * 48000 // 100))
            e = np.abs(ch[is0:is1]).sum(axis=0, dtype=np.float64) if is1 > is0 else np.zeros(2)
            labels.append((0 if e[0] > 1.1 * e[1] else 1 if e[1] > 1.1 * e[0] else -1, float(e[0]), float(e[1])))
        return segs, labels

    def same(last):
        segs = [v[0] for v in last.values()]
        assert all(s == segs[0] for s in segs[1:]) and len(segs[0]) >= 1, "the routes disagree on the transcription"
        want = last["mode 0 + NumPy loop per segment on a host f32 copy"][1]
        got = last["mode 1"][1]
        assert [g[0] for g in got] == [w[0] for w in want], "labels differ from the host route"
        assert all(abs(g[1] - w[1]) <= 1e-9 * max(w[1], 1e-30) and abs(g[2] - w[2]) <= 1e-9 * max(w[2], 1e-30) for g, w in zip(got, want))
    res = turns({"mode 0": lambda: run(0), "mode 1": lambda: run(1), "mode 2": lambda: run(2),
                 "mode 0 + NumPy loop per segment on a host f32 copy": host_route}, same)
    st4 = (C.c_int64 * 4)()
    run(1); lib.wmi_speaker_stats(ctx, st4)
    print(json.dumps({"leg": 1, "shape": args.shape, "clip": "30 s s16 stereo 48 kHz, converter 2", "segments": len(run(0)[0]),
                      "speaker_stats": list(st4), **res}), flush=True)
    lib.wmi_set_speaker(ctx, 0, 0.0)
    node.close()

    # ---- (2) the kernel alone, by device events
    out2 = {"leg": 2, "hbm_tb_s": HBM_TBS, "cases": {}}
    cases = [("s16 stereo 48 kHz, 30 s", S16, 30.0), ("s16 stereo 48 kHz, 600 s", S16, 600.0), ("f32 stereo 48 kHz, 30 s", F32, 30.0),
             ("f32 stereo 48 kHz, 600 s", F32, 600.0)]
    bufs = {}
    for name, fmt, sec in cases:
        xy2 = stereo_clip(48000, sec, 5)
        raw = s16_bytes(xy2) if fmt == S16 else np.ascontiguousarray(xy2, "<f4").tobytes()
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(len(raw))) == 0 and hip.hipMemcpy(d, raw, C.c_size_t(len(raw)), 1) == 0
        bufs[name] = (d, len(raw), fmt)
    ms = {name: [] for name, _, _ in cases}
    buf1 = (C.c_float * 1)()
    for it in range(args.reps + args.warm):
        for name, _, _ in (cases if it % 2 == 0 else cases[::-1]):
            d, nbytes, fmt = bufs[name]
            w = abi.wmi_wav(d, nbytes, fmt, 1, 48000, 1)
            assert lib.wmi_bench_channel_bins(0, C.byref(w), 1, buf1) == 0
            if it >= args.warm:
                ms[name].append(float(buf1[0]))
    for name, _, _ in cases:
        nbytes = bufs[name][1]
        s = summary(ms[name])
        s["bytes_read"] = nbytes
        s["bytes_over_hbm_ms"] = round(nbytes / (HBM_TBS * 1e12) * 1e3, 5)
        s["achieved_gb_s"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 1)
        out2["cases"][name] = s
        hip.hipFree(bufs[name][0])
    print(json.dumps(out2), flush=True)

    # ---- (3) one capture step, mode 0 | mode 1
    node = host.CaptureStreamToText(lib)
    node.set_language_model(synth.make_model(args.capture_shape, seed=1234))
    ctx = node.ctx
    out3 = {"leg": 3, "shape": args.capture_shape, "mix_rate": 44100, "accumulation": {}}
    for sec in (3, 9, 15):
        fr = stereo_clip(44100, float(sec), 21)
        with host.CaptureSession(node, 44100, 2) as sess:
            sess.push(fr)
            n, _ = sess.resample()
            p = node.full_params("", int(n / 16000 * 1500 / 30 + 128))

            def step(mode):
                lib.wmi_set_speaker(ctx, mode, 0.0)
                assert sess.full(p) == 0
                return node.segments()
            def agree(last):
                assert last["mode 0"] == last["mode 1"] and len(last["mode 0"]) >= 1, "the modes disagree"
            res3 = turns({"mode 0": lambda: step(0), "mode 1": lambda: step(1)}, agree)
        out3["accumulation"]["%d s" % sec] = res3
    lib.wmi_set_speaker(ctx, 0, 0.0)
    node.close()
    print(json.dumps(out3), flush=True)

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

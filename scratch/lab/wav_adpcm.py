"""Lab: what the IMA-ADPCM mode of the WAV calls (include/wmi_device.h wmi_set_wav_adpcm) costs beside the route the parent commit allows,
and the headline beside the parent commit's.

Routes take turns inside every repetition, the first --warm repetitions dropped; medians, minima and maxima of --reps.  Call times are a
host clock around calls that end in a device wait; the decode alone is by device events around its launches (wmi_bench_adpcm_decode).
  (1) decode launches alone, device-resident bytes: 30 s of stereo 48 kHz ADPCM (1 440 000 frames, 1.44 MB) and ten minutes of mono
      44.1 kHz (26 460 000 frames, 13.2 MB), at a source offset of 0 and of 5 bytes; beside them the sequential C++ loop on the host
      (wmi_selftest_adpcm_host, host clock).  The device result of the first clip is compared with the host loop's first.
  (2) whole call, --shape (base.en), the 30 s stereo clip, converter 2, host bytes: wmi_full_wav in mode 1 on the ADPCM bytes | the
      parent commit's route: wmi_selftest_adpcm_host, then wmi_full_wav on the s16 result | for scale, wmi_full_wav on the same clip as
      s16 (no decode at all).  The three results are compared first.
Then `bench.py --gpus 1` from a fresh child process, --bench-runs times; with --parent DIR (a built tree of the parent commit) the same
from that tree, the two taking turns.  One JSON line per leg.

    python scratch/lab/wav_adpcm.py [--root DIR] [--parent DIR] [--shape base.en] [--reps 20] [--warm 3] [--bench-runs 3]
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

S16, ADPCM = abi.WMI_WAV_S16, abi.WMI_WAV_IMA_ADPCM


def summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def encode_fast(x):
    """int16-range samples of one channel -> nibbles.  The encoder's quality does not matter here, only that the codes look like a voice
    line's: each sample's difference to the previous one, coded against a step that follows the signal's local level — no closed loop."""
    x = np.asarray(x, np.float64)
    d = np.diff(x, prepend=0.0)
    level = np.maximum(np.convolve(np.abs(d), np.ones(64) / 64, mode="same"), 4.0)
    q = np.clip(np.rint(np.abs(d) / level * 2.0), 0, 7).astype(np.uint8)
    return (q | np.where(d < 0, 8, 0).astype(np.uint8)).astype(np.uint8)


def pack(chans):
    """nibble arrays of equal even length, one per channel -> AudioStreamWAV bytes (byte 2k + c = frames 2k, 2k + 1 of channel c)"""
    nch, n = len(chans), chans[0].size
    out = np.zeros((n // 2, nch), np.uint8)
    for c, v in enumerate(chans):
        out[:, c] = v[0:n:2] | (v[1:n:2] << 4)
    return out.tobytes()


def voice_clip(rate, seconds, stereo, seed):
    n = int(seconds * rate) // 2 * 2
    base = synth.make_pcm(min(n, 1500000) / 16000, seed=seed)                  # (longer clips repeat it)
    chans = []
    for c in range(2 if stereo else 1):
        v = np.resize(np.roll(base, 4001 * c), n) * 20000.0
        chans.append(encode_fast(v))
    return pack(chans)


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

if args.reps > 0:
    def host_decode(data, stereo):
        frames = (len(data) // 2 * 2) if stereo else 2 * len(data)
        out = np.zeros(frames * (2 if stereo else 1), np.int16)
        assert lib.wmi_selftest_adpcm_host(data, len(data), stereo, out.ctypes.data_as(C.c_void_p), frames) == frames
        return out

    # ---- (1) the decode launches alone
    shape = (C.c_int * 5)()
    assert lib.wmi_selftest_adpcm_shape(shape) == 0
    out1 = {"leg": 1, "unit": "us", "launch_shape": dict(zip(("chunk_nibbles", "lanes", "chunks_per_workgroup", "partials_per_tile", "launches"), list(shape))),
            "cases": {}}
    clip30 = voice_clip(48000, 30.0, 1, 77)
    for name, data, stereo in (("30 s stereo 48 kHz", clip30, 1), ("10 min mono 44.1 kHz", voice_clip(44100, 600.0, 0, 78), 0)):
        frames = (len(data) // 2 * 2) if stereo else 2 * len(data)
        case = {"bytes": len(data), "frames": frames}
        if stereo:
            got = np.zeros(frames * 2, np.int16)
            fr = C.c_longlong(0)
            assert lib.wmi_selftest_adpcm_decode(0, data, len(data), 1, 0, got.ctypes.data_as(C.c_void_p), frames, C.byref(fr)) == 0
            assert got.tobytes() == host_decode(data, 1).tobytes(), "device and host decode differ"
        n = args.reps + args.warm
        for off in (0, 5):
            ms = (C.c_float * n)()
            assert lib.wmi_bench_adpcm_decode(0, data, len(data), stereo, off, n, ms) == 0
            case["device decode, source offset %d (device events)" % off] = {k + "_us": round(1e3 * v, 1) for k, v in summary(list(ms)[args.warm:]).items()}
        ts = []
        for it in range(min(n, 8)):
            t0 = time.perf_counter()
            host_decode(data, stereo)
            ts.append(1e6 * (time.perf_counter() - t0))
        case["sequential C++ on the host (host clock, incl. the output allocation)"] = {k + "_us": round(v, 1) for k, v in summary(ts[1:]).items()}
        out1["cases"][name] = case
    print(json.dumps(out1), flush=True)

    # ---- (2) the whole call
    node = host.SpeechToText(lib, wav_adpcm=True)
    node.set_language_model(synth.make_model(args.shape, seed=1234))
    s16 = host_decode(clip30, 1).tobytes()

    def params():
        p = node.full_params("", 0)
        p.temperature_inc = 0.0
        return p

    def stats():
        s = (C.c_int64 * 5)()
        assert lib.wmi_wav_stats(node.ctx, s) == 0
        return list(s)

    def adpcm_route():
        r = node.transcribe_wav(clip30, ADPCM, 1, 48000, params=params())
        assert node.last_ret == 0
        return r

    def host_route():
        r = node.transcribe_wav(host_decode(clip30, 1).tobytes(), S16, 1, 48000, params=params())
        assert node.last_ret == 0
        return r

    def s16_route():
        r = node.transcribe_wav(s16, S16, 1, 48000, params=params())
        assert node.last_ret == 0
        return r

    def same(last):
        assert last["wmi_full_wav, mode 1, ADPCM bytes"] == last["host C++ decode + wmi_full_wav on s16 (parent route)"] == last["wmi_full_wav on the clip as s16 (scale)"]
    res = turns({"wmi_full_wav, mode 1, ADPCM bytes": adpcm_route, "host C++ decode + wmi_full_wav on s16 (parent route)": host_route,
                 "wmi_full_wav on the clip as s16 (scale)": s16_route}, same)
    adpcm_route()
    st_adpcm = stats()
    s16_route()
    print(json.dumps({"leg": 2, "shape": args.shape, "clip": "30 s stereo 48 kHz, converter 2, host bytes", "wav_stats_adpcm": st_adpcm,
                      "wav_stats_s16": stats(), **res}), flush=True)
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

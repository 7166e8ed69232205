"""Lab: the transcribe step of N streaming speakers on ONE context (`small` shape), two ways:

  serial   N wmi_capture_full calls, one session after the other, each with the node's audio_ctx = total_time * 50 + 128
  batch    one wmi_capture_full_batch over the N sessions with those lengths (lock-step rows with a length each)

N = 2, 4, 8 speakers whose accumulations are spread over 3 .. 15 s.  Every step pushes another 0.3 s to every session and brings its PCM
up to date (untimed: both legs start from the same device-resident PCM), then times both legs on that state with the host clock around
the calls (they return with the results on the host), in alternating order.  The lengths change from step to step as in a live stream, so
no leg replays a captured step graph.  The first --warm steps are dropped; medians, minima and maxima over the rest, and for the batch
leg the phase split of wmi_get_batch_timings of the last step.  A library without wmi_capture_full_batch (a parent build: --root <its
tree>) runs the serial leg only.  Prints one JSON line per N.

--quant q5_1 (q4_0 / q4_1 / q5_0 / q8_0): the model block-quantised with synth.quantize_model (BASELINE configs[4] is large-v3 q5_1).  A parent
build whose batch call cuts the sessions into sets of one length is measured the same way: --root <its tree>.

    python scratch/lab/capture_batch.py [--root DIR] [--shape small] [--quant QTYPE] [--steps 12] [--warm 3]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(pathlib.Path(__file__).resolve().parents[2]))
ap.add_argument("--shape", default="small")
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--rate", type=int, default=44100)
ap.add_argument("--quant", default=None, help="block-quantise the model: q4_0, q4_1, q5_0, q5_1 or q8_0")
args = ap.parse_args()
sys.path.insert(0, args.root)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from godot_whisper_amd import host, runtime, synth  # noqa: E402

lib = runtime.require_gpu()
runtime.silence_logs(lib)
node = host.CaptureStreamToText(lib)
node.language = "en"
model = synth.make_model(args.shape, seed=1234)
if args.quant:
    model = synth.quantize_model(model, args.quant)
node.set_language_model(model)
del model
has_batch = hasattr(lib, "wmi_capture_full_batch")
rate, sr = args.rate, 16000
step = int(round(0.3 * rate))
total_steps = args.steps + args.warm


def speaker_frames(seed):
    pcm = synth.make_pcm(16.0, seed=seed)
    t = np.arange(int(15.9 * rate)) * (sr / rate)
    mono = np.interp(t, np.arange(pcm.size), pcm).astype(np.float32)
    return np.ascontiguousarray(np.stack([mono, (0.8 * mono).astype(np.float32)], axis=1))


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


for n in (2, 4, 8):
    frames = [speaker_frames(900 + i) for i in range(n)]
    # accumulations before the first step: spread over 3 s .. (15 s minus what the steps add)
    starts = np.linspace(3.0, 15.0 - 0.3 * total_steps, n)
    sessions = [host.CaptureSession(node, rate, 2, frames_hint=16 * rate) for _ in range(n)]
    pos = [int(s * rate) for s in starts]
    for s, f, p in zip(sessions, frames, pos):
        s.push(f[:p]); s.resample()
    t_serial, t_batch, same, phases, ctx_last = [], [], 0, None, None
    for it in range(total_steps):
        ctxs = []
        for i, s in enumerate(sessions):
            s.push(frames[i][pos[i]:pos[i] + step]); pos[i] += step
            size, _ = s.resample()
            ctxs.append(min(int(size / sr * 1500 / 30 + 128), 1500))
        params = [node.full_params("", a) for a in ctxs]

        def serial():
            t0 = time.perf_counter()
            out = []
            for s, p in zip(sessions, params):
                assert s.full(p) == 0
                out.append(node.collect())
            return 1e3 * (time.perf_counter() - t0), out

        def batch():
            t0 = time.perf_counter()
            assert host.CaptureSession.full_batch(sessions, node.full_params("", 0), ctxs) == 0
            out = node.collect_batch(n)
            return 1e3 * (time.perf_counter() - t0), out

        if not has_batch:
            ts, _ = serial()
            if it >= args.warm:
                t_serial.append(ts)
            continue
        (ts, a), (tb, b) = (serial(), batch()) if it % 2 == 0 else reversed((batch(), serial()))
        if it >= args.warm:
            t_serial.append(ts); t_batch.append(tb)
            same += sum(1 for x, y in zip(a, b) if x[0] == y[0])
        t4, ns = (C.c_int64 * 4)(), C.c_int32(0)
        lib.wmi_get_batch_timings(node.ctx, t4, C.byref(ns))
        phases = {"mel_us": t4[0], "encode_us": t4[1], "decode_us": t4[2], "emit_us": t4[3], "steps": ns.value, "lockstep_rows": node.last_modes.count(0)}
        ctx_last = ctxs
    out = {"shape": args.shape + (" " + args.quant if args.quant else ""), "speakers": n, "steps_timed": args.steps, "accumulated_s_at_end": [round(p / rate, 1) for p in pos],
           "audio_ctx_last_step": ctx_last, "serial": summary(t_serial)}
    if has_batch:
        out["batch"] = summary(t_batch)
        out["serial_over_batch_median"] = round(out["serial"]["median_ms"] / out["batch"]["median_ms"], 2)
        out["same_text_serial_vs_batch"] = f"{same} of {args.steps * n}"
        out["batch_phases_last_step"] = phases
    print(json.dumps(out), flush=True)
    for s in sessions:
        s.close()
node.close()

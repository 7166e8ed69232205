"""Lab: one step of the streaming node (addon/capture_stream_to_text.gd:69-120) — append 0.3 s of stereo capture frames, resample the
accumulation, VAD, transcribe with the node's parameters — timed two ways on the `small` shape at 3 / 9 / 15 s of accumulation at 44.1 kHz:

  session   wmi_capture_push + wmi_capture_resample + wmi_capture_vad + wmi_capture_full (frames and PCM stay on the device)
  calls     SpeechToText.resample (wmi_downmix_stereo + wmi_resample), wmi_vad, whisper_full on host arrays, the whole accumulation each

Median of --reps steps per point; every repetition starts from the same accumulation (the session is rebuilt outside the timed part).
A library without the session (a parent build: --root <its tree>) runs the `calls` leg only.  Prints one JSON line per point.

    python scratch/lab/capture_step.py [--root DIR] [--shape small] [--reps 50]
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(pathlib.Path(__file__).resolve().parents[2]))
ap.add_argument("--shape", default="small")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rate", type=int, default=44100)
args = ap.parse_args()
sys.path.insert(0, args.root)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from godot_whisper_amd import host, runtime, synth  # noqa: E402

lib = runtime.require_gpu()
runtime.silence_logs(lib)
node = host.CaptureStreamToText(lib)
node.language = "en"
node.set_language_model(synth.make_model(args.shape, seed=1234))
node.device_vad = True
has_session = hasattr(host, "CaptureSession")
rate, sr = args.rate, 16000
step = int(round(0.3 * rate))
pcm = synth.make_pcm(16.0, seed=77)
t = np.arange(int(15.6 * rate)) * (sr / rate)
mono = np.interp(t, np.arange(pcm.size), pcm).astype(np.float32)
frames = np.ascontiguousarray(np.stack([mono, (0.8 * mono).astype(np.float32)], axis=1))
vad_thold, freq_thold = 2.0, 200.0


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


for acc_s in (3, 9, 15):
    n_acc = acc_s * rate
    whole = frames[: n_acc + step]
    out = {"shape": args.shape, "mix_rate": rate, "accumulated_s": acc_s, "reps": args.reps}
    ts, tokens_calls = [], None
    for rep in range(args.reps + 3):
        t0 = time.perf_counter()
        resampled = node.resample(whole, 2, rate)
        quiet = node.voice_activity_detection(resampled)
        audio_ctx = min(int(resampled.size / sr * 1500 / 30 + 128), 1500)
        tokens_calls = node.transcribe(resampled, "", audio_ctx)
        ts.append(1e3 * (time.perf_counter() - t0))
    out["calls"] = summary(ts[3:])
    out["calls"]["bytes_host_to_device"] = int(whole.nbytes + 4 * whole.shape[0] + 4 * 3 * sr + 4 * resampled.size)
    out["n_samples"], out["audio_ctx"], out["n_tokens"] = int(resampled.size), audio_ctx, len(tokens_calls) - 1
    if has_session:
        ts, stats, same = [], None, True
        for rep in range(args.reps + 3):
            with host.CaptureSession(node, rate, 2, frames_hint=16 * rate) as sess:
                sess.push(frames[:n_acc]); sess.resample(); sess.vad(vad_thold, freq_thold)       # the state before the step (untimed)
                t0 = time.perf_counter()
                sess.push(frames[n_acc:n_acc + step])
                size, _ = sess.resample()
                quiet_s = bool(sess.vad(vad_thold, freq_thold))
                audio_ctx = min(int(size / sr * 1500 / 30 + 128), 1500)
                ret = sess.full(node.full_params("", audio_ctx))
                tokens = node.collect() if ret == 0 else []
                ts.append(1e3 * (time.perf_counter() - t0))
                stats = sess.stats()
                same = same and tokens == tokens_calls and quiet_s == quiet
        out["session"] = summary(ts[3:])
        out["session"]["stats_bytes_h2d_computed_reused_everything"] = list(stats)
        out["session_equals_calls"] = bool(same)
    print(json.dumps(out), flush=True)
node.close()

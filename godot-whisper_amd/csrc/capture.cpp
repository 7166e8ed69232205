// Capture session (include/wmi_device.h wmi_capture_*): the streaming node's step on device-resident frames.
//
// replaces: the per-step host traffic of CaptureStreamToText.transcribe_thread (bin/addons/godot_whisper/capture_stream_to_text.gd:69-120):
// every 0.3 s the node hands the WHOLE accumulated stereo buffer to resample(), the result to voice_activity_detection() and to
// transcribe().  Here the accumulation and its 16 kHz PCM stay in HBM for the life of the session: a push uploads the new frames only, the
// resampler reads the stereo frames directly (k_resample.hip, the fold of k_downmix per tap) and recomputes only the outputs whose taps
// reach past the frames the previous plan saw, the VAD and whisper_full read the PCM where it lies.  Every value equals what the one-shot
// calls (wmi_downmix_stereo + wmi_resample, wmi_vad, whisper_full) give on the same accumulation, bit for bit.
//
// Everything is queued on the state's stream.  The frame count of a resample comes from the host-side plan, so wmi_capture_resample does
// not wait; wmi_capture_vad waits once (its three results), wmi_capture_full as whisper_full does.

#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>
#include <vector>
#include "wmi.h"
#include "kernels.h"

using namespace wmi;

struct wmi_capture {
    whisper_context * ctx = nullptr;
    int mix_rate = 0, converter = 2;
    // accumulated stereo frames: `count` live frames from frame `off` of d_frames (keep_last moves `off`, nothing is copied)
    float * d_frames = nullptr; long long cap_frames = 0, off = 0, count = 0;
    float * d_pcm = nullptr; long long cap_pcm = 0;
    float * h_stage = nullptr; long long cap_stage = 0;             // pinned; reused once stage_done has passed
    hipEvent_t stage_done = nullptr; bool stage_busy = false;
    int * d_pos = nullptr; double * d_frac = nullptr; long long cap_tab = 0;   // positions of the rates without a closed form
    // what d_pcm holds: the outputs of plan `prev` over the first prev_frames live frames (valid = false: nothing usable)
    k::ResamplePlan prev; long long prev_frames = 0; bool valid = false;
    bool dirty = false;                                               // frames changed since the last resample
    long long n_pcm = 0; int expected = 0;
    int64_t pending_h2d = 0, stats[4] = {0, 0, 0, 0};
    // wmi_capture_set_draft: mode 1 arms the previous successful result's token ids (draft_last) in front of every wmi_capture_full
    int draft_mode = 0; std::vector<int32_t> draft_last;
};

namespace {

struct Scope {                                                         // the context's lock, then its own state's (api.cpp CtxScope)
    std::unique_lock<std::recursive_mutex> lk, lks;
    explicit Scope(whisper_context * c) : lk(c->mu) { if (State * st = c->state.own) lks = std::unique_lock<std::recursive_mutex>(st->mu); }
};

constexpr int RATE_16K = WHISPER_SAMPLE_RATE;

bool wait_stage(wmi_capture * c) {
    if (!c->stage_busy) return true;
    c->stage_busy = false;
    return HIP_OK(hipEventSynchronize(c->stage_done));
}

// room for `extra` more frames behind the live ones
bool reserve_frames(wmi_capture * c, long long extra, hipStream_t s) {
    if (c->off + c->count + extra <= c->cap_frames) return true;
    if (c->count + extra <= c->cap_frames && c->count <= c->off) {      // the live frames fit in front of themselves: slide them down
        if (c->count && !HIP_OK(hipMemcpyAsync(c->d_frames, c->d_frames + 2 * c->off, (size_t) c->count * 8, hipMemcpyDeviceToDevice, s))) return false;
        c->off = 0;
        return true;
    }
    const long long want = std::max<long long>(std::max(2 * c->cap_frames, c->count + extra), 4096);
    float * d = nullptr;
    if (!HIP_OK(hipMalloc((void **) &d, (size_t) want * 8))) return false;
    bool ok = true;
    if (c->count) ok = HIP_OK(hipMemcpyAsync(d, c->d_frames + 2 * c->off, (size_t) c->count * 8, hipMemcpyDeviceToDevice, s));
    ok = ok && HIP_OK(hipStreamSynchronize(s));                         // (kernels queued earlier may still read the old buffer)
    if (!ok) { (void) hipFree(d); return false; }
    if (c->d_frames) (void) hipFree(c->d_frames);
    c->d_frames = d; c->cap_frames = want; c->off = 0;
    return true;
}

// room for n outputs; the first `keep` of the old buffer survive
bool reserve_pcm(wmi_capture * c, long long n, long long keep, hipStream_t s) {
    if (n <= c->cap_pcm) return true;
    const long long want = std::max<long long>(std::max(2 * c->cap_pcm, n), 16384);
    float * d = nullptr;
    if (!HIP_OK(hipMalloc((void **) &d, (size_t) want * 4))) return false;
    bool ok = true;
    if (keep > 0 && c->d_pcm) ok = HIP_OK(hipMemcpyAsync(d, c->d_pcm, (size_t) keep * 4, hipMemcpyDeviceToDevice, s));
    ok = ok && HIP_OK(hipStreamSynchronize(s));
    if (!ok) { (void) hipFree(d); return false; }
    if (c->d_pcm) (void) hipFree(c->d_pcm);
    c->d_pcm = d; c->cap_pcm = want;
    return true;
}

// bring d_pcm up to date with the live frames; the caller holds the locks and has set the device.  Returns result_size or < 0.
int refresh(wmi_capture * c) {
    if (!c->dirty) return (int) c->n_pcm;
    hipStream_t s = c->ctx->state->dev.stream;
    const float * frames = c->d_frames + 2 * c->off;
    auto done = [&](long long n_out, long long first) {
        c->n_pcm = n_out; c->dirty = false;
        c->stats[0] = c->pending_h2d; c->stats[1] = n_out - first; c->stats[2] = first; c->stats[3] = first == 0 ? 1 : 0;
        c->pending_h2d = 0;
        return (int) n_out;
    };
    c->expected = (int) (c->count * RATE_16K / c->mix_rate);           // src/speech_to_text.cpp:356
    if (c->mix_rate == RATE_16K) {                                      // :38-42, the copy path: the fold alone
        const long long first = c->valid ? std::min(c->prev_frames, c->count) : 0;
        if (!reserve_pcm(c, c->count, first, s)) return -3;
        if (c->count > first) k::downmix_stereo(frames + 2 * first, (int) (c->count - first), c->d_pcm + first, s);
        c->prev_frames = c->count; c->valid = true;
        return done(c->count, first);
    }
    const double ratio = (double) (uint32_t) RATE_16K / (double) (uint32_t) c->mix_rate;              // :25-26
    const long long out_frames = (int) ((uint32_t) c->count * ratio);
    k::ResamplePlan pl = k::resample_plan(c->count, out_frames, ratio, c->converter);
    if (pl.error) {
        if (pl.error == -31) WMI_ERR("wmi_capture_resample: SRC_LINEAR cannot upsample a single frame, 0 frames\n");
        else WMI_ERR("wmi_capture_resample: converter error %d (src_simple would report it through src_strerror)\n", -pl.error);
        c->valid = false;
        return done(0, 0);                                              // the host returns 0 frames on a converter error (:33-36)
    }
    const long long first = c->valid ? k::resample_first_dirty(c->prev, c->prev_frames, pl) : 0;
    if (!reserve_pcm(c, pl.n_out, first, s)) return -3;
    if (pl.need_table && pl.n_out > 0) {                                // positions from the host's recurrence: everything is recomputed
        if (pl.n_out > c->cap_tab) {
            const long long want = std::max<long long>(std::max(2 * c->cap_tab, pl.n_out), 16384);
            if (!HIP_OK(hipStreamSynchronize(s))) return -3;
            if (c->d_pos) (void) hipFree(c->d_pos);
            if (c->d_frac) (void) hipFree(c->d_frac);
            c->d_pos = nullptr; c->d_frac = nullptr; c->cap_tab = 0;
            if (!HIP_OK(hipMalloc((void **) &c->d_pos, (size_t) want * 4)) || !HIP_OK(hipMalloc((void **) &c->d_frac, (size_t) want * 8))) return -3;
            c->cap_tab = want;
        }
        const int * hp; const double * hf;
        k::resample_table(pl, &hp, &hf);
        if (!HIP_OK(hipMemcpyAsync(c->d_pos, hp, (size_t) pl.n_out * 4, hipMemcpyHostToDevice, s)) ||
            !HIP_OK(hipMemcpyAsync(c->d_frac, hf, (size_t) pl.n_out * 8, hipMemcpyHostToDevice, s))) return -3;
        c->pending_h2d += pl.n_out * 12;
    }
    k::resample_launch_stereo(pl, frames, c->count, c->d_pcm, c->converter <= 2 ? c->ctx->d_sinc[c->converter] : nullptr, c->d_pos, c->d_frac, first, s);
    if (!HIP_OK(hipGetLastError())) return -3;
    c->prev = pl; c->prev_frames = c->count; c->valid = true;          // (the plan's tables stay alive behind the copies queued above)
    return done(pl.n_out, std::min(first, pl.n_out));
}

}  // namespace

extern "C" {

struct wmi_capture * wmi_capture_init(struct whisper_context * ctx, int mix_rate, int converter, int frames_hint) {
    if (!ctx || !ctx->state || ctx->host_only || ctx->weights_pending || mix_rate <= 0 || converter < 1 || converter > 4 || frames_hint < 0) return nullptr;
    wmi_capture * c = nullptr;
    try {
        Scope lk(ctx);
        if (!HIP_OK(hipSetDevice(ctx->device))) return nullptr;
        hipStream_t s = ctx->state->dev.stream;
        c = new wmi_capture();
        c->ctx = ctx; c->mix_rate = mix_rate; c->converter = converter;
        bool ok = HIP_OK(hipEventCreateWithFlags(&c->stage_done, hipEventDisableTiming));
        if (ok && converter <= 2 && !ctx->d_sinc[converter]) {         // the converter's table, shared with wmi_resample
            const float * coeffs; int count, inc;
            (void) k::sinc_table(converter, &coeffs, &count, &inc);
            float *& d_sinc = ctx->d_sinc[converter];
            ok = HIP_OK(hipMalloc((void **) &d_sinc, (size_t) count * 4)) && HIP_OK(hipMemcpyAsync(d_sinc, coeffs, (size_t) count * 4, hipMemcpyHostToDevice, s));
            if (!ok && d_sinc) { (void) hipFree(d_sinc); d_sinc = nullptr; }
        }
        ok = ok && reserve_frames(c, std::max(frames_hint, 4096), s);
        if (!ok) { wmi_capture_free(c); return nullptr; }
        return c;
    } catch (...) { WMI_ERR("wmi_capture_init: out of memory\n"); delete c; return nullptr; }
}

void wmi_capture_free(struct wmi_capture * c) {
    if (!c) return;
    {
        Scope lk(c->ctx);
        (void) hipSetDevice(c->ctx->device);
        (void) hipStreamSynchronize(c->ctx->state->dev.stream);
        if (c->d_frames) (void) hipFree(c->d_frames);
        if (c->d_pcm) (void) hipFree(c->d_pcm);
        if (c->d_pos) (void) hipFree(c->d_pos);
        if (c->d_frac) (void) hipFree(c->d_frac);
        if (c->h_stage) (void) hipHostFree(c->h_stage);
        if (c->stage_done) (void) hipEventDestroy(c->stage_done);
    }
    delete c;
}

int wmi_capture_push(struct wmi_capture * c, const float * frames_xy, int n_frames, int on_device) {
    if (!c || n_frames < 0 || (n_frames > 0 && !frames_xy)) return -1;
    if (n_frames == 0) return (int) c->count;
    if (c->count + n_frames > INT_MAX) return -1;
    Scope lk(c->ctx);
    if (!HIP_OK(hipSetDevice(c->ctx->device))) return -2;
    hipStream_t s = c->ctx->state->dev.stream;
    if (!reserve_frames(c, n_frames, s)) return -3;
    float * dst = c->d_frames + 2 * (c->off + c->count);
    if (on_device) {                                                    // the caller's buffer is free again when the call returns
        if (!HIP_OK(hipMemcpyAsync(dst, frames_xy, (size_t) n_frames * 8, hipMemcpyDeviceToDevice, s)) || !HIP_OK(hipStreamSynchronize(s))) return -3;
    } else {
        if (!wait_stage(c)) return -3;
        if (n_frames > c->cap_stage) {
            const long long want = std::max<long long>(std::max(2 * c->cap_stage, (long long) n_frames), 16384);
            if (c->h_stage) (void) hipHostFree(c->h_stage);
            c->h_stage = nullptr; c->cap_stage = 0;
            if (!HIP_OK(hipHostMalloc((void **) &c->h_stage, (size_t) want * 8, hipHostMallocDefault))) return -3;
            c->cap_stage = want;
        }
        memcpy(c->h_stage, frames_xy, (size_t) n_frames * 8);
        if (!HIP_OK(hipMemcpyAsync(dst, c->h_stage, (size_t) n_frames * 8, hipMemcpyHostToDevice, s)) || !HIP_OK(hipEventRecord(c->stage_done, s))) return -3;
        c->stage_busy = true;
        c->pending_h2d += (int64_t) n_frames * 8;
    }
    c->count += n_frames; c->dirty = true;
    return (int) c->count;
}

int wmi_capture_keep_last(struct wmi_capture * c, int n_frames) {
    if (!c || n_frames < 0) return -1;
    Scope lk(c->ctx);
    c->draft_last.clear();                                              // the sentence ended: the next text will be another
    if (n_frames < c->count) {
        c->off += c->count - n_frames; c->count = n_frames;
        c->valid = false; c->dirty = true;                              // other frames at every position: everything is recomputed
    }
    return (int) c->count;
}

int wmi_capture_resample(struct wmi_capture * c, int * expected) {
    if (!c) return -1;
    try {
        Scope lk(c->ctx);
        if (!HIP_OK(hipSetDevice(c->ctx->device))) return -2;
        const int r = refresh(c);
        if (expected) *expected = c->expected;
        return r;
    } catch (...) { WMI_ERR("wmi_capture_resample: out of memory\n"); return -3; }
}

const float * wmi_capture_pcm(struct wmi_capture * c, int * n_samples) {
    if (n_samples) *n_samples = 0;
    if (!c) return nullptr;
    try {
        Scope lk(c->ctx);
        if (!HIP_OK(hipSetDevice(c->ctx->device))) return nullptr;
        const int n = refresh(c);
        if (n <= 0) return nullptr;
        if (n_samples) *n_samples = n;
        return c->d_pcm;
    } catch (...) { return nullptr; }
}

int wmi_capture_read_pcm(struct wmi_capture * c, float * dst, int capacity) {
    if (!c || capacity < 0 || (capacity > 0 && !dst)) return -1;
    try {
        Scope lk(c->ctx);
        if (!HIP_OK(hipSetDevice(c->ctx->device))) return -2;
        const int n = refresh(c);
        if (n <= 0) return n;
        if (n > capacity) return -4;
        hipStream_t s = c->ctx->state->dev.stream;
        if (!HIP_OK(hipMemcpyAsync(dst, c->d_pcm, (size_t) n * 4, hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s))) return -3;
        return n;
    } catch (...) { return -3; }
}

int wmi_capture_vad(struct wmi_capture * c, float vad_thold, float freq_thold, float * energies) {
    if (!c) return -1;
    try {
        Scope lk(c->ctx);
        if (!c->dirty && c->n_pcm < RATE_16K * 3) return 0;            // fewer than 3 s: no device work
        if (!HIP_OK(hipSetDevice(c->ctx->device))) return -2;
        const int n = refresh(c);
        if (n < 0) return n;
        if (n < RATE_16K * 3) return 0;
        return wmi_vad(c->ctx, c->d_pcm, n, 1, vad_thold, freq_thold, energies);
    } catch (...) { return -3; }
}

int wmi_capture_full(struct wmi_capture * c, struct whisper_full_params params) {
    if (!c) return -1;
    try {
        Scope lk(c->ctx);
        if (!HIP_OK(hipSetDevice(c->ctx->device))) return -2;
        const int n = refresh(c);
        if (n < 0) { c->draft_last.clear(); return n; }
        State * st = c->ctx->state.get();
        if (c->draft_mode == 1 && st && !c->draft_last.empty()) st->draft = c->draft_last;
        // wmi_set_speaker: the channel energies of the accumulation as it lies in d_frames, one launch and one copy in front of the call's own
        // work on its stream (full() waits for its results behind them)
        const bool labels = n > 0 && st && speaker_begin(*c->ctx, 1);
        if (labels && (!speaker_reserve(*c->ctx, 0, k::SRC_F32_STEREO, c->count, c->mix_rate) ||
                       !speaker_queue(*c->ctx, 0, c->d_frames + 2 * c->off, st->dev.stream))) { c->draft_last.clear(); return -3; }
        const int ret = wmi_full_device_pcm(c->ctx, params, c->d_pcm, n, nullptr);
        if (labels && ret == 0) speaker_commit(*c->ctx, 1, params.token_timestamps);
        c->draft_last.clear();                                          // (a failed call forgets them)
        if (c->draft_mode == 1 && ret == 0 && st)
            for (const Segment & seg : st->result_all) for (const whisper_token_data & t : seg.tokens) c->draft_last.push_back(t.id);
        return ret;
    } catch (...) { c->draft_last.clear(); return -3; }
}

int wmi_capture_set_draft(struct wmi_capture * c, int mode) {
    if (!c) return -1;
    Scope lk(c->ctx);
    const int prev = c->draft_mode;
    c->draft_mode = mode != 0 ? 1 : 0;
    if (c->draft_mode == 0) c->draft_last.clear();
    return prev;
}

int wmi_capture_full_batch(struct wmi_capture * const * caps, int n, struct whisper_full_params params, const int * audio_ctx) {
    if (!caps || n <= 0) return -1;
    for (int i = 0; i < n; ++i) if (!caps[i] || caps[i]->ctx != caps[0]->ctx) return -1;
    whisper_context * ctx = caps[0]->ctx;
    try {
        Scope lk(ctx);                                                  // once, for the refreshes and the transcription alike
        DraftRefuse no_draft(ctx->state.get());                         // (dropped whatever the call returns)
        if (const int bad = check_audio_ctxs(*ctx, audio_ctx, n, __func__)) return bad;      // wmi_full_batch_ctx's checks, before any device work here too
        for (int i = 0; i < n; ++i) caps[i]->draft_last.clear();       // (a lock-step call carries no draft and leaves none)
        for (int i = 0; i < n; ++i) if (caps[i]->count <= 0) return -3; // an empty session: wmi_full_batch's empty chunk
        if (!HIP_OK(hipSetDevice(ctx->device))) return -2;
        std::vector<const float *> pcm(n); std::vector<int> ns(n);
        for (int i = 0; i < n; ++i) {
            const int r = refresh(caps[i]);
            if (r < 0) return r;
            if (r == 0) return -3;
            pcm[i] = caps[i]->d_pcm; ns[i] = r;                         // the sessions' own device buffers: nothing is copied
        }
        return wmi_full_batch_ctx(ctx, params, pcm.data(), ns.data(), audio_ctx, n, 1);
    } catch (...) { WMI_ERR("wmi_capture_full_batch: out of memory\n"); return -3; }
}

int wmi_capture_stats(struct wmi_capture * c, int64_t * out4) {
    if (!c || !out4) return -1;
    Scope lk(c->ctx);
    memcpy(out4, c->stats, sizeof(c->stats));
    return 0;
}

int wmi_selftest_capture_plan(int n_old, int n_new, int src_rate, int converter, long long * first_dirty, long long * n_out_old,
                              long long * n_out_new) {
    if (n_old < 0 || n_new < n_old || src_rate <= 0 || src_rate == RATE_16K || converter < 1 || converter > 4) return -1;
    try {
        const double ratio = (double) (uint32_t) RATE_16K / (double) (uint32_t) src_rate;
        const k::ResamplePlan a = k::resample_plan(n_old, (int) ((uint32_t) n_old * ratio), ratio, converter);
        const k::ResamplePlan b = k::resample_plan(n_new, (int) ((uint32_t) n_new * ratio), ratio, converter);
        if (b.error) return b.error;
        if (first_dirty) *first_dirty = a.error ? 0 : k::resample_first_dirty(a, n_old, b);
        if (n_out_old) *n_out_old = a.error ? 0 : a.n_out;
        if (n_out_new) *n_out_new = b.n_out;
        return 0;
    } catch (...) { return -3; }
}

}  // extern "C"

// Speaker labels from the two channels of a stereo clip (include/wmi_device.h wmi_speaker, wmi_set_speaker): the tables' bookkeeping, the
// accessors and the stand-alone call.
//
// replaces: whisper.cpp's --diarize (examples/main/main.cpp:237-268), a host loop per segment over an f32 copy of both channels.
//
// A transcription call that takes a mode asks for a table per stereo clip (speaker_reserve), queues k::channel_bins and the table's copy to
// pinned host memory behind the clip's conversion (speaker_queue, from wav_job_run / wmi_capture_full) and, once it has returned 0, says
// what its result is (speaker_commit).  Nothing here waits: the copy is complete behind the wait the call makes for its own results.  The
// accessors form a record from the table (speaker_ranges.h) when they are asked: the times are the selected result's own.

#include <atomic>
#include <climits>
#include <cstring>
#include <mutex>
#include <vector>
#include "wmi.h"
#include "kernels.h"
#include "speaker_ranges.h"

namespace wmi {

struct SpeakerTable {
    void * d = nullptr, * h = nullptr; size_t cap = 0;        // (nb + 1) * 16 bytes each, grow-only; h pinned
    int kind = 0, rate = 0; long long n = 0, nb = 0;
    bool live = false;                                        // the last call made this table (a mono clip's slot: false)
};

struct SpeakerWork {
    std::vector<SpeakerTable> tables;
    int mode = 0; double ratio = 1.1;                         // of the call in progress / the last one
    int n_clips = 0;
    std::atomic<int> family{0};                               // 0: the context's result carries no table
    bool token_times = false;
    int sel = -1;                                             // wmi_batch_select's chunk (-1: the one clip / the merged view)
    int64_t stats[4] = {0, 0, 0, 0};
};

namespace {

struct Scope {                                                         // the context's lock, then its own state's (api.cpp CtxScope)
    std::unique_lock<std::recursive_mutex> lk, lks;
    explicit Scope(whisper_context * c) : lk(c->mu) { if (State * st = c->state.own) lks = std::unique_lock<std::recursive_mutex>(st->mu); }
};

void table_free(SpeakerTable & t) {
    if (t.d) (void) hipFree(t.d);
    if (t.h) (void) hipHostFree(t.h);
    t = SpeakerTable();
}

bool table_reserve(SpeakerTable & t, int kind, long long n, int rate) {
    const long long nb = k::channel_bins_count(n, rate);
    if (nb > (long long) 1 << 40) return false;
    const size_t bytes = ((size_t) nb + 1) * 16;
    if (bytes > t.cap) {
        table_free(t);
        const size_t cap = bytes + bytes / 4;
        if (!HIP_OK(hipMalloc(&t.d, cap)) || !HIP_OK(hipHostMalloc(&t.h, cap, hipHostMallocDefault))) { table_free(t); return false; }
        t.cap = cap;
    }
    t.kind = kind; t.rate = rate; t.n = n; t.nb = nb; t.live = true;
    return true;
}

bool table_queue(SpeakerTable & t, const void * d_src, hipStream_t s, int64_t * stats) {
    const size_t bytes = ((size_t) t.nb + 1) * 16;
    if (t.n == 0) { memset(t.h, 0, bytes); return true; }
    if (!k::channel_bins(t.kind, d_src, t.n, t.rate, t.d, s)) return false;
    if (!HIP_OK(hipMemcpyAsync(t.h, t.d, bytes, hipMemcpyDeviceToHost, s))) return false;
    if (stats) { stats[2] += (int64_t) bytes; stats[3] += 1; }
    return true;
}

int kind_of_format(int format) { return format == WMI_WAV_S16 ? spk::KIND_S16 : format == WMI_WAV_S8 ? spk::KIND_S8 : format == WMI_WAV_F32 ? spk::KIND_F32 : 0; }

void fill(wmi_speaker * out, const spk::Range & r) {
    out->speaker = r.speaker; out->reserved = 0; out->is0 = r.is0; out->is1 = r.is1; out->e0 = r.e0; out->e1 = r.e1;
}

// the table behind the selected result and the shift that makes its times absolute; null: none
const SpeakerTable * selected_table(whisper_context & ctx, int64_t * shift) {
    *shift = 0;
    SpeakerWork * w = ctx.spk;
    if (!w || w->mode == 0) return nullptr;
    const int family = w->family.load();
    int slot = 0;
    if (family == 2) { if (w->sel < 0) return nullptr; slot = w->sel; }
    else if (family == 3) {
        if (w->sel >= 0) {                                             // a piece: its times are relative to its first frame (10 ms each)
            if (!ctx.batch || !ctx.batch->lng.valid || w->sel >= (int) ctx.batch->lng.pieces.size()) return nullptr;
            *shift = ctx.batch->lng.pieces[w->sel].frame0;
        }
    } else if (family != 1 || w->sel >= 0) return nullptr;              // (a wmi_batch_select behind a one-clip call shows another call's result)
    if (slot >= (int) w->tables.size() || slot >= w->n_clips || !w->tables[slot].live) return nullptr;
    return &w->tables[slot];
}

// the parts of a clip's plan the table needs (wav.cpp wav_plan's checks, without the resampler: any positive rate will do)
int clip_check(const wmi_wav * w, int * kind, long long * frames) {
    if (!w || !w->data) return -1;
    int sb = 0;
    switch (w->format) {
        case WMI_WAV_S8:  sb = 1; break;
        case WMI_WAV_S16: sb = 2; break;
        case WMI_WAV_F32: sb = 4; break;
        case 2: case 3:   return -11;
        default:          return -1;
    }
    if (w->stereo < 0 || w->stereo > 1 || w->mix_rate <= 0 || w->n_bytes < 0) return -1;
    const long long f = w->n_bytes / sb / (w->stereo ? 2 : 1);
    if (f > INT_MAX) return -1;
    if (w->on_device && ((uintptr_t) w->data % (uintptr_t) sb)) return -1;
    if (!w->stereo) return -12;
    *kind = kind_of_format(w->format); *frames = f;
    return 0;
}

}  // namespace

bool speaker_begin(whisper_context & ctx, int n_clips) {
    if (ctx.speaker_mode == 0) { if (ctx.spk) { ctx.spk->mode = 0; ctx.spk->family = 0; } return false; }
    if (!ctx.spk) ctx.spk = new SpeakerWork();
    SpeakerWork & w = *ctx.spk;
    w.mode = ctx.speaker_mode; w.ratio = ctx.speaker_ratio; w.family = 0; w.sel = -1; w.n_clips = n_clips;
    if ((int) w.tables.size() < n_clips) w.tables.resize((size_t) n_clips);
    for (auto & t : w.tables) t.live = false;
    memset(w.stats, 0, sizeof(w.stats));
    return true;
}

bool speaker_reserve(whisper_context & ctx, int slot, int kind, long long n_frames, int rate) {
    SpeakerWork * w = ctx.spk;
    if (!w || slot < 0 || slot >= (int) w->tables.size()) return false;
    if (n_frames < 0 || (kind != k::SRC_F32_STEREO && kind != k::SRC_S16_STEREO && kind != k::SRC_S8_STEREO)) return true;   // no table
    if (!table_reserve(w->tables[slot], kind, n_frames, rate)) return false;
    w->stats[0] += 1; w->stats[1] += w->tables[slot].nb;
    return true;
}

bool speaker_queue(whisper_context & ctx, int slot, const void * d_src, hipStream_t s) {
    SpeakerWork * w = ctx.spk;
    if (!w || slot < 0 || slot >= (int) w->tables.size() || !w->tables[slot].live) return true;
    return table_queue(w->tables[slot], d_src, s, w->stats);
}

void speaker_commit(whisper_context & ctx, int family, bool token_times) {
    if (!ctx.spk) return;
    ctx.spk->token_times = token_times; ctx.spk->sel = -1;
    ctx.spk->family = family;
}

void speaker_invalidate(whisper_context & ctx) { if (ctx.spk) ctx.spk->family = 0; }

void speaker_select(whisper_context & ctx, int chunk) { if (ctx.spk) ctx.spk->sel = chunk; }

void free_speaker(whisper_context & ctx) {
    if (!ctx.spk) return;
    for (auto & t : ctx.spk->tables) table_free(t);
    delete ctx.spk;
    ctx.spk = nullptr;
}

}  // namespace wmi

using namespace wmi;

extern "C" {

int wmi_set_speaker(struct whisper_context * ctx, int mode, double ratio) {
    if (!ctx) return -2;
    if (mode < 0 || mode > 2) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const int prev = ctx->speaker_mode;
    ctx->speaker_mode = mode;
    ctx->speaker_ratio = ratio > 0.0 ? ratio : 1.1;                    // (NaN compares false)
    return prev;
}

int wmi_full_get_segment_speaker(struct whisper_context * ctx, int i_segment, struct wmi_speaker * out) {
    if (!ctx || !out || !ctx->state) return -1;
    Scope lk(ctx);
    const State & st = *ctx->state;
    if (i_segment < 0 || i_segment >= (int) st.result_all.size()) return -1;
    int64_t shift = 0;
    const SpeakerTable * t = selected_table(*ctx, &shift);
    if (!t) return -2;
    const Segment & seg = st.result_all[i_segment];
    fill(out, spk::range_eval(t->h, t->nb, t->kind, t->n, t->rate, ctx->spk->ratio, seg.t0 + shift, seg.t1 + shift));
    return 0;
}

int wmi_full_get_token_speaker(struct whisper_context * ctx, int i_segment, int i_token, struct wmi_speaker * out) {
    if (!ctx || !out || !ctx->state) return -1;
    Scope lk(ctx);
    const State & st = *ctx->state;
    if (i_segment < 0 || i_segment >= (int) st.result_all.size()) return -1;
    const Segment & seg = st.result_all[i_segment];
    if (i_token < 0 || i_token >= (int) seg.tokens.size()) return -1;
    int64_t shift = 0;
    const SpeakerTable * t = selected_table(*ctx, &shift);
    if (!t || ctx->spk->mode != 2 || !ctx->spk->token_times) return -2;
    const whisper_token_data & tk = seg.tokens[i_token];
    if (tk.t0 < 0 || tk.t1 < 0) return -2;                             // a token without times
    fill(out, spk::range_eval(t->h, t->nb, t->kind, t->n, t->rate, ctx->spk->ratio, tk.t0 + shift, tk.t1 + shift));
    return 0;
}

int wmi_wav_speaker(struct whisper_context * ctx, const struct wmi_wav * wav, const int64_t * t0, const int64_t * t1, int n, double ratio,
                    struct wmi_speaker * out) {
    if (!ctx) return -1;
    try {
        int kind = 0; long long frames = 0;
        wmi_wav s16;                                                   // an IMA-ADPCM clip in mode 1 of wmi_set_wav_adpcm: the s16 clip its decode makes
        const bool adpcm = wav && wav->format == 2 && ctx->wav_adpcm_mode;
        if (adpcm) { if (const int e = adpcm_as_s16(wav, &s16)) return e; }
        if (const int e = clip_check(adpcm ? &s16 : wav, &kind, &frames)) return e;
        if (n < 0 || (n > 0 && (!t0 || !t1 || !out))) return -1;
        Scope lk(ctx);
        if (!ctx->state || !compute_ready(*ctx, __func__)) return -2;
        if (!HIP_OK(hipSetDevice(ctx->device))) return -2;
        hipStream_t s = ctx->state->dev.stream;
        SpeakerTable t;                                                // of this call alone: a transcription's tables stay as they are
        struct Free { SpeakerTable & t; void * d_bytes = nullptr; ~Free() { if (d_bytes) (void) hipFree(d_bytes); table_free(t); } } fr{t};
        if (!table_reserve(t, kind, frames, wav->mix_rate)) return -3;
        const void * src = wav->data;
        const size_t fb = (size_t) (kind == spk::KIND_F32 ? 8 : kind == spk::KIND_S16 ? 4 : 2);
        if (adpcm) { if (!adpcm_stage(*ctx, *wav, s, &src)) return -3; }
        else if (!wav->on_device && frames > 0) {
            if (!HIP_OK(hipMalloc(&fr.d_bytes, (size_t) frames * fb)) ||
                !HIP_OK(hipMemcpyAsync(fr.d_bytes, wav->data, (size_t) frames * fb, hipMemcpyHostToDevice, s))) return -3;
            src = fr.d_bytes;
        }
        bool ok = table_queue(t, src, s, nullptr);
        ok = HIP_OK(hipStreamSynchronize(s)) && ok;                    // the one wait
        if (!ok || !HIP_OK(hipGetLastError())) return -3;
        const double r = ratio > 0.0 ? ratio : 1.1;
        for (int i = 0; i < n; ++i) fill(out + i, spk::range_eval(t.h, t.nb, t.kind, t.n, t.rate, r, t0[i], t1[i]));
        return 0;
    } catch (...) { WMI_ERR("%s: out of memory\n", __func__); return -3; }
}

int wmi_speaker_stats(struct whisper_context * ctx, int64_t * out4) {
    if (!ctx || !out4) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    memset(out4, 0, 4 * sizeof(int64_t));
    if (ctx->spk) memcpy(out4, ctx->spk->stats, sizeof(ctx->spk->stats));
    return 0;
}

int wmi_selftest_channel_bins(int device, const struct wmi_wav * wav, void * bins, long long cap_bins, long long * n_bins, void * last2) {
    try {
        int kind = 0; long long frames = 0;
        if (const int e = clip_check(wav, &kind, &frames)) return e;
        if (device < 0 || cap_bins < 0 || !n_bins || !last2 || (cap_bins > 0 && !bins)) return -1;
        const long long nb = k::channel_bins_count(frames, wav->mix_rate);
        *n_bins = nb;
        if (nb > cap_bins) return -4;
        if (frames == 0) { memset(last2, 0, 16); return 0; }
        if (!HIP_OK(hipSetDevice(device))) return -2;
        // the table with a guard behind the last-frame pair: the launch may write (nb + 1) * 16 bytes and nothing else
        constexpr size_t GUARD = 256;
        const size_t bytes = ((size_t) nb + 1) * 16, total = bytes + GUARD;
        void * d_tab = nullptr, * d_bytes = nullptr; hipStream_t st = nullptr;
        struct Free { void *& a; void *& b; hipStream_t & s; ~Free() { if (s) (void) hipStreamDestroy(s); if (a) (void) hipFree(a); if (b) (void) hipFree(b); } } fr{d_tab, d_bytes, st};
        if (!HIP_OK(hipMalloc(&d_tab, total)) || !HIP_OK(hipStreamCreate(&st)) || !HIP_OK(hipMemsetAsync(d_tab, 0xA5, total, st))) return -3;
        const void * src = wav->data;
        const size_t fb = (size_t) (kind == spk::KIND_F32 ? 8 : kind == spk::KIND_S16 ? 4 : 2);
        if (!wav->on_device) {
            if (!HIP_OK(hipMalloc(&d_bytes, (size_t) frames * fb)) ||
                !HIP_OK(hipMemcpyAsync(d_bytes, wav->data, (size_t) frames * fb, hipMemcpyHostToDevice, st))) return -3;
            src = d_bytes;
        }
        std::vector<unsigned char> host(total);
        bool ok = k::channel_bins(kind, src, frames, wav->mix_rate, d_tab, st);
        ok = ok && HIP_OK(hipMemcpyAsync(host.data(), d_tab, total, hipMemcpyDeviceToHost, st));
        ok = HIP_OK(hipStreamSynchronize(st)) && ok;
        if (!ok || !HIP_OK(hipGetLastError())) return -3;
        for (size_t i = bytes; i < total; ++i) if (host[i] != 0xA5) return -5;     // the guard was written
        memcpy(bins, host.data(), (size_t) nb * 16);
        memcpy(last2, host.data() + (size_t) nb * 16, 16);
        return 0;
    } catch (...) { return -3; }
}

int wmi_bench_channel_bins(int device, const struct wmi_wav * wav, int iters, float * ms) {
    try {
        int kind = 0; long long frames = 0;
        if (const int e = clip_check(wav, &kind, &frames)) return e;
        if (device < 0 || iters < 1 || !ms || frames < 1) return -1;
        if (!HIP_OK(hipSetDevice(device))) return -2;
        const long long nb = k::channel_bins_count(frames, wav->mix_rate);
        void * d_tab = nullptr, * d_bytes = nullptr; hipStream_t st = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
        struct Free { void *& a; void *& b; hipStream_t & s; hipEvent_t * e;
                      ~Free() { for (int i = 0; i < 2; ++i) if (e[i]) (void) hipEventDestroy(e[i]); if (s) (void) hipStreamDestroy(s); if (a) (void) hipFree(a); if (b) (void) hipFree(b); } } fr{d_tab, d_bytes, st, ev};
        if (!HIP_OK(hipMalloc(&d_tab, ((size_t) nb + 1) * 16)) || !HIP_OK(hipStreamCreate(&st)) || !HIP_OK(hipEventCreate(&ev[0])) || !HIP_OK(hipEventCreate(&ev[1]))) return -3;
        const void * src = wav->data;
        const size_t fb = (size_t) (kind == spk::KIND_F32 ? 8 : kind == spk::KIND_S16 ? 4 : 2);
        if (!wav->on_device) {
            if (!HIP_OK(hipMalloc(&d_bytes, (size_t) frames * fb)) ||
                !HIP_OK(hipMemcpyAsync(d_bytes, wav->data, (size_t) frames * fb, hipMemcpyHostToDevice, st))) return -3;
            src = d_bytes;
        }
        for (int i = 0; i < iters; ++i) {
            if (!HIP_OK(hipEventRecord(ev[0], st)) || !k::channel_bins(kind, src, frames, wav->mix_rate, d_tab, st) || !HIP_OK(hipEventRecord(ev[1], st)) ||
                !HIP_OK(hipEventSynchronize(ev[1])) || !HIP_OK(hipEventElapsedTime(ms + i, ev[0], ev[1]))) return -3;
        }
        return 0;
    } catch (...) { return -3; }
}

int wmi_selftest_speaker_ranges(const void * bins, long long n_bins, const void * last2, int kind, long long n_frames, int rate, double ratio,
                                const int64_t * t0, const int64_t * t1, int n_ranges, struct wmi_speaker * out) {
    (void) last2;
    const int kd = kind_of_format(kind);
    if (!kd || n_frames < 0 || n_frames > INT_MAX || rate <= 0 || n_ranges < 0 || (n_ranges > 0 && (!t0 || !t1 || !out))) return -1;
    if (n_bins != spk::n_bins(n_frames, rate) || (n_bins > 0 && !bins)) return -1;
    const double r = ratio > 0.0 ? ratio : 1.1;
    for (int i = 0; i < n_ranges; ++i) fill(out + i, spk::range_eval(bins, n_bins, kd, n_frames, rate, r, t0[i], t1[i]));
    return 0;
}

}  // extern "C"

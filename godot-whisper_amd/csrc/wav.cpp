// AudioStreamWAV ingest (include/wmi_device.h wmi_wav_* / wmi_full_*_wav): the asset's bytes go to the device as bytes and become the
// mono 16 kHz f32 samples of the transcription in ONE launch per clip.
//
// replaces: AudioStreamToText.get_text (bin/addons/godot_whisper/audio_stream_to_text.gd:31-48) — a GDScript loop over every sample and a
// 4-byte float per 2-byte sample over PCIe, with the three misreadings INTEGRATION.md lists (stereo, other rates, every second 8-bit byte).
//
// A clip is planned on the host (format, frame count, the resampler's plan: nothing touches the device, every argument error is decided
// here), then queued: the upload of its bytes into the context's grow-only byte buffer, the position table of a rate without a closed
// form, and one launch — k_wav_decode at 16 kHz, else the resampler reading the packed frames (k_resample.hip in_frame<KIND>).  For
// wmi_full_wav the launch writes into the staging area behind pcm_to_mel's padded image, on the log-mel's stream (DeviceState::pcm_job);
// the long and the batch form convert into a buffer of the context and hand wmi_full_long / wmi_full_batch device pointers.
//
// IMA-ADPCM (format 2, wmi_set_wav_adpcm mode 1): the clip's bytes go up as they are, k::adpcm_decode (k_adpcm.hip: two prefix scans, five
// launches) writes the interleaved s16 samples into a grow-only image of the context on the same stream, and the job goes on as the
// device-resident WMI_WAV_S16 clip that image is — the conversion, the resampler's readers, the channel split and the speaker bins run as
// they are.  Mode 0 refuses the format as before and allocates nothing.

#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>
#include <vector>
#include "wmi.h"
#include "kernels.h"
#include "channel_merge.h"
#include "adpcm_map.h"

namespace wmi {

struct WavPlan {
    int err = 0;                          // a conversion error of wmi_device.h, or 0
    int kind = 0, sample_bytes = 0;       // k::SrcKind
    long long frames = 0, n_out = 0;
    bool resample = false; k::ResamplePlan pl;
    bool adpcm = false;                   // format 2 in mode 1: the bytes are decoded to s16 first; kind and frames are the decoded clip's
};

struct WavJob {
    const wmi_wav * wav = nullptr; int converter = 0;
    WavPlan plan;
    size_t bytes_off = 0, tab_off = 0;    // the clip's place in the byte buffer / the position tables (batch: one after the other)
    bool mark_begin = true, mark_end = true;   // record the events of wmi_wav_stats' timer around this job
    bool used = false;
    int spk_slot = -1;                    // >= 0: the clip's table of channel energies (speaker.cpp) is queued behind its conversion
    size_t s16_off = 0;                   // an ADPCM clip's place in the s16 image (in samples, a multiple of 8)
};

struct WavWork {
    unsigned char * d_bytes = nullptr; size_t bytes_cap = 0;       // the clips' bytes as uploaded (grow-only)
    int * d_pos = nullptr; double * d_frac = nullptr; size_t tab_cap = 0;
    float * d_out = nullptr; size_t out_cap = 0;                   // wmi_wav_to_pcm with a host dst
    float * d_pcm = nullptr; size_t pcm_cap = 0;                   // the samples of the long and the batch form
    int16_t * d_s16 = nullptr; size_t s16_cap = 0;                 // ADPCM clips decoded: interleaved s16, one clip after the other (grow-only)
    unsigned char * d_scan = nullptr; size_t scan_cap = 0;         // the scans' scratch (k::adpcm_scratch_bytes of the largest clip; the clips
                                                                   // of a call decode one behind the other on one stream)
    hipEvent_t ev[2] = {nullptr, nullptr}; bool ev_pending = false;
    int64_t stats[5] = {0, 0, 0, 0, 0};
    // wmi_full_wav_channels: the dialogue view of the last call (copies of the two channels' segments in channel_merge.h's order) and where
    // each came from; valid until the next transcription call, shown: the dialogue is what the accessors read now
    struct Channels { std::vector<Segment> merged; std::vector<wmi_channel_segment> from; int lang_id = -1; bool valid = false, shown = false; } ch;
};

namespace {

constexpr int RATE_16K = WHISPER_SAMPLE_RATE;

struct Scope {                                                         // the context's lock, then its own state's (api.cpp CtxScope)
    std::unique_lock<std::recursive_mutex> lk, lks;
    explicit Scope(whisper_context * c) : lk(c->mu) { if (State * st = c->state.own) lks = std::unique_lock<std::recursive_mutex>(st->mu); }
};

// everything that can be said about a clip without a device
WavPlan wav_plan(const wmi_wav * w, int converter, const char * who, int adpcm_mode) {
    WavPlan p;
    if (!w || !w->data) { p.err = -1; return p; }
    bool stereo = w->stereo == 1;
    switch (w->format) {
        case WMI_WAV_S8:  p.kind = stereo ? k::SRC_S8_STEREO : k::SRC_S8_MONO; p.sample_bytes = 1; break;
        case WMI_WAV_S16: p.kind = stereo ? k::SRC_S16_STEREO : k::SRC_S16_MONO; p.sample_bytes = 2; break;
        case WMI_WAV_F32: p.kind = stereo ? k::SRC_F32_STEREO : k::SRC_F32_MONO; p.sample_bytes = 4; break;
        case 2:
            if (adpcm_mode) { p.adpcm = true; p.kind = stereo ? k::SRC_S16_STEREO : k::SRC_S16_MONO; p.sample_bytes = 1; break; }   // (no alignment asked)
            [[fallthrough]];
        case 3:
            WMI_ERR("%s: format %d (%s) is not decoded here%s\n", who, w->format, w->format == 2 ? "IMA-ADPCM" : "QOA",
                    w->format == 2 ? ": wmi_set_wav_adpcm turns its decode on" : "");
            p.err = -11; return p;
        default: p.err = -1; return p;
    }
    if (w->stereo < 0 || w->stereo > 1 || w->mix_rate <= 0 || w->n_bytes < 0) { p.err = -1; return p; }
    p.frames = p.adpcm ? adpcm::frames_of(w->n_bytes, stereo)          // two frames per byte (and channel)
                       : w->n_bytes / p.sample_bytes / (stereo ? 2 : 1);   // a trailing incomplete sample or frame is ignored
    if (p.frames > INT_MAX) { p.err = -1; return p; }
    if (w->on_device && ((uintptr_t) w->data % (uintptr_t) p.sample_bytes)) { p.err = -1; return p; }
    if (w->mix_rate == RATE_16K) { p.n_out = p.frames; return p; }
    if (converter < 0 || converter > 4) { p.err = -1; return p; }
    p.resample = true;
    const double ratio = (double) (uint32_t) RATE_16K / (double) (uint32_t) w->mix_rate;         // src/speech_to_text.cpp:25-26, as wmi_resample
    const long long out_frames = (int) ((uint32_t) p.frames * ratio);
    p.pl = k::resample_plan(p.frames, out_frames, ratio, converter);
    if (p.pl.error == -10) { p.err = -10; return p; }
    if (p.pl.error == -31) WMI_ERR("%s: SRC_LINEAR cannot upsample a single frame, 0 frames\n", who);
    else if (p.pl.error) WMI_ERR("%s: converter error %d (src_simple would report it through src_strerror)\n", who, -p.pl.error);
    p.n_out = p.pl.error ? 0 : p.pl.n_out;                             // the host gets 0 frames on a converter error (:33-36)
    return p;
}

WavWork * work(whisper_context & ctx) {
    if (!ctx.wav) {
        WavWork * w = new WavWork();
        if (!HIP_OK(hipEventCreate(&w->ev[0])) || !HIP_OK(hipEventCreate(&w->ev[1]))) {
            for (hipEvent_t e : w->ev) if (e) (void) hipEventDestroy(e);
            delete w;
            return nullptr;
        }
        ctx.wav = w;
    }
    return ctx.wav;
}

// grow-only; the caller knows the buffer is idle (every call of this file waits for its launches before it returns)
template <typename T> bool reserve(T *& p, size_t & cap, size_t want, size_t slack) {
    if (want <= cap) return true;
    if (p) (void) hipFree(p);
    p = nullptr; cap = 0;
    if (!HIP_OK(hipMalloc((void **) &p, (want + slack) * sizeof(T)))) return false;
    cap = want + slack;
    return true;
}
bool reserve_tables(WavWork & w, size_t want) {
    if (want <= w.tab_cap) return true;
    if (w.d_pos) (void) hipFree(w.d_pos);
    if (w.d_frac) (void) hipFree(w.d_frac);
    w.d_pos = nullptr; w.d_frac = nullptr; w.tab_cap = 0;
    if (!HIP_OK(hipMalloc((void **) &w.d_pos, want * 4)) || !HIP_OK(hipMalloc((void **) &w.d_frac, want * 8))) return false;
    w.tab_cap = want;
    return true;
}

size_t up16(size_t n) { return (n + 15) & ~(size_t) 15; }

// room for the jobs' bytes and position tables, each job's place written into it; resets the counters of wmi_wav_stats
bool reserve_jobs(WavWork & w, WavJob * jobs, int n) {
    size_t bytes = 0, tab = 0, s16 = 0, scan = 0;
    for (int i = 0; i < n; ++i) {
        WavJob & j = jobs[i];
        if (j.plan.frames <= 0 || j.plan.n_out <= 0) continue;
        if (j.plan.adpcm) {                                                // (+ 8: the image may start up to 6 samples behind its place, adpcm_plan's out_skew)
            const bool stereo = j.wav->stereo == 1;
            j.s16_off = s16; s16 += ((size_t) j.plan.frames * (stereo ? 2 : 1) + 8 + 7) & ~(size_t) 7;
            scan = std::max(scan, k::adpcm_scratch_bytes(j.wav->n_bytes, stereo));
        }
        if (!j.wav->on_device) { j.bytes_off = bytes; bytes += up16((size_t) j.wav->n_bytes); }
        if (j.plan.resample && j.plan.pl.need_table) { j.tab_off = tab; tab += (size_t) j.plan.n_out; }
    }
    memset(w.stats, 0, sizeof(w.stats)); w.ev_pending = false;
    return reserve(w.d_bytes, w.bytes_cap, bytes, 4096) && reserve_tables(w, tab) &&
           reserve(w.d_s16, w.s16_cap, s16, 4096) && reserve(w.d_scan, w.scan_cap, scan, 4096);      // (nothing asked: nothing allocated)
}

// the tables of a call that takes a speaker mode (wmi_set_speaker): one per stereo clip that is converted; false: out of memory
bool reserve_speaker(whisper_context & ctx, WavJob * jobs, int n) {
    if (!speaker_begin(ctx, n)) return true;
    for (int i = 0; i < n; ++i) {
        const WavPlan & p = jobs[i].plan;
        const bool table = p.frames > 0 && p.n_out > 0 && jobs[i].wav->stereo == 1;
        if (!speaker_reserve(ctx, i, p.kind, table ? p.frames : -1, jobs[i].wav->mix_rate)) return false;
        if (table) jobs[i].spk_slot = i;
    }
    return true;
}

hipStream_t mel_stream_of(State & st) { return st.dev.mel_stream ? st.dev.mel_stream : st.dev.stream; }   // pcm_to_mel's choice

}  // namespace

bool wav_job_run(whisper_context & ctx, WavJob & job, float * d_dst, hipStream_t s, float * d_dst1) {
    WavWork * w = ctx.wav;
    if (!w) return false;
    const WavPlan & p = job.plan;
    job.used = true;
    if (job.mark_begin) HIP_TRY(hipEventRecord(w->ev[0], s));
    if (p.frames > 0 && p.n_out > 0) {
        const void * src = job.wav->data;
        if (!job.wav->on_device) {                                         // the bytes as they are: 1 or 2 per sample, not 4
            unsigned char * d = w->d_bytes + job.bytes_off;
            HIP_TRY(hipMemcpyAsync(d, job.wav->data, (size_t) job.wav->n_bytes, hipMemcpyHostToDevice, s));
            w->stats[0] += job.wav->n_bytes;
            src = d;
        }
        if (p.adpcm) {                                                     // bytes -> the s16 image; from here on the clip is that image
            const bool stereo = job.wav->stereo == 1;
            const k::AdpcmPlan ap = k::adpcm_plan(src, job.wav->n_bytes, stereo);
            int16_t * img = w->d_s16 + job.s16_off + ap.out_skew;
            if (!k::adpcm_decode(ap, src, stereo, img, w->d_scan, s)) return false;
            w->stats[3] += k::ADPCM_LAUNCHES;
            src = img;
        }
        if (!p.resample) {
            if (!(d_dst1 ? k::wav_split(p.kind, src, p.frames, d_dst, d_dst1, s) : k::wav_decode(p.kind, src, p.frames, d_dst, s))) return false;
        } else {
            const float * d_tab = nullptr;
            if (job.converter <= 2) {                                      // the converter's table, shared with wmi_resample
                float *& d_sinc = ctx.d_sinc[job.converter];
                if (!d_sinc) {
                    const float * coeffs; int count, inc;
                    (void) k::sinc_table(job.converter, &coeffs, &count, &inc);
                    const bool ok = HIP_OK(hipMalloc((void **) &d_sinc, (size_t) count * 4)) &&
                                    HIP_OK(hipMemcpyAsync(d_sinc, coeffs, (size_t) count * 4, hipMemcpyHostToDevice, s));
                    if (!ok) { if (d_sinc) { (void) hipFree(d_sinc); d_sinc = nullptr; } return false; }
                }
                d_tab = d_sinc;
            }
            const int * d_pos = nullptr; const double * d_frac = nullptr;
            if (p.pl.need_table) {                                         // positions from the host's recurrence (index bookkeeping)
                const int * hp; const double * hf;
                k::resample_table(p.pl, &hp, &hf);
                HIP_TRY(hipMemcpyAsync(w->d_pos + job.tab_off, hp, (size_t) p.n_out * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipMemcpyAsync(w->d_frac + job.tab_off, hf, (size_t) p.n_out * 8, hipMemcpyHostToDevice, s));
                w->stats[0] += p.n_out * 12;
                d_pos = w->d_pos + job.tab_off; d_frac = w->d_frac + job.tab_off;
            }
            if (d_dst1) k::resample_launch_split(p.pl, p.kind, src, p.frames, d_dst, d_dst1, d_tab, d_pos, d_frac, s);
            else k::resample_launch_kind(p.pl, p.kind, src, p.frames, d_dst, d_tab, d_pos, d_frac, 0, s);
            HIP_TRY(hipGetLastError());
        }
        w->stats[3] += 1;
        if (job.spk_slot >= 0 && !speaker_queue(ctx, job.spk_slot, src, s)) return false;       // the frames once more, where they lie
    }
    w->stats[1] += p.frames; w->stats[2] += d_dst1 ? 2 * p.n_out : p.n_out;
    if (job.mark_end) { HIP_TRY(hipEventRecord(w->ev[1], s)); w->ev_pending = true; }
    return true;
}

void free_wav(whisper_context & ctx) {
    WavWork * w = ctx.wav;
    if (!w) return;
    for (void * p : { (void *) w->d_bytes, (void *) w->d_pos, (void *) w->d_frac, (void *) w->d_out, (void *) w->d_pcm, (void *) w->d_s16, (void *) w->d_scan }) if (p) (void) hipFree(p);
    for (hipEvent_t e : w->ev) if (e) (void) hipEventDestroy(e);
    delete w;
    ctx.wav = nullptr;
}

int adpcm_as_s16(const wmi_wav * w, wmi_wav * s16) {
    if (!w || !w->data || w->format != 2 || w->stereo < 0 || w->stereo > 1 || w->mix_rate <= 0 || w->n_bytes < 0) return -1;   // wav_plan's checks; any rate
    const long long frames = adpcm::frames_of(w->n_bytes, w->stereo == 1);
    if (frames > INT_MAX) return -1;
    *s16 = wmi_wav{ w->data, frames * (w->stereo == 1 ? 4 : 2), WMI_WAV_S16, w->stereo, w->mix_rate, 0 };
    return 0;
}

bool adpcm_stage(whisper_context & ctx, const wmi_wav & wav, hipStream_t s, const void ** d_s16) {
    WavWork * w = work(ctx);
    if (!w) return false;
    WavJob job; job.wav = &wav;
    job.plan.adpcm = true;
    job.plan.frames = job.plan.n_out = adpcm::frames_of(wav.n_bytes, wav.stereo == 1);     // (n_out: reserve_jobs skips a clip without results)
    if (!reserve_jobs(*w, &job, 1)) return false;
    *d_s16 = nullptr;
    if (job.plan.frames <= 0) return true;
    const void * src = wav.data;
    if (!wav.on_device) {
        HIP_TRY(hipMemcpyAsync(w->d_bytes, wav.data, (size_t) wav.n_bytes, hipMemcpyHostToDevice, s));
        w->stats[0] += wav.n_bytes;
        src = w->d_bytes;
    }
    const bool stereo = wav.stereo == 1;
    const k::AdpcmPlan ap = k::adpcm_plan(src, wav.n_bytes, stereo);
    int16_t * img = w->d_s16 + ap.out_skew;
    if (!k::adpcm_decode(ap, src, stereo, img, w->d_scan, s)) return false;
    w->stats[1] += job.plan.frames; w->stats[3] += k::ADPCM_LAUNCHES;
    *d_s16 = img;
    return true;
}

void channels_invalidate(whisper_context & ctx) { if (ctx.wav) ctx.wav->ch.valid = ctx.wav->ch.shown = false; }

void channels_deselect(whisper_context & ctx) { if (ctx.wav) ctx.wav->ch.shown = false; }

namespace {

// a stereo clip's plan for the two-channel calls; a mono clip is -12 (wmi_wav_speaker's code), behind every other conversion error
WavPlan channels_plan(const wmi_wav * w, int converter, const char * who, int adpcm_mode) {
    WavPlan p = wav_plan(w, converter, who, adpcm_mode);
    if (!p.err && w->stereo != 1) p.err = -12;
    return p;
}

// the dialogue view (as long.cpp's select_merged): copies of the segments, channel 0's language, no windows and no speaker table
void select_dialogue(whisper_context & ctx) {
    WavWork::Channels & c = ctx.wav->ch;
    ctx.state->result_all = c.merged;
    ctx.state->windows.clear();
    if (c.lang_id >= 0) ctx.state->lang_id = c.lang_id;
    speaker_select(ctx, -1);
    c.shown = true;
}

// after wmi_full_batch returned 0 on the two channels: the dialogue view of its two results, left selected
void build_dialogue(whisper_context & ctx) {
    WavWork::Channels & c = ctx.wav->ch;
    const BatchWork & bw = *ctx.batch;
    std::vector<int64_t> t0[2];
    for (int ch = 0; ch < 2; ++ch) for (const Segment & seg : bw.results[ch]) t0[ch].push_back(seg.t0);
    const size_t n = t0[0].size() + t0[1].size();
    std::vector<int> channel(n), index(n);
    chm::merge(t0[0].data(), (int) t0[0].size(), t0[1].data(), (int) t0[1].size(), channel.data(), index.data());
    c.merged.clear(); c.from.clear();
    for (size_t i = 0; i < n; ++i) {
        c.merged.push_back(bw.results[channel[i]][index[i]]);           // a copy: text, tokens, times and t_dtw as they are
        c.from.push_back(wmi_channel_segment{ channel[i], index[i] });
    }
    c.lang_id = !bw.lang_id.empty() ? bw.lang_id[0] : -1;
    c.valid = true;
    select_dialogue(ctx);
}

}  // namespace

}  // namespace wmi

using namespace wmi;

extern "C" {

int wmi_selftest_wav_plan(const struct wmi_wav * wav, int converter, long long * frames, long long * n_out) {
    try {
        const WavPlan p = wav_plan(wav, converter, __func__, 0);          // (no context, no mode: format 2 is refused)
        if (p.err) return p.err;
        if (frames) *frames = p.frames;
        if (n_out) *n_out = p.n_out;
        return 0;
    } catch (...) { return -3; }
}

int wmi_set_wav_adpcm(struct whisper_context * ctx, int on) {
    if (!ctx) return -2;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const int prev = ctx->wav_adpcm_mode;
    ctx->wav_adpcm_mode = on ? 1 : 0;
    return prev;
}

int wmi_selftest_adpcm_plan(const struct wmi_wav * wav, int converter, long long * frames, long long * n_out) {
    try {
        const WavPlan p = wav_plan(wav, converter, __func__, 1);
        if (p.err) return p.err;
        if (frames) *frames = p.frames;
        if (n_out) *n_out = p.n_out;
        return 0;
    } catch (...) { return -3; }
}

int wmi_selftest_adpcm_shape(int * out5) {
    if (!out5) return -1;
    out5[0] = k::ADPCM_CHUNK; out5[1] = 64; out5[2] = k::ADPCM_WG; out5[3] = k::ADPCM_PART_TILE; out5[4] = k::ADPCM_LAUNCHES;
    return 0;
}

int wmi_selftest_adpcm_host(const unsigned char * bytes, long long n_bytes, int stereo, int16_t * out_s16, long long cap_frames) {
    if (n_bytes < 0 || stereo < 0 || stereo > 1 || (n_bytes > 0 && !bytes) || cap_frames < 0) return -1;
    const int nch = stereo ? 2 : 1;
    const long long frames = adpcm::frames_of(n_bytes, stereo == 1);
    if (frames > INT_MAX) return -1;
    if (frames > cap_frames) return -4;
    if (frames > 0 && !out_s16) return -1;
    for (int c = 0; c < nch; ++c) {                                        // the sequential loop: one stream per channel from (0, 0)
        int predictor = 0, index = 0;
        for (long long i = 0; i < frames; ++i) {
            adpcm::decode_nibble(adpcm::nibble_at(bytes, nch, c, i), predictor, index);
            out_s16[i * nch + c] = (int16_t) predictor;
        }
    }
    return (int) frames;
}

int wmi_selftest_adpcm_maps(const unsigned char * nibbles, long long n, int chunk, int32_t * out_predictor, int32_t * out_index, long long cap) {
    if (n < 0 || chunk < 1 || (n > 0 && !nibbles) || cap < 0) return -1;
    try {
        const long long chunks = (n + chunk - 1) / chunk;
        if (chunks + 1 > cap) return -4;
        if (!out_predictor || !out_index) return -1;
        for (long long i = 0; i < n; ++i) if (nibbles[i] > 15) return -1;
        // the plan of k_adpcm.hip with a sequential scan: the chunks' index maps, their prefix applied to 0 ...
        std::vector<adpcm::IdxMap> im((size_t) chunks);
        for (long long j = 0; j < chunks; ++j) {
            adpcm::IdxMap m = adpcm::idx_identity();
            for (long long i = j * chunk; i < std::min(n, (j + 1) * chunk); ++i) m = adpcm::compose(m, adpcm::idx_nibble(nibbles[i]));
            im[(size_t) j] = m;
        }
        adpcm::IdxMap pi = adpcm::idx_identity();
        for (long long j = 0; j <= chunks; ++j) { out_index[j] = adpcm::apply(pi, 0); if (j < chunks) pi = adpcm::compose(pi, im[(size_t) j]); }
        // ... then, from every chunk's entry index, the chunks' predictor maps, and their prefix applied to 0
        adpcm::PredMap pp = adpcm::pred_identity();
        for (long long j = 0; j <= chunks; ++j) {
            out_predictor[j] = adpcm::apply(pp, 0);
            if (j == chunks) break;
            adpcm::PredMap m = adpcm::pred_identity();
            int index = out_index[j];
            for (long long i = j * chunk; i < std::min(n, (j + 1) * chunk); ++i) {
                m = adpcm::compose(m, adpcm::pred_nibble(index, nibbles[i]));
                index = adpcm::apply(adpcm::idx_nibble(nibbles[i]), index);
            }
            pp = adpcm::compose(pp, m);
        }
        return (int) std::min<long long>(chunks, INT_MAX);
    } catch (...) { return -3; }
}

namespace {

// the kernels alone on `device`: source at `offset` bytes into an allocation, the image with a guard behind it; iters > 0: timed, no copy back
int adpcm_run(int device, const unsigned char * bytes, long long n_bytes, int stereo, int offset, int16_t * out_s16, long long cap_frames,
              long long * frames_out, int iters, float * ms) {
    if (device < 0 || n_bytes < 0 || stereo < 0 || stereo > 1 || (n_bytes > 0 && !bytes) || offset < 0 || offset > 4096 || cap_frames < 0) return -1;
    const bool st2 = stereo == 1;
    const long long frames = adpcm::frames_of(n_bytes, st2);
    if (frames > INT_MAX) return -1;
    if (frames_out) *frames_out = frames;
    if (!ms && frames > cap_frames) return -4;
    if (frames == 0) return ms ? -1 : 0;
    if (!ms && !out_s16) return -1;
    if (!HIP_OK(hipSetDevice(device))) return -2;
    constexpr size_t GUARD = 256;
    const size_t n_s16 = (size_t) frames * (st2 ? 2 : 1), img_bytes = 16 + n_s16 * 2, total = img_bytes + GUARD;
    void * d_src = nullptr, * d_img = nullptr, * d_scan = nullptr; hipStream_t s = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
    struct Free { void *& a; void *& b; void *& c; hipStream_t & s; hipEvent_t * e;
                  ~Free() { for (int i = 0; i < 2; ++i) if (e[i]) (void) hipEventDestroy(e[i]); if (s) (void) hipStreamDestroy(s);
                            for (void * p : { a, b, c }) if (p) (void) hipFree(p); } } fr{d_src, d_img, d_scan, s, ev};
    if (!HIP_OK(hipMalloc(&d_src, (size_t) n_bytes + (size_t) offset)) || !HIP_OK(hipMalloc(&d_img, total)) ||
        !HIP_OK(hipMalloc(&d_scan, k::adpcm_scratch_bytes(n_bytes, st2))) || !HIP_OK(hipStreamCreate(&s))) return -3;
    if (!HIP_OK(hipMemsetAsync(d_img, 0xA5, total, s)) ||
        !HIP_OK(hipMemcpyAsync((unsigned char *) d_src + offset, bytes, (size_t) n_bytes, hipMemcpyHostToDevice, s))) return -3;
    const unsigned char * src = (const unsigned char *) d_src + offset;
    const k::AdpcmPlan ap = k::adpcm_plan(src, n_bytes, st2);
    int16_t * img = (int16_t *) d_img + ap.out_skew;                       // (the guard starts right behind the last sample)
    if (ms) {
        if (!HIP_OK(hipEventCreate(&ev[0])) || !HIP_OK(hipEventCreate(&ev[1]))) return -3;
        for (int i = 0; i < iters; ++i)
            if (!HIP_OK(hipEventRecord(ev[0], s)) || !k::adpcm_decode(ap, src, st2, img, d_scan, s) || !HIP_OK(hipEventRecord(ev[1], s)) ||
                !HIP_OK(hipEventSynchronize(ev[1])) || !HIP_OK(hipEventElapsedTime(ms + i, ev[0], ev[1]))) return -3;
        return 0;
    }
    std::vector<unsigned char> host(total);
    bool ok = k::adpcm_decode(ap, src, st2, img, d_scan, s);
    ok = ok && HIP_OK(hipMemcpyAsync(host.data(), d_img, total, hipMemcpyDeviceToHost, s));
    ok = HIP_OK(hipStreamSynchronize(s)) && ok;
    if (!ok || !HIP_OK(hipGetLastError())) return -3;
    const size_t first = (size_t) ap.out_skew * 2, last = first + n_s16 * 2;
    for (size_t i = 0; i < total; ++i) if ((i < first || i >= last) && host[i] != 0xA5) return -5;       // written in front of or behind the image
    memcpy(out_s16, host.data() + first, n_s16 * 2);
    return 0;
}

}  // namespace

int wmi_selftest_adpcm_decode(int device, const unsigned char * bytes, long long n_bytes, int stereo, int src_byte_offset, int16_t * out_s16,
                              long long cap_frames, long long * frames) {
    try { return adpcm_run(device, bytes, n_bytes, stereo, src_byte_offset, out_s16, cap_frames, frames, 0, nullptr); }
    catch (...) { return -3; }
}

int wmi_bench_adpcm_decode(int device, const unsigned char * bytes, long long n_bytes, int stereo, int src_byte_offset, int iters, float * ms) {
    if (iters < 1 || !ms) return -1;
    try { return adpcm_run(device, bytes, n_bytes, stereo, src_byte_offset, nullptr, 0, nullptr, iters, ms); }
    catch (...) { return -3; }
}

int wmi_wav_to_pcm(struct whisper_context * ctx, const struct wmi_wav * wav, int converter, float * dst, int dst_capacity, int dst_on_device) {
    if (!ctx || !ctx->state) return -1;
    try {
        WavJob job; job.wav = wav; job.converter = converter;
        job.plan = wav_plan(wav, converter, __func__, ctx->wav_adpcm_mode);
        if (job.plan.err) return job.plan.err;
        if (!dst || dst_capacity < 0) return -1;
        if (job.plan.n_out > dst_capacity) return -4;
        Scope lk(ctx);
        if (!compute_ready(*ctx, __func__)) return -2;
        if (!HIP_OK(hipSetDevice(ctx->device))) return -2;
        WavWork * w = work(*ctx);
        if (!w) return -3;
        hipStream_t s = mel_stream_of(*ctx->state);
        const size_t n = (size_t) job.plan.n_out;
        if (!reserve_jobs(*w, &job, 1) || (!dst_on_device && !reserve(w->d_out, w->out_cap, n, 1024))) return -3;
        float * d_dst = dst_on_device ? dst : w->d_out;
        bool ok = wav_job_run(*ctx, job, d_dst, s);
        if (ok && !dst_on_device && n > 0) ok = HIP_OK(hipMemcpyAsync(dst, d_dst, n * 4, hipMemcpyDeviceToHost, s));
        ok = HIP_OK(hipStreamSynchronize(s)) && ok;                        // (the caller's bytes and the plan's tables are free again)
        return ok ? (int) n : -3;
    } catch (...) { WMI_ERR("%s: out of memory\n", __func__); return -3; }
}

int wmi_full_wav(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wav, int converter) {
    if (!ctx || !ctx->state) return -101;
    try {
        WavJob job; job.wav = wav; job.converter = converter;
        job.plan = wav_plan(wav, converter, __func__, ctx->wav_adpcm_mode);
        if (job.plan.err) return -100 + job.plan.err;
        Scope lk(ctx);                                                     // wmi_full_device_pcm's locks
        if (!compute_ready(*ctx, __func__)) return -102;
        if (!HIP_OK(hipSetDevice(ctx->device))) return -102;
        WavWork * w = work(*ctx);
        if (!w || !reserve_jobs(*w, &job, 1) || !reserve_speaker(*ctx, &job, 1)) return -103;
        DeviceState & d = ctx->state->dev;
        struct Hook { DeviceState & d; ~Hook() { d.pcm_job = nullptr; } } hook{d};
        d.pcm_job = &job;                                                  // the one pcm_to_mel of full() runs the job instead of copying host samples
        const int r = full(*ctx, params, nullptr, nullptr, (int) job.plan.n_out);
        if (job.used) (void) hipStreamSynchronize(mel_stream_of(*ctx->state));   // full() has waited for its results; an early error return may not have
        if (r == 0 && job.used && job.spk_slot >= 0) speaker_commit(*ctx, 1, params.token_timestamps);
        return r;
    } catch (...) { WMI_ERR("%s: out of memory\n", __func__); return -103; }
}

int wmi_full_long_wav(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wav, int converter,
                      const struct wmi_long_params * long_params) {
    if (!ctx || !ctx->state) return -101;
    try {
        { Scope lk(ctx); DraftRefuse no_draft(ctx->state.get()); }         // (no draft is carried: dropped whatever the call returns)
        WavJob job; job.wav = wav; job.converter = converter;
        job.plan = wav_plan(wav, converter, __func__, ctx->wav_adpcm_mode);
        if (job.plan.err) return -100 + job.plan.err;
        Scope lk(ctx);                                                     // wmi_full_long's locks
        if (!compute_ready(*ctx, __func__)) return -102;
        if (!HIP_OK(hipSetDevice(ctx->device))) return -102;
        WavWork * w = work(*ctx);
        const size_t n = (size_t) job.plan.n_out;
        if (!w || !reserve_jobs(*w, &job, 1) || !reserve(w->d_pcm, w->pcm_cap, std::max<size_t>(n, 1), 4096) || !reserve_speaker(*ctx, &job, 1)) return -103;
        hipStream_t s = mel_stream_of(*ctx->state);
        bool ok = wav_job_run(*ctx, job, w->d_pcm, s);
        ok = HIP_OK(hipStreamSynchronize(s)) && ok;                        // wmi_full_long takes device samples as ready, on whichever stream it reads them
        if (!ok) return -103;
        const int r = wmi_full_long(ctx, params, w->d_pcm, (int) n, 1, long_params);
        if (r == 0 && job.spk_slot >= 0) speaker_commit(*ctx, 3, params.token_timestamps);
        return r;
    } catch (...) { WMI_ERR("%s: out of memory\n", __func__); return -103; }
}

int wmi_full_batch_wav(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wavs, int n, int converter) {
    if (!ctx || !ctx->state) return -101;
    try {
        { Scope lk(ctx); DraftRefuse no_draft(ctx->state.get()); }         // (no draft is carried: dropped whatever the call returns)
        if (!wavs || n < 0) return -101;
        std::vector<WavJob> jobs((size_t) n);
        std::vector<size_t> off((size_t) n);
        size_t total = 0;
        for (int i = 0; i < n; ++i) {
            jobs[i].wav = wavs + i; jobs[i].converter = converter;
            jobs[i].plan = wav_plan(wavs + i, converter, __func__, ctx->wav_adpcm_mode);
            if (jobs[i].plan.err) return -100 + jobs[i].plan.err;
            jobs[i].mark_begin = i == 0; jobs[i].mark_end = i == n - 1;
            off[i] = total; total += ((size_t) jobs[i].plan.n_out + 63) & ~(size_t) 63;
        }
        Scope lk(ctx);                                                     // wmi_full_batch's locks
        if (!compute_ready(*ctx, __func__)) return -102;
        if (!HIP_OK(hipSetDevice(ctx->device))) return -102;
        WavWork * w = work(*ctx);
        if (!w || !reserve_jobs(*w, jobs.data(), n) || !reserve(w->d_pcm, w->pcm_cap, std::max<size_t>(total, 1), 4096) ||
            !reserve_speaker(*ctx, jobs.data(), n)) return -103;
        hipStream_t s = mel_stream_of(*ctx->state);
        bool ok = true;
        for (int i = 0; i < n && ok; ++i) ok = wav_job_run(*ctx, jobs[i], w->d_pcm + off[i], s);      // every conversion is queued ...
        ok = HIP_OK(hipStreamSynchronize(s)) && ok;                                                  // ... before the one wait
        if (!ok) return -103;
        std::vector<const float *> pcm((size_t) n); std::vector<int> ns((size_t) n);
        for (int i = 0; i < n; ++i) { pcm[i] = w->d_pcm + off[i]; ns[i] = (int) jobs[i].plan.n_out; }
        const int r = wmi_full_batch(ctx, params, pcm.data(), ns.data(), n, 1);
        if (r == 0) speaker_commit(*ctx, 2, params.token_timestamps);
        return r;
    } catch (...) { WMI_ERR("%s: out of memory\n", __func__); return -103; }
}

int wmi_wav_to_pcm_channels(struct whisper_context * ctx, const struct wmi_wav * wav, int converter, float * dst0, float * dst1, int dst_capacity,
                            int dst_on_device) {
    if (!ctx || !ctx->state) return -1;
    try {
        WavJob job; job.wav = wav; job.converter = converter;
        job.plan = channels_plan(wav, converter, __func__, ctx->wav_adpcm_mode);
        if (job.plan.err) return job.plan.err;
        if (!dst0 || !dst1 || dst_capacity < 0) return -1;
        if (job.plan.n_out > dst_capacity) return -4;
        Scope lk(ctx);
        if (!compute_ready(*ctx, __func__)) return -2;
        if (!HIP_OK(hipSetDevice(ctx->device))) return -2;
        WavWork * w = work(*ctx);
        if (!w) return -3;
        hipStream_t s = mel_stream_of(*ctx->state);
        const size_t n = (size_t) job.plan.n_out, off1 = (n + 63) & ~(size_t) 63;
        if (!reserve_jobs(*w, &job, 1) || (!dst_on_device && !reserve(w->d_out, w->out_cap, off1 + n, 1024))) return -3;
        float * d0 = dst_on_device ? dst0 : w->d_out, * d1 = dst_on_device ? dst1 : w->d_out + off1;
        bool ok = wav_job_run(*ctx, job, d0, s, d1);                       // the ONE launch writes both
        if (ok && !dst_on_device && n > 0)
            ok = HIP_OK(hipMemcpyAsync(dst0, d0, n * 4, hipMemcpyDeviceToHost, s)) && HIP_OK(hipMemcpyAsync(dst1, d1, n * 4, hipMemcpyDeviceToHost, s));
        ok = HIP_OK(hipStreamSynchronize(s)) && ok;
        return ok ? (int) n : -3;
    } catch (...) { WMI_ERR("%s: out of memory\n", __func__); return -3; }
}

int wmi_full_wav_channels(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wav, int converter) {
    if (!ctx || !ctx->state) return -101;
    try {
        { Scope lk(ctx); DraftRefuse no_draft(ctx->state.get()); }         // (no draft is carried: dropped whatever the call returns)
        WavJob job; job.wav = wav; job.converter = converter;
        job.plan = channels_plan(wav, converter, __func__, ctx->wav_adpcm_mode);
        if (job.plan.err) return -100 + job.plan.err;
        Scope lk(ctx);                                                     // wmi_full_batch's locks
        if (!compute_ready(*ctx, __func__)) return -102;
        if (!HIP_OK(hipSetDevice(ctx->device))) return -102;
        WavWork * w = work(*ctx);
        const size_t n = (size_t) job.plan.n_out, off1 = (n + 63) & ~(size_t) 63;      // the slices as wmi_full_batch_wav places its clips
        if (!w || !reserve_jobs(*w, &job, 1) || !reserve(w->d_pcm, w->pcm_cap, std::max<size_t>(2 * off1, 1), 4096)) return -103;
        hipStream_t s = mel_stream_of(*ctx->state);
        bool ok = wav_job_run(*ctx, job, w->d_pcm, s, w->d_pcm + off1);    // one upload, one launch, both channels ...
        ok = HIP_OK(hipStreamSynchronize(s)) && ok;                        // ... one wait
        if (!ok) return -103;
        const float * pcm[2] = { w->d_pcm, w->d_pcm + off1 }; const int ns[2] = { (int) n, (int) n };
        const int r = wmi_full_batch(ctx, params, pcm, ns, 2, 1);          // (a speaker mode is not served: the result carries no table)
        if (r == 0 && ctx->batch && ctx->batch->results.size() == 2) build_dialogue(*ctx);
        return r;
    } catch (...) { WMI_ERR("%s: out of memory\n", __func__); return -103; }
}

int wmi_channels_select(struct whisper_context * ctx, int channel) {
    if (!ctx) return -1;
    Scope lk(ctx);
    if (!ctx->state || !ctx->wav || !ctx->wav->ch.valid || !ctx->batch || ctx->batch->results.size() != 2 || channel < -1 || channel > 1) return -1;
    if (channel >= 0) return wmi_batch_select(ctx, channel);
    select_dialogue(*ctx);
    return (int) ctx->state->result_all.size();
}

int wmi_channels_get_segment(struct whisper_context * ctx, int i, struct wmi_channel_segment * out) {
    if (!ctx || !out) return -1;
    Scope lk(ctx);
    const WavWork * w = ctx->wav;
    if (!w || !w->ch.valid || !w->ch.shown || i < 0 || i >= (int) w->ch.from.size()) return -1;
    *out = w->ch.from[(size_t) i];
    return 0;
}

int wmi_selftest_channels_merge(const int64_t * t0_a, int n_a, const int64_t * t0_b, int n_b, int * out_channel, int * out_index) {
    if (n_a < 0 || n_b < 0 || (n_a > 0 && !t0_a) || (n_b > 0 && !t0_b) || (n_a + (long long) n_b > 0 && (!out_channel || !out_index))) return -1;
    return chm::merge(t0_a, n_a, t0_b, n_b, out_channel, out_index);
}

int wmi_wav_stats(struct whisper_context * ctx, int64_t * out5) {
    if (!ctx || !out5) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    memset(out5, 0, 5 * sizeof(int64_t));
    WavWork * w = ctx->wav;
    if (!w) return 0;
    if (w->ev_pending) {
        w->ev_pending = false;
        float ms = 0.0f;
        if (HIP_OK(hipSetDevice(ctx->device)) && hipEventSynchronize(w->ev[1]) == hipSuccess && hipEventElapsedTime(&ms, w->ev[0], w->ev[1]) == hipSuccess)
            w->stats[4] = (int64_t) (ms * 1e3);
    }
    memcpy(out5, w->stats, sizeof(w->stats));
    return 0;
}

}  // extern "C"

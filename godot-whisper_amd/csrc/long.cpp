// wmi_full_long: a long recording cut at its silences and decoded in lock-step (include/wmi_device.h has the contract).
//   front     the frame energies on the device (k::frame_energy) over the ONE PCM buffer, back in one copy behind one wait; the plan on the
//             host (segment.cpp)
//   decoding  wmi_full_batch / wmi_full_batch_ctx on device pointers into that buffer — the very calls a caller would make on the plan's slices
//   result    the pieces' segments in order, times shifted by each piece's first frame (as whisper_full_parallel shifts its pieces',
//             W/whisper.cpp:5893-5913, minus the clamp: these pieces are disjoint)
// Nothing here launches a decode kernel of its own.

#include "wmi.h"
#include "kernels.h"

#include <algorithm>
#include <cstring>

namespace wmi {

void free_long(BatchWork & w) {
    BatchWork::Long & l = w.lng;
    if (l.pcm) (void) hipFree(l.pcm);
    if (l.e) (void) hipFree(l.e);
    if (l.e_host) (void) hipHostFree(l.e_host);
    l.pcm = l.e = l.e_host = nullptr; l.pcm_cap = l.e_cap = 0;
}

namespace {

struct CtxLock {                                              // the context's lock, then its own state's (api.cpp: CtxScope)
    std::unique_lock<std::recursive_mutex> lk, lks;
    explicit CtxLock(whisper_context * c) : lk(c->mu) { if (State * st = c->state.own) lks = std::unique_lock<std::recursive_mutex>(st->mu); }
};

bool ensure_energy(BatchWork::Long & l, size_t F) {
    if (l.e_cap >= F) return true;
    if (l.e) (void) hipFree(l.e);
    if (l.e_host) (void) hipHostFree(l.e_host);
    l.e = l.e_host = nullptr; l.e_cap = 0;
    const size_t cap = F + F / 4 + 64;
    if (!HIP_OK(hipMalloc((void **) &l.e, cap * sizeof(float))) || !HIP_OK(hipHostMalloc((void **) &l.e_host, cap * sizeof(float), hipHostMallocDefault))) return false;
    l.e_cap = cap;
    return true;
}

void select_merged(whisper_context & ctx) {
    const BatchWork::Long & l = ctx.batch->lng;
    ctx.state->result_all = l.merged;
    ctx.state->windows = l.windows;
    if (l.lang_id >= 0) ctx.state->lang_id = l.lang_id;
    speaker_select(ctx, -1);
    channels_deselect(ctx);
}

int full_long(whisper_context * ctx, whisper_full_params params, const float * pcm, int n, bool on_device, const wmi_long_params & lp) {
    if (!ctx->batch) ctx->batch = new BatchWork();
    BatchWork::Long & l = ctx->batch->lng;
    l.valid = false; l.pieces.clear(); l.merged.clear(); l.windows.clear(); l.lang_id = -1;
    l.t_us[0] = l.t_us[1] = l.t_us[2] = 0; l.n_frames = 0;
    hipStream_t s = ctx->state->dev.stream;
    const int F = (n + 159) / 160;
    // ---- the one PCM buffer
    int64_t t0 = time_us();
    const float * d_pcm = pcm;
    if (!on_device) {
        if (l.pcm_cap < (size_t) n) {
            if (l.pcm) { (void) hipStreamSynchronize(s); (void) hipFree(l.pcm); }
            l.pcm = nullptr; l.pcm_cap = 0;
            if (!HIP_OK(hipMalloc((void **) &l.pcm, (size_t) n * sizeof(float)))) return -2;
            l.pcm_cap = (size_t) n;
        }
        if (!HIP_OK(hipMemcpyAsync(l.pcm, pcm, (size_t) n * sizeof(float), hipMemcpyHostToDevice, s))) return -2;
        d_pcm = l.pcm;
    }
    l.t_us[0] = time_us() - t0;
    // ---- energies: one launch, one copy, one wait
    t0 = time_us();
    if (!ensure_energy(l, (size_t) F)) return -2;
    if (!k::frame_energy(d_pcm, n, l.e, s)) return -2;
    if (!HIP_OK(hipMemcpyAsync(l.e_host, l.e, (size_t) F * sizeof(float), hipMemcpyDeviceToHost, s)) || !HIP_OK(hipStreamSynchronize(s)) ||
        !HIP_OK(hipGetLastError())) return -2;
    l.t_us[1] = time_us() - t0; l.n_frames = F;
    // ---- the plan, on the frames offset_ms / duration_ms leave
    t0 = time_us();
    int f0 = 0, f1 = 0, n_sub = 0;
    if (long_window(n, params.offset_ms, params.duration_ms, &f0, &f1, &n_sub) != 0) return -1;
    std::vector<wmi_long_piece> pieces;
    if (f1 > f0 && long_plan(l.e_host + f0, f1 - f0, n_sub, lp, ctx->model.hp.n_audio_ctx, pieces) < 0) return -1;
    for (auto & pc : pieces) { pc.frame0 += f0; pc.frame1 += f0; if (!lp.fit_audio_ctx) pc.audio_ctx = params.audio_ctx; }
    l.t_us[2] = time_us() - t0;
    const int np = (int) pieces.size();
    State & st = *ctx->state;
    if (np == 0) {                                            // no island: nothing is decoded
        ctx->batch->results.clear(); ctx->batch->windows.clear(); ctx->batch->redo.clear();
        ctx->batch->lang_id.clear(); ctx->batch->lang_detected.clear(); ctx->batch->lang_probs.clear();
        st.result_all.clear(); st.windows.clear();
        l.valid = true;
        return 0;
    }
    // ---- the pieces in lock-step: device pointers into the one buffer
    std::vector<const float *> ptrs(np); std::vector<int> ns(np), actx(np);
    for (int i = 0; i < np; ++i) {
        ptrs[i] = d_pcm + (size_t) 160 * pieces[i].frame0;
        ns[i] = std::min(160 * pieces[i].frame1, n) - 160 * pieces[i].frame0;
        actx[i] = pieces[i].audio_ctx;
    }
    params.offset_ms = 0; params.duration_ms = 0;
    const int rc = lp.fit_audio_ctx ? wmi_full_batch_ctx(ctx, params, ptrs.data(), ns.data(), actx.data(), np, 1)
                                    : wmi_full_batch(ctx, params, ptrs.data(), ns.data(), np, 1);
    if (rc != 0) return rc;
    // ---- the merged result
    BatchWork & bw = *ctx->batch;
    for (int i = 0; i < np; ++i) {
        const int64_t shift = pieces[i].frame0;
        pieces[i].mode = i < (int) bw.redo.size() ? bw.redo[i] : -1;
        pieces[i].i_segment = (int32_t) l.merged.size();
        pieces[i].n_segments = (int32_t) bw.results[i].size();
        if (i < (int) bw.windows.size()) for (WindowRec wr : bw.windows[i]) {
            wr.seek += (int32_t) shift; wr.seg0 += pieces[i].i_segment;
            l.windows.push_back(wr);
        }
        for (Segment seg : bw.results[i]) {
            seg.t0 += shift; seg.t1 += shift;
            for (auto & tk : seg.tokens) { if (tk.t0 >= 0) tk.t0 += shift; if (tk.t1 >= 0) tk.t1 += shift; }
            for (auto & t : seg.t_dtw) if (t >= 0) t += shift;
            l.merged.push_back(std::move(seg));
        }
    }
    l.lang_id = !bw.lang_id.empty() ? bw.lang_id[0] : -1;
    l.pieces = std::move(pieces);
    l.valid = true;
    select_merged(*ctx);
    return 0;
}

} // namespace

} // namespace wmi

using namespace wmi;

extern "C" {

struct wmi_long_params wmi_long_default_params(void) { return long_default_params(); }

int wmi_full_long(struct whisper_context * ctx, struct whisper_full_params params, const float * pcm, int n_samples, int pcm_on_device,
                  const struct wmi_long_params * long_params) {
    if (!ctx || !ctx->state) return -1;
    CtxLock lk(ctx);
    DraftRefuse no_draft(ctx->state.get());                 // (pieces in lock-step: no draft is carried; dropped whatever the call returns)
    if (!pcm || n_samples < 0) return -1;
    const wmi_long_params lp = long_params ? *long_params : long_default_params();
    if (!long_params_ok(lp) || params.offset_ms < 0 || params.duration_ms < 0) return -1;
    if (params.new_segment_callback || params.progress_callback || params.encoder_begin_callback || params.logits_filter_callback) {
        WMI_ERR("%s: callbacks are not served (their times and indices would be relative to a piece)\n", __func__);
        return -1;
    }
    if (n_samples == 0) { WMI_ERR("%s: no signal data available\n", __func__); return -3; }
    if (!compute_ready(*ctx, __func__)) return -2;
    try {
        (void) hipSetDevice(ctx->device);
        return full_long(ctx, params, pcm, n_samples, pcm_on_device != 0, lp);
    } catch (const std::exception & e) {
        WMI_ERR("%s: %s\n", __func__, e.what());
        return -10;
    }
}

int wmi_long_n_pieces(struct whisper_context * ctx) {
    if (!ctx) return -1;
    CtxLock lk(ctx);
    return ctx->batch && ctx->batch->lng.valid ? (int) ctx->batch->lng.pieces.size() : 0;
}

int wmi_long_get_piece(struct whisper_context * ctx, int i, struct wmi_long_piece * out) {
    if (!ctx || !out) return -1;
    CtxLock lk(ctx);
    if (!ctx->batch || !ctx->batch->lng.valid || i < 0 || i >= (int) ctx->batch->lng.pieces.size()) return -1;
    *out = ctx->batch->lng.pieces[i];
    return 0;
}

int wmi_long_select(struct whisper_context * ctx, int piece) {
    if (!ctx) return -1;
    CtxLock lk(ctx);
    if (!ctx->state || !ctx->batch || !ctx->batch->lng.valid || piece < -1 || piece >= (int) ctx->batch->lng.pieces.size()) return -1;
    if (piece >= 0) return ctx->batch->results.size() == ctx->batch->lng.pieces.size() ? wmi_batch_select(ctx, piece) : -1;
    select_merged(*ctx);
    return (int) ctx->state->result_all.size();
}

void wmi_get_long_timings(struct whisper_context * ctx, int64_t * us3, int32_t * n2) {
    if (us3) us3[0] = us3[1] = us3[2] = 0;
    if (n2) n2[0] = n2[1] = 0;
    if (!ctx) return;
    CtxLock lk(ctx);
    if (!ctx->batch) return;
    const BatchWork::Long & l = ctx->batch->lng;
    if (us3) { us3[0] = l.t_us[0]; us3[1] = l.t_us[1]; us3[2] = l.t_us[2]; }
    if (n2) { n2[0] = l.n_frames; n2[1] = (int32_t) l.pieces.size(); }
}

int wmi_long_stage_samples(void) { return k::SEG_FRAME * k::SEG_STAGE_FRAMES; }

int wmi_selftest_frame_energy(int device, const float * x, int n, float * e_out) {
    if (!x || !e_out || n < 1 || device < -1) return -1;
    if (device < 0) { frame_energy_host(x, n, e_out); return 0; }
    if (!HIP_OK(hipSetDevice(device))) return -2;
    const size_t F = ((size_t) n + 159) / 160;
    float * d_x = nullptr, * d_e = nullptr; hipStream_t st = nullptr;
    struct Free { float *& a; float *& b; hipStream_t & s; ~Free() { if (s) (void) hipStreamDestroy(s); if (a) (void) hipFree(a); if (b) (void) hipFree(b); } } fr{d_x, d_e, st};
    // the caller's e_out [F + 64] goes to the device as it is (its sentinel), the launch writes F words, all F + 64 come back
    const size_t Fg = F + 64;
    if (!HIP_OK(hipMalloc((void **) &d_x, (size_t) n * 4)) || !HIP_OK(hipMalloc((void **) &d_e, Fg * 4)) || !HIP_OK(hipStreamCreate(&st))) return -3;
    if (!HIP_OK(hipMemcpyAsync(d_x, x, (size_t) n * 4, hipMemcpyHostToDevice, st)) ||
        !HIP_OK(hipMemcpyAsync(d_e, e_out, Fg * 4, hipMemcpyHostToDevice, st))) return -3;
    if (!k::frame_energy(d_x, n, d_e, st)) return -3;
    if (!HIP_OK(hipMemcpyAsync(e_out, d_e, Fg * 4, hipMemcpyDeviceToHost, st)) || !HIP_OK(hipStreamSynchronize(st)) || !HIP_OK(hipGetLastError())) return -3;
    return 0;
}

int wmi_selftest_long_window(int n_samples, int offset_ms, int duration_ms, int * f0, int * f1, int * n_sub) {
    return long_window(n_samples, offset_ms, duration_ms, f0, f1, n_sub);
}

int wmi_selftest_long_plan(const float * e, int F, int n_samples, const struct wmi_long_params * long_params, int n_audio_ctx,
                           struct wmi_long_piece * out, int cap) {
    if (cap < 0 || (cap > 0 && !out)) return -1;
    try {
        std::vector<wmi_long_piece> pieces;
        const int np = long_plan(e, F, n_samples, long_params ? *long_params : long_default_params(), n_audio_ctx, pieces);
        for (int i = 0; i < np && i < cap; ++i) out[i] = pieces[i];
        return np;
    } catch (const std::exception &) { return -1; }
}

} // extern "C"

// The rest of the whisper.h surface (W/whisper.h v1.5.4): caller-owned states (whisper_init_state and the
// *_with_state / *_from_state families), the deprecated and *_no_state constructors, the loader-callback
// constructors, whisper_full_parallel, the by-reference parameter helpers and the bench entry points.
//
// A whisper_state is this backend's wmi::State: its own KV caches, encoder/decoder activation arenas, HIP stream and
// captured decode graph on the context's GPU — the same ownership split as the reference (W/whisper.cpp:3001-3120:
// weights belong to the context, everything mutable to the state).  The compute code reaches its working set through
// ctx.state, which resolves per THREAD: a *_with_state call installs the caller's state for the calling thread and holds
// that state's lock.  Calls on one state serialise; calls on different states of one context run concurrently, each on its
// state's own stream (round 6; before, they took turns on the context's lock).

#include "wmi.h"
#include "kernels.h"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <thread>

using namespace wmi;

namespace {

inline State * S(struct whisper_state * s) { return reinterpret_cast<State *>(s); }

// A *_with_state call: the caller's state is what ctx.state means on THIS thread for the duration of the call (wmi.h: StateSlot), under
// the STATE's lock — calls on one state serialise, calls on different states of one context run side by side (W/whisper.cpp:5837-5858).
struct StateScope {
    std::unique_lock<std::recursive_mutex> lk; StateInstall inst; BusyScope busy;      // (counted once the lock is held: a waiting caller is not on the GPU)
    StateScope(whisper_context * c, struct whisper_state * s) : lk(S(s)->mu), inst(c->state, S(s)), busy(c->device) {
        if (!c->host_only) (void) hipSetDevice(c->device);
    }
};

bool read_file(const char * path, std::vector<char> & buf) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { WMI_ERR("%s: failed to open '%s'\n", __func__, path); return false; }
    const std::streamsize n = f.tellg();
    f.seekg(0);
    buf.resize((size_t) n);
    if (!f.read(buf.data(), n)) { WMI_ERR("%s: failed to read '%s'\n", __func__, path); return false; }
    return true;
}

// drain a whisper_model_loader (W/whisper.h:108-114) into memory; the loader is closed in every case, as the
// reference does (W/whisper.cpp:3253-3269)
bool read_loader(struct whisper_model_loader * loader, std::vector<char> & buf) {
    if (!loader || !loader->read) return false;
    const size_t step = 8u << 20;
    size_t have = 0;
    for (;;) {
        buf.resize(have + step);
        const size_t got = loader->read(loader->context, buf.data() + have, step);
        have += got;
        if (got < step || (loader->eof && loader->eof(loader->context))) break;
    }
    buf.resize(have);
    if (loader->close) loader->close(loader->context);
    return have > 0;
}

} // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------- constructors
struct whisper_context * whisper_init_from_buffer_with_params_no_state(void * buffer, size_t buffer_size, struct whisper_context_params params) {
    whisper_context * ctx = init_context(buffer, buffer_size, 0, false);
    if (ctx) ctx->params = params;
    return ctx;
}
struct whisper_context * whisper_init_from_file_with_params_no_state(const char * path, struct whisper_context_params params) {
    WMI_INFO("%s: loading model from '%s'\n", __func__, path);
    std::vector<char> buf;
    if (!read_file(path, buf)) return nullptr;
    return whisper_init_from_buffer_with_params_no_state(buf.data(), buf.size(), params);
}
struct whisper_context * whisper_init_with_params_no_state(struct whisper_model_loader * loader, struct whisper_context_params params) {
    std::vector<char> buf;
    if (!read_loader(loader, buf)) { WMI_ERR("%s: failed to load model\n", __func__); return nullptr; }
    return whisper_init_from_buffer_with_params_no_state(buf.data(), buf.size(), params);
}
struct whisper_context * whisper_init_with_params(struct whisper_model_loader * loader, struct whisper_context_params params) {
    std::vector<char> buf;
    if (!read_loader(loader, buf)) { WMI_ERR("%s: failed to load model\n", __func__); return nullptr; }
    return whisper_init_from_buffer_with_params(buf.data(), buf.size(), params);
}
// deprecated forms: default context parameters (W/whisper.cpp:3316-3338)
struct whisper_context * whisper_init_from_file(const char * path) { return whisper_init_from_file_with_params(path, whisper_context_default_params()); }
struct whisper_context * whisper_init_from_buffer(void * buffer, size_t n) { return whisper_init_from_buffer_with_params(buffer, n, whisper_context_default_params()); }
struct whisper_context * whisper_init(struct whisper_model_loader * loader) { return whisper_init_with_params(loader, whisper_context_default_params()); }
struct whisper_context * whisper_init_from_file_no_state(const char * path) { return whisper_init_from_file_with_params_no_state(path, whisper_context_default_params()); }
struct whisper_context * whisper_init_from_buffer_no_state(void * buffer, size_t n) { return whisper_init_from_buffer_with_params_no_state(buffer, n, whisper_context_default_params()); }
struct whisper_context * whisper_init_no_state(struct whisper_model_loader * loader) { return whisper_init_with_params_no_state(loader, whisper_context_default_params()); }

struct whisper_state * whisper_init_state(struct whisper_context * ctx) {
    if (!ctx) return nullptr;
    if (ctx->host_only) { WMI_ERR("%s: host-only context has no compute path (this backend has no CPU fallback)\n", __func__); return nullptr; }
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    State * st = create_state(*ctx);
    if (!st) WMI_ERR("%s: failed to allocate the state on device %d\n", __func__, ctx->device);
    return reinterpret_cast<struct whisper_state *>(st);
}
void whisper_free_state(struct whisper_state * state) { destroy_state(S(state)); }        // NULL-safe, W/whisper.cpp:3340-3368

// not built with OpenVINO: the reference's answer in that configuration (W/whisper.cpp:3122-3134)
int whisper_ctx_init_openvino_encoder(struct whisper_context *, const char *, const char *, const char *) { return 1; }

struct whisper_context_params * whisper_context_default_params_by_ref(void) { return new whisper_context_params(whisper_context_default_params()); }
struct whisper_full_params * whisper_full_default_params_by_ref(enum whisper_sampling_strategy strategy) { return new whisper_full_params(whisper_full_default_params(strategy)); }
void whisper_free_context_params(struct whisper_context_params * params) { delete params; }
void whisper_free_params(struct whisper_full_params * params) { delete params; }

// ---------------------------------------------------------------------------------------------- compute on a caller-owned state
int whisper_pcm_to_mel_with_state(struct whisper_context * ctx, struct whisper_state * state, const float * samples, int n_samples, int) {
    if (!ctx || !state) return -1;
    StateScope sc(ctx, state);
    if (!pcm_to_mel(*ctx, samples, n_samples, false)) { WMI_ERR("%s: failed to compute mel spectrogram\n", __func__); return -1; }
    return 0;
}
// The reference's x2 phase-vocoder variant calls the mel routine with an 800-sample frame, whose 401 bins index the
// 201-bin filterbank out of bounds (W/whisper.cpp:3417-3425 -> :2764-2776) and which whisper_full itself refuses
// (:4973-4976).  There is no defined result to reproduce: fail the way whisper_full does.
int whisper_pcm_to_mel_phase_vocoder_with_state(struct whisper_context *, struct whisper_state *, const float *, int, int) {
    WMI_ERR("%s: failed to compute mel spectrogram (the x2 phase-vocoder front end is not supported)\n", __func__);
    return -1;
}
int whisper_pcm_to_mel_phase_vocoder(struct whisper_context * ctx, const float * samples, int n_samples, int n_threads) {
    return whisper_pcm_to_mel_phase_vocoder_with_state(ctx, ctx ? reinterpret_cast<struct whisper_state *>(ctx->state.get()) : nullptr, samples, n_samples, n_threads);
}
int whisper_set_mel_with_state(struct whisper_context * ctx, struct whisper_state * state, const float * data, int n_len, int n_mel) {
    if (!ctx || !state) return -1;
    if (n_mel != ctx->model.n_filt_mel) { WMI_ERR("%s: invalid number of mel bands: %d (expected %d)\n", __func__, n_mel, ctx->model.n_filt_mel); return -1; }
    StateScope sc(ctx, state);
    return set_mel(*ctx, data, n_len, n_mel) ? 0 : -1;
}
int whisper_encode_with_state(struct whisper_context * ctx, struct whisper_state * state, int offset, int) {
    if (!ctx || !state) return -1;
    StateScope sc(ctx, state);
    if (!encode(*ctx, offset)) { WMI_ERR("%s: failed to eval\n", __func__); return -1; }
    return 0;
}
int whisper_decode_with_state(struct whisper_context * ctx, struct whisper_state * state, const whisper_token * tokens, int n_tokens, int n_past, int) {
    if (!ctx || !state) { WMI_ERR("%s: ERROR state was not loaded.\n", __func__); return -1; }
    StateScope sc(ctx, state);
    State & st = *ctx->state;
    st.batch.prep_legacy(tokens, n_tokens, n_past, 0);
    kv_seq_rm(st.kv_self, 0, n_past, -1);
    if (!decode(*ctx, st.batch)) { WMI_ERR("%s: failed to eval\n", __func__); return 1; }
    return 0;
}
int whisper_lang_auto_detect_with_state(struct whisper_context * ctx, struct whisper_state * state, int offset_ms, int, float * lang_probs) {
    if (!ctx || !state) return -1;
    StateScope sc(ctx, state);
    return lang_auto_detect(*ctx, offset_ms, lang_probs);
}
int wmi_lang_detect(struct whisper_context * ctx, int offset_ms, float * lang_probs) {      // the same detection through the language head (wmi_device.h)
    if (!ctx || !ctx->state) return -1;
    StateScope sc(ctx, reinterpret_cast<struct whisper_state *>(ctx->state.get()));
    if (!k::lang_head_usable(ctx->model.hp.n_text_state)) return lang_auto_detect(*ctx, offset_ms, lang_probs);
    return lang_detect_head(*ctx, offset_ms, lang_probs);
}
int whisper_full_with_state(struct whisper_context * ctx, struct whisper_state * state, struct whisper_full_params params, const float * samples, int n_samples) {
    if (!ctx || !state) return -1;
    StateScope sc(ctx, state);
    return full(*ctx, params, samples, nullptr, n_samples);
}

// W/whisper.cpp:5817-5924.  The split, the per-piece parameters, the time offsets, the no-overlap clamp, the callback
// replay, the timing bookkeeping AND the threads are the reference's: pieces 1.. run on host threads of their own, each on
// its own state (own stream), piece 0 on the caller's thread.
int whisper_full_parallel(struct whisper_context * ctx, struct whisper_full_params params, const float * samples, int n_samples, int n_processors) {
    if (!ctx || !ctx->state || n_processors < 1) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    DraftRefuse no_draft(ctx->state.get());     // (pieces on states of their own: a draft of the whole does not fit one of them)
    if (n_processors == 1) return whisper_full(ctx, params, samples, n_samples);
    const int offset_samples = (WHISPER_SAMPLE_RATE * params.offset_ms) / 1000;
    const int per = (n_samples - offset_samples) / n_processors;
    // nothing to split (the reference would hand negative sample counts to its workers here): one plain call
    if (per <= 0) return whisper_full(ctx, params, samples, n_samples);

    std::vector<struct whisper_state *> states;
    for (int i = 0; i < n_processors - 1; ++i) {
        struct whisper_state * st = whisper_init_state(ctx);
        if (!st) { for (auto * s : states) whisper_free_state(s); return -1; }
        states.push_back(st);
    }
    // the pieces 1.. on threads of their own, piece 0 on this one (W/whisper.cpp:5837-5858): every piece computes on its own state, under that
    // state's lock, on that state's stream (round 6; before, the pieces took turns)
    int ret;
    {
        std::vector<std::thread> workers;
        struct Joiner { std::vector<std::thread> & t; ~Joiner() { for (auto & x : t) if (x.joinable()) x.join(); } } joiner{workers};
        for (int i = 0; i < n_processors - 1; ++i) {
            const int start = offset_samples + (i + 1) * per;
            const int n_cur = (i == n_processors - 2) ? n_samples - start : per;
            auto cur = params;
            cur.offset_ms = 0;
            cur.print_progress = false; cur.print_realtime = false;
            cur.new_segment_callback = nullptr; cur.new_segment_callback_user_data = nullptr;
            cur.progress_callback = nullptr;    cur.progress_callback_user_data = nullptr;
            struct whisper_state * st = states[i];
            auto piece = [ctx, st, cur, samples, start, n_cur]() { (void) whisper_full_with_state(ctx, st, cur, samples + start, n_cur); };   // the reference drops the workers' return codes too
            workers.emplace_back(piece);
        }
        auto cur = params;
        cur.print_realtime = false;
        ret = whisper_full_with_state(ctx, reinterpret_cast<struct whisper_state *>(ctx->state.get()), cur, samples, offset_samples + per);
    }

    const int64_t offset_t = (int64_t) (params.offset_ms / 10.0);
    State & main = *ctx->state;
    for (int i = 0; i < n_processors - 1; ++i) {
        State & si = *S(states[i]);
        // (no-speech modes: the piece's windows follow the main state's, seek and first segment shifted to the whole signal)
        for (WindowRec wr : si.windows) {
            wr.seek += (int32_t) (100 * (int64_t) ((i + 1) * per) / WHISPER_SAMPLE_RATE + offset_t);
            wr.seg0 += (int32_t) main.result_all.size();
            main.windows.push_back(wr);
        }
        for (auto & seg : si.result_all) {
            const int64_t shift = 100 * (int64_t) ((i + 1) * per) / WHISPER_SAMPLE_RATE + offset_t;
            seg.t0 += shift; seg.t1 += shift;
            if (!main.result_all.empty()) seg.t0 = std::max(seg.t0, main.result_all.back().t1);
            main.result_all.push_back(std::move(seg));
            if (params.new_segment_callback)
                params.new_segment_callback(ctx, reinterpret_cast<struct whisper_state *>(ctx->state.get()), 1, params.new_segment_callback_user_data);
        }
        main.t_mel_us += si.t_mel_us; main.t_sample_us += si.t_sample_us; main.t_encode_us += si.t_encode_us;
        main.t_decode_us += si.t_decode_us; main.t_batchd_us += si.t_batchd_us; main.t_prompt_us += si.t_prompt_us;
        main.n_sample += si.n_sample; main.n_encode += si.n_encode; main.n_decode += si.n_decode;
        main.n_batchd += si.n_batchd; main.n_prompt += si.n_prompt;
        whisper_free_state(states[i]);
    }
    main.t_mel_us /= n_processors; main.t_sample_us /= n_processors; main.t_encode_us /= n_processors; main.t_decode_us /= n_processors;

    WMI_WARN("\n");
    WMI_WARN("%s: the audio has been split into %d chunks at the following times:\n", __func__, n_processors);
    for (int i = 0; i < n_processors - 1; ++i) {
        const int64_t t = 100 * (int64_t) ((i + 1) * per) / WHISPER_SAMPLE_RATE + offset_t;       // 10 ms units
        const int64_t msec = t * 10, hr = msec / 3600000, mn = (msec / 60000) % 60, sec = (msec / 1000) % 60;
        WMI_WARN("%s: split %d - %02d:%02d:%02d.%03d\n", __func__, i + 1, (int) hr, (int) mn, (int) sec, (int) (msec % 1000));
    }
    WMI_WARN("%s: the transcription quality may be degraded near these boundaries\n", __func__);
    return ret;
}

// ---------------------------------------------------------------------------------------------- results of a state
int whisper_n_len_from_state(struct whisper_state * state) { return S(state)->mel.n_len_org; }
float * whisper_get_logits_from_state(struct whisper_state * state) { return S(state)->logits.data(); }
int whisper_full_n_segments_from_state(struct whisper_state * state) { return (int) S(state)->result_all.size(); }
int whisper_full_lang_id_from_state(struct whisper_state * state) { return S(state)->lang_id; }
int64_t whisper_full_get_segment_t0_from_state(struct whisper_state * state, int i) { return S(state)->result_all[i].t0; }
int64_t whisper_full_get_segment_t1_from_state(struct whisper_state * state, int i) { return S(state)->result_all[i].t1; }
bool whisper_full_get_segment_speaker_turn_next_from_state(struct whisper_state * state, int i) { return S(state)->result_all[i].speaker_turn_next; }
bool whisper_full_get_segment_speaker_turn_next(struct whisper_context * ctx, int i) { return ctx->state->result_all[i].speaker_turn_next; }
const char * whisper_full_get_segment_text_from_state(struct whisper_state * state, int i) { return S(state)->result_all[i].text.c_str(); }
int whisper_full_n_tokens_from_state(struct whisper_state * state, int i) { return (int) S(state)->result_all[i].tokens.size(); }
const char * whisper_full_get_token_text_from_state(struct whisper_context * ctx, struct whisper_state * state, int i, int j) {
    return ctx->model.vocab.id_to_token[S(state)->result_all[i].tokens[j].id].c_str();
}
whisper_token whisper_full_get_token_id_from_state(struct whisper_state * state, int i, int j) { return S(state)->result_all[i].tokens[j].id; }
whisper_token_data whisper_full_get_token_data_from_state(struct whisper_state * state, int i, int j) { return S(state)->result_all[i].tokens[j]; }
float whisper_full_get_token_p_from_state(struct whisper_state * state, int i, int j) { return S(state)->result_all[i].tokens[j].p; }

// the windows of a call made with a no-speech mode (wmi_device.h)
int wmi_full_n_windows_from_state(struct whisper_state * state) { return state ? (int) S(state)->windows.size() : 0; }
int wmi_full_get_window_from_state(struct whisper_state * state, int i, struct wmi_window * out) {
    if (!state || !out || i < 0 || i >= (int) S(state)->windows.size()) return -1;
    const WindowRec & w = S(state)->windows[i];
    out->seek = w.seek; out->no_speech_prob = w.p; out->outcome = w.outcome; out->i_segment = w.seg0; out->n_segments = w.n_seg;
    return 0;
}
float wmi_full_get_segment_no_speech_prob_from_state(struct whisper_state * state, int i_segment) {
    if (!state || i_segment < 0) return -1.0f;
    for (const WindowRec & w : S(state)->windows) if (i_segment >= w.seg0 && i_segment < w.seg0 + w.n_seg) return w.p;
    return -1.0f;
}
int wmi_full_n_windows(struct whisper_context * ctx) { return ctx && ctx->state ? wmi_full_n_windows_from_state(reinterpret_cast<struct whisper_state *>(ctx->state.get())) : 0; }
int wmi_full_get_window(struct whisper_context * ctx, int i, struct wmi_window * out) {
    return ctx && ctx->state ? wmi_full_get_window_from_state(reinterpret_cast<struct whisper_state *>(ctx->state.get()), i, out) : -1;
}
float wmi_full_get_segment_no_speech_prob(struct whisper_context * ctx, int i_segment) {
    return ctx && ctx->state ? wmi_full_get_segment_no_speech_prob_from_state(reinterpret_cast<struct whisper_state *>(ctx->state.get()), i_segment) : -1.0f;
}
int wmi_set_no_speech(struct whisper_context * ctx, int mode) {
    if (!ctx) return -2;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const int prev = ctx->no_speech_mode;
    ctx->no_speech_mode = mode < 0 ? 0 : (mode > 3 ? 3 : mode);
    return prev;
}
// the grammar on the device (wmi_device.h)
int wmi_set_grammar_device(struct whisper_context * ctx, int mode) {
    if (!ctx) return -2;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const int prev = ctx->grammar_device_mode;
    ctx->grammar_device_mode = mode != 0 ? 1 : 0;
    return prev;
}
int wmi_grammar_status(struct whisper_context * ctx, struct wmi_grammar_status * out) {
    if (!ctx || !out) return -2;
    out->steps_device = ctx->state ? ctx->state->gram_steps_dev : 0;
    out->rows_host = ctx->state ? ctx->state->gram_rows_host : 0;
    out->reject_us = ctx->state ? ctx->state->gram_reject_us : 0.0f;
    out->cap_stacks = ge::MAX_STACKS; out->cap_depth = ge::MAX_DEPTH; out->cap_words = ge::WS_WORDS;
    return 0;
}
// token times by DTW (wmi_device.h)
int wmi_set_token_dtw(struct whisper_context * ctx, int mode, const int32_t * layer_head, int n_pairs) {
    if (!ctx) return -2;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const HParams & hp = ctx->model.hp;
    if (n_pairs < 0 || (n_pairs > 0 && !layer_head)) return -1;
    std::vector<std::pair<int32_t, int32_t>> pr;
    for (int i = 0; i < n_pairs; ++i) {
        const int32_t l = layer_head[2 * i], h = layer_head[2 * i + 1];
        if (l < 0 || l >= hp.n_text_layer || h < 0 || h >= hp.n_text_head) return -1;
        pr.emplace_back(l, h);
    }
    std::sort(pr.begin(), pr.end());
    for (size_t i = 1; i < pr.size(); ++i) if (pr[i] == pr[i - 1]) return -1;
    const int prev = ctx->token_dtw_mode;
    ctx->token_dtw_mode = mode != 0 ? 1 : 0;
    ctx->dtw_pairs.clear();
    for (const auto & q : pr) { ctx->dtw_pairs.push_back(q.first); ctx->dtw_pairs.push_back(q.second); }
    return prev;
}
int wmi_token_dtw_heads(struct whisper_context * ctx, int32_t * layer_head, int cap) {
    if (!ctx) return -2;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const std::vector<int32_t> pr = ctx->dtw_pairs.empty() ? dtw_default_pairs(ctx->model.hp) : ctx->dtw_pairs;
    const int n = (int) pr.size() / 2;
    for (int i = 0; layer_head && i < n && i < cap; ++i) { layer_head[2 * i] = pr[2 * i]; layer_head[2 * i + 1] = pr[2 * i + 1]; }
    return n;
}
int64_t wmi_full_get_token_dtw_from_state(struct whisper_state * state, int i_segment, int i_token) {
    if (!state || i_segment < 0 || i_segment >= (int) S(state)->result_all.size()) return -1;
    const Segment & seg = S(state)->result_all[i_segment];
    if (i_token < 0 || i_token >= (int) seg.t_dtw.size()) return -1;
    return seg.t_dtw[i_token];
}
int64_t wmi_full_get_token_dtw(struct whisper_context * ctx, int i_segment, int i_token) {
    return ctx && ctx->state ? wmi_full_get_token_dtw_from_state(reinterpret_cast<struct whisper_state *>(ctx->state.get()), i_segment, i_token) : -1;
}
int wmi_token_dtw_dims(struct whisper_context * ctx, int * n, int * n_sot, int * R, int * M, int * n_pairs) {
    if (!ctx || !ctx->state) return -1;
    const State::DtwDims & dd = ctx->state->dtw_last;
    if (dd.R < 1) return -1;
    if (n) *n = dd.n; if (n_sot) *n_sot = dd.n_sot; if (R) *R = dd.R; if (M) *M = dd.M; if (n_pairs) *n_pairs = dd.n_pairs;
    return 0;
}
void wmi_get_token_dtw_timings(struct whisper_context * ctx, int64_t * us, int32_t * n_windows) {
    const bool have = ctx && ctx->state;
    if (us) *us = have ? ctx->state->t_dtw_us : 0;
    if (n_windows) *n_windows = have ? ctx->state->n_dtw : 0;
}
// candidate texts scored against the audio (wmi_device.h; score.cpp)
struct wmi_score_params wmi_score_default_params(void) {
    struct wmi_score_params p = { 0, 0, nullptr, 0, 1, 0 };
    return p;
}
int wmi_score_texts_with_state(struct whisper_context * ctx, struct whisper_state * state, struct wmi_score_params params, const whisper_token * tokens,
                               const int32_t * n_tokens, int n_texts, struct wmi_text_score * out, float * token_logprobs, float * logits_out) {
    if (!ctx) return -1;
    if (ctx->host_only) { WMI_ERR("%s: host-only context has no compute path (this backend has no CPU fallback)\n", __func__); return -2; }
    if (!state) state = reinterpret_cast<struct whisper_state *>(ctx->state.get());      // (NULL: the context's own state)
    if (!state) return -1;
    StateScope sc(ctx, state);
    return score_texts(*ctx, params, tokens, n_tokens, n_texts, out, token_logprobs, logits_out);
}
int wmi_score_texts(struct whisper_context * ctx, struct wmi_score_params params, const whisper_token * tokens, const int32_t * n_tokens, int n_texts,
                    struct wmi_text_score * out, float * token_logprobs) {
    return wmi_score_texts_with_state(ctx, ctx ? reinterpret_cast<struct whisper_state *>(ctx->state.get()) : nullptr, params, tokens, n_tokens, n_texts,
                                      out, token_logprobs, nullptr);
}
int wmi_score_pcm(struct whisper_context * ctx, struct wmi_score_params params, const float * pcm, int n_samples, int pcm_on_device, int audio_ctx,
                  const whisper_token * tokens, const int32_t * n_tokens, int n_texts, struct wmi_text_score * out, float * token_logprobs) {
    if (!ctx) return -1;
    if (ctx->host_only) { WMI_ERR("%s: host-only context has no compute path (this backend has no CPU fallback)\n", __func__); return -2; }
    if (!ctx->state || !pcm || n_samples < 1 || !out) return -1;
    if (audio_ctx < 0 || audio_ctx > ctx->model.hp.n_audio_ctx) return -1;
    StateScope sc(ctx, reinterpret_cast<struct whisper_state *>(ctx->state.get()));
    State & st = *ctx->state;
    {   // the arguments are judged before the log-mel and the encoder run
        ScorePlan pl;
        if (score_plan(ctx->model.vocab, ctx->model.hp, st.kv_self.size, params, tokens, n_tokens, n_texts, pl) != 0) return -1;
    }
    const int saved = st.exp_n_audio_ctx;
    st.exp_n_audio_ctx = audio_ctx;
    const bool ok = pcm_to_mel(*ctx, pcm, n_samples, pcm_on_device != 0) && encode(*ctx, 0);
    st.exp_n_audio_ctx = saved;
    if (!ok) { WMI_ERR("%s: failed to encode\n", __func__); return -3; }
    return score_texts(*ctx, params, tokens, n_tokens, n_texts, out, token_logprobs, nullptr);
}
void wmi_get_score_timings(struct whisper_context * ctx, int64_t * us, int32_t * n_calls, int32_t * n_launches) {
    const bool have = ctx && ctx->state;
    if (us) *us = have ? ctx->state->t_score_us : 0;
    if (n_calls) *n_calls = have ? ctx->state->n_score : 0;
    if (n_launches) *n_launches = have ? ctx->state->n_score_launches : 0;
}
int wmi_selftest_score_plan(struct whisper_context * ctx, struct wmi_score_params params, const whisper_token * tokens, const int32_t * n_tokens,
                            int n_texts, int32_t * prefix, int cap_prefix, int * n_prefix, int32_t * first, int32_t * prefix_target, int32_t * rows,
                            int cap_rows, int * n_rows, int32_t * pass_text0, int cap_passes) {
    if (!ctx) return -1;
    ScorePlan pl;
    // (a host-only context has no self cache: the size init_state would give it)
    const size_t kv_cells = ctx->state && ctx->state->kv_self.size > 0 ? ctx->state->kv_self.size : 3 * (size_t) ctx->model.hp.n_text_ctx;
    if (score_plan(ctx->model.vocab, ctx->model.hp, kv_cells, params, tokens, n_tokens, n_texts, pl) != 0) return -1;
    if (n_prefix) *n_prefix = (int) pl.prefix.size();
    for (int i = 0; prefix && i < cap_prefix && i < (int) pl.prefix.size(); ++i) prefix[i] = pl.prefix[i];
    for (int c = 0; first && c <= n_texts; ++c) first[c] = pl.first[c];
    for (int c = 0; prefix_target && c < n_texts; ++c) prefix_target[c] = pl.prefix_target[c];
    int nr = 0;
    for (size_t ip = 0; ip < pl.passes.size(); ++ip) {
        const ScorePass & ps = pl.passes[ip];
        if (pass_text0 && (int) ip < cap_passes) pass_text0[ip] = ps.c0;
        for (size_t i = 0; i < ps.token.size(); ++i, ++nr) {
            if (!rows || nr >= cap_rows) continue;
            int32_t * r = rows + (size_t) nr * 7;
            r[0] = (int32_t) ip; r[1] = ps.token[i]; r[2] = ps.pos[i]; r[3] = ps.seq[i]; r[4] = ps.flag[i]; r[5] = ps.target[i]; r[6] = ps.place[i];
        }
    }
    if (pass_text0 && (int) pl.passes.size() < cap_passes) pass_text0[pl.passes.size()] = n_texts;
    if (n_rows) *n_rows = nr;
    return (int) pl.passes.size();
}
int wmi_selftest_score_rows(int device, int rows, int n_vocab, const float * logits, const int32_t * targets, float * lp_out) {
    if (rows < 1 || n_vocab < 1 || n_vocab > k::NSP_MAX_VOCAB || !logits || !targets || !lp_out) return -1;
    for (int r = 0; r < rows; ++r) if (targets[r] < 0 || targets[r] >= n_vocab) return -1;
    if (!HIP_OK(hipSetDevice(device))) return -2;
    struct Bufs {
        std::vector<void *> dev; hipStream_t st = nullptr;
        ~Bufs() { if (st) (void) hipStreamDestroy(st); for (void * q : dev) (void) hipFree(q); }
        void * get(size_t bytes) { void * q = nullptr; if (!HIP_OK(hipMalloc(&q, bytes))) return nullptr; dev.push_back(q); return q; }
    } b;
    // as decode() works: a logits buffer of 8 rows, filled and scored group by group on one stream
    const int G = k::SCORE_MAX_ROWS;
    void * scratch = b.get(k::score_scratch_bytes(n_vocab));
    float * d_l = (float *) b.get((size_t) G * n_vocab * 4), * d_lp = (float *) b.get((size_t) rows * 4);
    int32_t * d_i = (int32_t *) b.get((size_t) 2 * rows * 4);
    if (!scratch || !d_l || !d_lp || !d_i || !HIP_OK(hipStreamCreate(&b.st))) return -3;
    std::vector<int32_t> items((size_t) 2 * rows);
    for (int r = 0; r < rows; ++r) { items[r] = targets[r]; items[(size_t) rows + r] = r; }
    if (!HIP_OK(hipMemcpyAsync(d_i, items.data(), items.size() * 4, hipMemcpyHostToDevice, b.st)) || !HIP_OK(hipStreamSynchronize(b.st))) return -3;
    for (int r0 = 0; r0 < rows; r0 += G) {
        const int nr = std::min(G, rows - r0);
        if (!HIP_OK(hipMemcpyAsync(d_l, logits + (size_t) r0 * n_vocab, (size_t) nr * n_vocab * 4, hipMemcpyHostToDevice, b.st))) return -3;
        k::ScoreRows sr{}; sr.n = nr; for (int r = 0; r < nr; ++r) sr.row[r] = r;
        if (!k::score_rows(d_l, n_vocab, sr, n_vocab, d_i + r0, d_i + rows + r0, scratch, d_lp, b.st)) return -3;
    }
    if (!HIP_OK(hipMemcpyAsync(lp_out, d_lp, (size_t) rows * 4, hipMemcpyDeviceToHost, b.st)) || !HIP_OK(hipStreamSynchronize(b.st)) ||
        !HIP_OK(hipGetLastError())) return -3;
    return 0;
}
// a draft transcript verified in one decoder pass (wmi_device.h; full.cpp, device.cpp: draft_*)
int wmi_set_draft_with_state(struct whisper_context * ctx, struct whisper_state * state, const whisper_token * tokens, int n) {
    if (!ctx || n < 0 || (n > 0 && !tokens)) return -1;
    if (!state) state = reinterpret_cast<struct whisper_state *>(ctx->state.get());      // (NULL: the context's own state)
    if (!state) return -1;
    const int NV = ctx->model.vocab.n_vocab;
    for (int i = 0; i < n; ++i) if (tokens[i] < 0 || tokens[i] >= NV) return -1;
    std::lock_guard<std::recursive_mutex> lk(S(state)->mu);
    S(state)->draft.assign(tokens, tokens + n);
    return 0;
}
int wmi_set_draft(struct whisper_context * ctx, const whisper_token * tokens, int n) { return wmi_set_draft_with_state(ctx, nullptr, tokens, n); }
int wmi_draft_status_from_state(struct whisper_state * state, struct wmi_draft_status * out) {
    if (!state || !out) return -1;
    std::lock_guard<std::recursive_mutex> lk(S(state)->mu);
    *out = S(state)->draft_status;
    return 0;
}
int wmi_draft_status(struct whisper_context * ctx, struct wmi_draft_status * out) {
    return ctx && ctx->state ? wmi_draft_status_from_state(reinterpret_cast<struct whisper_state *>(ctx->state.get()), out) : -1;
}
int wmi_selftest_draft_logits(struct whisper_context * ctx, float * buf, int cap_rows) {
    if (!ctx || !ctx->state || cap_rows < 0) return -1;
    std::lock_guard<std::recursive_mutex> lk(ctx->state->mu);
    ctx->state->draft_logits_out = cap_rows > 0 ? buf : nullptr; ctx->state->draft_logits_cap = buf ? cap_rows : 0;
    return 0;
}
int wmi_selftest_draft_plan(struct whisper_context * ctx, struct whisper_full_params params, const whisper_token * prompt, int n_prompt,
                            const whisper_token * draft, int n_draft, int32_t * n_rows, int32_t * logit_rows, int32_t * steps) {
    if (!ctx || !prompt || n_prompt < 1 || n_draft < 0 || (n_draft > 0 && !draft) || !n_rows || !logit_rows || !steps) return -1;
    const Vocab & v = ctx->model.vocab; const HParams & hp = ctx->model.hp;
    if (n_prompt > hp.n_text_ctx) return -1;
    for (int i = 0; i < n_prompt; ++i) if (prompt[i] < 0 || prompt[i] >= v.n_vocab) return -1;
    for (int i = 0; i < n_draft; ++i) if (draft[i] < 0 || draft[i] >= v.n_vocab) return -1;
    static_assert(sizeof(k::DecStep) == 16 * sizeof(int32_t), "a step record is 16 words");
    const int seek = params.offset_ms / 10, seek_end = seek + (params.duration_ms > 0 ? params.duration_ms / 10 : 100 * WHISPER_CHUNK_SIZE);
    const DraftPlan pl = draft_plan(*ctx, params, n_prompt, draft, n_draft, seek, seek_end);
    int space_id = -1; { auto sp = v.token_to_id.find(" "); if (sp != v.token_to_id.end()) space_id = sp->second; }
    *n_rows = pl.n + 1;
    for (int j = 0; j <= pl.n; ++j) {
        const StepFilter & f = pl.filters[j];
        k::DecStep st; memset(&st, 0, sizeof(st));
        st.flags = (f.ban_blank ? 1 : 0) | (f.last_ts ? 2 : 0) | (f.penult_ts ? 4 : 0);
        st.space_id = space_id; st.eot = v.eot; st.beg = v.beg; st.n_vocab = v.n_vocab;
        st.ts_floor_end = f.ts_floor_end; st.ts_initial_start = f.ts_initial_start;
        memcpy(steps + (size_t) j * 16, &st, sizeof(st));
        logit_rows[j] = n_prompt - 1 + j;
    }
    return 0;
}
int wmi_selftest_draft_rows(int device, int n_rows, int n_vocab, const float * logits, const uint8_t * ban, const int32_t * steps, const int32_t * targets,
                            int32_t * out, int32_t * accepted) {
    static_assert(sizeof(k::SampleOut) == 8 * sizeof(int32_t), "a record is 8 words");
    if (n_rows < 1 || n_rows > 4096 || n_vocab < 1 || n_vocab > 65536 || !logits || !ban || !steps || !out || !accepted || (n_rows > 1 && !targets)) return -1;
    std::vector<k::DecStep> hs((size_t) n_rows);
    memcpy(hs.data(), steps, (size_t) n_rows * sizeof(k::DecStep));
    for (int r = 0; r < n_rows; ++r) if (hs[r].n_vocab != n_vocab) return -1;      // (k_filter_stats takes the row length from the record)
    for (int r = 0; r + 1 < n_rows; ++r) if (targets[r] < 0 || targets[r] >= n_vocab) return -1;
    if (!HIP_OK(hipSetDevice(device))) return -2;
    struct Bufs {
        std::vector<void *> dev; void * host = nullptr; hipStream_t st = nullptr;
        ~Bufs() { if (st) (void) hipStreamDestroy(st); for (void * q : dev) (void) hipFree(q); if (host) (void) hipHostFree(host); }
        void * get(size_t bytes) { void * q = nullptr; if (!HIP_OK(hipMalloc(&q, bytes))) return nullptr; dev.push_back(q); return q; }
    } b;
    // as decode() works: a logits buffer of 8 rows, filled and picked group by group on one stream; one wait behind the finish
    const int G = 8, n_targets = n_rows - 1;
    const int32_t tag = hs[0].seq & k::SAMPLE_SEQ_MASK;
    float * d_l = (float *) b.get((size_t) G * n_vocab * 4);
    uint8_t * d_ban = (uint8_t *) b.get((size_t) n_vocab);
    k::DecStep * d_steps = (k::DecStep *) b.get((size_t) n_rows * sizeof(k::DecStep));
    int32_t * d_tm = (int32_t *) b.get((size_t) 2 * n_rows * 4);       // targets | match
    k::FsPartial * part = (k::FsPartial *) b.get(k::filter_scratch_bytes(G));
    const size_t host_bytes = 16 + (size_t) n_rows * sizeof(k::SampleOut);
    if (!d_l || !d_ban || !d_steps || !d_tm || !part || !HIP_OK(hipHostMalloc(&b.host, host_bytes, hipHostMallocDefault)) || !HIP_OK(hipStreamCreate(&b.st))) return -3;
    memset(b.host, 0, host_bytes);
    k::DraftOut * h_out = (k::DraftOut *) b.host; k::SampleOut * h_rec = (k::SampleOut *) ((char *) b.host + 16);
    std::vector<int32_t> tg((size_t) n_rows, 0);
    for (int r = 0; r < n_targets; ++r) tg[r] = targets[r];
    if (!HIP_OK(hipMemcpyAsync(d_ban, ban, (size_t) n_vocab, hipMemcpyHostToDevice, b.st)) ||
        !HIP_OK(hipMemcpyAsync(d_steps, hs.data(), (size_t) n_rows * sizeof(k::DecStep), hipMemcpyHostToDevice, b.st)) ||
        !HIP_OK(hipMemcpyAsync(d_tm, tg.data(), (size_t) n_rows * 4, hipMemcpyHostToDevice, b.st)) ||
        !HIP_OK(hipMemsetAsync(d_tm + n_rows, 0xff, (size_t) n_rows * 4, b.st)) || !HIP_OK(hipStreamSynchronize(b.st))) return -3;
    for (int r0 = 0; r0 < n_rows; r0 += G) {
        const int nr = std::min(G, n_rows - r0);
        if (!HIP_OK(hipMemcpyAsync(d_l, logits + (size_t) r0 * n_vocab, (size_t) nr * n_vocab * 4, hipMemcpyHostToDevice, b.st))) return -3;
        k::filter_stats(d_l, d_ban, d_steps + r0, part, b.st, nr);
        k::draft_pick(part, d_steps + r0, d_tm, r0, nr, n_targets, h_rec, d_tm + n_rows, b.st);
    }
    k::draft_finish(d_tm + n_rows, n_rows, tag, h_out, b.st);
    if (!HIP_OK(hipGetLastError()) || !HIP_OK(hipStreamSynchronize(b.st))) return -3;
    if (h_out->tag != tag || h_out->accepted < 0 || h_out->accepted > n_targets) return -3;
    memcpy(out, h_rec, (size_t) n_rows * sizeof(k::SampleOut));
    *accepted = h_out->accepted;
    return 0;
}
int wmi_selftest_no_speech_rule(int mode, float p, float thold, int failed, double avg_logprob, float logprob_thold) {
    return no_speech_rule(mode, p, thold, failed != 0, avg_logprob, logprob_thold);
}

const char * whisper_lang_str_full(int id) { return lang_str_full(id); }

// ---------------------------------------------------------------------------------------------- bench entry points
// The reference times host memcpy and ggml_mul_mat on n_threads cores (W/whisper.cpp:6027-6266).  The drop-in reports
// the same two quantities for what does the work here: device-to-device copy bandwidth in HBM, and the f16 MFMA GEMM
// of the encoder (k_gemm, every epilogue writes f16) on the same square sizes.  n_threads is accepted and ignored.
const char * whisper_bench_memcpy_str(int) {
    static std::string s;
    s.clear();
    char line[256];
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { s = "memcpy: no HIP device available\n"; return s.c_str(); }
    const size_t size = 1024ull * 1000 * 1000;       // the reference's 1 GB array
    char * src = nullptr, * dst = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipMalloc(&src, size) != hipSuccess || hipMalloc(&dst, size) != hipSuccess ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        s = "memcpy: device allocation failed\n";
    } else {
        (void) hipMemset(src, 1, size);
        (void) hipMemcpy(dst, src, size, hipMemcpyDeviceToDevice);           // heat-up
        const int n = 20;
        (void) hipEventRecord(e0, nullptr);
        for (int i = 0; i < n; ++i) (void) hipMemcpyAsync(dst, src, size, hipMemcpyDeviceToDevice, nullptr);
        (void) hipEventRecord(e1, nullptr);
        (void) hipEventSynchronize(e1);
        float ms = 0.0f; (void) hipEventElapsedTime(&ms, e0, e1);
        snprintf(line, sizeof(line), "memcpy: %7.2f GB/s (HBM, device to device; read + write traffic is twice that)\n", (double) n * size / (ms * 1e6));
        s += line;
        unsigned char probe[64] = {0};
        (void) hipMemcpy(probe, dst + size - 64, 64, hipMemcpyDeviceToHost);
        double sum = 0.0; for (unsigned char c : probe) sum += c;
        snprintf(line, sizeof(line), "sum:    %f\n", sum * (double) (size / 64));
        s += line;
    }
    if (e0) (void) hipEventDestroy(e0);
    if (e1) (void) hipEventDestroy(e1);
    if (src) (void) hipFree(src);
    if (dst) (void) hipFree(dst);
    return s.c_str();
}
int whisper_bench_memcpy(int n_threads) { fputs(whisper_bench_memcpy_str(n_threads), stderr); return 0; }

const char * whisper_bench_ggml_mul_mat_str(int) {
    static std::string s;
    s.clear();
    char line[256];
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { s = "mul_mat: no HIP device available\n"; return s.c_str(); }
    const size_t sizes[] = { 64, 128, 256, 512, 1024, 2048, 4096 };
    const size_t N_max = 4096;
    __half * a = nullptr, * b = nullptr, * c = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipMalloc(&a, N_max * N_max * 2) != hipSuccess || hipMalloc(&b, N_max * N_max * 2) != hipSuccess || hipMalloc(&c, N_max * N_max * 2) != hipSuccess ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        s = "mul_mat: device allocation failed\n";
    } else {
        (void) hipMemset(a, 0x3c, N_max * N_max * 2);         // f16 0x3c3c = 1.0586: finite operands
        (void) hipMemset(b, 0x3c, N_max * N_max * 2);
        for (const size_t N : sizes) {
            k::GemmArgs g{};
            g.A = a; g.lda = (int) N; g.W = b; g.ldw = (int) N; g.M = g.N = g.K = (int) N; g.bias = nullptr; g.C = c; g.ldc = (int) N;
            k::gemm(k::EPI_F16_BIAS, g, nullptr);             // heat-up
            (void) hipStreamSynchronize(nullptr);
            int n = 0; float ms = 0.0f;
            for (int rep = 8; rep <= 1024 && ms < 20.0f; rep *= 2) {       // grow the run until it lasts 20 ms (the reference stops at 1 s)
                (void) hipEventRecord(e0, nullptr);
                for (int i = 0; i < rep; ++i) k::gemm(k::EPI_F16_BIAS, g, nullptr);
                (void) hipEventRecord(e1, nullptr);
                (void) hipEventSynchronize(e1);
                (void) hipEventElapsedTime(&ms, e0, e1);
                n = rep;
            }
            const double gflops = 2.0 * N * N * N * n / (ms * 1e6);
            snprintf(line, sizeof(line), "%4zu x %4zu: F16  %9.1f GFLOPS (%4d runs) | MFMA f16 x f16 -> f32 accumulate, f16 out\n", N, N, gflops, n);
            s += line;
        }
    }
    if (e0) (void) hipEventDestroy(e0);
    if (e1) (void) hipEventDestroy(e1);
    if (a) (void) hipFree(a);
    if (b) (void) hipFree(b);
    if (c) (void) hipFree(c);
    return s.c_str();
}
int whisper_bench_ggml_mul_mat(int n_threads) { fputs(whisper_bench_ggml_mul_mat_str(n_threads), stderr); return 0; }

} // extern "C"

// Candidate texts scored against the encoded audio in one teacher-forced pass (include/wmi_device.h: wmi_score_texts).
// score_plan is pure host arithmetic; score_texts queues the prefix batch, the candidate passes — every text a sequence of the unified
// self cache that shares the prefix's cells — and the per-text sums on the state's stream and waits once.

#include "wmi.h"
#include "kernels.h"

#include <algorithm>
#include <cstring>

namespace wmi {

static_assert(sizeof(k::ScoreRec) == sizeof(wmi_text_score) && offsetof(k::ScoreRec, post) == offsetof(wmi_text_score, posterior) &&
              offsetof(k::ScoreRec, first) == offsetof(wmi_text_score, first), "the kernel writes wmi_text_score records");

int score_plan(const Vocab & v, const HParams & hp, size_t kv_cells, const wmi_score_params & p, const int32_t * tokens, const int32_t * n_tokens,
               int n_texts, ScorePlan & out) {
    out = ScorePlan{};
    if (!n_tokens || n_texts < 1 || n_texts > k::SCORE_MAX_TEXTS || p.prompt_n_tokens < 0 || (p.prompt_n_tokens > 0 && !p.prompt_tokens)) return -1;
    // the prefix, as full() builds a window's prompt
    if (p.prompt_n_tokens > 0) {
        const int n_take = std::min(hp.n_text_ctx / 2 - 1, p.prompt_n_tokens);
        out.prefix.push_back(v.prev);
        for (int i = p.prompt_n_tokens - n_take; i < p.prompt_n_tokens; ++i) {
            if (p.prompt_tokens[i] < 0 || p.prompt_tokens[i] >= v.n_vocab) return -1;
            out.prefix.push_back(p.prompt_tokens[i]);
        }
    }
    out.prefix.push_back(v.sot);
    if (v.is_multilingual()) {
        if (p.lang_id < 0 || p.lang_id >= v.num_languages()) return -1;
        out.prefix.push_back(v.sot + 1 + p.lang_id);
        out.prefix.push_back(p.translate ? v.translate : v.transcribe);
    }
    out.prefix.push_back(v.not_);
    const int P = (int) out.prefix.size();
    const bool eot = p.with_eot != 0;
    size_t n_ids = 0;
    for (int c = 0; c < n_texts; ++c) {
        const int n = n_tokens[c];
        if (n < 0 || (n == 0 && !eot) || n > hp.n_text_ctx - P || (n > 0 && !tokens)) return -1;
        for (int i = 0; i < n; ++i) if (tokens[n_ids + i] < 0 || tokens[n_ids + i] >= v.eot) return -1;
        n_ids += (size_t) n;
    }
    // a pass: texts in order, each whole, while the rows fit one batch and, with the prefix, the self cache
    const int cap = (int) std::min<size_t>((size_t) hp.n_text_ctx, kv_cells > (size_t) P ? kv_cells - (size_t) P : 0);
    out.first.assign((size_t) n_texts + 1, 0);
    out.prefix_target.resize((size_t) n_texts);
    out.passes.emplace_back();
    const int32_t * y = tokens;
    for (int c = 0; c < n_texts; ++c) {
        const int n = n_tokens[c], n_rows = eot ? n : n - 1;           // input rows: y_{n-1} is fed only to predict <eot>
        if (n_rows > cap) return -1;
        if ((int) out.passes.back().token.size() + n_rows > cap) { out.passes.emplace_back(); out.passes.back().c0 = c; }
        ScorePass & ps = out.passes.back();
        const int f = out.first[c];
        out.prefix_target[c] = n > 0 ? y[0] : v.eot;
        for (int i = 0; i < n_rows; ++i) {
            ps.token.push_back(y[i]); ps.pos.push_back(P + i); ps.seq.push_back(c + 1); ps.flag.push_back(1);
            ps.target.push_back(i + 1 < n ? y[i + 1] : v.eot); ps.place.push_back(f + 1 + i);
        }
        ps.c1 = c + 1;
        out.first[c + 1] = f + 1 + n_rows;
        y += n;
    }
    return 0;
}

bool score_group(whisper_context & ctx, const DeviceState::ScoreReq & rq, int r0, int nr, int & item) {
    State & st = *ctx.state; DeviceState & d = st.dev;
    const int NV = ctx.model.hp.n_vocab;
    while (item < rq.n_items && rq.item_row[item] < r0 + nr) {
        k::ScoreRows sr{};
        const int j0 = item;
        while (item < rq.n_items && rq.item_row[item] < r0 + nr && sr.n < k::SCORE_MAX_ROWS) {
            if (rq.item_row[item] < r0) return false;                  // (items ascend with the flagged rows)
            sr.row[sr.n++] = rq.item_row[item++] - r0;
        }
        if (!k::score_rows(d.logits, NV, sr, NV, rq.d_target + j0, rq.d_place + j0, d.score_scratch, d.score_lp, d.stream)) return false;
        st.n_score_launches += 2;
        for (int j = j0; rq.logits_out && j < item; ++j)
            HIP_TRY(hipMemcpyAsync(rq.logits_out + (size_t) rq.place[j] * NV, d.logits + (size_t) sr.row[j - j0] * NV, (size_t) NV * 4, hipMemcpyDeviceToHost, d.stream));
    }
    return true;
}

namespace {

size_t staging_bytes(int n, int n_kv) { return (((size_t) 3 * n + (size_t) n * n_kv) * 4 + 255) & ~(size_t) 255; }

// grow-only; the pinned block: ScoreOut (16 bytes) | ScoreRec [texts] | lp [rows] | items {target | place} [2 rows] | first [texts + 1] | staging
struct HostView { k::ScoreOut * out; k::ScoreRec * rec; float * lp; int32_t * items, * first; char * staging; };
bool score_ensure(whisper_context & ctx, DeviceState & d, int n_texts, int n_rows, size_t stage_bytes, HostView & hv) {
    const int NV = ctx.model.hp.n_vocab;
    if (NV > k::NSP_MAX_VOCAB) { WMI_ERR("%s: a vocabulary of %d entries is not covered (max %d)\n", __func__, NV, k::NSP_MAX_VOCAB); return false; }
    if (!d.score_scratch) HIP_TRY(hipMalloc(&d.score_scratch, k::score_scratch_bytes(NV)));
    const size_t n_items = (size_t) 2 * n_rows + (size_t) n_texts + 1;
    if (d.score_items_cap < n_items) {
        if (d.score_items) { (void) hipFree(d.score_items); d.score_items = nullptr; d.score_items_cap = 0; }
        HIP_TRY(hipMalloc((void **) &d.score_items, n_items * 4));
        d.score_items_cap = n_items;
    }
    if (d.score_lp_cap < (size_t) n_rows) {
        if (d.score_lp) { (void) hipFree(d.score_lp); d.score_lp = nullptr; d.score_lp_cap = 0; }
        HIP_TRY(hipMalloc((void **) &d.score_lp, (size_t) n_rows * 4));
        d.score_lp_cap = (size_t) n_rows;
    }
    const size_t o_rec = 16, o_lp = o_rec + (size_t) n_texts * sizeof(k::ScoreRec), o_items = o_lp + (size_t) n_rows * 4,
                 o_stage = (o_items + n_items * 4 + 255) & ~(size_t) 255, bytes = o_stage + stage_bytes;
    if (d.score_host_cap < bytes) {
        if (d.score_host) { (void) hipHostFree(d.score_host); d.score_host = nullptr; d.score_host_cap = 0; }
        HIP_TRY(hipHostMalloc(&d.score_host, bytes, hipHostMallocDefault));
        d.score_host_cap = bytes;
    }
    char * h = (char *) d.score_host;
    memset(h, 0, 16);
    hv.out = (k::ScoreOut *) h; hv.rec = (k::ScoreRec *) (h + o_rec); hv.lp = (float *) (h + o_lp); hv.items = (int32_t *) (h + o_items);
    hv.first = hv.items + (size_t) 2 * n_rows; hv.staging = h + o_stage;
    return true;
}

} // namespace

int score_texts(whisper_context & ctx, const wmi_score_params & p, const int32_t * tokens, const int32_t * n_tokens, int n_texts, wmi_text_score * out,
                float * token_logprobs, float * logits_out) {
    if (!out) return -1;
    if (!compute_ready(ctx, __func__)) return -2;
    State & st = *ctx.state; DeviceState & d = st.dev; const HParams & hp = ctx.model.hp;
    const int64_t t0 = time_us();
    ScorePlan pl;
    if (score_plan(ctx.model.vocab, hp, st.kv_self.size, p, tokens, n_tokens, n_texts, pl) != 0) return -1;
    if (st.enc_n_ctx <= 0) { WMI_ERR("%s: no encoder result in the state (whisper_encode, whisper_full or wmi_score_pcm first)\n", __func__); return -2; }
    (void) phase_settle(st, true);                            // (a deferred log-mel / encoder of an earlier call: their time is theirs)
    const int P = (int) pl.prefix.size(), R = pl.first[n_texts];
    size_t stage = staging_bytes(P, P);
    for (const ScorePass & ps : pl.passes) if (!ps.token.empty()) stage += staging_bytes((int) ps.token.size(), P + (int) ps.token.size());
    HostView hv{};
    if (!score_ensure(ctx, d, n_texts, R, stage, hv)) return -3;
    hipStream_t s = d.stream;

    // the items of the whole call, in launch order: the texts' first targets on the prefix's last row, then every pass's flagged rows
    int32_t * h_target = hv.items, * h_place = hv.items + R;
    std::vector<int32_t> item_row((size_t) R);
    int ni = 0;
    for (int c = 0; c < n_texts; ++c, ++ni) { h_target[ni] = pl.prefix_target[c]; h_place[ni] = pl.first[c]; item_row[ni] = 0; }
    for (const ScorePass & ps : pl.passes)
        for (size_t i = 0; i < ps.token.size(); ++i, ++ni) { h_target[ni] = ps.target[i]; h_place[ni] = ps.place[i]; item_row[ni] = (int32_t) i; }
    if (ni != R) return -3;
    memcpy(hv.first, pl.first.data(), ((size_t) n_texts + 1) * 4);
    if (!HIP_OK(hipMemcpyAsync(d.score_items, hv.items, ((size_t) 2 * R + (size_t) n_texts + 1) * 4, hipMemcpyHostToDevice, s))) return -3;
    const int32_t * d_target = d.score_items, * d_place = d.score_items + R, * d_first = d.score_items + (size_t) 2 * R;

    kv_clear(st.kv_self);
    char * stg = hv.staging;
    DeviceState::ScoreReq rq{};
    rq.logits_out = logits_out; rq.place = h_place;
    auto run = [&](int n, int n_kv, int item0, int n_items) {
        rq.item_row = item_row.data() + item0; rq.n_items = n_items; rq.d_target = d_target + item0; rq.d_place = d_place + item0;
        rq.place = h_place + item0; rq.staging = stg; rq.staging_bytes = staging_bytes(n, n_kv);
        stg += rq.staging_bytes;
        d.score_req = &rq;
        const bool ok = decode(ctx, st.batch);
        d.score_req = nullptr;
        return ok;
    };
    // the prefix as sequence 0, its last row flagged: every text's first target is scored there
    st.batch.prep_legacy(pl.prefix.data(), P, 0, 0);
    if (!run(P, P, 0, n_texts)) return -3;
    int item0 = n_texts;
    for (const ScorePass & ps : pl.passes) {
        const int n = (int) ps.token.size();
        if (n == 0) continue;
        for (int c = ps.c0; c < ps.c1; ++c) kv_seq_cp(st.kv_self, 0, c + 1, 0, P);
        Batch & b = st.batch;
        b.n_tokens = n;
        if ((int) b.token.size() < n) { b.token.resize(n); b.pos.resize(n); b.seq_id.resize(n); b.logits.resize(n); }
        for (int i = 0; i < n; ++i) { b.token[i] = ps.token[i]; b.pos[i] = ps.pos[i]; b.seq_id[i] = ps.seq[i]; b.logits[i] = ps.flag[i]; }
        const bool ok = run(n, P + n, item0, n);
        for (int c = ps.c0; c < ps.c1; ++c) kv_seq_rm(st.kv_self, c + 1, -1, -1);
        if (!ok) return -3;
        item0 += n;
    }
    d.score_seq = d.score_seq >= 0x7fffffff ? 1 : d.score_seq + 1;
    if (!k::score_finish(d.score_lp, d_first, n_texts, p.length_norm != 0, hv.rec, hv.lp, hv.out, d.score_seq, s)) return -3;
    st.n_score_launches += 1;
    if (!HIP_OK(hipStreamSynchronize(s)) || !HIP_OK(hipGetLastError())) return -3;      // the call's one wait
    if (((volatile k::ScoreOut *) hv.out)->tag != d.score_seq) { WMI_ERR("%s: the scores' record did not arrive\n", __func__); return -3; }
    memcpy(out, hv.rec, (size_t) n_texts * sizeof(wmi_text_score));
    if (token_logprobs) memcpy(token_logprobs, hv.lp, (size_t) R * 4);
    d.chain_valid = false;
    st.t_score_us += time_us() - t0; st.n_score++;
    return 0;
}

} // namespace wmi

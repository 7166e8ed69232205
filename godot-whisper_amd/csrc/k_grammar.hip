// Grammar-constrained decoding on the device (wmi_set_grammar_device; reference W/whisper.cpp:4114-4176 and :4657-4709).
//
// k_grammar_reject: the set of tokens the grammar rejects depends on the parse state only, not on the logits — one thread per
// token id runs grammar_eval.h (the text the host library compiles too) against the row's stacks and writes a byte of the reject
// mask [rows][n_vocab], the same shape as the static ban.  A token's working set (two runs of ge::WS_WORDS 16-bit words) lives in
// LDS, interleaved over the 256 threads of the workgroup: 2 * 120 * 2 B = 480 B per thread, 120 KB per workgroup, one workgroup per
// CU (203 of them cover a vocabulary) — no scratch: a per-thread array indexed dynamically would go there.  The row's state and the
// rules (up to 3072 elements; longer grammars are read from global memory) are staged in LDS beside them.
//
// The penalised second pass: the UNPENALISED statistics (k_filter_stats, as is) decide "the timestamp mass beats every text token";
// if it does the grammar is not applied and the row's partials are handed on unchanged (every later result is then bit for bit the
// grammar-free one); otherwise every rejected, allowed, finite text logit loses grammar_penalty AFTER the temperature division, the
// statistics are taken again over the penalised row, and no timestamp is forced (the reference does not look at the rule again).
// The predicate allowed(), the geometry (NB = 64 workgroups of NT = 256, the block ranges) and the arithmetic of the pick and of
// the draws are those of k_sample.hip.

#include "kernels.h"
#include <algorithm>
#include "wave_ops.h"

namespace wmi { namespace k {

namespace {

constexpr int NB = 64;
constexpr int NT = 256;

using MaxIdx = FsMaxIdx;
using Partial = FsPartial;
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ MaxIdx wave_max(MaxIdx m) {
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) { MaxIdx t; t.v = WMI_SHX(m.v, o); t.i = WMI_SHX(m.i, o); m = better(m, t); }
    return m;
}
__device__ __forceinline__ float wave_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += WMI_SHX(v, o); return v; }

constexpr int LDS_ELEMS = 3072, LDS_RULES = 1024;      // 24 KB + 4 KB beside the 120 KB of working sets and the 2 KB state (160 KB per CU)
__global__ __launch_bounds__(NT) void k_grammar_reject(const ge::Elem * __restrict__ elems, const uint32_t * __restrict__ rule_off, int n_rules,
                                                       const uint8_t * __restrict__ vbytes, const uint32_t * __restrict__ voff, int eot,
                                                       const ge::RowState * __restrict__ states, int n_vocab,
                                                       uint8_t * __restrict__ reject, uint32_t * __restrict__ overflow) {
    __shared__ uint16_t ws[2 * ge::WS_WORDS * NT];
    // the row's state and — where they fit — the rules beside it in LDS: every thread walks them through chains of dependent loads
    // (from global memory the initial state of the colour-list grammar took 135 us, see profiles/r15a_grammar_device.txt)
    __shared__ ge::RowState s_st;
    __shared__ ge::Elem s_elems[LDS_ELEMS];
    __shared__ uint32_t s_off[LDS_RULES + 1];
    const ge::RowState & gst = states[blockIdx.y];       // grid.y: a decoder of the step, each with its own parse state
    const int n_stacks = gst.n_stacks;
    if (n_stacks < 0) return;                             // over the state's capacities: the host has written this row of the mask
    const int n_words = min(max(gst.n_words, 0), ge::STATE_WORDS), n_elems = (int) rule_off[n_rules];
    const bool staged = n_elems <= LDS_ELEMS && n_rules <= LDS_RULES;
    if (threadIdx.x == 0) { s_st.partial_value = gst.partial_value; s_st.partial_n_remain = gst.partial_n_remain; s_st.n_stacks = n_stacks; s_st.n_words = n_words; }
    for (int i = threadIdx.x; i < n_words; i += NT) s_st.words[i] = gst.words[i];
    if (staged) {
        for (int i = threadIdx.x; i < n_elems; i += NT) s_elems[i] = elems[i];
        for (int i = threadIdx.x; i <= n_rules; i += NT) s_off[i] = rule_off[i];
    }
    __syncthreads();
    const int id = blockIdx.x * NT + threadIdx.x;
    if (id >= eot || id >= n_vocab) return;               // (ids from eot on are never candidates: their bytes stay 0)
    const ge::Rules R{ staged ? s_elems : elems, staged ? s_off : rule_off, n_rules };
    const ge::Vocab V{ vbytes, voff, eot };
    uint8_t r = ge::eval_token(R, V, s_st, id, ws + threadIdx.x, NT);
    if (r == ge::OVERFLOW) { overflow[blockIdx.y] = 1u; r = ge::ACCEPTED; }      // (the host redoes the row: the byte is not used)
    reject[(size_t) blockIdx.y * n_vocab + id] = r;
}

__device__ __forceinline__ bool allowed(const DecStep & st, unsigned char bn, int i) {
    const bool ban_blank = st.flags & 1, last_ts = st.flags & 2, pen_ts = st.flags & 4;
    bool a = !bn;
    if (ban_blank && (i == st.eot || i == st.space_id)) a = false;
    if (last_ts) { if (pen_ts) { if (i >= st.beg) a = false; } else { if (i < st.eot) a = false; } }
    if (i >= st.ts_initial_start) a = false;
    if (i >= st.beg && i < st.ts_floor_end) a = false;
    return a;
}
struct RowStats { float M, lse; int force_ts; MaxIdx all, ts; float sum_ts; };
// the 64 partials of a row -> global max, log-sum-exp, "timestamp mass beats every text token" (all lanes get the result)
__device__ __forceinline__ RowStats row_stats(const Partial * part, int lane) {
    const Partial p = part[lane];
    const MaxIdx a = wave_max(p.all), t = wave_max(p.txt), z = wave_max(p.ts);
    const float M = a.v;
    const float w = p.all.v > -INFINITY ? expf(p.all.v - M) : 0.0f;
    const float sum = wave_sum(p.sum * w), sum_ts = wave_sum(p.sum_ts * w);
    RowStats r;
    r.M = M; r.lse = logf(sum) + M;
    const float ts_logprob = sum_ts > 0.0f ? logf(sum_ts) + M - r.lse : -INFINITY;
    const float max_text = t.v > -INFINITY ? t.v - r.lse : -INFINITY;
    r.force_ts = ts_logprob > max_text ? 1 : 0;
    r.all = a; r.ts = z; r.sum_ts = sum_ts;
    return r;
}

// k_filter_stats over (logits, ban, reject mask, penalty): part_in = the row's unpenalised partials, part_out = what the pick / the
// draws read, applied[row] = 1 when the grammar was applied (no timestamp is forced then)
__global__ __launch_bounds__(NT) void k_grammar_stats(const float * __restrict__ logits, const uint8_t * __restrict__ ban,
                                                      const uint8_t * __restrict__ reject, float penalty, const DecStep * __restrict__ stp,
                                                      const Partial * __restrict__ part_in, Partial * __restrict__ part_out,
                                                      int32_t * __restrict__ applied) {
    __shared__ MaxIdx s_all[4], s_txt[4], s_ts[4];
    __shared__ float s_sum[4], s_sum_ts[4];
    __shared__ float b_M;
    const DecStep st = stp[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NV = st.n_vocab, beg = st.beg;
    logits += (size_t) blockIdx.y * NV; reject += (size_t) blockIdx.y * NV;
    part_in += (size_t) blockIdx.y * NB; part_out += (size_t) blockIdx.y * NB;
    const RowStats un = row_stats(part_in, lane);
    if (un.force_ts) {                                   // the grammar is not applied: nothing changes
        if (tid == 0) { part_out[blockIdx.x] = part_in[blockIdx.x]; if (blockIdx.x == 0) applied[blockIdx.y] = 0; }
        return;
    }
    if (tid == 0 && blockIdx.x == 0) applied[blockIdx.y] = 1;
    const int per = (NV + NB - 1) / NB, i0 = blockIdx.x * per, i1 = min(NV, i0 + per);

    constexpr int MAXE = 4;                            // ceil(51866 / 64 / 256)
    float lv[MAXE]; bool ok[MAXE];
    unsigned char bn[MAXE], rj[MAXE]; float lraw[MAXE];
#pragma unroll
    for (int e = 0; e < MAXE; ++e) { const int i = i0 + e * NT + tid, ic = i < i1 ? i : i0; bn[e] = ban[ic]; rj[e] = reject[ic]; lraw[e] = logits[ic]; }
    MaxIdx m_all = {-INFINITY, 0x7fffffff}, m_txt = m_all, m_ts = m_all;
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
        const int i = i0 + e * NT + tid;
        ok[e] = false; lv[e] = -INFINITY;
        if (i < i1 && allowed(st, bn[e], i) && lraw[e] > -INFINITY) {
            ok[e] = true; lv[e] = st.temperature > 0.0f ? lraw[e] / st.temperature : lraw[e];
            if (rj[e]) lv[e] -= penalty;                 // divided first, penalised after (W/whisper.cpp:4500-4506, :4684-4706)
            const MaxIdx c = {lv[e], i};
            m_all = better(m_all, c);
            if (i < beg) m_txt = better(m_txt, c); else m_ts = better(m_ts, c);
        }
    }
    m_all = wave_max(m_all); m_txt = wave_max(m_txt); m_ts = wave_max(m_ts);
    if (lane == 0) { s_all[wave] = m_all; s_txt[wave] = m_txt; s_ts[wave] = m_ts; }
    __syncthreads();
    if (tid == 0) {
        MaxIdx a = s_all[0], t = s_txt[0], z = s_ts[0];
        for (int w = 1; w < 4; ++w) { a = better(a, s_all[w]); t = better(t, s_txt[w]); z = better(z, s_ts[w]); }
        s_all[0] = a; s_txt[0] = t; s_ts[0] = z; b_M = a.v;
    }
    __syncthreads();
    const float M = b_M;
    float sum = 0.0f, sum_ts = 0.0f;
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
        if (!ok[e]) continue;
        const float x = expf(lv[e] - M);
        sum += x;
        if (i0 + e * NT + tid >= beg) sum_ts += x;
    }
    sum = wave_sum(sum); sum_ts = wave_sum(sum_ts);
    if (lane == 0) { s_sum[wave] = sum; s_sum_ts[wave] = sum_ts; }
    __syncthreads();
    if (tid == 0) {
        Partial p;
        p.all = s_all[0]; p.txt = s_txt[0]; p.ts = s_ts[0];
        p.sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        p.sum_ts = (s_sum_ts[0] + s_sum_ts[1]) + (s_sum_ts[2] + s_sum_ts[3]);
        p.pad[0] = p.pad[1] = 0.0f;
        part_out[blockIdx.x] = p;
    }
}

// the row's statistics as the pick and the draws use them: with the grammar applied no timestamp is forced
__device__ __forceinline__ RowStats row_stats_g(const Partial * part, int32_t applied, int lane) {
    RowStats rs = row_stats(part, lane);
    if (applied) rs.force_ts = 0;
    return rs;
}

// best = true: k_filter_pick's decision and record (one partial per lane, no chained step) on the penalised partials
__global__ __launch_bounds__(64) void k_grammar_pick(const Partial * __restrict__ part, const int32_t * __restrict__ applied,
                                                     const DecStep * __restrict__ stp, SampleOut * __restrict__ out) {
    const int lane = threadIdx.x, row = blockIdx.x;
    const RowStats rs = row_stats_g(part + (size_t) row * NB, applied[row], lane);
    const MaxIdx pick = rs.force_ts ? rs.ts : rs.all;
    if (lane == 0) {
        const float M = rs.M, lse = rs.lse;
        SampleOut r;
        const int seqv = stp[row].seq & SAMPLE_SEQ_MASK;
        r.id = pick.i; r.plog = pick.v - lse; r.p = expf(r.plog); r.seq0 = seqv; r.seq = seqv;
        const float p_ts_max = rs.ts.v > -INFINITY ? expf(rs.ts.v - lse) : 0.0f;
        const double sum_ts_p = (double) rs.sum_ts * (double) expf(M - lse);
        r.tid = p_ts_max > 0.0f ? rs.ts.i : 0;
        r.pt = (float) ((double) p_ts_max / (sum_ts_p + 1e-10));
        r.ptsum = (float) sum_ts_p;
        if (r.id >= stp[row].beg) { r.tid = r.id; r.pt = r.p; }
        out[row] = r;
    }
}

// the penalised logit of entry i as the statistics took it, and its probability
__device__ __forceinline__ float logit_of(const DecStep & st, int32_t applied, float lraw, unsigned char rj, float penalty) {
    float l = st.temperature > 0.0f ? lraw / st.temperature : lraw;
    if (applied && rj) l -= penalty;
    return l;
}
__device__ __forceinline__ float prob_of(const DecStep & st, const RowStats & rs, int32_t applied, float lraw, unsigned char bn,
                                         unsigned char rj, float penalty, int i) {
    if (!allowed(st, bn, i) || (rs.force_ts && i < st.beg)) return 0.0f;
    return expf(logit_of(st, applied, lraw, rj, penalty) - rs.lse);
}

// k_prob_blocks / k_draw over the penalised row (beam search, t > 0)
__global__ __launch_bounds__(NT) void k_grammar_prob_blocks(const float * __restrict__ logits, const uint8_t * __restrict__ ban,
                                                            const uint8_t * __restrict__ reject, float penalty,
                                                            const DecStep * __restrict__ stp, const Partial * __restrict__ part,
                                                            const int32_t * __restrict__ applied, double * __restrict__ bsum) {
    __shared__ double s_w[4];
    const DecStep st = stp[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NV = st.n_vocab;
    logits += (size_t) blockIdx.y * NV; reject += (size_t) blockIdx.y * NV;
    const int32_t ap = applied[blockIdx.y];
    const RowStats rs = row_stats_g(part + (size_t) blockIdx.y * NB, ap, lane);
    const int per = (NV + NB - 1) / NB, i0 = blockIdx.x * per, i1 = min(NV, i0 + per);
    double acc = 0.0;
    for (int i = i0 + tid; i < i1; i += NT) acc += (double) prob_of(st, rs, ap, logits[i], ban[i], reject[i], penalty, i);
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) acc += WMI_SHX(acc, o);
    if (lane == 0) s_w[wave] = acc;
    __syncthreads();
    if (tid == 0) bsum[(size_t) blockIdx.y * NB + blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}
__global__ __launch_bounds__(64) void k_grammar_draw(const float * __restrict__ logits, const uint8_t * __restrict__ ban,
                                                     const uint8_t * __restrict__ reject, float penalty,
                                                     const DecStep * __restrict__ stp, const Partial * __restrict__ part,
                                                     const int32_t * __restrict__ applied, const double * __restrict__ bsum,
                                                     const double * __restrict__ u, int k, int tid_default, SampleOut * __restrict__ out) {
    const int lane = threadIdx.x, dr = blockIdx.x, row = blockIdx.y;
    const DecStep st = stp[row];
    const int NV = st.n_vocab;
    logits += (size_t) row * NV; reject += (size_t) row * NV;
    const int32_t ap = applied[row];
    const RowStats rs = row_stats_g(part + (size_t) row * NB, ap, lane);
    const double mine = bsum[(size_t) row * NB + lane];
    double pre = mine;
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(pre, o); if (lane >= o) pre += t; }
    const double total = __shfl(pre, 63);
    const double target = u[(size_t) row * k + dr] * total;
    const unsigned long long hit = __ballot(pre >= target && mine > 0.0);
    const unsigned long long nz = __ballot(mine > 0.0);
    int b = hit ? __ffsll((long long) hit) - 1 : (nz ? 63 - __clzll((long long) nz) : 0);
    const double before = __shfl(pre, b) - __shfl(mine, b);
    const int per = (NV + NB - 1) / NB, i0 = b * per, i1 = min(NV, i0 + per);
    const int run = (per + 63) / 64, j0 = i0 + lane * run, j1 = min(i1, j0 + run);
    double loc = 0.0;
    for (int i = j0; i < j1; ++i) loc += (double) prob_of(st, rs, ap, logits[i], ban[i], reject[i], penalty, i);
    double lpre = loc;
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(lpre, o); if (lane >= o) lpre += t; }
    const double want = target - before;
    const unsigned long long lh = __ballot(lpre >= want && loc > 0.0), lnz = __ballot(loc > 0.0);
    const int L = lh ? __ffsll((long long) lh) - 1 : (lnz ? 63 - __clzll((long long) lnz) : 0);
    const double lbefore = __shfl(lpre, L) - __shfl(loc, L);
    if (lane == L) {
        int pick = -1, last_nz = -1; double c = lbefore;
        for (int i = j0; i < j1; ++i) {
            const float p = prob_of(st, rs, ap, logits[i], ban[i], reject[i], penalty, i);
            if (p > 0.0f) { last_nz = i; c += (double) p; if (pick < 0 && c >= want) pick = i; }
        }
        if (pick < 0) pick = last_nz >= 0 ? last_nz : 0;
        SampleOut r;
        const float l = logit_of(st, ap, logits[pick], reject[pick], penalty);
        r.id = pick; r.plog = l - rs.lse; r.p = expf(r.plog); r.seq0 = dr; r.seq = dr;
        const float p_ts_max = rs.ts.v > -INFINITY ? expf(rs.ts.v - rs.lse) : 0.0f;
        const double sum_ts_p = (double) rs.sum_ts * (double) expf(rs.M - rs.lse);
        r.tid = p_ts_max > 0.0f ? rs.ts.i : tid_default;
        r.pt = (float) ((double) p_ts_max / (sum_ts_p + 1e-10));
        r.ptsum = (float) sum_ts_p;
        if (r.id >= st.beg) { r.tid = r.id; r.pt = r.p; }
        out[(size_t) row * k + dr] = r;
    }
}

} // namespace

void grammar_reject(const GrammarDev & g, const ge::RowState * states, int n_rows, int n_vocab, uint8_t * reject, uint32_t * overflow,
                    hipStream_t st) {
    hipLaunchKernelGGL(k_grammar_reject, dim3((g.eot + NT - 1) / NT, n_rows), dim3(NT), 0, st, g.elems, g.rule_off, g.n_rules, g.vbytes, g.voff,
                       g.eot, states, n_vocab, reject, overflow);
}

size_t grammar_sample_scratch_bytes(int n_rows) {
    return filter_scratch_bytes(n_rows) + (size_t) n_rows * NB * (sizeof(Partial) + sizeof(double)) + (size_t) n_rows * sizeof(int32_t);
}

namespace {
struct GScratch { Partial * un, * pen; double * bsum; int32_t * applied; };
GScratch carve(void * scratch, int n_rows) {
    GScratch s;
    s.un = (Partial *) scratch;
    s.pen = (Partial *) ((char *) scratch + filter_scratch_bytes(n_rows));
    s.bsum = (double *) (s.pen + (size_t) n_rows * NB);
    s.applied = (int32_t *) (s.bsum + (size_t) n_rows * NB);
    return s;
}
}

void grammar_argmax(const float * logits, const uint8_t * static_ban, const uint8_t * reject, float penalty, const DecStep * step,
                    SampleOut * out, void * scratch, hipStream_t st, int n_rows) {
    const GScratch s = carve(scratch, n_rows);
    filter_stats(logits, static_ban, step, s.un, st, n_rows);
    hipLaunchKernelGGL(k_grammar_stats, dim3(NB, n_rows), dim3(NT), 0, st, logits, static_ban, reject, penalty, step, s.un, s.pen, s.applied);
    hipLaunchKernelGGL(k_grammar_pick, dim3(n_rows), dim3(64), 0, st, s.pen, s.applied, step, out);
}

void grammar_draw(const float * logits, const uint8_t * static_ban, const uint8_t * reject, float penalty, const DecStep * step,
                  const double * u, int k, SampleOut * out, void * scratch, hipStream_t st, int n_rows, int tid_default) {
    const GScratch s = carve(scratch, n_rows);
    filter_stats(logits, static_ban, step, s.un, st, n_rows);
    hipLaunchKernelGGL(k_grammar_stats, dim3(NB, n_rows), dim3(NT), 0, st, logits, static_ban, reject, penalty, step, s.un, s.pen, s.applied);
    hipLaunchKernelGGL(k_grammar_prob_blocks, dim3(NB, n_rows), dim3(NT), 0, st, logits, static_ban, reject, penalty, step, s.pen, s.applied, s.bsum);
    hipLaunchKernelGGL(k_grammar_draw, dim3(k, n_rows), dim3(64), 0, st, logits, static_ban, reject, penalty, step, s.pen, s.applied, s.bsum, u, k,
                       tid_default, out);
}

}} // namespace wmi::k

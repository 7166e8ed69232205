// The text scorer for gfx950: log-probabilities of given tokens in the soft-max of decoder rows' raw logits, and per text their sum and the
// posterior over the call's texts (kernels.h has the definition and the fixed arithmetic).  The block pass is k_nospeech.hip's
// (nsp_block.h): a workgroup of one wavefront owns one block of NSP_BLOCK vocabulary entries of one row (row = grid.y); the combine is the
// next launch on the stream, the per-text sums one launch behind the last combine.  Nothing is shared between workgroups of a launch.

#include "kernels.h"
#include "wave_ops.h"
#include "nsp_block.h"

#include <cmath>

namespace wmi { namespace k {

namespace {

struct ScoreScratch { double * s; float * m; float * lt; int nb; };
__host__ __device__ __forceinline__ ScoreScratch score_scratch(void * base, int n_vocab) {
    ScoreScratch r; r.nb = nsp_blocks(n_vocab);
    r.s = (double *) base; r.m = (float *) (r.s + (size_t) SCORE_MAX_ROWS * r.nb); r.lt = r.m + (size_t) SCORE_MAX_ROWS * r.nb;
    return r;
}

// one wavefront per (block, row); both loads unconditional from clamped indices.  The block that holds the row's target parks its raw logit.
__global__ __launch_bounds__(64) void k_score_blocks(const float * __restrict__ logits, int ld, const ScoreRows rows, int n_vocab,
                                                     const int32_t * __restrict__ targets, void * scratch) {
    const int lane = threadIdx.x, blk = blockIdx.x, y = blockIdx.y;
    const ScoreScratch sc = score_scratch(scratch, n_vocab);
    const float * l = logits + (size_t) rows.row[y] * ld;
    const int i0 = blk * NSP_BLOCK + lane, i1 = i0 + 64;
    const float v0 = l[i0 < n_vocab ? i0 : n_vocab - 1], v1 = l[i1 < n_vocab ? i1 : n_vocab - 1];
    float m; double s;
    nsp_block_partial(v0, i0 < n_vocab, v1, i1 < n_vocab, m, s);
    if (lane == 0) { sc.s[(size_t) y * sc.nb + blk] = s; sc.m[(size_t) y * sc.nb + blk] = m; }
    const int t = targets[y], j = t - blk * NSP_BLOCK;
    if (t < n_vocab && j >= 0 && j < NSP_BLOCK && lane == (j & 63)) sc.lt[y] = j < 64 ? v0 : v1;
}

// the combine: one wavefront per row.  Every lane scales the blocks b = lane, lane + 64, .. to the row's maximum and parks the terms in
// LDS; lane 0 adds them in ascending block order and stores lp = f32(double(f32(l[t] - M)) - log(S)) at the row's place in lp.
__global__ __launch_bounds__(64) void k_score_combine(void * scratch, int n_vocab, const int32_t * __restrict__ targets,
                                                      const int32_t * __restrict__ place, float * __restrict__ lp) {
    __shared__ double term[NSP_MAX_VOCAB / NSP_BLOCK];
    const int lane = threadIdx.x, y = blockIdx.x;
    const ScoreScratch sc = score_scratch(scratch, n_vocab);
    const float * mb = sc.m + (size_t) y * sc.nb; const double * sb = sc.s + (size_t) y * sc.nb;
    float M = -INFINITY;
    for (int b = lane; b < sc.nb; b += 64) M = fmaxf(M, mb[b]);
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, WMI_SHX(M, o));
    for (int b = lane; b < sc.nb; b += 64) term[b] = sb[b] > 0.0 ? sb[b] * exp((double) (mb[b] - M)) : 0.0;
    __syncthreads();
    if (lane != 0) return;
    double S = 0.0;
    for (int b = 0; b < sc.nb; ++b) S += term[b];
    const int t = targets[y];
    float r;
    if (t < 0 || t >= n_vocab) r = NAN;                      // (the host refuses such a target before anything is launched)
    else {
        const float lt = sc.lt[y];
        r = (lt != -INFINITY && S > 0.0) ? (float) ((double) (lt - M) - log(S)) : -INFINITY;
    }
    lp[place[y]] = r;
}

// per text the sum of its rows in ascending order in double, then the posterior over the texts; one workgroup.  Thread c, c + 256, ..
// owns text c; thread 0 takes the maximum and the denominator over the texts in ascending order.  Records, the per-token values and
// the tag go to (pinned host) memory with plain vector stores.
__global__ __launch_bounds__(SCORE_FINISH_THREADS) void k_score_finish(const float * __restrict__ lp, const int32_t * __restrict__ first, int n_texts,
                                                                       int length_norm, ScoreRec * __restrict__ rec, float * __restrict__ lp_out,
                                                                       ScoreOut * __restrict__ out, int32_t tag) {
    __shared__ double v[SCORE_MAX_TEXTS];
    __shared__ double top[2];
    const int tid = threadIdx.x;
    for (int c = tid; c < n_texts; c += SCORE_FINISH_THREADS) {
        const int f = first[c], e = first[c + 1];
        double sum = 0.0;
        for (int i = f; i < e; ++i) sum += (double) lp[i];
        const double avg = sum / (double) (e - f);
        v[c] = length_norm ? avg : sum;
        rec[c].sum = sum; rec[c].avg = (float) avg; rec[c].n_scored = e - f; rec[c].first = f;
    }
    __syncthreads();
    if (tid == 0) {
        double vmax = -INFINITY, den = 0.0;
        for (int c = 0; c < n_texts; ++c) vmax = fmax(vmax, v[c]);
        for (int c = 0; c < n_texts; ++c) if (v[c] != -INFINITY) den += exp(v[c] - vmax);
        top[0] = vmax; top[1] = den;
    }
    __syncthreads();
    const double vmax = top[0], den = top[1];
    for (int c = tid; c < n_texts; c += SCORE_FINISH_THREADS)
        rec[c].post = (v[c] != -INFINITY && den > 0.0) ? (float) (exp(v[c] - vmax) / den) : 0.0f;
    const int total = first[n_texts];
    if (lp_out) for (int i = tid; i < total; i += SCORE_FINISH_THREADS) lp_out[i] = lp[i];
    __syncthreads();
    if (tid == 0) {
        union { ScoreOut o; int2 w; } r;
        r.o.n_texts = n_texts; r.o.tag = tag;
        *(int2 *) out = r.w;
    }
}

} // namespace

size_t score_scratch_bytes(int n_vocab) {
    return (size_t) SCORE_MAX_ROWS * nsp_blocks(n_vocab) * (sizeof(double) + sizeof(float)) + SCORE_MAX_ROWS * sizeof(float);
}

bool score_rows(const float * logits, int ld, const ScoreRows & rows, int n_vocab, const int32_t * targets, const int32_t * place, void * scratch,
                float * lp, hipStream_t st) {
    if (rows.n < 1 || rows.n > SCORE_MAX_ROWS || n_vocab < 1 || n_vocab > NSP_MAX_VOCAB || ld < n_vocab || !logits || !targets || !place || !scratch || !lp) return false;
    for (int r = 0; r < rows.n; ++r) if (rows.row[r] < 0) return false;
    hipLaunchKernelGGL(k_score_blocks, dim3(nsp_blocks(n_vocab), rows.n), dim3(64), 0, st, logits, ld, rows, n_vocab, targets, scratch);
    hipLaunchKernelGGL(k_score_combine, dim3(rows.n), dim3(64), 0, st, scratch, n_vocab, targets, place, lp);
    return true;
}

bool score_finish(const float * lp, const int32_t * first, int n_texts, bool length_norm, ScoreRec * rec, float * lp_out, ScoreOut * out, int32_t tag,
                  hipStream_t st) {
    if (n_texts < 1 || n_texts > SCORE_MAX_TEXTS || !lp || !first || !rec || !out) return false;
    hipLaunchKernelGGL(k_score_finish, dim3(1), dim3(SCORE_FINISH_THREADS), 0, st, lp, first, n_texts, length_norm ? 1 : 0, rec, lp_out, out, tag);
    return true;
}

}} // namespace wmi::k

// The no-speech head for gfx950: the probability of <|nospeech|> in the soft-max of a decoder row's raw logits (kernels.h has the
// definition and the fixed arithmetic).  Two forms of the block pass — logits from HBM, or made on the spot from the f32 residual row and
// the f16 token embedding as k_lang_head makes its hundred — and one combine launch.  A workgroup owns one block of NSP_BLOCK vocabulary
// entries of one row (row = grid.y): nothing is shared between workgroups of a launch, the combine is the next launch on the stream.

#include "kernels.h"
#include "wave_ops.h"
#include "ln_row.h"
#include "nsp_block.h"

#include <cmath>

namespace wmi { namespace k {

namespace {

struct NspScratch { double * s; float * m; float * lnosp; int nb; };
__host__ __device__ __forceinline__ NspScratch nsp_scratch(void * base, int n_vocab) {
    NspScratch r; r.nb = nsp_blocks(n_vocab);
    r.s = (double *) base; r.m = (float *) (r.s + (size_t) NSP_MAX_ROWS * r.nb); r.lnosp = r.m + (size_t) NSP_MAX_ROWS * r.nb;
    return r;
}

__device__ __forceinline__ void nsp_block_store(const NspScratch sc, int y, int blk, int lane, int nosp, float v0, float v1, float m, double s) {
    if (lane == 0) { sc.s[(size_t) y * sc.nb + blk] = s; sc.m[(size_t) y * sc.nb + blk] = m; }
    const int j = nosp - blk * NSP_BLOCK;                    // the block that holds <|nospeech|> also keeps its raw logit
    if (j >= 0 && j < NSP_BLOCK && lane == (j & 63)) sc.lnosp[y] = j < 64 ? v0 : v1;
}

// form 1: one wavefront per (block, row); both loads unconditional from clamped indices
__global__ __launch_bounds__(64) void k_nsp_logits(const float * __restrict__ logits, int ld, const NoSpeechRows rows, int n_vocab, int nosp, void * scratch) {
    const int lane = threadIdx.x, blk = blockIdx.x, y = blockIdx.y;
    const NspScratch sc = nsp_scratch(scratch, n_vocab);
    const float * l = logits + (size_t) rows.row[y] * ld;
    const int i0 = blk * NSP_BLOCK + lane, i1 = i0 + 64;
    const float v0 = l[i0 < n_vocab ? i0 : n_vocab - 1], v1 = l[i1 < n_vocab ? i1 : n_vocab - 1];
    float m; double s;
    nsp_block_partial(v0, i0 < n_vocab, v1, i1 < n_vocab, m, s);
    nsp_block_store(sc, y, blk, lane, nosp, v0, v1, m, s);
}

// form 0: a workgroup of four wavefronts makes the block's 128 logits — wavefront w the rows 32 w .. 32 w + 31 of the block, four at a
// time — with k_lang_head's operations in k_lang_head's order (ln_row_compute on the row, one fmaf chain per lane over (chunk, element),
// the 64-lane sum in the xor order 32 .. 1), parks them in LDS, and its first wavefront takes the block's (max, sum) as form 1 does.
template <int NCH>
__global__ __launch_bounds__(256) void k_nsp_head(const float * __restrict__ x, const float * __restrict__ ln_g, const float * __restrict__ ln_b,
                                                  float eps, int K, const __half * __restrict__ W, int n_vocab, int nosp, void * scratch) {
    constexpr int RIF = 4, PER_WAVE = NSP_BLOCK / 4;
    __shared__ float lg[NSP_BLOCK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int blk = blockIdx.x, y = blockIdx.y;
    float xv[NCH][8], gv[NCH][8], bv[NCH][8], av[NCH][8];
    ln_row_load<NCH>(x + (size_t) y * K, K, lane, xv);
    ln_row_load<NCH>(ln_g, K, lane, gv);
    ln_row_load<NCH>(ln_b, K, lane, bv);
    ln_row_mask<NCH>(xv, K, lane); ln_row_mask<NCH>(gv, K, lane); ln_row_mask<NCH>(bv, K, lane);
    ln_row_compute<NCH>(xv, gv, bv, K, eps, lane, av);
#pragma unroll 2
    for (int it = 0; it < PER_WAVE / RIF; ++it) {
        const int j0 = wave * PER_WAVE + it * RIF, o0 = blk * NSP_BLOCK + j0;
        uint4 w[NCH][RIF];
#pragma unroll
        for (int t = 0; t < NCH; ++t) {
            const int c = lane * 8 + 512 * t, cc = c < K ? c : 0;    // (columns past K: the activation there is exactly 0)
#pragma unroll
            for (int u = 0; u < RIF; ++u) {
                int o = o0 + u; if (o > n_vocab - 1) o = n_vocab - 1;
                w[t][u] = *(const uint4 *) (W + (size_t) o * K + cc);
            }
        }
        float acc[RIF];
#pragma unroll
        for (int u = 0; u < RIF; ++u) acc[u] = 0.0f;
#pragma unroll
        for (int t = 0; t < NCH; ++t)
#pragma unroll
            for (int u = 0; u < RIF; ++u) {
                const __half2 * h = (const __half2 *) &w[t][u];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 f = __half22float2(h[e]);
                    acc[u] = fmaf(f.x, av[t][2 * e], acc[u]);
                    acc[u] = fmaf(f.y, av[t][2 * e + 1], acc[u]);
                }
            }
        _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int u = 0; u < RIF; ++u) acc[u] += WMI_SHX(acc[u], o);
        }
        float v = acc[0];
#pragma unroll
        for (int u = 1; u < RIF; ++u) v = lane == u ? acc[u] : v;
        if (lane < RIF) lg[j0 + lane] = v;
    }
    __syncthreads();
    if (wave != 0) return;
    const NspScratch sc = nsp_scratch(scratch, n_vocab);
    const int i0 = blk * NSP_BLOCK + lane, i1 = i0 + 64;
    const float v0 = lg[lane], v1 = lg[lane + 64];
    float m; double s;
    nsp_block_partial(v0, i0 < n_vocab, v1, i1 < n_vocab, m, s);
    nsp_block_store(sc, y, blk, lane, nosp, v0, v1, m, s);
}

// the combine: one wavefront per row.  Every lane scales the blocks b = lane, lane + 64, .. to the row's maximum and parks the terms in
// LDS; lane 0 adds them in ascending block order.
__global__ __launch_bounds__(64) void k_nsp_combine(void * scratch, int n_vocab, NoSpeechOut * __restrict__ out, int32_t tag) {
    __shared__ double term[NSP_MAX_VOCAB / NSP_BLOCK];
    const int lane = threadIdx.x, y = blockIdx.x;
    const NspScratch sc = nsp_scratch(scratch, n_vocab);
    const float * mb = sc.m + (size_t) y * sc.nb; const double * sb = sc.s + (size_t) y * sc.nb;
    float M = -INFINITY;
    for (int b = lane; b < sc.nb; b += 64) M = fmaxf(M, mb[b]);
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, WMI_SHX(M, o));
    for (int b = lane; b < sc.nb; b += 64) term[b] = sb[b] > 0.0 ? sb[b] * exp((double) (mb[b] - M)) : 0.0;
    __syncthreads();
    if (lane != 0) return;
    double S = 0.0;
    for (int b = 0; b < sc.nb; ++b) S += term[b];
    const float ln = sc.lnosp[y];
    const double p = (ln != -INFINITY && S > 0.0) ? exp((double) (ln - M)) / S : 0.0;
    union { NoSpeechOut o; int2 v; } r;
    r.o.p = (float) p; r.o.tag = tag;
    *(int2 *) (out + y) = r.v;                               // {p, tag} in one store: a record whose tag matches is whole
}

bool nsp_args_ok(int rows, int n_vocab, int nosp) {
    return rows >= 1 && rows <= NSP_MAX_ROWS && n_vocab >= 1 && n_vocab <= NSP_MAX_VOCAB && nosp >= 0 && nosp < n_vocab;
}

} // namespace

size_t no_speech_scratch_bytes(int n_vocab) {
    return (size_t) NSP_MAX_ROWS * nsp_blocks(n_vocab) * (sizeof(double) + sizeof(float)) + NSP_MAX_ROWS * sizeof(float);
}

bool no_speech_logits(const float * logits, int ld, const NoSpeechRows & rows, int n_vocab, int nosp, void * scratch, NoSpeechOut * out, int32_t tag, hipStream_t st) {
    if (!nsp_args_ok(rows.n, n_vocab, nosp)) return false;
    hipLaunchKernelGGL(k_nsp_logits, dim3(nsp_blocks(n_vocab), rows.n), dim3(64), 0, st, logits, ld, rows, n_vocab, nosp, scratch);
    hipLaunchKernelGGL(k_nsp_combine, dim3(rows.n), dim3(64), 0, st, scratch, n_vocab, out, tag);
    return true;
}

bool no_speech_head(const float * x, int rows, int S, const float * ln_g, const float * ln_b, float eps, const __half * te, int n_vocab, int nosp,
                    void * scratch, NoSpeechOut * out, int32_t tag, hipStream_t st) {
    if (!nsp_args_ok(rows, n_vocab, nosp) || !lang_head_usable(S)) return false;
    const dim3 grid(nsp_blocks(n_vocab), rows), block(256);
    switch ((S + 511) / 512) {
        case 1: hipLaunchKernelGGL(k_nsp_head<1>, grid, block, 0, st, x, ln_g, ln_b, eps, S, te, n_vocab, nosp, scratch); break;
        case 2: hipLaunchKernelGGL(k_nsp_head<2>, grid, block, 0, st, x, ln_g, ln_b, eps, S, te, n_vocab, nosp, scratch); break;
        default: hipLaunchKernelGGL(k_nsp_head<3>, grid, block, 0, st, x, ln_g, ln_b, eps, S, te, n_vocab, nosp, scratch); break;
    }
    hipLaunchKernelGGL(k_nsp_combine, dim3(rows), dim3(64), 0, st, scratch, n_vocab, out, tag);
    return true;
}

}} // namespace wmi::k

// LayerNorm of one decoder row in the registers of one wavefront: shared by the kernels whose dot products must carry k_gemv1's bits
// (k_dec.hip: the projections, the language head; k_nospeech.hip: the no-speech head).
#pragma once
#include "kernels.h"
#include "wave_ops.h"

namespace wmi { namespace k {

namespace {

__device__ __forceinline__ float round_f16(float x) { return __half2float(f2h(x)); }

// LayerNorm of one row by one wavefront, lane L holding the slices x[512 t + 8 L .. + 8) (the slices its dot products
// need).  y = f16((x - mean) * rstd * g + b) as separate mul / add (SURVEY App. B rule 6); sums in f32: per lane over
// (t, e) in order, then the 64-lane butterfly.  MAXCH chunks of 512 columns; av[t][e] = 0 outside the row.
// the loads of ln_row_regs: MAXCH chunks of one f32 vector (x, gain or bias), zeros outside the row
template <int MAXCH>
__device__ __forceinline__ void ln_row_load(const float * __restrict__ p, int K, int lane, float (&v)[MAXCH][8]) {
#pragma unroll
    for (int t = 0; t < MAXCH; ++t) {
        // unconditional from a clamped column, masked afterwards: a load inside `if (c < K)` is its own basic block, and the
        // s_waitcnt pass cannot count loads it is not sure were issued — every wait after such a block became vmcnt(0 or 1),
        // i.e. "everything", instead of "the row" 
        // (the mask is ln_row_mask, called where the values are first needed: a select here is a use, i.e. a wait in front of
        // whatever the caller requests next)
        const int c = lane * 8 + 512 * t, cc = c < K ? c : 0;
        const float4 x0 = *(const float4 *) (p + cc), x1 = *(const float4 *) (p + cc + 4);
        v[t][0] = x0.x; v[t][1] = x0.y; v[t][2] = x0.z; v[t][3] = x0.w; v[t][4] = x1.x; v[t][5] = x1.y; v[t][6] = x1.z; v[t][7] = x1.w;
    }
}
template <int MAXCH>
__device__ __forceinline__ void ln_row_mask(float (&v)[MAXCH][8], int K, int lane) {
#pragma unroll
    for (int t = 0; t < MAXCH; ++t) {
        const bool on = lane * 8 + 512 * t < K;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[t][e] = on ? v[t][e] : 0.0f;
    }
}
// the arithmetic of ln_row_regs on loaded values (xv is consumed)
template <int MAXCH>
__device__ __forceinline__ void ln_row_compute(float (&xv)[MAXCH][8], const float (&gv)[MAXCH][8], const float (&bv)[MAXCH][8],
                                               int K, float eps, int lane, float (&av)[MAXCH][8]) {
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < MAXCH; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += xv[t][e];
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) sum += WMI_SHX(sum, o);
    const float mean = sum / (float) K;
    float sq = 0.0f;
#pragma unroll
    for (int t = 0; t < MAXCH; ++t) {
        const bool on = lane * 8 + 512 * t < K;
#pragma unroll
        for (int e = 0; e < 8; ++e) if (on) { xv[t][e] -= mean; sq += xv[t][e] * xv[t][e]; }
    }
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) sq += WMI_SHX(sq, o);
    const float sc = 1.0f / sqrtf(sq / (float) K + eps);
#pragma unroll
    for (int t = 0; t < MAXCH; ++t) {
        const bool on = lane * 8 + 512 * t < K;
#pragma unroll
        for (int e = 0; e < 8; ++e) av[t][e] = on ? round_f16(__fadd_rn(__fmul_rn(xv[t][e] * sc, gv[t][e]), bv[t][e])) : 0.0f;
    }
}

} // namespace

}} // namespace wmi::k

// Frame energies for gfx950: the detector in front of wmi_full_long (kernels.h has the definition).  For every 10 ms frame f of 16 kHz PCM
//   e[f] = sum over i in [160 f, min(160 f + 160, n)) of | x[i] - x[i - 1] |,   x[-1] := 0
// subtraction and |.| in f32, the sum the LEFT-TO-RIGHT f32 sum from 0.0f — the bits of the sequential loop, not of a tree.
// A workgroup stages SEG_STAGE_FRAMES frames into LDS with coalesced 16-byte loads (all four wavefronts), then one lane per frame adds
// its 160 terms in order.  Rows are SEG_ROW = 161 words apart: at 160 every lane of the summing wavefront would sit on banks 0 and 32
// (160 = 5 x 32), at 161 the 64 lanes read 64 consecutive banks modulo 32 — conflict-free for ds_read_b32 (two 32-lane groups).  The
// staging writes are scalar (a 161-word period keeps no row 16-byte aligned) and 4-way conflicted: 160 wave-instructions per workgroup,
// behind the loads they wait for.  The sample in front of a frame is the previous row's last word; in front of the stage it is read from
// global memory by the one lane that needs it (0 at the start of the signal).  The kernel reads 4 bytes per sample once and writes
// 4 bytes per 160 samples: it is bound by HBM, and by nothing else once a few workgroups per CU overlap their two phases.
// Only vector loads and stores.

#include "kernels.h"

#include <cmath>

namespace wmi { namespace k {

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_ROW = SEG_FRAME + 1;                         // odd: see above
constexpr int SEG_STAGE = SEG_STAGE_FRAMES * SEG_FRAME;        // samples of a full stage

__global__ void __launch_bounds__(SEG_THREADS) k_frame_energy(const float * __restrict__ x, int n, float * __restrict__ e, int vec_ok) {
    __shared__ float s[SEG_STAGE_FRAMES * SEG_ROW];
    const long long base = (long long) blockIdx.x * SEG_STAGE;           // (n < 2^31: the product is, the difference below as well)
    const int n_loc = (int) ((long long) n - base < (long long) SEG_STAGE ? (long long) n - base : (long long) SEG_STAGE);   // >= 1 by the grid
    const float * xb = x + base;
    // full 16-byte pieces of the stage, then the up to three samples behind them
    const int n4 = vec_ok ? n_loc >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += SEG_THREADS) {
        const float4 v = *reinterpret_cast<const float4 *>(xb + 4 * i);
        const int q = 4 * i, row = q / SEG_FRAME, col = q - row * SEG_FRAME;     // 160 % 4 == 0: the four samples share a row
        float * d = s + row * SEG_ROW + col;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    for (int q = 4 * n4 + threadIdx.x; q < n_loc; q += SEG_THREADS) {
        const int row = q / SEG_FRAME, col = q - row * SEG_FRAME;
        s[row * SEG_ROW + col] = xb[q];
    }
    __syncthreads();
    const int r = threadIdx.x;
    const int frames = (n_loc + SEG_FRAME - 1) / SEG_FRAME;
    if (r >= frames) return;
    const int len = n_loc - r * SEG_FRAME < SEG_FRAME ? n_loc - r * SEG_FRAME : SEG_FRAME;
    float prev = r > 0 ? s[(r - 1) * SEG_ROW + SEG_FRAME - 1] : base > 0 ? xb[-1] : 0.0f;
    const float * row = s + r * SEG_ROW;
    float acc = 0.0f;
    if (len == SEG_FRAME) {
        _Pragma("unroll 16") for (int i = 0; i < SEG_FRAME; ++i) { const float v = row[i]; acc += fabsf(v - prev); prev = v; }
    } else {
        for (int i = 0; i < len; ++i) { const float v = row[i]; acc += fabsf(v - prev); prev = v; }
    }
    e[(long long) blockIdx.x * SEG_STAGE_FRAMES + r] = acc;
}

} // namespace

bool frame_energy(const float * x, int n, float * e, hipStream_t st) {
    if (!x || !e || n < 1) return false;
    const int grid = (int) (((long long) n + SEG_STAGE - 1) / SEG_STAGE);
    const int vec_ok = ((uintptr_t) x & 15) == 0 ? 1 : 0;                  // a stage is a multiple of 16 bytes: aligned once, aligned in every workgroup
    hipLaunchKernelGGL(k_frame_energy, dim3(grid), dim3(SEG_THREADS), 0, st, x, n, e, vec_ok);
    return hipGetLastError() == hipSuccess;
}

} } // namespace wmi::k

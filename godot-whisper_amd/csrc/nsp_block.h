// The block pass of a soft-max denominator over the vocabulary (kernels.h: NSP_BLOCK), shared by the no-speech head
// (k_nospeech.hip) and the text scorer (k_score.hip): equal logits give equal bits in both.
#pragma once
#include "kernels.h"
#include "wave_ops.h"

#include <cmath>

namespace wmi { namespace k {

__host__ __device__ __forceinline__ int nsp_blocks(int n_vocab) { return (n_vocab + NSP_BLOCK - 1) / NSP_BLOCK; }

// (max, sum) of one block held by one wavefront: lane L has entries L (v0) and L + 64 (v1) of the block, ok* = inside the vocabulary.
// Every lane returns the block's values.
__device__ __forceinline__ void nsp_block_partial(float v0, bool ok0, float v1, bool ok1, float & m_out, double & s_out) {
    float m = fmaxf(ok0 ? v0 : -INFINITY, ok1 ? v1 : -INFINITY);
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, WMI_SHX(m, o));
    // (an entry of -inf adds 0 whatever m is: -inf - -inf is never formed)
    const double e0 = ok0 && v0 != -INFINITY ? exp((double) (v0 - m)) : 0.0;
    const double e1 = ok1 && v1 != -INFINITY ? exp((double) (v1 - m)) : 0.0;
    double s = e0 + e1;
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) s += WMI_SHX(s, o);
    m_out = m; s_out = s;
}

}} // namespace wmi::k

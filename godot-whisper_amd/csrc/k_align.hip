// Token alignment for gfx950: the cross-attention weights of chosen (layer, head) pairs over a teacher-forced pass, normalised per key
// frame, median-filtered along time, averaged over the pairs, and a monotone token-to-frame path through the result by dynamic time
// warping (kernels.h has the definition and the fixed arithmetic).  Five plain launches on one stream: workgroups are
// independent inside every launch, the next step is the next launch.  No atomics: an element of A belongs to one thread, and the pairs
// reach it in ascending (layer, head) order because the launches of the layers are issued in that order.

#include "kernels.h"
#include "wave_ops.h"

#include <cmath>

namespace wmi { namespace k {

namespace {

constexpr int SC_ROWS = 4;                  // query rows per workgroup of the score kernel: one wavefront each in the soft-max

// scores + soft-max.  Workgroup (row tile, head of the layer's list): thread t takes the keys t, t + 256, ..; a key's 64 f16 are read
// once (eight 16-byte loads) and meet the tile's four query rows, which sit in LDS as f32.  s = sum over c ascending of q[c] k[c]: the
// products of two f16 are exact in f32, the sum is a 64-term f32 sum.  Then wavefront r owns row r: m = max s, e = expf(s - m),
// w = e / sum e, over exactly the M keys.
__global__ __launch_bounds__(256) void k_align_scores(const __half * __restrict__ q, int n, int S, const AlignHeads hs, int pair0,
                                                      const __half * __restrict__ kc, int M, float * __restrict__ w, __half * __restrict__ q_out) {
    __shared__ float sq[SC_ROWS][ALIGN_HEAD_DIM];
    __shared__ float ss[SC_ROWS][ALIGN_MAX_M];
    const int tid = threadIdx.x, hi = blockIdx.y, h = hs.head[hi], r0 = blockIdx.x * SC_ROWS;
    {
        const int r = tid >> 6, c = tid & 63, row = r0 + r;
        const __half v = q[(size_t) (row < n ? row : n - 1) * S + ALIGN_HEAD_DIM * h + c];
        sq[r][c] = __half2float(v);
        if (q_out && row < n) q_out[((size_t) (pair0 + hi) * n + row) * ALIGN_HEAD_DIM + c] = v;
    }
    __syncthreads();
    for (int t = tid; t < M; t += 256) {
        const uint4 * kp = (const uint4 *) (kc + (size_t) t * S + ALIGN_HEAD_DIM * h);      // (S and 64 h are multiples of 8 halves: 16-byte aligned)
        float acc[SC_ROWS];
        _Pragma("unroll") for (int r = 0; r < SC_ROWS; ++r) acc[r] = 0.0f;
        _Pragma("unroll") for (int g = 0; g < ALIGN_HEAD_DIM / 8; ++g) {
            const uint4 u = kp[g];
            const __half * kh = (const __half *) &u;
            _Pragma("unroll") for (int e = 0; e < 8; ++e) {
                const float kv = __half2float(kh[e]);
                _Pragma("unroll") for (int r = 0; r < SC_ROWS; ++r) acc[r] = fmaf(sq[r][8 * g + e], kv, acc[r]);
            }
        }
        _Pragma("unroll") for (int r = 0; r < SC_ROWS; ++r) ss[r][t] = acc[r];
    }
    __syncthreads();
    const int r = tid >> 6, lane = tid & 63, row = r0 + r;
    if (row >= n) return;                                    // (a whole wavefront: no barrier below)
    float m = -INFINITY;
    for (int t = lane; t < M; t += 64) m = fmaxf(m, ss[r][t]);
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.0f;
    for (int t = lane; t < M; t += 64) { const float e = expf(ss[r][t] - m); ss[r][t] = e; sum += e; }
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    float * wr = w + ((size_t) hi * n + row) * M;
    for (int t = lane; t < M; t += 64) wr[t] = ss[r][t] / sum;
}

// per (head, key frame): mean and population standard deviation of the weights over all n rows, two passes in f32
__global__ __launch_bounds__(256) void k_align_colstats(const float * __restrict__ w, int n, int M, float * __restrict__ mu, float * __restrict__ sigma) {
    const int t = blockIdx.x * 256 + threadIdx.x, hi = blockIdx.y;
    if (t >= M) return;
    const float * c = w + (size_t) hi * n * M + t;
    float s = 0.0f;
    for (int i = 0; i < n; ++i) s += c[(size_t) i * M];
    const float mean = s / (float) n;
    float v = 0.0f;
    for (int i = 0; i < n; ++i) { const float d = c[(size_t) i * M] - mean; v = fmaf(d, d, v); }
    mu[(size_t) hi * M + t] = mean;
    sigma[(size_t) hi * M + t] = sqrtf(v / (float) n);
}

__device__ __forceinline__ void cswap(float & a, float & b) { const float lo = fminf(a, b), hi = fmaxf(a, b); a = lo; b = hi; }
// the median of seven: a 16-exchange sorting network, the middle element
__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5, float v6) {
    cswap(v0, v6); cswap(v2, v3); cswap(v4, v5); cswap(v0, v2); cswap(v1, v4); cswap(v3, v6); cswap(v0, v1); cswap(v2, v5);
    cswap(v3, v4); cswap(v1, v2); cswap(v4, v6); cswap(v2, v3); cswap(v4, v5); cswap(v1, v2); cswap(v3, v4); cswap(v5, v6);
    return v3;
}

// normalise + median + accumulate: thread (r, t) adds the layer's heads, in the list's order, to its element of A
__global__ __launch_bounds__(256) void k_align_accum(const float * __restrict__ w, const float * __restrict__ mu, const float * __restrict__ sigma,
                                                     int nh, int n, int n_sot, int M, int first, float * __restrict__ A) {
    const int t = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (t >= M) return;
    float a = first ? 0.0f : A[(size_t) r * M + t];
    for (int hi = 0; hi < nh; ++hi) {
        const float * row = w + ((size_t) hi * n + n_sot + r) * M, * m_ = mu + (size_t) hi * M, * s_ = sigma + (size_t) hi * M;
        auto z = [&](int u) { const float sg = s_[u]; return sg == 0.0f ? 0.0f : (row[u] - m_[u]) / sg; };
        if (M <= 3) { a += z(t); continue; }
        float v[7];
        _Pragma("unroll") for (int o = -3; o <= 3; ++o) {
            int u = t + o;
            u = u < 0 ? -u : (u >= M ? 2 * (M - 1) - u : u);            // reflect, the edge sample not repeated (M >= 4: in range)
            v[o + 3] = z(u);
        }
        a += median7(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
    }
    A[(size_t) r * M + t] = a;
}

// A = sum / pairs, and the cost -A diagonal-major: element (r, t) at [r + t][r], so that a DTW diagonal is one contiguous read
__global__ __launch_bounds__(256) void k_align_finish(float * __restrict__ A, int R, int M, int n_pairs, float * __restrict__ cost) {
    const int t = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (t >= M) return;
    const float a = A[(size_t) r * M + t] / (float) n_pairs;
    A[(size_t) r * M + t] = a;
    cost[(size_t) (r + t) * R + r] = -a;
}

// DTW, one workgroup.  Thread i owns row i of D (0: the border row), the sweep goes over the anti-diagonals d = i + j; the two previous
// diagonals sit in LDS (three rotating rows, one barrier per diagonal).  The step bytes go to trace [R][M]; thread 0 walks them back.
__global__ __launch_bounds__(ALIGN_DTW_THREADS) void k_align_dtw(const float * __restrict__ cost, int R, int M, uint8_t * trace,
                                                                 int32_t * __restrict__ path, int32_t * jumps, AlignOut * out, int32_t tag) {
    __shared__ float D[3][ALIGN_DTW_THREADS];
    __shared__ int32_t sj[ALIGN_DTW_THREADS];
    const int i = threadIdx.x;
    sj[i] = -1;
    float * p2 = D[0], * p1 = D[1], * p0 = D[2];             // diagonals d - 2, d - 1, d
    // the cost of this thread's cell on diagonal d: (i - 1, d - i - 1) at [d - 2][i - 1]; loaded one diagonal ahead
    auto cell = [&](int d) { const int j = d - i; return i >= 1 && i <= R && j >= 1 && j <= M; };
    float c_next = 0.0f;
    for (int d = 0; d <= R + M; ++d) {
        const int j = d - i;
        const float c = c_next;
        if (cell(d + 1)) c_next = cost[(size_t) (d - 1) * R + i - 1];
        if (i <= R && j >= 0 && j <= M) {
            float v;
            if (i == 0 || j == 0) v = d == 0 ? 0.0f : INFINITY;
            else {
                const float c0 = p2[i - 1], c1 = p1[i - 1], c2 = p1[i];
                uint8_t s; float best;
                if (c0 < c1 && c0 < c2) { s = 0; best = c0; }
                else if (c1 < c0 && c1 < c2) { s = 1; best = c1; }
                else { s = 2; best = c2; }
                v = c + best;
                trace[(size_t) (i - 1) * M + j - 1] = s;
            }
            p0[i] = v;
        }
        __syncthreads();
        float * const tmp = p2; p2 = p1; p1 = p0; p0 = tmp;
    }
    if (i == 0) {
        int a = R, b = M, k = 0;
        while ((a > 0 || b > 0) && k < R + M) {
            if (a >= 1 && b >= 1) sj[a - 1] = b - 1;           // (the walk only goes down in b inside a row: the last store is the row's first frame)
            if (path) { path[2 * (size_t) (R + M - 1 - k)] = a - 1; path[2 * (size_t) (R + M - 1 - k) + 1] = b - 1; }
            const int s = a == 0 ? 2 : (b == 0 ? 1 : trace[(size_t) (a - 1) * M + b - 1]);
            if (s == 0) { --a; --b; } else if (s == 1) --a; else --b;
            ++k;
        }
        out->n_path = k;
    }
    __syncthreads();
    if (i < R) jumps[i] = sj[i];
    __threadfence_system();
    __syncthreads();
    if (i == 0) out->tag = tag;
}

} // namespace

size_t align_w_floats(int nh, int n, int M)  { return (size_t) nh * n * M; }
size_t align_cost_floats(int R, int M)       { return (size_t) (R + M) * R; }

bool align_shape_ok(int n, int n_sot, int M, int S, int H) {
    return H >= 1 && S == ALIGN_HEAD_DIM * H && n_sot >= 1 && n - n_sot - 1 >= 1 && n - n_sot - 1 <= ALIGN_MAX_R && M >= 1 && M <= ALIGN_MAX_M;
}

bool align_layer(const AlignBufs & b, const __half * q, int n, int S, const __half * kc, int M, const AlignHeads & hs, int pair0, int n_sot,
                 hipStream_t st) {
    if (hs.n < 1 || hs.n > ALIGN_MAX_HEADS || !align_shape_ok(n, n_sot, M, S, S / ALIGN_HEAD_DIM)) return false;
    const int R = n - n_sot - 1;
    k_align_scores<<<dim3((n + SC_ROWS - 1) / SC_ROWS, hs.n), 256, 0, st>>>(q, n, S, hs, pair0, kc, M, b.w, b.q);
    k_align_colstats<<<dim3((M + 255) / 256, hs.n), 256, 0, st>>>(b.w, n, M, b.mu, b.sigma);
    k_align_accum<<<dim3((M + 255) / 256, R), 256, 0, st>>>(b.w, b.mu, b.sigma, hs.n, n, n_sot, M, pair0 == 0 ? 1 : 0, b.A);
    return true;
}

bool align_finish(const AlignBufs & b, int R, int M, int n_pairs, hipStream_t st) {
    if (R < 1 || R > ALIGN_MAX_R || M < 1 || n_pairs < 1) return false;
    k_align_finish<<<dim3((M + 255) / 256, R), 256, 0, st>>>(b.A, R, M, n_pairs, b.cost);
    return true;
}

bool align_dtw(const float * cost, int R, int M, uint8_t * trace, int32_t * path, int32_t * jumps, AlignOut * out, int32_t tag, hipStream_t st) {
    if (R < 1 || R > ALIGN_MAX_R || M < 1) return false;
    k_align_dtw<<<1, ALIGN_DTW_THREADS, 0, st>>>(cost, R, M, trace, path, jumps, out, tag);
    return true;
}

namespace {
__global__ __launch_bounds__(256) void k_align_cost(const float * __restrict__ A, int R, int M, float * __restrict__ cost) {
    const int t = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (t < M) cost[(size_t) (r + t) * R + r] = -A[(size_t) r * M + t];
}
}
void align_cost_from_matrix(const float * A, int R, int M, float * cost, hipStream_t st) {
    k_align_cost<<<dim3((M + 255) / 256, R), 256, 0, st>>>(A, R, M, cost);
}

} } // namespace wmi::k

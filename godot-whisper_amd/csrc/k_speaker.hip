// Channel energies of a stereo clip per centisecond (kernels.h channel_bins; include/wmi_device.h wmi_speaker): ONE pass over the packed
// stereo frames as they lie in HBM — the uploaded bytes of an AudioStreamWAV, or a capture session's resident f32 frames.
//
// replaces: the sample loop of estimate_diarization_speaker (whisper.cpp examples/main/main.cpp:237-268), which walks a host f32 copy of
// both channels once per segment.  Here the samples are read once, per clip, and every segment and token range is a run of table bins
// (speaker_ranges.h has the definition and the host side).
//
// Bin b holds the sums of |x_left| and |x_right| over frames [B(b), min(B(b + 1), n - 1)), B(b) = (b * rate) / 100; behind the nb bins
// stand the two magnitudes of frame n - 1, which no range of the definition counts.
//   integer kinds: exact unsigned 64-bit sums of |v|, v widened BEFORE the absolute value (|-32768| and |-128| do not fit the sample's type)
//   f32:           double sums; every lane adds its pieces in order, then its head and tail sample, then a fixed xor butterfly (32 .. 1):
//                  the order depends on the source's alignment and on nothing else, so a run repeats bit for bit.  No atomics.
//
// A wavefront per bin, RUN consecutive bins per 256-thread workgroup (wave w takes bins w, w + 4, ..).  A bin is a run of SAMPLES
// [2 B(b), 2 f1): a sample's channel is the parity of its index, so the 16-byte pieces need no frame alignment — a source that starts one
// sample off its frame grid only flips which half of a piece is left.  Lanes stride the pieces from the first 16-byte boundary; the
// samples in front of it and behind the last whole piece (fewer than a piece each) go one per lane with sample-sized loads.

#include "kernels.h"

namespace wmi { namespace k {

namespace {

constexpr int BINS_RUN = 8;                                                     // bins per workgroup

template <int KIND> struct BinTraits;
template <> struct BinTraits<SRC_F32_STEREO> { using acc = double; static constexpr int SB = 4; };
template <> struct BinTraits<SRC_S16_STEREO> { using acc = unsigned long long; static constexpr int SB = 2; };
template <> struct BinTraits<SRC_S8_STEREO>  { using acc = unsigned long long; static constexpr int SB = 1; };

__device__ __forceinline__ unsigned mag_s16(uint32_t half) { const int v = (int) (int16_t) (uint16_t) half; return (unsigned) (v < 0 ? -v : v); }
__device__ __forceinline__ unsigned mag_s8(uint32_t byte)  { const int v = (int) (int8_t) (uint8_t) byte;   return (unsigned) (v < 0 ? -v : v); }

// |sample s| of the source, sample-sized load
template <int KIND>
__device__ __forceinline__ typename BinTraits<KIND>::acc sample_mag(const unsigned char * __restrict__ src, long long s) {
    if (KIND == SRC_F32_STEREO) return (typename BinTraits<KIND>::acc) (double) fabsf(((const float *) src)[s]);
    if (KIND == SRC_S16_STEREO) return (typename BinTraits<KIND>::acc) mag_s16(((const uint16_t *) src)[s]);
    return (typename BinTraits<KIND>::acc) mag_s8(src[s]);
}

// the sums of one 16-byte piece: even samples of the piece into e, odd ones into o
template <int KIND>
__device__ __forceinline__ void piece_add(const uint4 v, typename BinTraits<KIND>::acc & e, typename BinTraits<KIND>::acc & o) {
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    if (KIND == SRC_F32_STEREO) {
        e += (double) fabsf(__uint_as_float(w[0])); o += (double) fabsf(__uint_as_float(w[1]));
        e += (double) fabsf(__uint_as_float(w[2])); o += (double) fabsf(__uint_as_float(w[3]));
    } else if (KIND == SRC_S16_STEREO) {
        unsigned pe = 0, po = 0;                                                 // at most 4 * 32768 each
#pragma unroll
        for (int i = 0; i < 4; ++i) { pe += mag_s16(w[i] & 0xffffu); po += mag_s16(w[i] >> 16); }
        e += pe; o += po;
    } else {
        unsigned pe = 0, po = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { pe += mag_s8(w[i] & 0xffu) + mag_s8((w[i] >> 16) & 0xffu); po += mag_s8((w[i] >> 8) & 0xffu) + mag_s8(w[i] >> 24); }
        e += pe; o += po;
    }
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_channel_bins(const unsigned char * __restrict__ src, long long n, long long rate, long long nb,
                                                      typename BinTraits<KIND>::acc * __restrict__ bins) {
    using acc_t = typename BinTraits<KIND>::acc;
    constexpr int SB = BinTraits<KIND>::SB;
    constexpr int PER = 16 / SB;                                                 // samples per piece: 4, 8, 16 (even: a piece keeps the parity)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b0 = (long long) blockIdx.x * BINS_RUN;
    const long long b1 = b0 + BINS_RUN < nb ? b0 + BINS_RUN : nb;
    for (long long b = b0 + wave; b < b1; b += 4) {
        const long long f0 = b * rate / 100;                                     // < n: b < nb
        long long f1 = (b + 1) * rate / 100;
        if (f1 > n - 1) f1 = n - 1;                                              // frame n - 1 enters no range
        const long long s0 = 2 * f0, s1 = 2 * f1;
        acc_t c0 = 0, c1 = 0;                                                    // by channel = parity of the sample index (s0 is even)
        if (s1 > s0) {
            const uintptr_t a = (uintptr_t) src + (uintptr_t) s0 * SB;
            long long head = (long long) (((uintptr_t) 0 - a) & 15) / SB;       // samples in front of the first 16-byte boundary (< PER)
            if (head > s1 - s0) head = s1 - s0;
            const long long body = s0 + head;
            const long long pieces = (s1 - body) / PER;
            const long long tail = body + pieces * PER;
            acc_t e = 0, o = 0;
            const uint4 * p = (const uint4 *) (src + body * SB);
            for (long long q = lane; q < pieces; q += 64) piece_add<KIND>(p[q], e, o);
            const bool flip = (body & 1) != 0;                                   // the pieces start on a right sample
            c0 = flip ? o : e; c1 = flip ? e : o;
            if (lane < head) { const acc_t m = sample_mag<KIND>(src, s0 + lane); if (lane & 1) c1 += m; else c0 += m; }
            if (lane < s1 - tail) { const acc_t m = sample_mag<KIND>(src, tail + lane); if ((tail + lane) & 1) c1 += m; else c0 += m; }
        }
        const acc_t l = wave_sum64(c0), r = wave_sum64(c1);
        if (lane == 0) { bins[2 * b] = l; bins[2 * b + 1] = r; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && n > 0) {
        bins[2 * nb] = sample_mag<KIND>(src, 2 * (n - 1));
        bins[2 * nb + 1] = sample_mag<KIND>(src, 2 * (n - 1) + 1);
    }
}

}  // namespace

long long channel_bins_count(long long n, long long rate) { return n <= 0 || rate <= 0 ? 0 : (100 * n + rate - 1) / rate; }

bool channel_bins(int kind, const void * d_src, long long n, long long rate, void * d_bins, hipStream_t st) {
    if ((kind != SRC_F32_STEREO && kind != SRC_S16_STEREO && kind != SRC_S8_STEREO) || n < 0 || n > INT_MAX || rate <= 0 || rate > INT_MAX) return false;
    if (n == 0) return true;
    if (!d_src || !d_bins) return false;
    const long long nb = channel_bins_count(n, rate);
    const long long groups = (nb + BINS_RUN - 1) / BINS_RUN;
    if (groups > INT_MAX) return false;
    const dim3 grid((unsigned) groups);
    const unsigned char * s = (const unsigned char *) d_src;
    switch (kind) {
        case SRC_F32_STEREO: hipLaunchKernelGGL((k_channel_bins<SRC_F32_STEREO>), grid, dim3(256), 0, st, s, n, rate, nb, (double *) d_bins); break;
        case SRC_S16_STEREO: hipLaunchKernelGGL((k_channel_bins<SRC_S16_STEREO>), grid, dim3(256), 0, st, s, n, rate, nb, (unsigned long long *) d_bins); break;
        default:             hipLaunchKernelGGL((k_channel_bins<SRC_S8_STEREO>), grid, dim3(256), 0, st, s, n, rate, nb, (unsigned long long *) d_bins); break;
    }
    return hipGetLastError() == hipSuccess;
}

}}  // namespace wmi::k

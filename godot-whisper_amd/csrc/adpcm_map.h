// IMA-ADPCM as two chains of clamped additions (include/wmi_device.h wmi_set_wav_adpcm), compiled from this text into the host library
// (wav.cpp: the sequential decoder, wmi_selftest_adpcm_maps), into the kernels (k_adpcm.hip) and into a stand-alone sanitizer program
// (scratch/lab/adpcm_map_asan.cpp).
//
// A nibble n moves the state (predictor, step_index) by
//   step_index' = clamp(step_index + INDEX[n], 0, 88)
//   predictor'  = clamp(predictor + diff(STEP[step_index], n), -32768, 32767)
// Both are maps x -> min(max(x + a, lo), hi) with lo <= hi, written (a, lo, hi).  That family is closed under composition: for f then g
//   g(f(x)) = clamp(clamp(x + a_f, lo_f, hi_f) + a_g, lo_g, hi_g)
//           = clamp(clamp(x + a_f + a_g, lo_f + a_g, hi_f + a_g), lo_g, hi_g)               (adding a_g commutes with a clamp whose bounds move along)
//           = clamp(x + a_f + a_g, clamp(lo_f + a_g, lo_g, hi_g), clamp(hi_f + a_g, lo_g, hi_g))     (a clamp into [l, h], then into [L, H], is the clamp
//                                                                                                into [clamp(l, L, H), clamp(h, L, H)]: clamp is monotone)
// — integer arithmetic without rounding, so the composed map of a run of nibbles gives exactly the state the sequential loop reaches, for
// every entry state.  Composition is associative and not commutative: a run is composed in stream order, and a prefix scan of the chunks'
// maps gives every chunk's entry state.  The index maps depend on the nibbles alone; a chunk's predictor map needs the chunk's entry index.
//
// Widths: the bounds of a composed map lie inside the last clamp's.  The additive term of an index map is at most 8 per nibble (int);
// that of a predictor map is at most 61438 (= 32767 * 15 / 8, rounded down term by term) per nibble in magnitude and passes 2^31 behind
// 35 000 nibbles at the top step: it is kept in 64 bits, which 2^31 nibbles (INT_MAX frames) cannot fill.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define WMI_AD_HD __host__ __device__ inline
#else
#define WMI_AD_HD inline
#endif

namespace wmi { namespace adpcm {

constexpr int IDX_MAX = 88, PRED_MIN = -32768, PRED_MAX = 32767;

struct IdxMap  { int a, lo, hi; };                     // on step_index, domain [0, 88]
struct PredMap { long long a; int lo, hi; };           // on predictor, domain [-32768, 32767]

WMI_AD_HD IdxMap  idx_identity()  { return IdxMap{ 0, 0, IDX_MAX }; }
WMI_AD_HD PredMap pred_identity() { return PredMap{ 0, PRED_MIN, PRED_MAX }; }

WMI_AD_HD long long clampll(long long x, long long lo, long long hi) { return x < lo ? lo : x > hi ? hi : x; }

// the map "f, then g"
WMI_AD_HD IdxMap compose(const IdxMap & f, const IdxMap & g) {
    return IdxMap{ f.a + g.a, (int) clampll((long long) f.lo + g.a, g.lo, g.hi), (int) clampll((long long) f.hi + g.a, g.lo, g.hi) };
}
WMI_AD_HD PredMap compose(const PredMap & f, const PredMap & g) {
    return PredMap{ f.a + g.a, (int) clampll(f.lo + g.a, g.lo, g.hi), (int) clampll(f.hi + g.a, g.lo, g.hi) };
}
WMI_AD_HD int apply(const IdxMap & m, int x)  { return (int) clampll((long long) x + m.a, m.lo, m.hi); }
WMI_AD_HD int apply(const PredMap & m, int x) { return (int) clampll(x + m.a, m.lo, m.hi); }

// STEP[i]: the standard table, held as a function so that host and device read the same text
WMI_AD_HD int step_of(int i) {
    constexpr int16_t STEP[89] = {
        7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173,
        190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066,
        2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818,
        18500, 20350, 22385, 24623, 27086, 29794, 32767 };
    return STEP[i];
}
// INDEX[n] = {-1, -1, -1, -1, 2, 4, 6, 8} twice
WMI_AD_HD int index_of(int n) { return (n & 4) ? 2 * (n & 3) + 2 : -1; }

WMI_AD_HD int diff_of(int step, int n) {               // 32 bits: at step >= 18500 and n & 7 == 7 it passes 32767
    int d = step >> 3;
    if (n & 1) d += step >> 2;
    if (n & 2) d += step >> 1;
    if (n & 4) d += step;
    return (n & 8) ? -d : d;
}

// one nibble as its two maps (the predictor's from the index the nibble is met with)
WMI_AD_HD IdxMap  idx_nibble(int n)             { return IdxMap{ index_of(n), 0, IDX_MAX }; }
WMI_AD_HD PredMap pred_nibble(int index, int n) { return PredMap{ diff_of(step_of(index), n), PRED_MIN, PRED_MAX }; }

// one nibble of the sequential decoder: the definition
WMI_AD_HD void decode_nibble(int n, int & predictor, int & index) {
    const int step = step_of(index);
    index = (int) clampll(index + index_of(n), 0, IDX_MAX);
    predictor = (int) clampll((long long) predictor + diff_of(step, n), PRED_MIN, PRED_MAX);
}

// nibble i of channel c in AudioStreamWAV's layout: the low nibble of a byte first; mono byte k = frames 2k, 2k + 1; stereo byte 2k + c =
// frames 2k, 2k + 1 of channel c
WMI_AD_HD int nibble_at(const unsigned char * bytes, int channels, int c, long long i) {
    const unsigned char b = bytes[(i >> 1) * channels + c];
    return (i & 1) ? b >> 4 : b & 15;
}
WMI_AD_HD long long frames_of(long long n_bytes, bool stereo) { return stereo ? 2 * (n_bytes / 2) : 2 * n_bytes; }

}}  // namespace wmi::adpcm

// Speaker labels from the two channels of a stereo clip (include/wmi_device.h wmi_speaker): the range arithmetic, on the host, over the
// table of centisecond bins that k_channel_bins (k_speaker.hip) writes.  Plain C++ without a device: compiled into the library
// (speaker.cpp) and into a stand-alone sanitizer program (scratch/lab/speaker_ranges_asan.cpp).
//
// replaces: estimate_diarization_speaker / timestamp_to_sample of whisper.cpp's --diarize (examples/main/main.cpp:41-43, 237-268): a host
// loop over every sample of both f32 channels per segment.  Here no sample is read: a range is a run of whole bins.
//
// The definition, for a clip of n frames at `rate` Hz and times t in centiseconds:
//   is(t)     = max(0, min(n - 1, (t * rate) / 100))                     truncating, 64-bit: main.cpp's clamp at any rate
//   E_c       = sum over frames [is(t0), is(t1)) of |x_c|                in double; s16 as v / 32768, s8 as v / 128
//   speaker   = 0 if E_0 > ratio * E_1, else 1 if E_1 > ratio * E_0, else -1 ("?")
// The clamp keeps is(t) <= n - 1 and the end is exclusive, so NO range ever counts frame n - 1.  The table says the same: bin b holds the
// channel sums over frames [B(b), min(B(b + 1), n - 1)), B(b) = (b * rate) / 100, for b < nb = the smallest b with B(b) >= n; the
// magnitudes of frame n - 1 stand behind it on their own (last2) and enter no range.  With is(t) = B(t) wherever the clamp does not bite,
// a range is bins [t0, min(t1, nb)) — additions only, so nothing cancels in the f32 kind.
//   integer kinds: bins are exact unsigned 64-bit sums of |v|; they are added as integers and converted once, double(sum) / 32768 (/ 128):
//                  equal to the reference's sequential double loop bit for bit (every partial sum there is a multiple of 2^-15 below 2^31).
//   f32 kind:      bins are doubles; they are added left to right in double.
#pragma once
#include <cstdint>

namespace wmi { namespace spk {

enum : int { KIND_F32 = 1, KIND_S16 = 3, KIND_S8 = 5 };              // k::SRC_F32_STEREO, SRC_S16_STEREO, SRC_S8_STEREO

struct Range { int speaker; long long is0, is1; double e0, e1; };

// the smallest b with (b * rate) / 100 >= n
inline long long n_bins(long long n, long long rate) { return n <= 0 ? 0 : (100 * n + rate - 1) / rate; }

// is(t); t at or beyond nb is clamped without forming t * rate (which may not fit)
inline long long sample_of(long long t, long long n, long long rate, long long nb) {
    if (n <= 0 || t <= 0) return 0;
    if (t >= nb) return n - 1;
    const long long s = t * rate / 100;                                // t < nb: t * rate < 100 n + rate
    return s < n - 1 ? s : n - 1;
}

inline int label_of(double e0, double e1, double ratio) { return e0 > ratio * e1 ? 0 : e1 > ratio * e0 ? 1 : -1; }

// bins: nb pairs {left, right}, uint64_t for the integer kinds, double for f32 (8 bytes each either way)
inline Range range_eval(const void * bins, long long nb, int kind, long long n, long long rate, double ratio, long long t0, long long t1) {
    Range r{ -1, 0, 0, 0.0, 0.0 };
    if (n <= 0 || rate <= 0) return r;
    if (t0 < 0) t0 = 0;
    if (t1 < 0) t1 = 0;
    r.is0 = sample_of(t0, n, rate, nb);
    r.is1 = sample_of(t1, n, rate, nb);
    const long long hi = t1 < nb ? t1 : nb;
    if (r.is1 > r.is0 && t0 < hi && bins) {
        if (kind == KIND_F32) {
            const double * b = (const double *) bins;
            double e0 = 0.0, e1 = 0.0;
            for (long long i = t0; i < hi; ++i) { e0 += b[2 * i]; e1 += b[2 * i + 1]; }
            r.e0 = e0; r.e1 = e1;
        } else {
            const uint64_t * b = (const uint64_t *) bins;
            uint64_t s0 = 0, s1 = 0;
            for (long long i = t0; i < hi; ++i) { s0 += b[2 * i]; s1 += b[2 * i + 1]; }
            const double scale = kind == KIND_S16 ? 32768.0 : 128.0;
            r.e0 = (double) s0 / scale; r.e1 = (double) s1 / scale;
        }
    }
    r.speaker = label_of(r.e0, r.e1, ratio);
    return r;
}

}}  // namespace wmi::spk

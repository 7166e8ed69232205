// Resampler of the streaming node on the device: the two SINC converters, zero-order hold and linear.
//
// replaces: _resample_audio_buffer (src/speech_to_text.cpp:16-43) -> src_simple(SRC_SINC_FASTEST | SRC_SINC_MEDIUM_QUALITY,
// 1 channel) of libsamplerate (thirdparty/libsamplerate/src/samplerate.c:469-483, src_sinc.c:283-427, 1166-1239).
//
// libsamplerate walks the output sequentially through a ring buffer; at a fixed ratio that machinery reduces to
//   out[n] = float( (float_inc / index_inc) * (left_n + right_n) )
// over the zero-extended input, where output n sits at input position pos_n + frac_n (the recurrence
// x += 1/ratio; frac = x - floor(x) in double), left/right are the two half-filter sums in DOUBLE, taps visited from the
// far end towards the centre, each coefficient linearly interpolated between table entries at a 12-bit fixed-point filter
// index.  One thread computes one output with exactly that operation order (separate f64 multiply and add: the build runs
// under -ffp-contract=off), so the result equals the sequential CPU code bit for bit.
//
// The position recurrence itself is exact — no rounding ever happens — when every partial sum x + 1/ratio stays
// representable on the grid of 1/ratio's last mantissa bit (inc = m * 2^q, inc + 1 <= 2^(q+53): 48 k, 44.1 k, 32 k, 96 k,
// 192 k -> 16 k all qualify).  Then pos_n / frac_n are the integer and fractional part of n * m * 2^q, evaluated per thread
// with a 64 x 64 -> 128-bit product.  Otherwise (e.g. 22.05 k -> 16 k, where sums cross a binade and are rounded) the host
// runs the recurrence once in double, as index bookkeeping, and the kernel reads the (pos, frac) table.
// How many outputs libsamplerate emits depends on its ring-buffer refills and on a termination test evaluated in buffer
// coordinates in double; plan() replays exactly that index state machine (refill to refill, not sample by sample).
//
// SRC_ZERO_ORDER_HOLD and SRC_LINEAR (src_zoh.c:59-126, src_linear.c:61-135) walk the same positions without a ring buffer: output n
// is in[pos_n - 1] held, or in[pos_n - 1] + frac_n * (in[pos_n] - in[pos_n - 1]) with an f32 difference and a separate f64 multiply
// and add; while pos_n is still 0 both give in[0] (their last_value).  They stop at the capacity or when the position runs off the
// input (plan_simple), which is also what keeps every read inside the array.
//
// What an input frame is read from is a template parameter (kernels.h SrcKind, in_frame<KIND>): a mono f32 buffer, the capture session's
// f32 stereo frames, or the packed s16 / s8 frames of an AudioStreamWAV, mono or stereo (wav_frame.h: decode and fold per tap).  Plan,
// positions, tap order and accumulators do not depend on it: the output equals that of a mono f32 buffer decoded first, bit for bit.
// k_resample_split / k_resample_simple_split keep the two channels of a stereo kind apart instead of folding them: one thread, one tap
// walk, two results.

#include "kernels.h"
#include "wav_frame.h"
#include <cmath>
#include <cstring>
#include <algorithm>

extern "C" {
extern const unsigned char wmi_sinc_fastest_bin[];
extern const unsigned char wmi_sinc_medium_bin[];
}

namespace wmi { namespace k {

namespace {

struct ResampleArgs {
    const float * in; long long n_in;
    float * out; long long n_out;
    const float * coeffs; int half_len;
    double float_inc, out_scale;
    int increment;
    unsigned long long m; int sh; double frac_scale;          // closed form: position n = (n * m) >> sh, fraction = low bits * 2^-sh
    const int * pos_tab; const double * frac_tab;             // or the host's recurrence
    const float2 * in2;                                       // SRC_F32_STEREO: the capture frames themselves (in is unused)
    long long n0;                                             // the launch computes outputs [n0, n_out)
    const void * raw;                                         // the packed-frame kinds: the frames as an AudioStreamWAV holds them
};

// f32 stereo frames that start on a 4-byte boundary only (a device source one sample off its frame grid): two loads instead of a float2
constexpr int SRC_F32_STEREO_U = 6;

// input frame i: the mono sample, or the capture frame folded exactly as k_downmix folds it (a float add, then an exact halving) —
// the same bits as a mono buffer written first, without writing one.  The packed integer kinds (SrcKind) decode the frame first
// (wav_frame.h): no f32 image of the input exists anywhere.
template <int KIND>
__device__ __forceinline__ float in_frame(const ResampleArgs & a, long long i) {
    if (KIND == SRC_F32_STEREO) { const float2 f = a.in2[i]; return (float) ((double) (f.x + f.y) / 2.0); }
    if (KIND == SRC_F32_MONO) return a.in[i];
    if (KIND == SRC_F32_STEREO_U) return wav_frame<SRC_F32_STEREO>(a.raw, i);
    return wav_frame<KIND>(a.raw, i);
}

// where output n sits on the input: the host's table, or integer and fractional part of n * m * 2^-sh
__device__ __forceinline__ void out_position(const ResampleArgs & a, long long n, long long * pos_out, double * frac_out) {
    long long pos; double frac;
    if (a.pos_tab) { pos = a.pos_tab[n]; frac = a.frac_tab[n]; }
    else {
        const unsigned long long lo = (unsigned long long) n * a.m, hi = __umul64hi((unsigned long long) n, a.m);
        if (a.sh == 0) { pos = (long long) lo; frac = 0.0; }
        else {
            pos = (long long) ((hi << (64 - a.sh)) | (lo >> a.sh));
            frac = (double) (lo & ((1ull << a.sh) - 1ull)) * a.frac_scale;
        }
    }
    *pos_out = pos; *frac_out = frac;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_resample(const ResampleArgs a) {
    const long long n = a.n0 + (long long) blockIdx.x * 256 + threadIdx.x;
    if (n >= a.n_out) return;
    long long pos; double frac;
    out_position(a, n, &pos, &frac);
    const int increment = a.increment;
    const int start_index = (int) __builtin_rint(frac * a.float_inc * 4096.0);     // double_to_fp, src_sinc.c:71-74
    const int max_index = a.half_len << 12;
    const long long last = a.n_in - 1;
    const float * __restrict__ c = a.coeffs;

    // left half: taps from the far end towards the centre sample, src_sinc.c:293-314
    int fi = start_index;
    int cnt = (max_index - fi) / increment;
    fi += cnt * increment;
    long long di = pos - cnt;
    double left = 0.0;
    do {
        const double fraction = (double) (fi & 4095) * (1.0 / 4096.0);
        const int ix = fi >> 12;
        const float c0 = c[ix], c1 = c[ix + 1];
        const double ic = (double) c0 + fraction * (double) (c1 - c0);
        const long long dc = di < 0 ? 0 : (di > last ? last : di);
        float v = in_frame<KIND>(a, dc);
        v = (di < 0 || di > last) ? 0.0f : v;                 // zero history before the first sample, zero tail after the last
        left += ic * (double) v;
        fi -= increment;
        di += 1;
    } while (fi >= 0);

    // right half, src_sinc.c:316-334
    fi = increment - start_index;
    cnt = (max_index - fi) / increment;
    fi += cnt * increment;
    di = pos + 1 + cnt;
    double right = 0.0;
    do {
        const double fraction = (double) (fi & 4095) * (1.0 / 4096.0);
        const int ix = fi >> 12;
        const float c0 = c[ix], c1 = c[ix + 1];
        const double ic = (double) c0 + fraction * (double) (c1 - c0);
        const long long dc = di > last ? last : di;
        float v = in_frame<KIND>(a, dc);
        v = di > last ? 0.0f : v;
        right += ic * (double) v;
        fi -= increment;
        di -= 1;
    } while (fi > 0);

    a.out[n] = (float) (a.out_scale * (left + right));
}

// SRC_ZERO_ORDER_HOLD (LINEAR = false, src_zoh.c:80, :99) and SRC_LINEAR (src_linear.c:82-83, :107-108).  The plan emits output n only
// while pos_n - 1 (and pos_n for LINEAR) are frames of the input; the clamp keeps a wrong plan from reading outside it.
template <bool LINEAR, int KIND>
__global__ __launch_bounds__(256) void k_resample_simple(const ResampleArgs a) {
    const long long n = a.n0 + (long long) blockIdx.x * 256 + threadIdx.x;
    if (n >= a.n_out) return;
    long long pos; double frac;
    out_position(a, n, &pos, &frac);
    const long long last = a.n_in - 1;
    const long long i0 = pos <= 0 ? 0 : (pos - 1 > last ? last : pos - 1);     // pos 0: last_value = in[0]
    const float v0 = in_frame<KIND>(a, i0);
    if (!LINEAR) { a.out[n] = v0; return; }
    const long long i1 = pos <= 0 ? 0 : (pos > last ? last : pos);
    const float d = in_frame<KIND>(a, i1) - v0;                                               // float difference, then double multiply and add
    a.out[n] = (float) ((double) v0 + frac * (double) d);
}

// The two channels of a stereo kind resampled apart in one launch (kernels.h resample_launch_split): k_resample's thread with two
// accumulator pairs.  What does not depend on the channel is computed once — the position, start_index, the tap walk and every tap's
// interpolated coefficient ic —; each channel's sums then receive exactly the operations k_resample applies to a mono buffer holding that
// channel (the same taps in the same order, the zero history and tail, left half then right half, out_scale * (left + right)), so
// out0 / out1 equal two single-channel launches bit for bit.  A frame's two samples come from one load where the source lies on its frame
// grid (WHOLE, wav_frame.h wav_channel).  a.raw holds the frames of every kind, a.out is out0; a.n0 is not served.
template <int KIND, bool WHOLE>
__global__ __launch_bounds__(256) void k_resample_split(const ResampleArgs a, float * __restrict__ out1) {
    const long long n = (long long) blockIdx.x * 256 + threadIdx.x;
    if (n >= a.n_out) return;
    long long pos; double frac;
    out_position(a, n, &pos, &frac);
    const int increment = a.increment;
    const int start_index = (int) __builtin_rint(frac * a.float_inc * 4096.0);
    const int max_index = a.half_len << 12;
    const long long last = a.n_in - 1;
    const float * __restrict__ c = a.coeffs;

    int fi = start_index;
    int cnt = (max_index - fi) / increment;
    fi += cnt * increment;
    long long di = pos - cnt;
    double left0 = 0.0, left1 = 0.0;
    do {
        const double fraction = (double) (fi & 4095) * (1.0 / 4096.0);
        const int ix = fi >> 12;
        const float c0 = c[ix], c1 = c[ix + 1];
        const double ic = (double) c0 + fraction * (double) (c1 - c0);
        const long long dc = di < 0 ? 0 : (di > last ? last : di);
        float v0, v1;
        wav_channel<KIND, WHOLE>(a.raw, dc, &v0, &v1);
        const bool off = di < 0 || di > last;
        v0 = off ? 0.0f : v0; v1 = off ? 0.0f : v1;
        left0 += ic * (double) v0;
        left1 += ic * (double) v1;
        fi -= increment;
        di += 1;
    } while (fi >= 0);

    fi = increment - start_index;
    cnt = (max_index - fi) / increment;
    fi += cnt * increment;
    di = pos + 1 + cnt;
    double right0 = 0.0, right1 = 0.0;
    do {
        const double fraction = (double) (fi & 4095) * (1.0 / 4096.0);
        const int ix = fi >> 12;
        const float c0 = c[ix], c1 = c[ix + 1];
        const double ic = (double) c0 + fraction * (double) (c1 - c0);
        const long long dc = di > last ? last : di;
        float v0, v1;
        wav_channel<KIND, WHOLE>(a.raw, dc, &v0, &v1);
        v0 = di > last ? 0.0f : v0; v1 = di > last ? 0.0f : v1;
        right0 += ic * (double) v0;
        right1 += ic * (double) v1;
        fi -= increment;
        di -= 1;
    } while (fi > 0);

    a.out[n] = (float) (a.out_scale * (left0 + right0));
    out1[n] = (float) (a.out_scale * (left1 + right1));
}

// k_resample_simple for the two channels: the two frames are read once, each channel gets the hold or the interpolation of its own samples
template <bool LINEAR, int KIND, bool WHOLE>
__global__ __launch_bounds__(256) void k_resample_simple_split(const ResampleArgs a, float * __restrict__ out1) {
    const long long n = (long long) blockIdx.x * 256 + threadIdx.x;
    if (n >= a.n_out) return;
    long long pos; double frac;
    out_position(a, n, &pos, &frac);
    const long long last = a.n_in - 1;
    const long long i0 = pos <= 0 ? 0 : (pos - 1 > last ? last : pos - 1);
    float l0, r0;
    wav_channel<KIND, WHOLE>(a.raw, i0, &l0, &r0);
    if (!LINEAR) { a.out[n] = l0; out1[n] = r0; return; }
    const long long i1 = pos <= 0 ? 0 : (pos > last ? last : pos);
    float l1, r1;
    wav_channel<KIND, WHOLE>(a.raw, i1, &l1, &r1);
    const float dl = l1 - l0, dr = r1 - r0;
    a.out[n] = (float) ((double) l0 + frac * (double) dl);
    out1[n] = (float) ((double) r0 + frac * (double) dr);
}

double frac_one(double x) {                                   // thirdparty/libsamplerate/src/common.h:149-158
    const double r = x - (double) lrint(x);
    return r < 0.0 ? r + 1.0 : r;
}

}  // namespace

bool sinc_table(int converter, const float ** coeffs, int * count, int * increment) {
    const unsigned char * blob = converter == 2 ? wmi_sinc_fastest_bin : converter == 1 ? wmi_sinc_medium_bin : nullptr;
    if (!blob) return false;                                  // SRC_SINC_BEST_QUALITY: its table is a missing blob of the reference checkout
    int32_t hdr[2];
    memcpy(hdr, blob, 8);
    *increment = hdr[0]; *count = hdr[1];
    *coeffs = (const float *) (blob + 8);
    return true;
}

// Positions of the outputs: closed form when the recurrence is exact, else the recurrence itself.
struct Stepper {
    bool closed = false;
    unsigned long long m = 0; int sh = 0;
    std::vector<int> pos_tab; std::vector<double> frac_tab;

    void init(double inc, long long cap) {
        int e = 0;
        const double fr = frexp(inc, &e);                                        // inc = fr * 2^e, fr in [0.5, 1)
        unsigned long long mant = (unsigned long long) ldexp(fr, 53);            // 53-bit integer
        int q = e - 53;
        while ((mant & 1ull) == 0) { mant >>= 1; q += 1; }
        closed = q >= -53 && q <= 10 && inc + 1.0 <= ldexp(1.0, q + 53);
        if (closed) {
            if (q > 0) { mant <<= q; q = 0; }
            m = mant; sh = -q;
            return;
        }
        pos_tab.resize((size_t) cap + 1); frac_tab.resize((size_t) cap + 1);
        double x = 0.0; long long pos = 0;
        for (long long n = 0; n <= cap; ++n) {                                   // src_sinc.c:411-416, literally
            pos_tab[(size_t) n] = (int) pos; frac_tab[(size_t) n] = x;
            x += inc;
            const double rem = frac_one(x);
            pos += lrint(x - rem);
            x = rem;
        }
    }
    void at(long long n, long long * pos, double * frac) const {
        if (!closed) { *pos = pos_tab[(size_t) n]; *frac = frac_tab[(size_t) n]; return; }
        const unsigned __int128 t = (unsigned __int128) (unsigned long long) n * m;
        *pos = (long long) (t >> sh);
        *frac = sh == 0 ? 0.0 : ldexp((double) (unsigned long long) (t & (((unsigned __int128) 1 << sh) - 1)), -sh);
    }
    // smallest k in [lo, cap] with pos_k >= target (cap if none)
    long long first_at_or_past(long long target, long long lo, long long cap) const {
        long long hi = cap;
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            long long p; double f; at(mid, &p, &f);
            if (p >= target) hi = mid; else lo = mid + 1;
        }
        return lo;
    }
};

// libsamplerate's ring-buffer index state machine without the data: how many frames src_simple emits (and consumes).
// Returns the frame count, or < 0: -6 ratio out of range (SRC_ERR_BAD_SRC_RATIO), -21 internal length check
// (SRC_ERR_SINC_PREPARE_DATA_BAD_LEN), -30 ratio beyond what the zero tail of the ring buffer covers.
static long long plan(long long N, long long cap, double ratio, int half_len, int index_inc, const Stepper & P, int hl, int b_len,
                      long long * used) {
    int b_current = 0, b_end = 0, b_real_end = -1;
    long long in_used = 0, n = 0, pos_n = 0;
    const double terminate = 1.0 / ratio + 1e-20;
    auto refill = [&]() -> int {                                                 // src_sinc.c:1166-1239
        if (b_real_end >= 0) return 0;
        int len;
        if (b_current == 0) { len = b_len - 2 * hl; b_current = b_end = hl; }
        else if (b_end + hl + 1 < b_len) len = std::max(b_len - b_current - hl, 0);
        else {
            len = b_end - b_current;
            b_current = hl; b_end = hl + len;
            len = std::max(b_len - b_current - hl, 0);
        }
        len = (int) std::min<long long>(N - in_used, len);
        if (len < 0 || b_end + len > b_len) return -21;
        b_end += len; in_used += len;
        if (in_used == N && b_end - b_current < 2 * hl) {
            if (b_len - b_end < hl + 5) { len = b_end - b_current; b_current = hl; b_end = hl + len; }
            b_real_end = b_end;
            if (b_end + hl + 5 > b_len) return -30;                              // the reference would run its right taps into stale samples
            b_end += hl + 5;
        }
        return 0;
    };
    while (n < cap) {
        if (b_end - b_current <= hl) {
            const int e = refill();
            if (e) return e;
            if (b_end - b_current <= hl) break;
        }
        const int avail = b_end - b_current - hl;                                // outputs go on while the position has advanced by less
        long long stop = P.first_at_or_past(pos_n + avail, n + 1, cap);
        if (b_real_end >= 0) {                                                   // termination test per output, src_sinc.c:389-393
            auto terminated = [&](long long k) {
                long long p; double f; P.at(k, &p, &f);
                const int bc = b_current + (int) (p - pos_n);
                return bc + f + terminate > b_real_end;
            };
            long long lo = n, hi = stop;                                         // first k in [n, stop) that terminates (stop if none)
            while (lo < hi) { const long long mid = lo + (hi - lo) / 2; if (terminated(mid)) hi = mid; else lo = mid + 1; }
            if (lo < stop) { n = lo; break; }
        }
        long long p; double f; P.at(stop, &p, &f);
        b_current += (int) (p - pos_n);
        pos_n = p; n = stop;
    }
    if (used) *used = in_used;
    return n;
}

// src_zoh.c:59-126 / src_linear.c:61-135 for one channel, one call, a constant ratio: the number of frames emitted (and consumed).
// Output n is emitted while n < cap and its position is still on the input: with pos_n == 0 (the converters' first loop)
// ZOH goes on while frac_n < N and LINEAR while 1.0 + frac_n < N; after that ZOH while pos_n + frac_n <= N, LINEAR while
// pos_n + frac_n < N.  Both sums grow with n, so the first output that fails is found by bisection in either part.
// LINEAR leaving its first loop for lack of input enters the second with pos 0 and reads data_in[-1] (one input frame and a
// ratio above 1): nothing to reproduce, answered -31.
static long long plan_simple(long long N, long long cap, bool linear, const Stepper & P, long long * used) {
    *used = 0;
    if (N <= 0) return 0;                                                        // src_zoh.c:44-45, src_linear.c:46-47
    auto first_off = [&](long long lo, long long hi, auto off) {               // first k in [lo, hi) that is off the input (hi if none)
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            long long p; double f; P.at(mid, &p, &f);
            if (off(p, f)) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    const double dN = (double) N;
    const long long head = P.first_at_or_past(1, 0, cap);                        // outputs [0, head) sit before the first input sample
    long long n = first_off(0, head, [&](long long, double f) { return linear ? 1.0 + f >= dN : f >= dN; });
    if (n < head) { if (linear) return -31; }
    else n = first_off(head, cap, [&](long long p, double f) { return linear ? !((double) p + f < dN) : !((double) p + f <= dN); });
    long long p; double f; P.at(n, &p, &f);
    *used = std::min(p, N);
    return n;
}

// One call of src_simple on the device.  d_in / d_out: device pointers (n_in frames in, room for out_cap frames out).
// d_coeffs: the converter's table on the device.  d_pos / d_frac: device scratch for the (pos, frac) table, filled here when
// the recurrence is not exact (may be null when `need_table` comes back false from resample_plan).
ResamplePlan resample_plan(long long n_in, long long out_cap, double ratio, int converter) {
    ResamplePlan pl;
    pl.converter = converter;
    const bool simple = converter == 3 || converter == 4;                                       // SRC_ZERO_ORDER_HOLD, SRC_LINEAR: no table
    const float * coeffs; int count, table_inc;
    if (!simple && !sinc_table(converter, &coeffs, &count, &table_inc)) { pl.error = -10; return pl; }     // SRC_ERR_BAD_CONVERTER
    if (ratio < 1.0 / 256 || ratio > 256.0) { pl.error = -6; return pl; }
    if (n_in < 0) n_in = 0;
    if (out_cap < 0) out_cap = 0;
    if (simple) {
        pl.stepper = std::make_shared<Stepper>();
        pl.stepper->init(1.0 / ratio, out_cap);
        long long used = 0;
        const long long gen = plan_simple(n_in, out_cap, converter == 4, *pl.stepper, &used);
        if (gen < 0) { pl.error = (int) gen; return pl; }
        pl.n_out = gen; pl.n_used = used; pl.need_table = !pl.stepper->closed;
        return pl;
    }
    pl.half_len = count - 2; pl.index_inc = table_inc;
    int b_len = 3 * (int) lrint((pl.half_len + 2.0) / table_inc * 256 + 1);                    // src_sinc.c:213-216
    b_len = std::max(b_len, 4096) + 1;
    double cnt = (pl.half_len + 2.0) / table_inc;
    if (ratio < 1.0) cnt /= ratio;
    const int hl = (int) (lrint(cnt) + 1);
    pl.float_inc = table_inc * (ratio < 1.0 ? ratio : 1.0);
    pl.increment = (int) lrint(pl.float_inc * 4096.0);
    pl.out_scale = pl.float_inc / table_inc;
    pl.stepper = std::make_shared<Stepper>();
    pl.stepper->init(1.0 / ratio, out_cap);
    long long used = 0;
    const long long gen = plan(n_in, out_cap, ratio, pl.half_len, table_inc, *pl.stepper, hl, b_len, &used);
    if (gen < 0) { pl.error = (int) gen; return pl; }
    pl.n_out = gen; pl.n_used = used; pl.need_table = !pl.stepper->closed;
    return pl;
}

void resample_table(const ResamplePlan & pl, const int ** pos, const double ** frac) {
    *pos = pl.stepper->pos_tab.data(); *frac = pl.stepper->frac_tab.data();
}

void resample_positions(const ResamplePlan & pl, long long n, long long * pos, double * frac) {
    for (long long i = 0; i < n; ++i) pl.stepper->at(i, pos + i, frac + i);
}

template <int KIND>
static void launch_as(const ResamplePlan & pl, const dim3 grid, const ResampleArgs & a, hipStream_t st) {
    if (pl.converter == 3) hipLaunchKernelGGL((k_resample_simple<false, KIND>), grid, dim3(256), 0, st, a);
    else if (pl.converter == 4) hipLaunchKernelGGL((k_resample_simple<true, KIND>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_resample<KIND>), grid, dim3(256), 0, st, a);
}

static void launch(const ResamplePlan & pl, int kind, const void * d_src, long long n_in, float * d_out, const float * d_coeffs,
                   const int * d_pos, const double * d_frac, long long first, hipStream_t st) {
    if (first < 0) first = 0;
    if (pl.n_out <= first) return;
    if (kind == SRC_F32_STEREO && ((uintptr_t) d_src & 7)) kind = SRC_F32_STEREO_U;
    ResampleArgs a;
    a.in = kind == SRC_F32_MONO ? (const float *) d_src : nullptr; a.in2 = kind == SRC_F32_STEREO ? (const float2 *) d_src : nullptr;
    a.raw = kind >= SRC_S16_MONO ? d_src : nullptr;
    a.n_in = n_in; a.out = d_out; a.n_out = pl.n_out; a.n0 = first;
    a.coeffs = d_coeffs; a.half_len = pl.half_len;
    a.float_inc = pl.float_inc; a.out_scale = pl.out_scale; a.increment = pl.increment;
    a.m = pl.stepper->m; a.sh = pl.stepper->sh; a.frac_scale = ldexp(1.0, -pl.stepper->sh);
    a.pos_tab = pl.need_table ? d_pos : nullptr; a.frac_tab = pl.need_table ? d_frac : nullptr;
    const dim3 grid((unsigned) ((pl.n_out - first + 255) / 256));
    switch (kind) {
        case SRC_F32_MONO:     launch_as<SRC_F32_MONO>(pl, grid, a, st); break;
        case SRC_F32_STEREO:   launch_as<SRC_F32_STEREO>(pl, grid, a, st); break;
        case SRC_S16_MONO:     launch_as<SRC_S16_MONO>(pl, grid, a, st); break;
        case SRC_S16_STEREO:   launch_as<SRC_S16_STEREO>(pl, grid, a, st); break;
        case SRC_S8_MONO:      launch_as<SRC_S8_MONO>(pl, grid, a, st); break;
        case SRC_S8_STEREO:    launch_as<SRC_S8_STEREO>(pl, grid, a, st); break;
        case SRC_F32_STEREO_U: launch_as<SRC_F32_STEREO_U>(pl, grid, a, st); break;
        default: break;
    }
}

void resample_launch(const ResamplePlan & pl, const float * d_in, long long n_in, float * d_out, const float * d_coeffs,
                     const int * d_pos, const double * d_frac, hipStream_t st) {
    launch(pl, SRC_F32_MONO, d_in, n_in, d_out, d_coeffs, d_pos, d_frac, 0, st);
}

void resample_launch_stereo(const ResamplePlan & pl, const float * d_frames_xy, long long n_in, float * d_out, const float * d_coeffs,
                            const int * d_pos, const double * d_frac, long long first, hipStream_t st) {
    launch(pl, SRC_F32_STEREO, d_frames_xy, n_in, d_out, d_coeffs, d_pos, d_frac, first, st);
}

void resample_launch_kind(const ResamplePlan & pl, int kind, const void * d_src, long long n_in, float * d_out, const float * d_coeffs,
                          const int * d_pos, const double * d_frac, long long first, hipStream_t st) {
    if (kind < SRC_F32_MONO || kind > SRC_S8_STEREO) return;
    launch(pl, kind, d_src, n_in, d_out, d_coeffs, d_pos, d_frac, first, st);
}

template <int KIND, bool WHOLE>
static void launch_split_as(const ResamplePlan & pl, const dim3 grid, const ResampleArgs & a, float * out1, hipStream_t st) {
    if (pl.converter == 3) hipLaunchKernelGGL((k_resample_simple_split<false, KIND, WHOLE>), grid, dim3(256), 0, st, a, out1);
    else if (pl.converter == 4) hipLaunchKernelGGL((k_resample_simple_split<true, KIND, WHOLE>), grid, dim3(256), 0, st, a, out1);
    else hipLaunchKernelGGL((k_resample_split<KIND, WHOLE>), grid, dim3(256), 0, st, a, out1);
}

void resample_launch_split(const ResamplePlan & pl, int kind, const void * d_src, long long n_in, float * out0, float * out1,
                           const float * d_coeffs, const int * d_pos, const double * d_frac, hipStream_t st) {
    if ((kind != SRC_F32_STEREO && kind != SRC_S16_STEREO && kind != SRC_S8_STEREO) || pl.n_out <= 0) return;
    ResampleArgs a;
    a.in = nullptr; a.in2 = nullptr; a.raw = d_src;
    a.n_in = n_in; a.out = out0; a.n_out = pl.n_out; a.n0 = 0;
    a.coeffs = d_coeffs; a.half_len = pl.half_len;
    a.float_inc = pl.float_inc; a.out_scale = pl.out_scale; a.increment = pl.increment;
    a.m = pl.stepper->m; a.sh = pl.stepper->sh; a.frac_scale = ldexp(1.0, -pl.stepper->sh);
    a.pos_tab = pl.need_table ? d_pos : nullptr; a.frac_tab = pl.need_table ? d_frac : nullptr;
    const dim3 grid((unsigned) ((pl.n_out + 255) / 256));
    const bool whole = ((uintptr_t) d_src % (uintptr_t) wav_frame_bytes(kind)) == 0;      // on the frame grid: a frame is one load
    switch (kind) {
        case SRC_F32_STEREO: if (whole) launch_split_as<SRC_F32_STEREO, true>(pl, grid, a, out1, st); else launch_split_as<SRC_F32_STEREO, false>(pl, grid, a, out1, st); break;
        case SRC_S16_STEREO: if (whole) launch_split_as<SRC_S16_STEREO, true>(pl, grid, a, out1, st); else launch_split_as<SRC_S16_STEREO, false>(pl, grid, a, out1, st); break;
        default:             if (whole) launch_split_as<SRC_S8_STEREO, true>(pl, grid, a, out1, st); else launch_split_as<SRC_S8_STEREO, false>(pl, grid, a, out1, st); break;
    }
}

// Output k of a plan does not depend on the input length as long as every frame it reads exists: its position comes from k alone and the
// input is zero-extended, so only a tap past the last frame can change when frames are appended.  The furthest frame output k reads is
// pos_k + 1 + cnt for the SINC converters (the right half starts cnt = (max_index - (increment - start_index)) / increment taps out, bounded
// by max_index / increment + 1) and pos_k for ZOH / LINEAR.  first_dirty = the first output whose reach is not inside the old input, or that
// the old plan had not emitted; a bound, not the exact index (recomputing an unchanged output writes the same bits again).
long long resample_first_dirty(const ResamplePlan & old_pl, long long n_old, const ResamplePlan & new_pl) {
    if (old_pl.error || new_pl.error || !old_pl.stepper || !new_pl.stepper || old_pl.need_table || new_pl.need_table ||
        old_pl.converter != new_pl.converter || old_pl.n_out <= 0) return 0;
    const long long reach = old_pl.converter <= 2 ? ((long long) old_pl.half_len << 12) / std::max(old_pl.increment, 1) + 3 : 1;
    const long long limit = n_old - reach;                                       // outputs with pos_k < limit read existing frames only
    if (limit <= 0) return 0;
    const long long k = new_pl.stepper->first_at_or_past(limit, 0, old_pl.n_out);
    return std::min(std::min(k, old_pl.n_out), new_pl.n_out);
}

}}  // namespace wmi::k

// One frame of an AudioStreamWAV as the mono f32 sample the transcription reads (kernels.h SrcKind): written once for the decode kernel
// (k_wav.hip) and for the resampler's reader (k_resample.hip in_frame), so that both give the same bits.
//   s16: float(v) / 32768, little-endian, v signed        s8: float(v) / 128, v SIGNED (int8_t, never plain char)        f32: as is
// Both divisions are exact in f32 (a power of two under at most 16 significant bits).  A stereo frame is folded as k_downmix folds it: an
// f32 add, then a halving through double.  The integer kinds are read sample by sample: the source needs sample alignment only.
#pragma once
#include <cstdint>
#include "kernels.h"

namespace wmi { namespace k {

#if defined(__HIPCC__)
__device__ __forceinline__ float wav_s16(int16_t v) { return (float) v / 32768.0f; }
__device__ __forceinline__ float wav_s8(int8_t v) { return (float) v / 128.0f; }
__device__ __forceinline__ float wav_fold(float l, float r) { return (float) ((double) (l + r) / 2.0); }

template <int KIND>
__device__ __forceinline__ float wav_frame(const void * __restrict__ src, long long i) {
    if (KIND == SRC_F32_MONO) return ((const float *) src)[i];
    if (KIND == SRC_F32_STEREO) { const float * p = (const float *) src + 2 * i; return wav_fold(p[0], p[1]); }
    if (KIND == SRC_S16_MONO) return wav_s16(((const int16_t *) src)[i]);
    if (KIND == SRC_S16_STEREO) { const int16_t * p = (const int16_t *) src + 2 * i; return wav_fold(wav_s16(p[0]), wav_s16(p[1])); }
    if (KIND == SRC_S8_MONO) return wav_s8(((const int8_t *) src)[i]);
    const int8_t * p = (const int8_t *) src + 2 * i;
    return wav_fold(wav_s8(p[0]), wav_s8(p[1]));
}

// Frame i of a STEREO kind as its two samples, no fold (k_wav.hip k_wav_split, k_resample.hip k_resample_split: the two channels of a
// dialogue kept apart).  WHOLE: `src` lies on the frame grid (frame bytes: 8 / 4 / 2), so the frame is one load; otherwise the source is
// only sample-aligned and each sample is a load of its own.  Either way the same divisions as wav_frame.
template <int KIND, bool WHOLE = false>
__device__ __forceinline__ void wav_channel(const void * __restrict__ src, long long i, float * l, float * r) {
    static_assert(KIND == SRC_F32_STEREO || KIND == SRC_S16_STEREO || KIND == SRC_S8_STEREO, "a stereo kind");
    if (KIND == SRC_F32_STEREO) {
        if (WHOLE) { const float2 f = ((const float2 *) src)[i]; *l = f.x; *r = f.y; }
        else { const float * p = (const float *) src + 2 * i; *l = p[0]; *r = p[1]; }
    } else if (KIND == SRC_S16_STEREO) {
        if (WHOLE) { const uint32_t w = ((const uint32_t *) src)[i]; *l = wav_s16((int16_t) (uint16_t) w); *r = wav_s16((int16_t) (uint16_t) (w >> 16)); }
        else { const int16_t * p = (const int16_t *) src + 2 * i; *l = wav_s16(p[0]); *r = wav_s16(p[1]); }
    } else {
        if (WHOLE) { const uint16_t w = ((const uint16_t *) src)[i]; *l = wav_s8((int8_t) (uint8_t) w); *r = wav_s8((int8_t) (uint8_t) (w >> 8)); }
        else { const int8_t * p = (const int8_t *) src + 2 * i; *l = wav_s8(p[0]); *r = wav_s8(p[1]); }
    }
}
#endif

constexpr int wav_frame_bytes(int kind) {
    return kind == SRC_F32_MONO ? 4 : kind == SRC_F32_STEREO ? 8 : kind == SRC_S16_MONO ? 2 : kind == SRC_S16_STEREO ? 4 : kind == SRC_S8_MONO ? 1 : 2;
}

}}  // namespace wmi::k

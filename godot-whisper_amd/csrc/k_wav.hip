// AudioStreamWAV bytes -> mono f32 at the rate the asset has (kernels.h wav_decode; include/wmi_device.h wmi_wav_*).
//
// replaces: the per-sample GDScript loop of AudioStreamToText.get_text (bin/addons/godot_whisper/audio_stream_to_text.gd:40-46), which
// appends decode_s16(i * 2) / 32768.0 or decode_s8(i * 2) / 128.0 to a PackedFloat32Array one sample at a time — and reads a stereo
// asset as interleaved mono and every second byte only of an 8-bit one.  Here every sample is decoded (wav_frame.h: the same divisions,
// exact in f32) and a stereo frame is folded as k_downmix folds it.
//
// One thread per output group, nothing shared between threads: the launch covers
//   [0, head)                 the frames in front of the first one that starts on a 16-byte boundary, one per thread
//   [head, head + 8 * body)   groups of eight frames, one group per thread: 8 * frame bytes read with 8- or 16-byte loads (the group starts
//                             on a 16-byte boundary, or an 8-byte one for every other group of 8-bit mono)
//   the rest                  fewer than eight frames, one per thread
// and with no frame on a 16-byte boundary at all (a stereo source that starts one sample off its frame grid) body = 0: every frame goes
// the one-per-thread way, whose loads are sample-sized.  The eight results leave as two 16-byte stores when the destination allows.

#include "kernels.h"
#include "wav_frame.h"

namespace wmi { namespace k {

namespace {

constexpr int WAV_GROUP = 8;

// sample s (0 .. per-group count) of a group held in registers as little-endian 32-bit words
template <int KIND>
__device__ __forceinline__ float group_sample(const uint32_t * w, int s) {
    if (KIND == SRC_F32_MONO || KIND == SRC_F32_STEREO) return __uint_as_float(w[s]);
    if (KIND == SRC_S16_MONO || KIND == SRC_S16_STEREO) return wav_s16((int16_t) (uint16_t) (w[s >> 1] >> (16 * (s & 1))));
    return wav_s8((int8_t) (uint8_t) (w[s >> 2] >> (8 * (s & 3))));
}

template <int KIND>
__global__ __launch_bounds__(256) void k_wav_decode(const unsigned char * __restrict__ src, long long n_frames, long long head, long long body,
                                                    float * __restrict__ out) {
    constexpr int FB = wav_frame_bytes(KIND);
    constexpr bool STEREO = KIND == SRC_F32_STEREO || KIND == SRC_S16_STEREO || KIND == SRC_S8_STEREO;
    constexpr int WORDS = WAV_GROUP * FB / 4;                                    // 2 (8-bit mono) .. 16 (f32 stereo)
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t < body) {
        const long long f0 = head + t * WAV_GROUP;
        uint32_t w[WORDS];
        const unsigned char * p = src + f0 * FB;
        if (WORDS == 2) { const uint2 v = *(const uint2 *) p; w[0] = v.x; w[1] = v.y; }
        else {
#pragma unroll
            for (int q = 0; q < WORDS / 4; ++q) { const uint4 v = ((const uint4 *) p)[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
        }
        float r[WAV_GROUP];
#pragma unroll
        for (int j = 0; j < WAV_GROUP; ++j)
            r[j] = STEREO ? wav_fold(group_sample<KIND>(w, 2 * j), group_sample<KIND>(w, 2 * j + 1)) : group_sample<KIND>(w, j);
        float * o = out + f0;
        if (((uintptr_t) o & 15) == 0) {
            ((float4 *) o)[0] = make_float4(r[0], r[1], r[2], r[3]);
            ((float4 *) o)[1] = make_float4(r[4], r[5], r[6], r[7]);
        } else {
#pragma unroll
            for (int j = 0; j < WAV_GROUP; ++j) o[j] = r[j];
        }
        return;
    }
    // the frames around the groups: thread body + i takes frame i of the head, then the frames behind the last group
    const long long i = t - body;
    const long long f = i < head ? i : head + body * WAV_GROUP + (i - head);
    if (f < n_frames) out[f] = wav_frame<KIND>(src, f);
}

// k_wav_decode's scheme for the two channels of a stereo kind kept apart (kernels.h wav_split): the same head / body / tail, every frame
// read once, no fold — out0[f] the left sample, out1[f] the right.  A group's eight pairs leave as two 16-byte stores per destination
// where that destination allows (out0 and out1 are aligned independently), else as eight scalar stores.
__device__ __forceinline__ void store_group(float * o, const float * r) {
    if (((uintptr_t) o & 15) == 0) {
        ((float4 *) o)[0] = make_float4(r[0], r[1], r[2], r[3]);
        ((float4 *) o)[1] = make_float4(r[4], r[5], r[6], r[7]);
    } else {
#pragma unroll
        for (int j = 0; j < WAV_GROUP; ++j) o[j] = r[j];
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_wav_split(const unsigned char * __restrict__ src, long long n_frames, long long head, long long body,
                                                   float * __restrict__ out0, float * __restrict__ out1) {
    constexpr int FB = wav_frame_bytes(KIND);
    constexpr int WORDS = WAV_GROUP * FB / 4;                                    // 4 (8-bit) .. 16 (f32): whole 16-byte pieces
    const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
    if (t < body) {
        const long long f0 = head + t * WAV_GROUP;
        uint32_t w[WORDS];
        const unsigned char * p = src + f0 * FB;
#pragma unroll
        for (int q = 0; q < WORDS / 4; ++q) { const uint4 v = ((const uint4 *) p)[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
        float l[WAV_GROUP], r[WAV_GROUP];
#pragma unroll
        for (int j = 0; j < WAV_GROUP; ++j) { l[j] = group_sample<KIND>(w, 2 * j); r[j] = group_sample<KIND>(w, 2 * j + 1); }
        store_group(out0 + f0, l);
        store_group(out1 + f0, r);
        return;
    }
    // the frames around the groups, as in k_wav_decode; sample-sized loads (the source may be one sample off its frame grid)
    const long long i = t - body;
    const long long f = i < head ? i : head + body * WAV_GROUP + (i - head);
    if (f < n_frames) {
        float l, r;
        wav_channel<KIND>(src, f, &l, &r);
        out0[f] = l; out1[f] = r;
    }
}

}  // namespace

bool wav_split(int kind, const void * d_src, long long n_frames, float * out0, float * out1, hipStream_t st) {
    if ((kind != SRC_F32_STEREO && kind != SRC_S16_STEREO && kind != SRC_S8_STEREO) || n_frames < 0 || (n_frames > 0 && (!d_src || !out0 || !out1))) return false;
    if (n_frames == 0) return true;
    const int fb = wav_frame_bytes(kind);
    long long head = -1;                                                         // as wav_decode: the first frame on a 16-byte boundary
    for (int h = 0; h < 16; ++h) if ((((uintptr_t) d_src + (uintptr_t) h * fb) & 15) == 0) { head = h; break; }
    long long body = 0;
    if (head < 0 || head > n_frames) head = n_frames;
    else body = (n_frames - head) / WAV_GROUP;
    const long long threads = body + (n_frames - body * WAV_GROUP);
    const dim3 grid((unsigned) ((threads + 255) / 256));
    const unsigned char * s = (const unsigned char *) d_src;
    switch (kind) {
        case SRC_F32_STEREO: hipLaunchKernelGGL((k_wav_split<SRC_F32_STEREO>), grid, dim3(256), 0, st, s, n_frames, head, body, out0, out1); break;
        case SRC_S16_STEREO: hipLaunchKernelGGL((k_wav_split<SRC_S16_STEREO>), grid, dim3(256), 0, st, s, n_frames, head, body, out0, out1); break;
        default:             hipLaunchKernelGGL((k_wav_split<SRC_S8_STEREO>), grid, dim3(256), 0, st, s, n_frames, head, body, out0, out1); break;
    }
    return hipGetLastError() == hipSuccess;
}

bool wav_decode(int kind, const void * d_src, long long n_frames, float * out, hipStream_t st) {
    if (kind < SRC_F32_MONO || kind > SRC_S8_STEREO || n_frames < 0 || (n_frames > 0 && (!d_src || !out))) return false;
    if (n_frames == 0) return true;
    const int fb = wav_frame_bytes(kind);
    // the first frame on a 16-byte boundary: frame bytes are a power of two <= 8, so it is among the first 16 frames or nowhere
    long long head = -1;
    for (int h = 0; h < 16; ++h) if ((((uintptr_t) d_src + (uintptr_t) h * fb) & 15) == 0) { head = h; break; }
    long long body = 0;
    if (head < 0 || head > n_frames) head = n_frames;
    else body = (n_frames - head) / WAV_GROUP;
    const long long rest = n_frames - body * WAV_GROUP;                          // head + tail, one thread each
    const long long threads = body + rest;
    const dim3 grid((unsigned) ((threads + 255) / 256));
    const unsigned char * s = (const unsigned char *) d_src;
    switch (kind) {
        case SRC_F32_MONO:   hipLaunchKernelGGL((k_wav_decode<SRC_F32_MONO>), grid, dim3(256), 0, st, s, n_frames, head, body, out); break;
        case SRC_F32_STEREO: hipLaunchKernelGGL((k_wav_decode<SRC_F32_STEREO>), grid, dim3(256), 0, st, s, n_frames, head, body, out); break;
        case SRC_S16_MONO:   hipLaunchKernelGGL((k_wav_decode<SRC_S16_MONO>), grid, dim3(256), 0, st, s, n_frames, head, body, out); break;
        case SRC_S16_STEREO: hipLaunchKernelGGL((k_wav_decode<SRC_S16_STEREO>), grid, dim3(256), 0, st, s, n_frames, head, body, out); break;
        case SRC_S8_MONO:    hipLaunchKernelGGL((k_wav_decode<SRC_S8_MONO>), grid, dim3(256), 0, st, s, n_frames, head, body, out); break;
        default:             hipLaunchKernelGGL((k_wav_decode<SRC_S8_STEREO>), grid, dim3(256), 0, st, s, n_frames, head, body, out); break;
    }
    return hipGetLastError() == hipSuccess;
}

}}  // namespace wmi::k

// IMA-ADPCM bytes of an AudioStreamWAV -> interleaved s16 on the device (kernels.h adpcm_decode; include/wmi_device.h wmi_set_wav_adpcm).
//
// replaces: decoding the clip on the host — in the node a GDScript loop per nibble — and uploading two or four bytes per sample.  The
// decoder's two recurrences are chains of clamped additions, which compose (adpcm_map.h), so each is a prefix scan over chunks of the
// stream; the bytes go up as they are, half a byte per sample.
//
// A thread owns one chunk: ADPCM_CHUNK nibbles of each channel (16 source bytes per channel).  Chunk 0 is the head — the bytes in front of
// the first 16-byte boundary of the source (none when the source starts on one, and in stereo at an odd address, where no chunk can start
// on one: every chunk is then read byte by byte) — so that every full chunk behind it is read with 16-byte loads; the last chunk is the
// tail.  Five launches, queued one behind the other on one stream; inside a launch workgroups are independent, no workgroup waits for another:
//   1 k_adpcm_idx_reduce    every chunk's step-index map, composed over the workgroup: one partial per workgroup and channel
//   2 k_adpcm_scan_parts    one workgroup per channel walks the partials in tiles of ADPCM_PART_TILE: every workgroup's entry index
//   3 k_adpcm_pred_reduce   the index maps again, scanned inside the workgroup from its entry index: every chunk's entry index; with it
//                           the chunk's predictor map (kept, with the index, in a 16-byte record per chunk and channel) and the
//                           workgroup's partial
//   4 k_adpcm_scan_parts    the same walk over the predictor partials: every workgroup's entry predictor
//   5 k_adpcm_write         the records scanned inside the workgroup: every chunk's entry predictor; the chunk is decoded from its entry
//                           state and leaves as 16-byte stores (mono 4, stereo 8 per chunk, the channels interleaved) where the image
//                           allows, else sample by sample
// Scans: Hillis-Steele over the 64 lanes by shuffles, the wavefronts' totals through LDS, composed in stream order (not commutative).

#include "kernels.h"
#include "adpcm_map.h"

namespace wmi { namespace k {

namespace {

using namespace wmi::adpcm;

constexpr int WG = ADPCM_WG, WAVES = WG / 64, C = ADPCM_CHUNK;
static_assert(C == 32 && WG % 64 == 0 && ADPCM_PART_TILE == WG, "the chunk is one 16-byte load per channel; the partials are walked by one workgroup");

struct alignas(16) ChunkRec { long long a; int16_t lo, hi; int32_t index; };       // a chunk's predictor map and its entry index

struct Geo { const unsigned char * src; long long n_used, n_chunks; int head; };   // n_used: bytes that hold frames

// chunk t holds the bytes [b0, b1)
template <int NCH>
__device__ __forceinline__ void chunk_range(const Geo & g, long long t, long long * b0, long long * b1) {
    constexpr int CB = C / 2 * NCH;
    if (t >= g.n_chunks) { *b0 = *b1 = g.n_used; return; }
    const long long lo = t == 0 ? 0 : g.head + (t - 1) * CB, hi = g.head + t * CB;
    *b0 = lo; *b1 = hi < g.n_used ? hi : g.n_used;
}

// the chunk's bytes as little-endian words; a short chunk, or one that is not on a 16-byte boundary, byte by byte (missing bytes: 0)
template <int NCH>
__device__ __forceinline__ void chunk_load(const Geo & g, long long b0, long long b1, uint32_t (&w)[4 * NCH]) {
    constexpr int CB = C / 2 * NCH;
    const unsigned char * p = g.src + b0;
    if (b1 - b0 == CB && ((uintptr_t) p & 15) == 0) {
#pragma unroll
        for (int q = 0; q < NCH; ++q) { const uint4 v = ((const uint4 *) p)[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
        return;
    }
#pragma unroll
    for (int q = 0; q < 4 * NCH; ++q) w[q] = 0;
#pragma unroll
    for (int i = 0; i < CB; ++i) if (b0 + i < b1) w[i >> 2] |= (uint32_t) p[i] << (8 * (i & 3));
}

// nibble i (compile-time under the unrolled loops) of channel c of the chunk
template <int NCH>
__device__ __forceinline__ int chunk_nibble(const uint32_t (&w)[4 * NCH], int c, int i) {
    const int b = (i >> 1) * NCH + c;
    return (int) ((w[b >> 2] >> (8 * (b & 3) + 4 * (i & 1))) & 15u);
}

template <int NCH>
__device__ __forceinline__ IdxMap chunk_idx_map(const uint32_t (&w)[4 * NCH], int c, int n_nib) {
    IdxMap m = idx_identity();
#pragma unroll
    for (int i = 0; i < C; ++i) if (i < n_nib) m = compose(m, idx_nibble(chunk_nibble<NCH>(w, c, i)));
    return m;
}

__device__ __forceinline__ IdxMap shfl_up_map(const IdxMap & m, int o) { return IdxMap{ __shfl_up(m.a, o), __shfl_up(m.lo, o), __shfl_up(m.hi, o) }; }
__device__ __forceinline__ PredMap shfl_up_map(const PredMap & m, int o) { return PredMap{ __shfl_up(m.a, o), __shfl_up(m.lo, o), __shfl_up(m.hi, o) }; }

// The maps of the workgroup's threads in thread order: returns the composition of those in front of this thread (the identity for
// thread 0), *total = the composition of all.  tot: LDS room for WAVES maps.  Every thread of the workgroup calls it.
template <typename M>
__device__ __forceinline__ M block_scan_excl(M v, const M ident, M * tot, M * total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const M u = shfl_up_map(v, o); if (lane >= o) v = compose(u, v); }
    if (lane == 63) tot[wave] = v;
    M ex = shfl_up_map(v, 1);
    if (lane == 0) ex = ident;
    __syncthreads();
    M pre = ident, all = ident;
#pragma unroll
    for (int q = 0; q < WAVES; ++q) { const M t = tot[q]; if (q < wave) pre = compose(pre, t); all = compose(all, t); }
    __syncthreads();                                                       // tot may be written again
    *total = all;
    return compose(pre, ex);
}

template <int NCH>
__global__ __launch_bounds__(WG) void k_adpcm_idx_reduce(Geo g, IdxMap * __restrict__ part) {
    __shared__ IdxMap tot[WAVES];
    const long long t = (long long) blockIdx.x * WG + threadIdx.x;
    long long b0, b1;
    chunk_range<NCH>(g, t, &b0, &b1);
    uint32_t w[4 * NCH];
    chunk_load<NCH>(g, b0, b1, w);
    const int n_nib = (int) ((b1 - b0) / NCH) * 2;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        IdxMap all;
        (void) block_scan_excl(chunk_idx_map<NCH>(w, c, n_nib), idx_identity(), tot, &all);
        if (threadIdx.x == 0) part[(size_t) blockIdx.x * NCH + c] = all;
    }
}

// entry[i * nch + c] = the state in front of workgroup i of channel c = blockIdx.x, from the state 0 in front of the stream
template <typename M>
__global__ __launch_bounds__(WG) void k_adpcm_scan_parts(const M * __restrict__ part, int n_groups, int nch, M ident, int * __restrict__ entry) {
    __shared__ M tot[WAVES];
    const int c = blockIdx.x;
    int carry = 0;
    for (int base = 0; base < n_groups; base += WG) {                      // (uniform: every thread makes every pass)
        const int i = base + threadIdx.x;
        M all;
        const M ex = block_scan_excl(i < n_groups ? part[(size_t) i * nch + c] : ident, ident, tot, &all);
        if (i < n_groups) entry[(size_t) i * nch + c] = apply(ex, carry);
        carry = apply(all, carry);
    }
}

template <int NCH>
__global__ __launch_bounds__(WG) void k_adpcm_pred_reduce(Geo g, const int * __restrict__ entry_idx, ChunkRec * __restrict__ recs,
                                                          PredMap * __restrict__ part) {
    __shared__ IdxMap tot_i[WAVES];
    __shared__ PredMap tot_p[WAVES];
    const long long t = (long long) blockIdx.x * WG + threadIdx.x;
    long long b0, b1;
    chunk_range<NCH>(g, t, &b0, &b1);
    uint32_t w[4 * NCH];
    chunk_load<NCH>(g, b0, b1, w);
    const int n_nib = (int) ((b1 - b0) / NCH) * 2;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        IdxMap all_i;
        const IdxMap ex = block_scan_excl(chunk_idx_map<NCH>(w, c, n_nib), idx_identity(), tot_i, &all_i);
        const int index0 = apply(ex, entry_idx[(size_t) blockIdx.x * NCH + c]);
        int index = index0;
        PredMap m = pred_identity();
#pragma unroll
        for (int i = 0; i < C; ++i) if (i < n_nib) {
            const int n = chunk_nibble<NCH>(w, c, i);
            m = compose(m, pred_nibble(index, n));
            index = apply(idx_nibble(n), index);
        }
        if (t < g.n_chunks) recs[(size_t) t * NCH + c] = ChunkRec{ m.a, (int16_t) m.lo, (int16_t) m.hi, index0 };
        PredMap all_p;
        (void) block_scan_excl(m, pred_identity(), tot_p, &all_p);
        if (threadIdx.x == 0) part[(size_t) blockIdx.x * NCH + c] = all_p;
    }
}

template <int NCH>
__global__ __launch_bounds__(WG) void k_adpcm_write(Geo g, const ChunkRec * __restrict__ recs, const int * __restrict__ entry_pred,
                                                    int16_t * __restrict__ out) {
    __shared__ PredMap tot[WAVES];
    constexpr int CB = C / 2 * NCH;
    const long long t = (long long) blockIdx.x * WG + threadIdx.x;
    long long b0, b1;
    chunk_range<NCH>(g, t, &b0, &b1);
    uint32_t w[4 * NCH];
    chunk_load<NCH>(g, b0, b1, w);
    const int n_nib = (int) ((b1 - b0) / NCH) * 2;
    uint32_t o[C / 2 * NCH];                                               // the chunk's samples, interleaved, two per word
#pragma unroll
    for (int q = 0; q < C / 2 * NCH; ++q) o[q] = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        PredMap m = pred_identity();
        int index = 0;
        if (t < g.n_chunks) { const ChunkRec r = recs[(size_t) t * NCH + c]; m = PredMap{ r.a, r.lo, r.hi }; index = r.index; }
        PredMap all;
        const PredMap ex = block_scan_excl(m, pred_identity(), tot, &all);
        int pred = apply(ex, entry_pred[(size_t) blockIdx.x * NCH + c]);
#pragma unroll
        for (int i = 0; i < C; ++i) if (i < n_nib) {
            decode_nibble(chunk_nibble<NCH>(w, c, i), pred, index);
            const int s = i * NCH + c;                                     // the sample's place in the chunk's image
            o[s >> 1] |= ((uint32_t) pred & 0xffffu) << (16 * (s & 1));
        }
    }
    int16_t * dst = out + b0 / NCH * 2 * NCH;                              // byte pair k of a channel = frames 2k, 2k + 1
    if (b1 - b0 == CB && ((uintptr_t) dst & 15) == 0) {
#pragma unroll
        for (int q = 0; q < C / 8 * NCH; ++q) ((uint4 *) dst)[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    } else {
#pragma unroll
        for (int s = 0; s < C * NCH; ++s) if (s < n_nib * NCH) dst[s] = (int16_t) (uint16_t) (o[s >> 1] >> (16 * (s & 1)));
    }
}

struct Scratch { ChunkRec * recs; IdxMap * part_i; PredMap * part_p; int * entry_i, * entry_p; };

size_t up256(size_t n) { return (n + 255) & ~(size_t) 255; }

// the scratch's pieces for at most `chunks` chunks; returns the bytes they take
size_t scratch_carve(void * base, long long chunks, int nch, Scratch * s) {
    const size_t groups = (size_t) ((chunks + WG - 1) / WG);
    size_t off = 0;
    unsigned char * p = (unsigned char *) base;
    s->recs = (ChunkRec *) (p + off);   off += up256((size_t) chunks * nch * sizeof(ChunkRec));
    s->part_p = (PredMap *) (p + off);  off += up256(groups * nch * sizeof(PredMap));
    s->part_i = (IdxMap *) (p + off);   off += up256(groups * nch * sizeof(IdxMap));
    s->entry_i = (int *) (p + off);     off += up256(groups * nch * sizeof(int));
    s->entry_p = (int *) (p + off);     off += up256(groups * nch * sizeof(int));
    return off;
}

long long chunks_bound(long long n_bytes, bool stereo) { return 2 + n_bytes / (C / 2 * (stereo ? 2 : 1)); }     // head + full chunks + tail

template <int NCH>
bool launch_all(const Geo & g, const Scratch & s, int16_t * d_out, hipStream_t st) {
    const int groups = (int) ((g.n_chunks + WG - 1) / WG);
    hipLaunchKernelGGL((k_adpcm_idx_reduce<NCH>), dim3((unsigned) groups), dim3(WG), 0, st, g, s.part_i);
    hipLaunchKernelGGL((k_adpcm_scan_parts<IdxMap>), dim3(NCH), dim3(WG), 0, st, (const IdxMap *) s.part_i, groups, NCH, idx_identity(), s.entry_i);
    hipLaunchKernelGGL((k_adpcm_pred_reduce<NCH>), dim3((unsigned) groups), dim3(WG), 0, st, g, (const int *) s.entry_i, s.recs, s.part_p);
    hipLaunchKernelGGL((k_adpcm_scan_parts<PredMap>), dim3(NCH), dim3(WG), 0, st, (const PredMap *) s.part_p, groups, NCH, pred_identity(), s.entry_p);
    hipLaunchKernelGGL((k_adpcm_write<NCH>), dim3((unsigned) groups), dim3(WG), 0, st, g, (const ChunkRec *) s.recs, (const int *) s.entry_p, d_out);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

size_t adpcm_scratch_bytes(long long n_bytes, bool stereo) {
    Scratch s;
    return scratch_carve(nullptr, chunks_bound(n_bytes, stereo), stereo ? 2 : 1, &s);
}

AdpcmPlan adpcm_plan(const void * d_src, long long n_bytes, bool stereo) {
    AdpcmPlan p;
    const int nch = stereo ? 2 : 1, cb = C / 2 * nch;
    p.n_used = stereo ? n_bytes & ~1ll : n_bytes;
    p.frames = frames_of(n_bytes, stereo);
    // the head: the bytes in front of the first chunk start (a whole byte pair in stereo) on a 16-byte boundary; none there: every chunk by bytes
    long long head = 0;
    for (int h = 0; h < 16; h += nch) if ((((uintptr_t) d_src + (uintptr_t) h) & 15) == 0) { head = h; break; }
    if (head > p.n_used) head = p.n_used;
    p.head = (int) head;
    p.n_chunks = 1 + (p.n_used - head + cb - 1) / cb;
    p.out_skew = (int) ((16 - (4 * head) % 16) % 16 / 2);
    return p;
}

bool adpcm_decode(const AdpcmPlan & p, const void * d_src, bool stereo, int16_t * d_out, void * d_scratch, hipStream_t st) {
    if (p.frames < 0 || (p.frames > 0 && (!d_src || !d_out || !d_scratch))) return false;
    if (p.frames == 0) return true;
    Scratch s;
    (void) scratch_carve(d_scratch, p.n_chunks, stereo ? 2 : 1, &s);       // (p.n_chunks <= the bound adpcm_scratch_bytes sizes for)
    const Geo g{ (const unsigned char *) d_src, p.n_used, p.n_chunks, p.head };
    return stereo ? launch_all<2>(g, s, d_out, st) : launch_all<1>(g, s, d_out, st);
}

}}  // namespace wmi::k

// Launch prototypes of the gfx950 kernels (definitions in k_*.hip).
// Conventions: activations are token-major ([row][feature], feature contiguous); every matrix
// operand is K-contiguous; f16 = IEEE half (the reference's rounding points).
#pragma once
#include <memory>
#include <vector>
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <atomic>
#include <cstdint>
#include "grammar_eval.h"

namespace wmi { namespace k {

// Kernels with more than 48 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize once per device (a context per
// GPU, launches from several host threads).  The attribute is set to the whole 160 KB of a CU — it permits, the launch decides —
// so it never depends on the sizes seen so far; `mask` = one bit per device, one static per kernel instantiation.
inline void allow_full_lds(const void * kernel, std::atomic<uint64_t> & mask) {
    int dev = 0;
    (void) hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (mask.load(std::memory_order_acquire) & bit) return;
    (void) hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    mask.fetch_or(bit, std::memory_order_release);        // two threads may both set it: idempotent
}

// f32 -> f16 with the value pinned in a register first.  Without the empty asm the AMDGPU back end folds SOME of the
// `cvt(mul)` / `cvt(add)` pairs of an unrolled epilogue into v_fma_mixlo_f16 — one rounding instead of the reference's
// two (f32 op, then f16 store) — and which elements get the fused form depends on their slot in the tile, so identical
// inputs gave results that differed in the last f16 bit with the position of a row in M (found by the lock-step
// bit-exactness test; scratch/lab/pos_test.hip reproduces it).  -ffp-contract=off does not stop this fold.
#if defined(__HIPCC__)
__device__ __forceinline__ float pin_f32(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ __half f2h(float x) { return __float2half_rn(pin_f32(x)); }
// Time index inside an encoder V^T row ([S][Tpad], written by the q|k|v GEMM epilogues, read only by the encoder attention): bits 2
// and 3 of t are swapped, i.e. within every 16 keys the four-key groups sit in the order 0, 2, 1, 3.  A lane of the 32x32x16 MFMA
// holds the soft-max numerators of keys 8j + 4g + r (g = lane / 32): with this order the eight V values that pair with them —
// keys {4g..4g+3} and {8+4g..8+4g+3} of a 16-key slice — are ONE aligned 16-byte piece, so the tile goes global -> LDS by DMA
// untouched and a fragment is a single ds_read_b128.
__host__ __device__ __forceinline__ int vt_pos(int t) { return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1); }
#endif

// Compute units of the CURRENT device, rounded down to a multiple of the 8 XCDs (persistent grids: one workgroup per CU).  One slot per
// device ordinal — a process may hold contexts on several GPUs (wmi_pool_*), and a count cached from the first device a kernel saw
// would size the grids of all the others.
inline int cu_count_x8() {
    static std::atomic<int> cache[64];
    int dev = 0;
    (void) hipGetDevice(&dev);
    std::atomic<int> & c = cache[dev & 63];
    int n = c.load(std::memory_order_relaxed);
    if (n > 0) return n;
    n = 256;
    (void) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    n = n > 8 ? n & ~7 : 8;
    c.store(n, std::memory_order_relaxed);
    return n;
}

// Kernel arguments, all requested at the kernel's first instructions.  hipcc places the s_load of a by-value argument struct's field in
// the basic block that first uses it: a kernel with early branches (probe switch, helper workgroups, optional operands) walks through
// half a dozen DEPENDENT scalar-load round trips to the kernarg segment (~0.25-0.3 us each, cold in the scalar cache at every launch)
// before its first vector load goes out — 1.7 us of a 5.8 us launch in k_qrows (in-kernel stamps, profiles/r05c_*).  Naming a field as an
// asm input makes it live here, so the loads of everything named leave together and one wait covers them.
// The hot kernels (k_front, k_mlp_pair, k_gemv1, k_xback, k_gemm, k_filter_pick) go one step further: the operands of their first
// loads are plain leading parameters, which arrive in SGPRs with the wavefront (kernarg preload, csrc/Makefile: 13 - 14 dwords; a by-value
// struct in front gets none), followed by the argument struct by value for everything else.  The launchers pass both from the same host
// struct; tests/test_kernarg_preload.py holds the layouts.
#if defined(__HIPCC__)
#define WMI_ARG_NOW(x) asm volatile("" :: "s"(x))
#endif

// ---------------------------------------------------------------- in-kernel time stamps (probe: wmi_step_stamps)
// Body / boundary split of a dependent chain of launches: when stamping is on, lane 0 of every wavefront of a stamped launch
// writes (s_memrealtime at its first instruction, s_memrealtime behind its last store) to
// base[(slot * STAMP_WAVES + wave index) * 4] (+ two optional mid points); the host takes min start / max end per launch.  Off (base == null) costs one
// scalar compare per kernel.  The launchers draw their slot from stamp_next() in launch order; the switch is THREAD-LOCAL: only launches
// enqueued by the thread that called stamp_enable() are stamped (pool workers and replica contexts launching beside a probe see "off").
constexpr int STAMP_WAVES = 4096;                       // wavefront records per launch
struct Stamp { unsigned long long * base; int slot; };
void  stamp_enable(unsigned long long * base);          // null = off; resets the slot counter
Stamp stamp_next();                                     // {base, slot++} or {null, 0}
int   stamp_count();
#if defined(__HIPCC__)
__device__ __forceinline__ unsigned long long stamp_t0(const unsigned long long * base) { return base ? wall_clock64() : 0ull; }
// the first stamp of a kernel whose leading arguments are preloaded: `on` = (base != null) travels as a bit of a preloaded word (STAMP_ON_BIT
// of its `dims`), so the kernel's first instructions do not wait for Stamp, which sits behind the preloaded dwords in the argument segment
constexpr uint32_t STAMP_ON_BIT = 1u << 31;
__device__ __forceinline__ unsigned long long stamp_t0_if(bool on) { return on ? wall_clock64() : 0ull; }
__device__ __forceinline__ void stamp_end(unsigned long long * base, int slot, int widx, unsigned long long t0,
                                          unsigned long long tm1 = 0, unsigned long long tm2 = 0) {
    if (base && (threadIdx.x & 63) == 0 && widx < STAMP_WAVES) {
        unsigned long long * s = base + ((size_t) slot * STAMP_WAVES + widx) * 4;       // start, two optional mid points, end
        s[0] = t0; s[1] = wall_clock64(); s[2] = tm1; s[3] = tm2;
    }
}
#endif

// ---------------------------------------------------------------- mel (k_mel.hip)
// pcm_pad: [200 reflect | n_samples | zeros] ; frames [0, n_fft_frames) get an FFT, the rest up to
// n_len the constant log10(1e-10).  mel: [n_mel][n_len] f32.  gmax: ordered-int encoded running max.
void mel_pad(const float * pcm, int n_samples, float * pcm_pad, int n_pad_total, hipStream_t st, int * gmax_reset);   // also resets mel_frames' gmax
void mel_frames(const float * pcm_pad, int n_valid, int n_fft_frames, int n_len, int n_mel,
                const float * filters, const int32_t * ranges, const float * taps, float * mel, int * gmax, hipStream_t st);
void mel_normalize(float * mel, int n, const int * gmax, hipStream_t st);
// lock-step chunks (batch.cpp): the mel kernels and the envelope kernel of up to 16 chunks in ONE launch each — per chunk the samples
// (device), the padded image, the mel image, the running-maximum word and the envelope with its block extrema
struct MelBatch { const float * pcm[16]; float * pad[16]; float * mel[16]; int * gmax[16]; float * energy[16]; float * bmin[16]; float * bmax[16]; int n[16]; };
void mel_batch(const MelBatch & b, int nb, int n_mel, const float * filters, const int32_t * ranges, const float * taps, hipStream_t st);
void signal_energy_batch(const MelBatch & b, int nb, int hw, hipStream_t st);
// token-major f16 slice for the conv front-end: out[r][c], r in [0, rows_total), row r holds frame
// (offset + r - 1); rows outside [1, n_frames] and frames >= n_len are zero.
// lock-step chunks: the slices of up to 16 chunks in one launch (chunk c -> rows c * rows_total ..), and the guard rows between stacked chunks
struct MelSliceBatch { const float * mel[16]; int n_len[16]; int offset[16];
                       int n_frames[16]; };                  // > 0: chunk c takes that many frames (an encoder length of its own), 0: the launch's n_frames
void mel_slice_batch(const MelSliceBatch & mb, int nb, int n_mel, int n_frames, __half * out, int ld, int rows_total, hipStream_t st);
void fill_zero_strided(void * p, size_t bytes, size_t stride_bytes, int count, hipStream_t st);
// Lock-step chunks with an encoder length of their own (batch.cpp encode_rows): t[z] = encoder length of chunk row z.  n = 0: every
// chunk has the launch's common length (the kernels then are what they were).  Passed by value: no allocation, nothing for a replay to miss.
struct RowLens { int n; int t[16]; };
// zeros with a start of its own per run: run c (< count <= 16) zeroes p + c * stride_bytes + [first_row.t[c] * row_bytes, end_bytes) — the conv1
// rows behind each chunk's own 2 T + 1 rows, up to and including the next chunk's guard row
void fill_zero_tails(void * p, const RowLens & first_row, size_t row_bytes, size_t end_bytes, size_t stride_bytes, int count, hipStream_t st);
void mel_slice(const float * mel, int n_len, int n_mel, int offset, int n_frames, __half * out, int ld,
               int rows_total, hipStream_t st);

// |x| envelope for the token-level timestamp heuristics (W/whisper.cpp:6352-6366), bit-identical to the CPU loop
// out[n] plus the minimum / maximum of each 256-sample block of out (bmin, bmax: ceil(n / 256) entries)
void signal_energy(const float * pcm, int n, int hw, float * out, float * bmin, float * bmax, hipStream_t st);
// Token-level timestamps, the envelope side (W/whisper.cpp:6500-6590, csrc/full.cpp token_level_timestamps): per token the sequential f32 sum of
// the envelope over its window, the threshold, and the four walks the reference may take from the token's start / end sample.  One
// wavefront per token; every result equals the host loop's (sequential sum in index order; walks stop on the same sample).
struct TsTok { int32_t s0, s1, a0, a1;                      // start / end sample of the token, window [a0, a1) of the sum
               const float * en; int32_t n_samples, ext_off; };   // optional (en != null): this token's own envelope, its length, and the offset of its block minima (maxima: + n_samples / 256 + 2) — tokens of several chunks in one launch
struct TsOut { float sum, thold; int32_t e0, e1;            // e0 = en[s0] > thold, e1 = en[s1] > thold
               int32_t w_down_above_s0, w_up_below_s0, w_up_above_s1, w_down_below_s1; };   // walk results (bounds: 0, s1, n - 1, 0)
void ts_refine(const float * en, const float * bmin, const float * bmax, int n_samples, const TsTok * in, TsOut * out, int n_tok, hipStream_t st);
// device -> pinned host (or anywhere) by `wgs` workgroups only: a deliberately slow copy that keeps the PCIe write queue short

// host-adjacent DSP of the streaming node: stereo -> mono and the energy VAD, bit-identical to the host's C++
// (src/speech_to_text.cpp:45-51, 53-104).  res = {no-activity decision, energy_all, energy_last}
void downmix_stereo(const float * frames, int n_frames, float * out, hipStream_t st);
void vad_window(const float * x, int n, int n_last, float alpha, bool filter, float vad_thold, float * res, hipStream_t st);
// The same answer bit for bit with the filter cut into blocks of VAD_BLOCK samples, one lane each (k_mel.hip: k_vad_blocks, k_vad_finish).
// warm: samples a block's lane runs ahead of its block (0 .. VAD_BLOCK; < 0: VAD_WARM_DEFAULT).  scratch: vad_scratch_bytes(n) of device
// memory.  res: 8 words — {decision, energy_all, energy_last} as floats, then {blocks, blocks re-run} as int32 at res[4], res[5].
constexpr int VAD_BLOCK = 64, VAD_WARM_DEFAULT = 32;
size_t vad_scratch_bytes(int n);
void vad_window_blocks(const float * x, int n, int n_last, float alpha, bool filter, float vad_thold, int warm, void * scratch, float * res,
                       hipStream_t st);

// Resampler (k_resample.hip): src_simple(SRC_SINC_FASTEST = 2 | SRC_SINC_MEDIUM_QUALITY = 1 | SRC_ZERO_ORDER_HOLD = 3 | SRC_LINEAR = 4,
// one channel) of libsamplerate as the host calls it (src/speech_to_text.cpp:16-43), bit-identical to the sequential CPU code.  resample_plan replays the converter's index
// state machine on the host (how many frames come out, whether the position recurrence has a closed form), resample_launch
// computes every output frame in its own thread.
struct Stepper;
struct ResamplePlan {
    int error = 0;                       // 0, or libsamplerate's error number negated (-6 ratio, -10 converter, -21 length check), -30 ratio unsupported,
                                         // -31 SRC_LINEAR on one input frame at a ratio above 1 (the library reads data_in[-1])
    int converter = 2;
    long long n_out = 0, n_used = 0;     // output_frames_gen, input_frames_used
    int half_len = 0, index_inc = 0, increment = 0;              // SINC converters only, like float_inc and out_scale
    double float_inc = 0.0, out_scale = 0.0;
    bool need_table = false;             // the (pos, frac) table of resample_table() has to be on the device
    std::shared_ptr<Stepper> stepper;
};
bool sinc_table(int converter, const float ** coeffs, int * count, int * increment);
ResamplePlan resample_plan(long long n_in, long long out_cap, double ratio, int converter);
void resample_table(const ResamplePlan & pl, const int ** pos, const double ** frac);       // host arrays, n_out (+1) entries
void resample_positions(const ResamplePlan & pl, long long n, long long * pos, double * frac);   // first n positions (tests)
void resample_launch(const ResamplePlan & pl, const float * d_in, long long n_in, float * d_out, const float * d_coeffs,
                     const int * d_pos, const double * d_frac, hipStream_t st);
// The capture session's form (capture.cpp): the input is the interleaved stereo capture frames, folded per tap as downmix_stereo folds them
// (no mono buffer), and only outputs [first, pl.n_out) are computed.  resample_first_dirty: the outputs below it are the same in both plans
// (n_old = the frames old_pl was made for); 0 = recompute everything (table positions, an error in either plan).
void resample_launch_stereo(const ResamplePlan & pl, const float * d_frames_xy, long long n_in, float * d_out, const float * d_coeffs,
                            const int * d_pos, const double * d_frac, long long first, hipStream_t st);
long long resample_first_dirty(const ResamplePlan & old_pl, long long n_old, const ResamplePlan & new_pl);
// What a resampler input frame is read from (in_frame<KIND>, k_resample.hip): the two f32 forms above, and the packed integer frames of an
// AudioStreamWAV (k_wav.hip has the decode: s16 / 32768, s8 / 128, little-endian, a stereo frame folded as downmix_stereo folds it).
// The integer kinds need only sample alignment (2 bytes for s16, none for s8).
enum SrcKind : int { SRC_F32_MONO = 0, SRC_F32_STEREO = 1, SRC_S16_MONO = 2, SRC_S16_STEREO = 3, SRC_S8_MONO = 4, SRC_S8_STEREO = 5 };
// resample_launch / resample_launch_stereo for any kind: d_src holds n_in frames of `kind`; SRC_F32_MONO and SRC_F32_STEREO launch exactly
// what those two launch.  No f32 image of the input is written.
void resample_launch_kind(const ResamplePlan & pl, int kind, const void * d_src, long long n_in, float * d_out, const float * d_coeffs,
                          const int * d_pos, const double * d_frac, long long first, hipStream_t st);

// AudioStreamWAV frames -> mono f32 at the rate they have (k_wav.hip): out[i] = frame i of `kind` decoded (and folded).  One launch; eight
// frames per thread with 16-byte loads from the first frame that starts on a 16-byte boundary, the frames before it and behind the last full
// group of eight one per thread — or every frame so when no frame starts on such a boundary (a stereo source one sample off its frame grid).
// d_src: sample-aligned; out: any f32 pointer.  false: bad kind / launch error.  n_frames = 0 launches nothing.
bool wav_decode(int kind, const void * d_src, long long n_frames, float * out, hipStream_t st);
// The two channels of a STEREO kind kept apart, one launch each (wmi_full_wav_channels): every frame is read once, out0 gets the left and
// out1 the right samples — no fold.  wav_split is wav_decode's scheme at the source's own rate; resample_launch_split is
// resample_launch_kind's thread with the channel-independent work (position, tap walk, interpolated coefficients) shared, and each of its
// outputs equals resample_launch on a mono buffer of that channel bit for bit.  d_src: sample-aligned; out0 / out1: any f32 pointers, room
// for n_frames / pl.n_out each.  A mono kind: false / nothing is launched.
bool wav_split(int kind, const void * d_src, long long n_frames, float * out0, float * out1, hipStream_t st);
void resample_launch_split(const ResamplePlan & pl, int kind, const void * d_src, long long n_in, float * out0, float * out1,
                           const float * d_coeffs, const int * d_pos, const double * d_frac, hipStream_t st);
// IMA-ADPCM bytes of an AudioStreamWAV -> interleaved s16 (k_adpcm.hip; adpcm_map.h has the definition and the map algebra): two prefix
// scans over chunks of ADPCM_CHUNK nibbles per channel, one chunk per thread, ADPCM_WG chunks per workgroup, the workgroups' partials walked
// in tiles of ADPCM_PART_TILE — ADPCM_LAUNCHES launches on `st`, no workgroup waits for another.
//   adpcm_plan          host only.  n_used: the bytes that hold frames (stereo: a trailing odd byte is ignored); frames = 2 * n_used / channels;
//                       head: the bytes of chunk 0, in front of the source's first 16-byte boundary; out_skew: how many s16 the image should
//                       start behind a 16-byte boundary for the full chunks to leave as 16-byte stores (any 2-byte aligned d_out is served)
//   adpcm_scratch_bytes what d_scratch must hold for a source of n_bytes, wherever it lies (256-byte aligned)
//   adpcm_decode        d_src: any byte address; d_out: room for frames * channels s16.  frames = 0 launches nothing.  false: launch error.
constexpr int ADPCM_CHUNK = 32, ADPCM_WG = 256, ADPCM_PART_TILE = 256, ADPCM_LAUNCHES = 5;
struct AdpcmPlan { long long n_used = 0, frames = 0, n_chunks = 0; int head = 0, out_skew = 0; };
AdpcmPlan adpcm_plan(const void * d_src, long long n_bytes, bool stereo);
size_t adpcm_scratch_bytes(long long n_bytes, bool stereo);
bool adpcm_decode(const AdpcmPlan & p, const void * d_src, bool stereo, int16_t * d_out, void * d_scratch, hipStream_t st);
// Channel energies per centisecond of a STEREO source (k_speaker.hip; speaker_ranges.h has the definition): one launch over n frames of
// `kind` (SRC_F32_STEREO, SRC_S16_STEREO, SRC_S8_STEREO) at `rate` Hz writes nb = channel_bins_count(n, rate) pairs {left, right} of 8-byte
// sums over frames [B(b), min(B(b + 1), n - 1)), B(b) = (b * rate) / 100, and behind them the two magnitudes of frame n - 1: (nb + 1) * 16
// bytes at d_bins (8-byte aligned) — unsigned 64-bit sums of |v| for the integer kinds, doubles for f32.  d_src: sample-aligned.
// n = 0 launches nothing.  false: bad kind / size / launch error.
long long channel_bins_count(long long n, long long rate);
bool channel_bins(int kind, const void * d_src, long long n, long long rate, void * d_bins, hipStream_t st);

// ---------------------------------------------------------------- GEMM (k_gemm.hip)
enum Epi : int {
    EPI_F16_BIAS = 0,       // C f16 = acc + bias
    EPI_F16_BIAS_GELU,      // C f16 = gelu16(acc + bias)
    EPI_F32_BIAS_RESID,     // C f32 = acc + bias + resid
    EPI_CONV2,              // x f32 = gelu16(acc + bias) + pe ; aux f32 = gelu16(acc + bias)
    EPI_QKV_ENC,            // q | k | v^T split (encoder)
    EPI_QKV_DEC,            // q*s | k*s -> cache | v -> cache (decoder self-attention)
    EPI_CROSS_KV,           // per decoder layer: k*s | v+b into the cross cache
    EPI_Q_SCALED,           // C f16 = (acc + bias) * scale  (decoder cross-attention query)
};
struct GemmArgs {
    const __half * A;  int lda;     // [M][K]
    const __half * W;  int ldw;     // [N][K]
    int M, N, K;                    // K multiple of 32 (weights zero-padded)
    const float * bias;             // [N] or null
    void *  C;   int ldc;           // primary output
    const float * resid; int ldr;   // EPI_F32_BIAS_RESID / EPI_CONV2 (pe)
    void *  aux; int ldaux;         // second output (EPI_CONV2: embd_conv; QKV: k / cache k)
    void *  aux2; int ldaux2;       // third output (QKV: v^T / cache v)
    float   scale;                  // q/k scale
    int     S;                      // split width for the QKV / cross epilogues
    int64_t layer_stride;           // EPI_CROSS_KV: elements between layers in the cross cache
    int     rows_per_chunk;         // EPI_QKV_ENC, batched encode: M = chunks * rows_per_chunk (0: one chunk)
    int     conv2_out_rows;         // EPI_CONV2 with rows_per_chunk: rows between the chunks of the output (0: rows_per_chunk - 4, back to back)
    int64_t chunk_stride_aux2;      //   elements between the chunks' V^T images
    int     no_glds;                // debug: keep 128x128 tiles on the register-staged loop
    unsigned long long * probe;     // probe (wmi_bench_kernel 7): per workgroup {entry, first tile landed, K loop done, epilogue done, SE/CU id}
};
void gemm(int epi, const GemmArgs & a, hipStream_t st);
// Probe (wmi_encoder_gemm_stamps): while a log is installed on the calling THREAD, every gemm() launch that has no probe of its own gets a
// slice of `buf` as GemmArgs::probe (5 words per workgroup: entry ... done, wall-clock ticks) and an entry here — the in-situ duration of
// each GEMM of an encoder pass is then max(done) - min(entry) over its workgroups, with the cache state the pass itself leaves.
struct GemmLogEntry { int epi, M, N, K; size_t off; int cap; };
struct GemmLog { unsigned long long * buf = nullptr; size_t cap_words = 0, used = 0; std::vector<GemmLogEntry> entries; };
void gemm_log_install(GemmLog * log);       // null = off
// k_gemm8.hip: the eight-wavefront ping-pong form for the big grids (M = chunks x 1500): BM x 256 tiles, bm in {96, 128, 160, 192, 256},
// swapped = transposed accumulator fragments (row-major f16 / f32 epilogues), ks = k extent of a slot.  Bit-identical to gemm().
// false = not served (N % 256, K % 64, epilogue): the caller keeps gemm().
bool gemm8(int epi, int bm, bool swapped, const GemmArgs & a, hipStream_t st, int ks = 64);

// gemm()'s decision, apart from its launch: gemm() is launch(gemm_plan(...)).  Pure host arithmetic over (epilogue, M, N, K, S, the lab bits
// in GemmArgs::no_glds, the CU count): no device, no launch — wmi_selftest_gemm_plan hands it to the CPU tests, wmi_selftest_gemm reports the
// plan that served a call, and tests/gemm_f64.py holds the table of plans the product reaches.
enum GemmOrient : int {
    GEMM_ORIENT_ROWS = 0,       // first orientation, mfma(A rows, W rows): epilogue_rows
    GEMM_ORIENT_COLS = 1,       // transposed, mfma(W rows, A rows): epilogue_cols / epilogue_cols_wide
    GEMM_ORIENT_PER_TILE = 2,   // EPI_QKV_ENC: q and k column tiles transposed, the V^T third (n0 >= 2 S) in the first orientation
};
struct GemmPlan {
    int epi = 0;
    int kernel = 0;             // 0 = not served, 1 = k_gemm, 8 = k_gemm8
    int bm = 0, bn = 0;         // tile
    int waves = 0;              // wavefronts per workgroup
    int ring = 0, ring_w = 0;   // LDS ring depth (k_gemm8: of the A image and of the W image)
    int dma = 0;                // 1 = DMA ring (global_load_lds), 0 = register-staged loop
    int orient = 0;             // GemmOrient: the rule the kernel applies
    int ks = 0;                 // k extent of a slot (k_gemm8: 32 or 64; k_gemm: one 64-wide LDS tile)
};
GemmPlan gemm_plan(int epi, const GemmArgs & a, int n_cu);        // n_cu: cu_count_x8() of the device that will run it
GemmPlan gemm8_plan(int epi, int bm, bool swapped, const GemmArgs & a, int ks);     // what gemm8() launches for these arguments (kernel = 0: not served)
// The two run-time choices a k_gemm workgroup makes itself, written once for the kernel and for gemm_plan().  Macros, not functions: the
// kernel's code stays what it was instruction for instruction (an inlined function evaluates its arguments — loads of kernel arguments —
// ahead of the short-circuits, and hipcc then schedules the prologue differently).
//   the K loop: 64-row tiles take the DMA ring while the grid is small, the register-staged loop with thousands of tiles or a half K tile
#define WMI_GEMM_TAKES_DMA_RING(bm, nwg, K, no_glds) (((bm) >= 96 || (nwg) <= 1024) && ((K) % 64) == 0 && !((no_glds) & 1))
//   the orientation of the accumulator fragments of a tile (vt_third: its first column is >= 2 S, the V^T third of the encoder's q|k|v), for
//   the epilogues that have a transposed form at all (all but EPI_QKV_DEC); measurements: k_gemm.hip
#define WMI_GEMM_BIG_GRID(M) ((M) >= 4096)
#define WMI_GEMM_TILE_TRANSPOSED(epi, big, no_glds, vt_third) \
    (!((epi) == EPI_QKV_ENC && ((vt_third) || ((big) && !((no_glds) & 8)))) && !((epi) == EPI_F32_BIAS_RESID && (big) && !((no_glds) & 32)))
inline int gemm_orient_rule(int epi, int M, int no_glds) {
#ifdef WMI_GEMM_NO_SWAP
    return GEMM_ORIENT_ROWS;
#else
    if (epi == EPI_QKV_DEC) return GEMM_ORIENT_ROWS;
    const bool big = WMI_GEMM_BIG_GRID(M);
    const bool qk = WMI_GEMM_TILE_TRANSPOSED(epi, big, no_glds, false), v = WMI_GEMM_TILE_TRANSPOSED(epi, big, no_glds, epi == EPI_QKV_ENC);
    return qk && v ? GEMM_ORIENT_COLS : qk ? GEMM_ORIENT_PER_TILE : GEMM_ORIENT_ROWS;
#endif
}

// ---------------------------------------------------------------- LayerNorm (k_norm.hip)
// y = (x - mean) / sqrt(var + eps) * g + b ; one wave per row. out16 and/or out32 may be null.
void layernorm(const float * x, int rows, int S, const float * g, const float * b, float eps,
               __half * out16, float * out32, hipStream_t st, int rows_per_chunk_in = 0, int rows_per_chunk_out = 0);      // > 0: output row = chunk * out + t for input row chunk * in + t

// ---------------------------------------------------------------- attention (k_attn.hip)
// encoder: q,k [T][S] f16 ; vt [S][Tpad] f16 ; out [T][S] f16 ; scale applied to q.k before softmax
// B > 1: B chunks back to back (q,k,out [B][T][S]; vt [B][S][Tpad]), one grid.z slice each
// out32 != null: the result is written as f32 to out32 instead (models whose out-projection is block-quantised quantise that
// f32 tensor directly, as the reference does); same for the decoder kernels below
// second form (k_attn_enc.hip): 32-row wavefronts; one_sweep = running maximum, else exact maximum first; split = four key groups
void attn_encoder2(const __half * q, const __half * k, const __half * vt, int T, int Tpad, int S, int H, __half * out, hipStream_t st,
                   int B, float * out32, bool one_sweep, bool split, int qk_chunk_rows = 0, const RowLens * row_lens = nullptr, int out_chunk_rows = 0);
void attn_encoder(const __half * q, const __half * k, const __half * vt, int T, int Tpad, int S, int H,
                  float scale, __half * out, hipStream_t st, int B = 1, float * out32 = nullptr,
                  int qk_chunk_rows = 0,      // rows between the chunks of q and k (0 = T; lock-step chunks start on 16-row boundaries, batch.cpp)
                  const RowLens * row_lens = nullptr,   // B > 1: chunk z attends row_lens->t[z] queries and keys (T = the largest: grid and key split are
                  int out_chunk_rows = 0,               // decided once per launch by it); out_chunk_rows: rows between the chunks of out (0 = T)
                  int split = -1);                      // the key split: -1 by the launch (attn_encoder_splits), 0 / 1 named by the caller
// would a one-chunk pass of T rows split its keys (attn_encoder at B = 1)?  The block-quantised stacked pass launches its chunks so
// (device_q.cpp): the activation quantiser amplifies what the other summation order changes
bool attn_encoder_splits_alone(int T, int Tpad, int H, float scale);
// the same launch with the form (WMI_ATTN_FORM's values: 2, 1, 0) and the key-group choice given by the caller (split: four key groups
// of the second form, two of the first) — attn_encoder() is this with the environment's form and attn_encoder_splits()' answer, its rule
// for the launch (form, largest length, grid); the test hook wmi_selftest_attn_encoder names both itself
bool attn_encoder_splits(int form, int T, int Tpad, int H, float scale, int B);
void attn_encoder_form(const __half * q, const __half * k, const __half * vt, int T, int Tpad, int S, int H, float scale,
                       __half * out, hipStream_t st, int B, float * out32, int qk_chunk_rows, const RowLens * row_lens, int out_chunk_rows,
                       int form, bool split);
// decoder: one (token, head) per workgroup.  kc/vc: [n_kv][S] caches (this layer), mask: [n][ld_mask] or null
void attn_decoder(const __half * q, int n, int S, int H, const __half * kc, const __half * vc, int n_kv,
                  const float * mask, int ld_mask, __half * out, hipStream_t st,
                  const int32_t * n_kv_dev = nullptr, int n_kv_max = 0,    // n_kv_dev: read n_kv on the device (graph replay)
                  float * out32 = nullptr);

// decoder cross-attention split over the key axis (3 small launches, NS x H x n workgroups); same numerics
void attn_cross_split(const __half * q, int n, int S, int H, const __half * kc, const __half * vc, int T,
                      float * scratch, __half * out, hipStream_t st, int64_t kv_row_stride = 0, float * out32 = nullptr);
// same without the combine launch: the consumer GEMV combines the partials in its prologue (GemvArgs::comb_*)
void attn_cross_split_partials(const __half * q, int n, int S, int H, const __half * kc, const __half * vc, int T,
                               float * scratch, const float ** part_o, const float ** part_l, const float ** part_m, int * ns, hipStream_t st,
                               int64_t kv_row_stride = 0,    // row i reads kc/vc + i * kv_row_stride (lock-step chunks)
                               const RowLens * row_lens = nullptr);   // one-launch form only: row i attends row_lens->t[i] keys in the slices the one-row path
                                                             // takes at that length; T = the largest (layout, grid); slices a row does not have write neutral
                                                             // partials (m = -inf, l = 0, o = 0), which the consumers' combine passes over bit for bit
// part_m: null when the partials are relative to the row's global maximum (two-launch form), else the slice maxima the
// consumer rescales by (one-launch form, k_xattn_fused) — pass it on as GemvArgs::comb_m / to attn_cross_combine
// the same with the query projection folded into the score kernel: q = (W_cq . LN(x32) + b_cq) * qscale is recomputed per
// (slice, head) workgroup (bit-identical to gemv + EPI_Q_SCALED); saves one launch per decoder layer
// where the one-launch form of the cross-attention puts a step's partials, and its grid: for the form whose query projection is a
// block-quantised matrix (k_quant.hip: qattn_cross_qsplit_partials).  fused = false: the key slices are too long for one launch
struct XattnPlan { int ns, ks; float * pmax, * part_l, * part_o; bool fused, head_major; };
XattnPlan attn_cross_plan(int n, int H, int T, float * scratch);
void attn_cross_qsplit_partials(const float * x32, const float * ln_g, const float * ln_b, float eps, const __half * wq,
                                const float * bq, float qscale, int n, int S, int H, const __half * kc, const __half * vc, int T,
                                float * scratch, const float ** part_o, const float ** part_l, const float ** part_m, int * ns, hipStream_t st,
                                int64_t kv_row_stride = 0, const RowLens * row_lens = nullptr);
bool attn_cross_takes_row_lens(int H, int T);      // is the form the two functions above launch at T the one-launch form (the only one with row_lens)?
size_t attn_cross_scratch_floats(int n, int H, int T);

// ---------------------------------------------------------------- decoder small-batch (k_dec.hip)
void dec_embed(const int32_t * tokens, const int32_t * pos, int n, int S, const __half * te, const float * pe,
               float * x, hipStream_t st);
// per-workgroup partial statistics of a row of filtered logits (k_sample.hip: k_filter_stats writes 64 of them per row; the one-row
// vocabulary projection writes one per workgroup from its epilogue, GemvArgs::fs_*): maxima with first-index tie-break over all /
// text / timestamp tokens, and sums of exp(l - all.v) — combined exactly by k_filter_pick (online soft-max identity)
struct FsMaxIdx { float v; int i; };
struct FsPartial { FsMaxIdx all, txt, ts; float sum, sum_ts; float pad[2]; };
constexpr int FS_MAX_PARTS = 768;                 // partials of the fused form (= the vocabulary projection's workgroup cap)
// rows <= 8 "GEMV" path: out[i][o] = sum_k W[o][k] * a[i][k] with the same epilogues as the GEMM.
// If ln_g != null the A operand is LayerNorm(x32) computed in the prologue (fused), else a16.
struct GemvArgs {
    const float * x32; const float * ln_g; const float * ln_b; float eps;   // fused-LN input [n][K]
    const __half * a16;                                                     // or plain f16 input [n][K]
    int n, K, N;
    const __half * W; const float * bias;
    int epi;                                  // Epi (F16_BIAS, F16_BIAS_GELU, F32_BIAS_RESID, QKV_DEC, Q_SCALED) or EPI_LOGITS
    void * C; int ldc;
    const float * resid; int ldr;
    void * aux; int ldaux; void * aux2; int ldaux2;
    float scale; int S;
    const int32_t * rows;                     // optional row gather for the A operand (logits)
    const int32_t * row_off;                  // optional device scalar: aux/aux2 row offset (KV cache head), graph replay
    const float * comb_o; const float * comb_l; int comb_ns;   // optional: A operand = combined split cross-attention partials
    const float * comb_m;                     // slice maxima the partials are relative to (null: the row's global maximum)
    // optional (n == 1): A operand = self-attention output computed in the prologue from q and this layer's KV cache
    const __half * sa_q; const __half * sa_k; const __half * sa_v; const int32_t * sa_nkv; int sa_cap;
    // lock-step chunks (lanes != 0): row r belongs to chunk r with its own KV cache and step record.
    //   aux/aux2 row = row_off[r * step_stride] (no "+ r"), cache base + r * cache_row_stride ; sa_nkv[r * step_stride] ;
    //   sa_k / sa_v + r * cache_row_stride
    int lanes; int step_stride; int64_t cache_row_stride;
    // chained greedy steps: mirror *step_copy_src (DecStep in pinned host memory) into *step_copy_dst by an extra workgroup
    // (one-row f16 rows x plain projection + residual only: the last mlp.2 of the step)
    const void * step_copy_src; void * step_copy_dst;
    // chained lock-step steps: the rows' records (words 4.. of each DecStep) mirrored by an extra workgroup of the vocabulary
    // projection on the matrix cores (k_rows_mfma); ask gemv_rows_carries_mirror() first, the other row kernels ignore these
    const void * rows_mirror_src; void * rows_mirror_dst;
    // weight prefetch for the NEXT launch of a dependent chain (k_qrows): pf_groups row groups of pf_group_bytes each, contiguous at
    // pf_ptr; workgroup i touches one dword per 128-byte line of the groups g = i (mod grid) — the workgroup of the next launch
    // that streams group g sits on the same XCD when both grids are multiples of 8
    const void * pf_ptr; uint32_t pf_group_bytes; uint32_t pf_groups;
    unsigned long long * stamps; int stamp_slot;      // probe (stamp_next()): filled in by gemv() itself
    // greedy step, EPI_LOGITS at one row: the logit filters' statistics pass folded into the epilogue — fs_part[workgroup] gets the
    // partial of the rows the workgroup produced (fs_step: DecStep of the row, fs_ban: static ban bytes); gemv_fused_parts() tells
    // how many partials this launch will write (0: the arguments do not take the fused path — run filter_argmax's own pass)
    const uint8_t * fs_ban; const void * fs_step; FsPartial * fs_part;
    // k_qrows, K split over workgroups (ksplit = 2: mlp.2 of the wide models — N = S is only S / 32 row groups, K = 4 S is 4 S / 64 tiles
    // each): workgroup (row group, half) multiplies its half of K; the lower half runs the epilogue as usual (bias, residual, in
    // place), the upper half leaves its sums in kpart [n][N] f32.  The launches that read that row next take them as `pend` and add
    // them — x = C + kpart, one f32 addition per element, the same in every consumer: the LayerNorm prologue of the next projection /
    // of the vocabulary projection (x32 + pend) and the residual of the next out projection (resid + pend), which writes the row whole again.
    int ksplit; float * kpart;
    const float * pend;
};
int gemv_fused_parts(const GemvArgs & a);
bool gemv_rows_carries_mirror(const GemvArgs & a);
bool gemv_rows_take_self_attention(const GemvArgs & a);      // lock-step rows: will gemv() run this out projection with the self-attention in its prologue?
// lock-step chunks: single-token self-attention of n rows, row r against the cache at kc/vc + r * cache_row_stride with
// n_kv[r * step_stride] cells; same arithmetic as the fused prologue of gemv (GemvArgs::sa_*).  out [n][K] f16
void self_attn_rows(const __half * q, int n, int K, const __half * kc, const __half * vc, int64_t cache_row_stride,
                    const int32_t * n_kv, int step_stride, int cap, __half * out, hipStream_t st, float * out32 = nullptr,
                    bool long_cache = false,    // long_cache: the host knows a row has > 64 cells: four wavefronts per (row, head)
                    const void * mirror_src = nullptr, void * mirror_dst = nullptr);   // chained lock-step steps: + one workgroup per row copying
                                                // words 4.. of the row's DecStep from pinned host memory to the device record (short-cache form only)
// split cross-attention partials -> out [n][S] f16 (the separate form of GemvArgs::comb_*)
void set_xattn_probe_skip(int mask);      // probe only
void attn_cross_partials_layout(int n, int H, int T, float * scratch, const float ** po, const float ** pl, const float ** pm, int * pns);
void attn_cross_combine(const float * part_o, const float * part_l, const float * part_m, int ns, int n, int S, int H, __half * out, hipStream_t st,
                        float * out32 = nullptr);
enum { EPI_LOGITS = 100 };                    // C f32 [n][N] = acc
void gemv(const GemvArgs & a, hipStream_t st);
// The language head (k_lang_head): the logits of the 100 language tokens behind <sot> and nothing else of the vocabulary —
// out[r][i] = te_lang[i] . f16(LN(x[r])), r < rows (grid.y, the lock-step convention), te_lang = te + (sot + 1) S.  Always LANG_HEAD_N rows,
// whatever the vocabulary holds there (W/whisper.cpp:3603-3606).  Every value equals, bit for bit, the entry the one-row vocabulary
// projection (gemv, EPI_LOGITS) writes for the same row: ln_row_compute's LayerNorm, the activation rounded to f16 at the same point, the
// same per-lane fmaf chain over the columns and the same 64-lane butterfly.  out may be pinned host memory.  S <= 1536, S % 8 == 0.
constexpr int LANG_HEAD_N = 100;
bool lang_head_usable(int S);
void lang_head(const float * x, int rows, int S, const float * ln_g, const float * ln_b, float eps, const __half * te_lang, float * out, hipStream_t st);
// block-quantised models: the language rows are cut out of the row kernel's output over the 32-row tiles that cover them (k_qrows'
// per-row results do not depend on the rows that share a launch): out[r][i] = src[r * ld + off + i], i < LANG_HEAD_N
void lang_gather(const float * src, int ld, int off, int rows, float * out, hipStream_t st);

// The no-speech head (k_nospeech.hip): p = soft-max(l)[nosp] of a decoder row's RAW logits l, OpenAI's no_speech_prob.  The arithmetic is
// fixed: the vocabulary is cut into blocks of NSP_BLOCK entries; a block keeps m_b = max l and s_b = sum exp(double(l - m_b))
// — the difference in f32, exp and the sums in double, lane L of one wavefront adding entries L and L + 64 and the 64 lanes in the xor
// order 32 .. 1; an entry of -inf adds 0.  A second launch combines the blocks in ascending order: M = max m_b,
// S = sum_b s_b exp(double(m_b - M)), p = float(exp(double(l[nosp] - M)) / S) — one rounding to f32 — and stores {p, tag} as ONE 8-byte
// store, usually into pinned host memory.  Workgroups are independent: no atomics, no hand-off inside a launch; a row's result does not
// depend on the rows that share the launch, and both forms give the same bits on the same logits.
//   form 1 (no_speech_logits): logits already in HBM, row r of the launch reads logits + rows.row[r] * ld
//   form 0 (no_speech_head):   the logits are k_lang_head's — gemv's one-row EPI_LOGITS bits — for ALL rows of the token embedding, from
//                              the f32 residual row x + r * S; they live in LDS only.  S as lang_head_usable says.
constexpr int NSP_BLOCK = 128, NSP_MAX_ROWS = 16, NSP_MAX_VOCAB = 65536;
struct NoSpeechOut { float p; int32_t tag; };
struct NoSpeechRows { int n; int row[NSP_MAX_ROWS]; };          // logits row of launch row r (form 1)
size_t no_speech_scratch_bytes(int n_vocab);                    // the block partials of NSP_MAX_ROWS rows
bool no_speech_logits(const float * logits, int ld, const NoSpeechRows & rows, int n_vocab, int nosp, void * scratch, NoSpeechOut * out, int32_t tag, hipStream_t st);
bool no_speech_head(const float * x, int rows, int S, const float * ln_g, const float * ln_b, float eps, const __half * te, int n_vocab, int nosp,
                    void * scratch, NoSpeechOut * out, int32_t tag, hipStream_t st);

// The text scorer (k_score.hip): lp = log soft-max(l)[t] of a decoder row's RAW logits l for a given target t, with the
// no-speech head's block pass (nsp_block.h: the same bits for m_b and s_b on the same logits), the blocks combined in ascending order:
// M = max m_b, S = sum_b s_b exp(double(m_b - M)), lp = float(double(float(l[t] - M)) - log(S)) — one rounding to f32; l[t] = -inf gives -inf.
//   score_rows:   rows.n <= SCORE_MAX_ROWS launch rows; launch row r reads logits + rows.row[r] * ld (several launch rows may read one
//                 logits row with different targets), its target is targets[r], its result goes to lp[place[r]] (targets, place, lp: device).
//                 Two launches: blocks (grid = blocks x rows, one wavefront each), combine (one wavefront per row).
//   score_finish: one workgroup.  Text c owns lp[first[c] .. first[c + 1]): sum in double in ascending order, avg = sum / count,
//                 v = length_norm ? avg : sum (double), posterior = float(exp(v_c - max v) / sum_c exp(v_c - max v)), the maximum and the sum
//                 taken over the texts in ascending order in double; v = -inf gives 0, every v = -inf gives 0 everywhere.  rec [n_texts],
//                 lp_out (optional copy of lp[0 .. first[n_texts])) and out = {n_texts, tag} are stored with plain vector stores, usually
//                 into pinned host memory.
// Workgroups are independent inside every launch; no atomics.
constexpr int SCORE_MAX_ROWS = 8, SCORE_MAX_TEXTS = 4096, SCORE_FINISH_THREADS = 256;
struct ScoreRows { int n; int row[SCORE_MAX_ROWS]; };
struct ScoreRec { double sum; float avg, post; int32_t n_scored, first; };      // the layout of wmi_text_score (wmi_device.h)
struct ScoreOut { int32_t n_texts; int32_t tag; };
size_t score_scratch_bytes(int n_vocab);                        // the block partials of SCORE_MAX_ROWS rows
bool score_rows(const float * logits, int ld, const ScoreRows & rows, int n_vocab, const int32_t * targets, const int32_t * place, void * scratch,
                float * lp, hipStream_t st);
bool score_finish(const float * lp, const int32_t * first, int n_texts, bool length_norm, ScoreRec * rec, float * lp_out, ScoreOut * out, int32_t tag,
                  hipStream_t st);

// Token alignment (k_align.hip): DTW over the cross-attention of chosen (layer, head) pairs.  For a pass of n rows over
// M key frames and a pair (l, h): s[i][t] = sum_{c < 64} q_l[i][64 h + c] k_l[t][64 h + c] (f16 operands as stored — both carry
// d^-1/4 —, f32 sum), w = soft-max over exactly the first M keys, z = (w - mean) / sigma per (pair, t) over all n rows (population
// sigma; sigma == 0 gives 0), a median of 7 along t with reflect padding (none for M <= 3), A[r][t] = mean over the pairs of
// z[n_sot + r][t], r < R = n - n_sot - 1, the pairs added in ascending (layer, head) order and divided by their count once.
//   align_layer:  the layer's heads (ascending) into A — scores + soft-max into w [heads][n][M], column statistics, normalise + median +
//                 accumulate; pair0 = the pairs of earlier layers (0: A starts from zero).  q [n][S], kc [>= M][S], S = 64 H.  The query
//                 rows used go to b.q [pairs][n][64] when it is not null.
//   align_finish: A /= pairs, and -A diagonal-major into b.cost: element (r, t) at [r + t][r]
//   align_dtw:    D[0][0] = 0, the other border cells +inf; D[i][j] = c[i-1][j-1] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) in f32 with
//                 OpenAI's tie rule (diagonal only if strictly below both, then up only if strictly below both, else left); one workgroup,
//                 a thread per row, anti-diagonals; thread 0 walks the step bytes back from (R, M).  jumps[r] = first frame of row r and
//                 out = {path length, tag} are stored with plain vector stores, usually into pinned host memory; path (device, may be null)
//                 takes the (row, frame) points, the LAST point at [R + M - 1], the first at [R + M - n_path].
// Workgroups are independent inside every launch; no atomics.
constexpr int ALIGN_HEAD_DIM = 64, ALIGN_MAX_HEADS = 32, ALIGN_MAX_M = 1500, ALIGN_DTW_THREADS = 512, ALIGN_MAX_R = ALIGN_DTW_THREADS - 1;
struct AlignHeads { int n; int head[ALIGN_MAX_HEADS]; };
struct AlignOut { int32_t n_path; int32_t tag; };
struct AlignBufs { float * w, * mu, * sigma, * A, * cost; uint8_t * trace; __half * q; };
size_t align_w_floats(int nh, int n, int M);                    // w; mu and sigma hold nh * M each, A R * M, trace R * M bytes
size_t align_cost_floats(int R, int M);
bool align_shape_ok(int n, int n_sot, int M, int S, int H);
bool align_layer(const AlignBufs & b, const __half * q, int n, int S, const __half * kc, int M, const AlignHeads & hs, int pair0, int n_sot, hipStream_t st);
bool align_finish(const AlignBufs & b, int R, int M, int n_pairs, hipStream_t st);
bool align_dtw(const float * cost, int R, int M, uint8_t * trace, int32_t * path, int32_t * jumps, AlignOut * out, int32_t tag, hipStream_t st);
void align_cost_from_matrix(const float * A, int R, int M, float * cost, hipStream_t st);      // -A diagonal-major (the path hook)

// Frame energies (k_segment.hip): the detector in front of wmi_full_long.  x [n] 16 kHz f32 PCM on the device, e [ceil(n / 160)]:
//   e[f] = sum over i in [160 f, min(160 f + 160, n)) of | x[i] - x[i - 1] |, x[-1] := 0 — f32 throughout, the sum left to right from 0.0f.
// A workgroup owns SEG_STAGE_FRAMES frames (its staging extent in LDS); nothing is shared between workgroups.  false: bad argument / launch error.
constexpr int SEG_FRAME = 160, SEG_STAGE_FRAMES = 64;
bool frame_energy(const float * x, int n, float * e, hipStream_t st);

// One decoder MLP of the one-row step as ONE launch: x += W2 . gelu(W1 . LN(x) + b1) + b2 (k_mlp_pair, k_dec.hip).  The hidden row goes
// from the workgroups that produce it to every workgroup of the same launch through data-tagged 8-byte granules ({two f16, tag}, written
// and read past the caches): no launch boundary between the two projections.  `hand` holds 2 S granules (16 S bytes, zeroed once),
// `epoch` two 32-bit words (zeroed once; the launches' tags, see the kernel).  false = shape not covered (S > 1024: measured slower at S = 1280; or the launch's workgroups
// would not all be resident at once): run the two projections as two launches.
struct MlpPairArgs {
    const float * x; const float * ln_g, * ln_b; float eps; int S;
    const __half * W1; const float * b1; const __half * W2; const float * b2;
    uint32_t * epoch; int par; void * hand;                    // epoch[2] (zeroed once), par = 0 / 1 alternating from launch to launch
    // sticky status word of the hand-off (zeroed once, cleared by the host after it has acted): PAIR_FAULT_TIMEOUT a consumer gave up waiting
    // (its rows of this launch are garbage), PAIR_FAULT_PARITY two launches in a row with the same `par` (stale granules pass the tag test),
    // PAIR_SLOW a sweep needed more than PAIR_SLOW_POLLS polls (correct, but something else owns the GPU: the two-launch form is the faster one).
    // The step's pick kernel reports the word in the sequence tags of SampleOut (ChainNext::fault), the host re-runs / switches form.
    uint32_t * fault; uint32_t spin_cap;                       // spin_cap: polls before a consumer gives up (0 = 1 << 20, about a second)
    int withhold;                                              // tests: wavefront `withhold - 1` never publishes its granules; < 0: wavefront `-withhold - 1` publishes ~0.2 ms late (0 = off)
    const void * step_copy_src; void * step_copy_dst;          // chained greedy steps: see GemvArgs::step_copy_src
    __half * h_out;                                            // optional plain copy of the hidden row (tests / debugging)
};
enum : uint32_t { PAIR_FAULT_TIMEOUT = 1u, PAIR_FAULT_PARITY = 2u, PAIR_SLOW = 4u };
constexpr uint32_t PAIR_SLOW_POLLS = 64;
// decided ONCE per step for all its layers (the launches' parity must alternate: a layer that alone fell back to two launches would break
// it): shape covered, and the widest launch of the step (+ 1 workgroup with the step-record mirror) resident at once on the CURRENT device
bool mlp_pair_usable(int S, bool with_mirror);
void mlp_pair(const MlpPairArgs & a, float * x_inout, hipStream_t st);
// The front of a decoder layer of the one-row step as one launch (k_dec.hip: k_front): LayerNorm + q|k|v with EPI_QKV_DEC's stores, the
// self-attention over the cache computed once per head (a form for <= 64 cells, one for longer caches), the out projection + residual (in place: xout = x).  gq: 3 S / 2
// granules, ga: S / 2 granules (8 bytes each, zeroed once); epoch / par / fault / spin_cap / withhold as in MlpPairArgs (own epoch words).
struct FrontArgs {
    const float * x; float * xout; const float * ln_g, * ln_b; float eps; int S;
    const __half * Wqkv; const float * bqkv; float scale; __half * q16; __half * ck, * cv;       // ck / cv: the layer's self cache [cell][S]
    const int32_t * kv_head, * n_kv; int cap;                                                    // the step record's cache head / key count; cells in the cache
    const __half * Wo; const float * bo;
    unsigned long long * gq, * ga; uint32_t * epoch; int par; uint32_t * fault; uint32_t spin_cap; int withhold;
    // lock-step rows (grid.y = row): row y has its own activation row (x + y S), q16 row, self cache (+ y cache_row_stride), step record
    // (+ y step_stride words) and granules (+ y 2 S); rows = 0 / 1: one row
    int64_t cache_row_stride; int step_stride; int rows;
};
// The back of the cross-attention of the one-row step as one launch (k_attn.hip: k_xback): LN + cross query + key slices, the combine of a
// head's slices (once per head) and the out projection + residual (in place: xout = x).  gp: H * ns * 66 granules of partials, ga: S / 2
// granules of the attention row (8 bytes each, zeroed once); epoch / par / fault / spin_cap / withhold as in MlpPairArgs (own epoch words).
// ks / ns / pmax / part_o / part_l are filled in by xback() from the cross-attention's scratch layout.
struct XbackArgs {
    const float * x; float * xout; const float * ln_g, * ln_b; float eps; int S;
    const __half * wq; const float * bq; float qscale; const __half * kc, * vc; int T, ks, ns;
    float * pmax, * part_o, * part_l;
    const __half * Wo; const float * bo;
    unsigned long long * gp, * ga; uint32_t * epoch; int par; uint32_t * fault; uint32_t spin_cap; int withhold;
    // lock-step rows (grid.z = row): row z has its own activation row (x + z S), cross cache (+ z kv_row_stride) and granules
    // (+ z XBACK_ROW_GRANULES); rows = 0 / 1: one row
    int64_t kv_row_stride; int rows;
};
constexpr int XBACK_ROW_GRANULES = 8 * 8 * 66 + 256;        // a row's partials (<= 8 heads x 8 slices x 66) + its attention row (S / 2 <= 256)
bool xback_usable(int S, int H, int T, int rows = 1);
void xback(XbackArgs a, int H, float * scratch, hipStream_t st);
// long_cap > 0: the long-cache form (caches of more than 64 cells, one row) for a cache of long_cap cells; front(): long_kv launches it
bool front_usable(int S, int rows = 1, int long_cap = 0);
void front(const FrontArgs & a, hipStream_t st, bool long_kv = false);
// front() and xback() of one layer as ONE launch (k_dec.hip: k_attn_join): workgroups [0, 3 S / 16) run k_front's body, the H x ns behind
// them k_xback's, and the residual row crosses from the first role's out projection to the second's LayerNorm as S granules {f32, tag}
// (gx, 8 bytes each, zeroed once) instead of through memory and a launch boundary.  f / x: the two launches' arguments, each with its own
// granules, epoch words and `withhold` (x.x is not read: the row arrives through gx; f.xout is not written: x.xout is the launch's only
// store of the row).  epoch: the hop's own pair of words, tags by MlpPairArgs' rules with f.par; time-outs and slow polls go to x.fault,
// the polls are bounded by x.spin_cap.  withhold: tests, front-role wavefront `withhold - 1` never publishes its granules of the row.
// One row, caches of <= 64 cells (the long-cache form of the front keeps its own launch), S <= 512.  Both roles are stamped: two slots
// of stamp_next(), the front's first, whose records overlap in time.
struct JoinArgs { FrontArgs f; XbackArgs x; unsigned long long * gx; uint32_t * epoch; int withhold; Stamp spx; };
bool attn_join_usable(int S, int H, int T);                 // front_usable(S) and xback_usable(S, H, T) hold, and the joined grid is resident at once
void attn_join(JoinArgs a, int H, float * scratch, hipStream_t st);
void xback_plan(XbackArgs & a, int H, float * scratch);     // fills ks / ns / pmax / part_o / part_l from the cross-attention's scratch layout
// A/B switches of the launch paths that are read from the environment: once per process (reload_knobs(): lab scripts that flip them between
// probe calls of one process, exported as wmi_reload_knobs — not while a transcription runs on another thread)
struct Knobs { bool no_mlp_pair; int sa_wpb; bool gemv1_wide_generic; bool host_draws; bool debug_sync; int pair_withhold; uint32_t pair_spin_cap; bool no_front; int front_withhold; bool no_xback; int xback_withhold; int front_wpb; bool no_join; int join_withhold; };
const Knobs & knobs();
void reload_knobs();
void set_attn_one_group(bool on);              // encoder attention: never split the keys over two wave groups (bit-identical for any batch)
bool rows_valu_enabled();
void set_rows_valu(bool on);                  // lock-step rows: true = VALU kernel (bit-identical to the one-row path), false = MFMA
int  mode_epoch();                             // bumped by every run-time switch that changes which kernels a step launches: a captured
void bump_mode_epoch();                        // step graph is replayed only under the epoch it was captured in

// ---------------------------------------------------------------- device-side logit filters + greedy pick (k_sample.hip)
// One decode step's dynamic inputs; lives in device memory, refreshed by a 64-byte H2D copy per step so that
// the captured HIP graph of the step stays static.
struct DecStep {
    int32_t token, pos, n_kv, kv_head;
    int32_t flags;                 // bit0 ban eot + " " (initial & suppress_blank) ; bit1 last token was a timestamp ; bit2 penultimate too
    int32_t space_id, eot, beg, n_vocab;
    int32_t ts_floor_end;          // timestamps in [beg, ts_floor_end) are banned (monotonic rule) ; = beg when inactive
    int32_t ts_initial_start;      // timestamps in [ts_initial_start, n_vocab) are banned (max_initial_ts) ; = n_vocab when inactive
    int32_t seq;                   // step sequence number, echoed in SampleOut::seq (the host polls pinned memory for it)
    float   temperature;           // > 0: logits are divided by it before the filters (W/whisper.cpp:4500-4506); 0 = as they are
    int32_t pad[3];
};
// Two self-tagged 16-byte halves: the pick kernel writes each half to pinned host memory with ONE 16-byte store, the host accepts
// a half when its tag (seq0 / seq) is the step it waits for — no fence, no read of host memory by the device (the fenced form,
// record + __threadfence_system + seq + fence, cost 0.65 us more per step: profiles/r03a_chain_lab_boundary_and_variants.txt)
struct alignas(16) SampleOut { int32_t id, tid; float p; int32_t seq0; float plog, pt, ptsum; int32_t seq; };
// logits [n_vocab] -> filtered soft-max statistics and the arg-max token (W/whisper.cpp:4493-4830 at temperature 0)
// n_rows > 1: lock-step chunks — logits [n_rows][n_vocab], step[n_rows], out[n_rows]
// chain (one row): the pick kernel also prepares the NEXT greedy step on the device — token = the pick, pos / n_kv / kv_head + 1 in
// *step_rw, and the next activation row x = te[pick] + pe[pos + 1] — so that the next step needs no embedding launch
struct ChainNext { DecStep * step_rw; const __half * te; const float * pe; float * x; int S; int n_pos;
                   const uint32_t * fault; };             // MlpPairArgs::fault of the step's launches (nullptr: none): reported in the tags, see SAMPLE_TAG_*
// SampleOut::seq0 / seq = the step's sequence number (SAMPLE_SEQ_MASK bits) | status of the step's in-launch hand-offs
constexpr int32_t SAMPLE_SEQ_MASK = 0x0FFFFFFF, SAMPLE_TAG_FAULT = 0x40000000, SAMPLE_TAG_SLOW = 0x20000000;
// fused_parts > 0 (one row): scratch already holds that many partials (GemvArgs::fs_part): only the pick kernel runs
void filter_argmax(const float * logits, const uint8_t * static_ban, const DecStep * step, SampleOut * out, void * scratch, hipStream_t st,
                   SampleOut * out_host = nullptr, int n_rows = 1, const ChainNext * chain = nullptr, int fused_parts = 0);
size_t filter_scratch_bytes(int n_rows = 1);
// Draws from the filtered distribution on the device (beam search candidates, t > 0 sampling: whisper_sample_token(best = false)
// and whisper_sample_token_topk, W/whisper.cpp:4777-4909).  The reference draws with std::discrete_distribution on the 51 866
// probabilities: id = first i with cdf(i) >= u, u = generate_canonical(mt19937).  The host keeps the generator and passes the
// uniform numbers u [n_rows][k]; the device filters the logits (same rules as filter_argmax), forms p = exp(l - lse), sums them in
// double (tree order) and finds the k ids per row — k (id, p, plog) and the timestamp statistics come back instead of 207 KB
// of logits per row.  out [n_rows][k] (SampleOut::seq = draw index); scratch: filter_draw_scratch_bytes.
void filter_draw(const float * logits, const uint8_t * static_ban, const DecStep * step, const double * u, int k, SampleOut * out,
                 void * scratch, hipStream_t st, int n_rows, int tid_default);
size_t filter_draw_scratch_bytes(int n_rows);
void filter_stats(const float * logits, const uint8_t * static_ban, const DecStep * step, FsPartial * part, hipStream_t st, int n_rows);
// The draft verifier (k_draft.hip): the filtered greedy picks of teacher-forced rows, checked against the draft on the device.
//   draft_pick:   behind filter_stats(logits, ban, steps, part, st, n_group) on a group of n_group <= 8 rows: group row g is row row0 + g of
//                 the call.  Its 64 partials are combined with k_filter_pick<.., 1>'s arithmetic (filter_combine.h) — the record equals
//                 filter_argmax's bit for bit — and stored to out_host[row0 + g] (pinned; two 16-byte stores tagged steps[g].seq);
//                 match[row0 + g] = 1 where row0 + g < n_targets and the pick is targets[row0 + g], else 0.  steps, part: the group's;
//                 targets, out_host, match: the call's.  targets holds at least one entry.
//   draft_finish: one wavefront behind the last group: accepted = the number of leading 1s of match[0 .. n_rows), {accepted, tag} as ONE
//                 8-byte store (pinned).
// Workgroups are independent inside every launch; no atomics.
struct DraftOut { int32_t accepted, tag; };
void draft_pick(const FsPartial * part, const DecStep * steps, const int32_t * targets, int row0, int n_group, int n_targets,
                SampleOut * out_host, int32_t * match, hipStream_t st);
void draft_finish(const int32_t * match, int n_rows, int32_t tag, DraftOut * out, hipStream_t st);
// Grammar-constrained decoding on the device (k_grammar.hip; the evaluator is grammar_eval.h).  grammar_reject: grid (ceil(eot / 256), rows),
// one thread per token id — reject [n_rows][n_vocab] gets ge::REJECTED / ge::ACCEPTED for ids below eot (the bytes from eot on are never
// written: the caller keeps them 0), overflow[row] = 1 (a plain store; the caller zeroes the words) when a token's working set exceeded its
// capacity; a row whose state says n_stacks < 0 is left alone.  states: device memory.
// grammar_argmax / grammar_draw: filter_argmax / filter_draw with the penalised second pass of W/whisper.cpp:4657-4709 — unless the
// unpenalised timestamp mass beats every text token, every rejected, allowed, finite text logit loses `penalty` behind the temperature
// division and the log-soft-max is taken again.  scratch: grammar_sample_scratch_bytes.
struct GrammarDev { const ge::Elem * elems; const uint32_t * rule_off; int n_rules; const uint8_t * vbytes; const uint32_t * voff; int eot; };
void grammar_reject(const GrammarDev & g, const ge::RowState * states, int n_rows, int n_vocab, uint8_t * reject, uint32_t * overflow,
                    hipStream_t st);
void grammar_argmax(const float * logits, const uint8_t * static_ban, const uint8_t * reject, float penalty, const DecStep * step,
                    SampleOut * out, void * scratch, hipStream_t st, int n_rows);
void grammar_draw(const float * logits, const uint8_t * static_ban, const uint8_t * reject, float penalty, const DecStep * step,
                  const double * u, int k, SampleOut * out, void * scratch, hipStream_t st, int n_rows, int tid_default);
size_t grammar_sample_scratch_bytes(int n_rows);
// first kernel of a replayed step: fetch DecStep from pinned host memory, mirror it on the device, embed the token
void dec_embed_step(const DecStep * host_step, DecStep * dev_step, int S, const __half * te, const float * pe, float * x, hipStream_t st,
                    int n_rows = 1);

// ---------------------------------------------------------------- block-quantised weights (k_quant.hip)
// The reference keeps q4_0 / q4_1 / q5_0 / q5_1 / q8_0 matrices quantised, turns every activation row of a mul_mat into
// q8_0 / q8_1 blocks and takes an integer dot per 32-element block, scaled by d_w * d_a (+ m_w * s_a)
// (SURVEY App. B rule 1; W/ggml-quants.c:837-870, 2442-3560).  Same here: the blocks stay quantised in HBM, the integer
// dots run on v_mfma_i32_32x32x32_i8 (one q block = the K of one instruction, so the dot of a block is exact), the
// per-block f32 scales are applied on the way out of the accumulator.
//
// HBM layout of a quantised matrix [N][K] ("tiles"): a tile = 32 weight rows x 2 blocks (K = 64) = 64 blocks, one per
// lane: lane (n = lane % 32, g = lane / 32) owns block 2 * tp + g of row 32 * tn + n.  A tile stores the 64 quant
// payloads first ([lane][QB bytes]), then the 64 headers ([lane][HB bytes]); tiles of a row group are consecutive
// in tp, row groups follow each other: tile index = tn * (K / 64) + tp.  A wavefront reads a tile with two fully
// coalesced loads; nothing is rewritten, the file's blocks are only permuted (headers of the 2- and 6-byte kinds are
// padded to 4 / 8 bytes).  N is padded to a multiple of 32 with zero blocks.
enum QType : int { QT_NONE = 0, QT_Q4_0 = 2, QT_Q4_1 = 3, QT_Q5_0 = 6, QT_Q5_1 = 7, QT_Q8_0 = 8 };   // ggml_type ids
struct QGeom { int qb, hb, file_bytes; bool has_m; };     // payload / header bytes of a block in the tile layout; *_1 kinds carry m
QGeom  q_geom(int qtype);
inline size_t q_tile_bytes(int qtype) { const QGeom g = q_geom(qtype); return (size_t) 64 * (g.qb + g.hb); }
inline size_t q_matrix_bytes(int qtype, int64_t N, int64_t K) { return (size_t) ((N + 31) / 32) * (size_t) (K / 64) * q_tile_bytes(qtype); }
// host: permute the ggml blocks of rows [0, N) (row stride K / 32 blocks of file_bytes) into the tile layout at dst
void   q_repack_host(int qtype, const uint8_t * src, int64_t N, int64_t K, uint8_t * dst);
struct QMat { const uint8_t * tiles = nullptr; int qtype = QT_NONE; };

// activation rows as q8 blocks in global memory (the GEMM's A operand): qs [M][K] int8; scales block-major d [K / 32][ldm],
// s [K / 32][ldm] (the GEMM fetches the scales of 64 / 128 consecutive rows of one block with one load per wavefront);
// s = d * sum(q) for the q8_1 kinds; for the q8_0 kinds d is rounded to f16 as the reference stores it and s = 0
// deq (optional): the same rows as f16(d * q) [M][K] — the A operand of the f16 form of qgemm; wdeq / wdeq_elems: scratch image for one
// dequantised weight matrix (or a group of cross K | V layers) [rows][K] f16
// wdeq_ready: the image already holds the matrix the next qgemm multiplies with (written by quantize_rows' fused launch)
// The form of a projection over q8 rows: the block-dot kernel (integer dots per block, the reference's arithmetic) or the f16 MFMA form (both
// operands expanded to f16, k_qdequant).  QFORM_BY_M: the f16 form from WMI_QGEMM_F16_ROWS rows of the LAUNCH on (qgemm_takes_f16_form(M)) —
// every one-chunk and uniform pass.  The two forms do not give the same bits, so a pass that stacks chunks with lengths of their own names
// the form each chunk's own one-chunk pass would take (batch.cpp: encode_rows) instead of letting the stacked M decide.
enum QForm : int { QFORM_BY_M = 0, QFORM_BLOCK_DOT = 1, QFORM_F16 = 2 };
// the side of the threshold: does a pass of `rows` activation rows take the f16 form when nothing else is said?  (host only)
bool qgemm_takes_f16_form(int rows);
struct Q8Rows { int8_t * qs; float * d; float * s; int ldm; __half * deq = nullptr; __half * wdeq = nullptr; size_t wdeq_elems = 0; bool wdeq_ready = false;
                const void * wdeq_of = nullptr;        // wdeq_of: the matrix (QMat::tiles) whose f16 image wdeq holds when wdeq_ready — qgemm checks it
                bool w_resident_ok = false;            // the caller's matrices may be kept as resident f16 images (the encoder's: k_quant.hip qweights_f16_get)
                int form = QFORM_BY_M; };              // which form the projection of these rows takes (QForm above): by the launch's M unless the caller names one
// rows -> q8.  Exactly one source: x32 (+ optional LayerNorm gain/bias: y = LN(x) * g + b in f32, the reference quantises that
// f32 tensor) or x16 (an f16 tensor, e.g. the GELU output, widened exactly).  out32 / out16: optional copy of the LN result.
// W_next / N_next (optional): the [N_next][K] matrix of the projection these rows feed.  When that projection will take the f16 form
// (qgemm), its weight image is written by the same launch; returns true then (the caller sets Q8Rows::wdeq_ready for that qgemm).
bool quantize_rows(const float * x32, const __half * x16, int M, int K, const float * ln_g, const float * ln_b, float eps,
                   int qtype, Q8Rows out, float * out32, __half * out16, hipStream_t st, const QMat * W_next = nullptr, int N_next = 0);

// C[M][N] = A_q8[M][K] . W_q[N][K]^T with the GEMM's epilogues (Epi above; GemmArgs fields A / W / lda / ldw unused).
// N % 128 == 0, K % 64 == 0.
void qgemm(int epi, const GemmArgs & a, Q8Rows A, QMat W, hipStream_t st);
// resident f16 images of the matrices the f16 form multiplies with (k_quant.hip: qweights_f16_get): bytes held by the process, and the
// release of every image whose matrix lies in the arena [lo, hi) (free_weights)
size_t qweights_f16_cached_bytes();
void   qweights_f16_release(const void * lo, const void * hi);
// rows [row0, row0 + rows) of a quantised matrix (row0 % 32 == 0) as f16(d * q + m) [rows][K]
void qdequant(QMat W, int64_t row0, int64_t rows, int K, __half * out, hipStream_t st);

// <= 32 activation rows against a quantised matrix: the weight tiles are streamed once, the rows are quantised in the
// prologue of every workgroup (LayerNorm of x32 if ln_g, plain f32 rows a32, or f16 rows a16) — GemvArgs as for gemv();
// the fused attention prologues (sa_*, comb_*) are not available here.
void qrows(const GemvArgs & a, const float * a32, QMat W, hipStream_t st);
bool qrows_ksplit_ok(const GemvArgs & a, int parts);        // may this launch split K over `parts` workgroups per row group (GemvArgs::ksplit)?
// the cross-attention of a row of a block-quantised model (more rows: WMI_Q_XATTN_ROWS, slower) with the query projection inside (LayerNorm(x32) . W_cq, scaled, f16) — one
// launch instead of qrows(EPI_Q_SCALED) + attn_cross_split_partials, the same bits; partials as attn_cross_split_partials.  pfW / pfN / pfK:
// the next weight-streaming launch's matrix (prefetched).  false: not available for this shape (nothing launched; take the two launches) —
// always so for rows with lengths of their own (row_lens->n > 0): this kernel has one key range for every row
bool qattn_cross_qsplit_partials(const float * x32, const float * ln_g, const float * ln_b, float eps, QMat Wcq, const float * bq, float qscale,
                                 int n, int S, int H, const __half * kc, const __half * vc, int T, float * scratch,
                                 const float ** po, const float ** pl, const float ** pm, int * pns, hipStream_t st, int64_t kv_row_stride,
                                 QMat pfW, int pfN, int pfK, const RowLens * row_lens = nullptr);

// token embedding gather from a quantised matrix: x[i] = dequant(te[token[i]]) + pe[pos[i]]   (W/ggml.c get_rows, dequantize_row_*)
void qdec_embed(const int32_t * tokens, const int32_t * pos, int n, int S, QMat te, const float * pe, float * x, hipStream_t st);
void qdec_embed_step(const DecStep * host_step, DecStep * dev_step, int S, QMat te, const float * pe, float * x, hipStream_t st, int n_rows = 1);

// misc
void touch(int * p, int blocks, hipStream_t st);     // trivial dependent kernel (launch-floor probe)
void fill_zero(void * p, size_t bytes, hipStream_t st);

}} // namespace wmi::k

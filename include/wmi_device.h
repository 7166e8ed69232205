/*
 * wmi_device.h — the thin device-level C ABI of libwhisper_mi355.so (new in this repository).
 *
 * whisper.h hands the library HOST buffers (the Godot host owns PackedFloat32Array /
 * PackedByteArray).  The entry points below are what a batching front end, the bench and the
 * parity tests bind: PCM that is already resident in HBM, access to the tensors the reference
 * keeps in its `whisper_state` (W/whisper.cpp:769-844), and the per-stage timers.
 * Shape follows the reference's encoder-plugin precedent
 * (W/openvino/whisper-openvino-encoder.h:12-27, W/coreml/whisper-encoder.h:14-22):
 * init / encode / free with plain pointers and sizes.  No torch types, no C++ types.
 *
 * Threading: a context owns one HIP stream and one set of activation / cache arenas; every entry point that touches them
 * (whisper_full*, whisper_encode / decode, *_with_state, wmi_full_batch, wmi_get_tensor, wmi_set_audio_ctx, the timers and
 * batch accessors) takes the context's recursive mutex, so calls on ONE context serialise (whisper.h:535 asks callers for
 * that anyway).  Concurrency comes from several contexts — one per device (wmi_pool_*) or several per device — which share
 * nothing but the process-wide switches wmi_set_lockstep_exact / WMI_* environment knobs.
 */
#ifndef WMI_DEVICE_H
#define WMI_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#include "whisper_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Library / device identification; aborts nothing, returns 0 on a box without a usable GPU. */
WHISPER_API int          wmi_device_count(void);
WHISPER_API const char * wmi_version(void);

/* Like whisper_init_from_buffer_with_params but pins the context to HIP device `device`
 * (one process per GPU: pass LOCAL_RANK).  replaces: W/whisper.h:151 for multi-GPU hosts. */
WHISPER_API struct whisper_context * wmi_init_from_buffer_on_device(const void * buffer, size_t buffer_size, int device);

/* Vocabulary + host-side decision logic only (tokenizer, logit filters, sampling): no device is touched
 * and every compute entry point (mel / encode / decode / whisper_full with audio) fails with an error.
 * Exists so the host logic can be unit-tested on machines without a GPU; it is NOT a CPU fallback. */
WHISPER_API struct whisper_context * wmi_init_host_only(const void * buffer, size_t buffer_size);

/* Multi-GPU load without re-parsing ("one RCCL broadcast of the packed weight blob").  The device weight
 * arena — every matrix already in the layout the kernels stream, quantised blocks still quantised — has the same byte layout on
 * every rank, because it is derived from the tensor directory alone:
 *   rank 0:      ctx = wmi_init_from_buffer_on_device(model, n, dev);  h = wmi_model_header(model, n, buf, cap)
 *   every rank:  receives the h bytes of buf (a ~1 MB header image: hyper-parameters, mel filters, vocabulary, tensor directory)
 *   rank != 0:   ctx = wmi_init_from_header(buf, h, dev)     -> arena allocated, ZEROED and laid out; the context is "weights
 *                pending": every compute entry point (mel / encode / decode / whisper_full / wmi_full_batch) fails with an error
 *   every rank:  ncclBroadcast(wmi_arena_ptr(ctx), wmi_weights_bytes(ctx, 0), root 0)   (godot-whisper_amd/shard.py)
 *   rank != 0:   wmi_arena_commit(ctx)                        -> device synchronised, the context may compute
 * The header image is accepted by wmi_init_from_header ONLY: whisper_init_from_buffer* and wmi_init_from_buffer_on_device reject it
 * (a context that "loads fine" and transcribes from an unfilled arena must not exist).
 * wmi_model_header returns the image size (call with out == NULL to size the buffer), 0 for an invalid model.
 * wmi_weights_bytes: which = 0 the whole arena, 1 the matrices only (what a decoded token streams; quantised models: their
 * blocks), 2 the ggml type of the quantised matrices (0: f16), 3 the bytes of resident f16 images of quantised ENCODER matrices held by
 * the process (opt-in, WMI_QENC_F16_CACHE=1: written on first use beside the blocks; 0 by default — the weights are held quantised only). */
WHISPER_API size_t wmi_model_header(const void * model, size_t model_size, void * out, size_t cap);
WHISPER_API void * wmi_arena_ptr(struct whisper_context * ctx);
WHISPER_API struct whisper_context * wmi_init_from_header(const void * header, size_t header_size, int device);
WHISPER_API int    wmi_arena_commit(struct whisper_context * ctx);      /* 0 ok; < 0: no arena / device error */
WHISPER_API int    wmi_weights_pending(struct whisper_context * ctx);   /* 1 while a header-image context waits for its arena */
WHISPER_API size_t wmi_weights_bytes(struct whisper_context * ctx, int which);

/* PCM already in HBM (f32 mono 16 kHz, device pointer on the context's device) -> log-mel in the
 * context.  replaces: whisper_pcm_to_mel (W/whisper.h:240) when the samples never touch the host. */
WHISPER_API int wmi_pcm_to_mel_device(struct whisper_context * ctx, const float * d_samples, int n_samples);

/* whisper_full over device-resident PCM: identical control flow and results, minus the H2D copy.
 * `h_samples_for_timestamps` may always be NULL: the |x| envelope of the token timestamps (W/whisper.cpp:5003-5010) is computed on the
 * device from the samples the log-mel stage has just staged, the host pointer is never read (kept for source compatibility). */
WHISPER_API int wmi_full_device_pcm(struct whisper_context * ctx, struct whisper_full_params params,
                                    const float * d_samples, int n_samples, const float * h_samples_for_timestamps);

/* Several GPUs behind ONE host process (a Godot host is one process).  Ownership as in whisper_full_parallel
 * (W/whisper.cpp:5837-5913: shared read-only model, one state + one worker thread per piece, results gathered by the caller),
 * with a GPU per worker: devices[0] parses the file, the others receive the header image and a peer-to-peer copy of the
 * weight arena (nothing is re-parsed or re-quantised); chunk c -> devices[c mod n]; the chunks of a device advance in lock-step
 * (wmi_full_batch) on their own host thread; no collective and no cross-device traffic after the load.
 *   wmi_pool_full     host PCM pointers; returns whisper_full's codes (first failing device wins)
 *   wmi_pool_select   routes the whisper_full_n_segments / whisper_full_get_* accessors: returns the context that owns the
 *                     chunk's result, already selected (NULL for a bad index)
 * A device id may repeat (several contexts on one GPU: used by the tests on a one-GPU box). */
struct wmi_pool;
WHISPER_API struct wmi_pool * wmi_pool_init(const void * model, size_t model_size, const int * devices, int n_devices);
WHISPER_API void wmi_pool_free(struct wmi_pool * pool);
WHISPER_API int  wmi_pool_size(struct wmi_pool * pool);
WHISPER_API struct whisper_context * wmi_pool_context(struct wmi_pool * pool, int i);
WHISPER_API int  wmi_pool_full(struct wmi_pool * pool, struct whisper_full_params params, const float * const * pcm,
                               const int * n_samples, int n_chunks);
WHISPER_API struct whisper_context * wmi_pool_select(struct wmi_pool * pool, int chunk);
WHISPER_API int64_t wmi_pool_device_time_us(struct wmi_pool * pool, int i);

/* Host-adjacent DSP of the streaming node on the device, so that raw capture frames need not be touched by the
 * CPU.
 *   wmi_downmix_stereo   interleaved stereo f32 frames [n_frames][2] -> mono (x + y) / 2
 *                        replaces: _vector2_array_to_float_array, src/speech_to_text.cpp:45-51
 *   wmi_vad              SpeechToText::voice_activity_detection (src/speech_to_text.cpp:53-104, 378-399) on the last 3 s of
 *                        `pcm` (16 kHz mono): 1 = no voice activity in the last 500 ms, 0 = activity or fewer than 3 s of audio.
 *                        energies (optional, 2 floats) receives energy_all, energy_last.  The filter runs in blocks of 64 samples
 *                        side by side with a bitwise hand-over check between neighbours (wmi_selftest_vad): the sequential code's bits.
 * `on_device` != 0: the input (and `mono_out`) are device pointers on the context's device, else host pointers. */
WHISPER_API int wmi_downmix_stereo(struct whisper_context * ctx, const float * frames, int n_frames, int on_device, float * mono_out);

/* The node's 16 kHz resampler on the device.
 *   replaces: _resample_audio_buffer (src/speech_to_text.cpp:16-43) = libsamplerate's src_simple(&data, interpolator_type, 1)
 *             (thirdparty/libsamplerate/src/samplerate.c:469-483; SINC converters thirdparty/libsamplerate/src/src_sinc.c:283-427,
 *             src_zoh.c:59-126, src_linear.c:61-135)
 * converter: the host's InterpolatorType (src/speech_to_text.h:151-156), all five values:
 *   0 = SRC_SINC_BEST_QUALITY    answers -10: its coefficient table is a missing blob of the reference checkout
 *   1 = SRC_SINC_MEDIUM_QUALITY
 *   2 = SRC_SINC_FASTEST         (what capture_stream_to_text.gd:76 asks for)
 *   3 = SRC_ZERO_ORDER_HOLD      each output repeats the input frame before its position
 *   4 = SRC_LINEAR               f32 difference of the two neighbours, double multiply and add, one rounding.  One frame in at a ratio
 *                                above 1 has no defined result (the library reads data_in[-1]): logged, 0 frames, no kernel runs
 * Any other value answers -1 before the device is touched.  Mono f32 frames at src_rate -> dst (room for dst_capacity >= int(n_frames * dst_rate / src_rate) frames) at dst_rate
 * (the host passes WHISPER_SAMPLE_RATE).  Returns the frames written — the host's result_size; equal rates copy — or 0 where
 * src_simple reports an error (ratio outside [1/256, 256]); < 0: -1 arguments, -2 / -3 device, -4 dst_capacity too small.
 * Every output frame equals the sequential CPU code bit for bit (SINC: double accumulators, taps in its order). */
WHISPER_API int wmi_resample(struct whisper_context * ctx, const float * src, int n_frames, int src_rate, int dst_rate, int converter,
                             int on_device, float * dst, int dst_capacity);
WHISPER_API int wmi_vad(struct whisper_context * ctx, const float * pcm, int n_samples, int on_device, float vad_thold, float freq_thold,
                        float * energies);

/* Capture session: the streaming node's step (bin/addons/godot_whisper/capture_stream_to_text.gd:69-120 — append the new capture frames,
 * resample the whole accumulation, VAD, transcribe) on frames that STAY in HBM.  The accumulated stereo frames and their 16 kHz PCM live
 * on the context's device for the life of the session and grow geometrically (frames_hint sizes the first allocation, there is no cap); a
 * push uploads the new frames only, through a pinned staging buffer of the session; the resampler reads the stereo frames directly,
 * folding each tap's frame as wmi_downmix_stereo does, and computes only the outputs a push can have changed.  Every value is what the
 * one-shot calls give on the whole accumulation, bit for bit.  Everything is queued on the state's stream; a call waits only where it
 * returns device results to the host (wmi_capture_vad once, wmi_capture_read_pcm, wmi_capture_full as whisper_full; a push of DEVICE frames
 * waits for its copy so that the caller's buffer is free on return).  The calls take the context's lock; free the session before its context.
 *   wmi_capture_init      NULL: bad arguments, a host-only / weights-pending context, converter 0 (no table) or outside 1 - 4
 *   wmi_capture_push      append [n_frames][2] f32 frames (host pointer, or device pointer with on_device != 0); returns the frames held,
 *                         < 0 on error (-1 arguments, -2 / -3 device); n_frames = 0 is a no-op
 *   wmi_capture_keep_last the node's `_accumulated_frames.slice(size - 0.2 * mix_rate)` (:111): keep the last n_frames; returns the frames held
 *   wmi_capture_resample  bring the PCM up to date.  Returns result_size exactly as wmi_downmix_stereo + wmi_resample on the whole
 *                         accumulation would (0 where src_simple errors; the frame count at equal rates, where only the fold runs);
 *                         *expected = frames * 16000 / mix_rate (src/speech_to_text.cpp:356).  Does not wait: the count comes from the
 *                         host-side plan.  The calls below bring the PCM up to date themselves when frames were pushed since.
 *   wmi_capture_pcm       device pointer to the PCM and its length (NULL, 0 when empty); valid until the next push / keep_last / free
 *   wmi_capture_read_pcm  copy of the PCM to the host; returns the samples written, -4 when capacity is too small
 *   wmi_capture_vad       wmi_vad's answer on the session's PCM; 0, without device work, with fewer than 3 s
 *   wmi_capture_full      whisper_full on the session's PCM; results through the whisper_full_* accessors of the context
 *   wmi_capture_stats     of the pushes since the previous resample and the last resample: out4 = { bytes copied host -> device, outputs
 *                         computed, outputs reused, 1 if everything was recomputed }.  Everything is recomputed on the first resample,
 *                         after keep_last dropped frames, after a converter error, and at rates whose positions come from the host's
 *                         table (closed_form = 0 of wmi_selftest_resample_plan, e.g. 22.05 kHz; the table is uploaded and counted too). */
struct wmi_capture;
WHISPER_API struct wmi_capture * wmi_capture_init(struct whisper_context * ctx, int mix_rate, int converter, int frames_hint);
WHISPER_API void          wmi_capture_free(struct wmi_capture * cap);
WHISPER_API int           wmi_capture_push(struct wmi_capture * cap, const float * frames_xy, int n_frames, int on_device);
WHISPER_API int           wmi_capture_keep_last(struct wmi_capture * cap, int n_frames);
WHISPER_API int           wmi_capture_resample(struct wmi_capture * cap, int * expected);
WHISPER_API const float * wmi_capture_pcm(struct wmi_capture * cap, int * n_samples);
WHISPER_API int           wmi_capture_read_pcm(struct wmi_capture * cap, float * dst, int capacity);
WHISPER_API int           wmi_capture_vad(struct wmi_capture * cap, float vad_thold, float freq_thold, float * energies);
WHISPER_API int           wmi_capture_full(struct wmi_capture * cap, struct whisper_full_params params);
WHISPER_API int           wmi_capture_stats(struct wmi_capture * cap, int64_t * out4);
/* The transcribe step of several capture sessions of ONE context in lock-step: brings every session's PCM up to date, then
 * wmi_full_batch_ctx over the sessions' device PCM.  Results per session index through wmi_batch_select & co.
 * audio_ctx[i] (NULL: params.audio_ctx for all) is session i's encoder length, e.g. the node's total_time * 50 + 128.  The call takes the
 * context's lock once and copies no PCM: it hands on the pointers wmi_capture_pcm returns.  -1 for n <= 0, a NULL session or sessions of
 * different contexts; -3 when a session is empty (as wmi_full_batch for an empty chunk), before any device work; else wmi_full_batch_ctx's codes. */
WHISPER_API int           wmi_capture_full_batch(struct wmi_capture * const * caps, int n, struct whisper_full_params params, const int * audio_ctx);
/* Host half of the session's incremental resample (no device needed): for an accumulation that grew from n_old to n_new frames at
 * src_rate -> 16 kHz, the first output the session recomputes (outputs below it are the same bytes for both inputs; 0 = everything, e.g.
 * at rates without a closed form) and the frame counts of both plans.  Returns 0, -1 bad arguments, or the converter error of the new plan. */
WHISPER_API int wmi_selftest_capture_plan(int n_old, int n_new, int src_rate, int converter, long long * first_dirty,
                                          long long * n_out_old, long long * n_out_new);
/* Test hook for the two forms of the energy VAD on a host window of n samples (_vad_simple, src/speech_to_text.cpp:68-104, with the
 * host's high-pass filter): form 0 = the sequential kernel (one lane, sample order: the definition), form 1 = the filter in blocks of 64
 * samples, a lane each, started `warm` samples early (0 .. 64; < 0: the default, 32) with the bitwise hand-over check and re-run, which is
 * what wmi_vad and the session run.  Same decision and energy bits.  stats2 (optional) = { blocks, blocks re-run } (0 0 for form 0).
 * Returns the decision; 0 without device work when sample_rate * last_ms / 1000 >= n; -1 arguments, -2 / -3 device. */
WHISPER_API int wmi_selftest_vad(struct whisper_context * ctx, const float * pcm, int n, int sample_rate, int last_ms, float vad_thold,
                                 float freq_thold, int form, int warm, float * energies, int32_t * stats2);

/* Several independent chunks on one GPU in lock-step (BASELINE config 4: 8 chunks per GPU).  Every chunk is
 * transcribed as by whisper_full(ctx, params, pcm[c], n_samples[c]) on a freshly initialised context
 * (params.no_context = true, decoder RNGs at their initial seed);
 * the chunks share the weights and advance together: encoder GEMMs over all chunks at once (M = chunks * n_ctx),
 * one decode step = one token for every chunk.  Up to 16 chunks advance together; more are processed in groups of 16.
 * replaces: the per-worker loop of whisper_full_parallel (W/whisper.cpp:5809-5935: shared model, one
 * whisper_state per worker) — workers are rows of the same kernels instead of threads.
 * Lock-step needs greedy sampling at temperature 0 without callbacks; otherwise, and for any chunk that triggers the
 * temperature fallback, the chunk is run alone through the whisper_full driver.  The language need not be known: with
 * params.language "auto" / empty / NULL (or params.detect_language) a multilingual model detects every chunk's language in ONE
 * lock-step step in front of the windows — the encoder over all chunks at seek 0 and the full audio context (each chunk is
 * whisper_full on a fresh context), <sot> through the decoder layers, the language head (100 logits per chunk) — after which the
 * chunks' prompts differ in their language token only, which the per-row step records carry anyway.  The first window reuses that
 * encoder pass when params.audio_ctx and params.offset_ms are 0.  Chunks shorter than 1 s are detected too and report their
 * language without segments; an empty chunk makes the call return -3 (as whisper_full does) before any device work of its group;
 * with params.detect_language the call ends after the detection.  English-only models with "auto" keep the one-at-a-time path.
 * wmi_batch_lang_id / wmi_batch_lang_probs read the results.
 * pcm[c] are host pointers, or device pointers when pcm_on_device != 0.  Returns whisper_full's codes. */
WHISPER_API int wmi_full_batch(struct whisper_context * ctx, struct whisper_full_params params, const float * const * pcm,
                               const int * n_samples, int n_chunks, int pcm_on_device);
/* wmi_full_batch with an encoder length per chunk: chunk c is transcribed as whisper_full with params.audio_ctx = audio_ctx[c]
 * on a fresh context (0 = the model's n_audio_ctx).  audio_ctx == NULL: params.audio_ctx for every chunk (= wmi_full_batch).
 * The chunks still share every launch: the rows of a group are stacked with a common row period (the group's largest length rounded up
 * to 16), and the kernels that must know a row's own length — mel slice, conv guard rows, encoder attention, decoder cross-attention —
 * take the lengths by value; each row's cross-attention uses the key slices the one-chunk path takes at its length.  The call orders its
 * lock-step chunks by length (longest first) before dealing them into groups of 16 and into wmi_set_lockstep_groups ranges, and reports
 * results in the caller's order; in the exact mode (wmi_set_lockstep_exact) a chunk's result does not depend on that order, on the other
 * chunks or on the grouping, and equals whisper_full's bit for bit.  With lengths given, a single chunk runs in lock-step form too.
 * Block-quantised models stack their chunks the same way, with one rule more: the projections of a quantised encoder pass run in one of
 * two forms — the block-dot kernel below WMI_QGEMM_F16_ROWS (256) activation rows, the f16 MFMA form from there on — and the two do not
 * give the same bits.  In a pass whose rows have lengths of their own every projection takes the form the chunk's own one-chunk pass takes,
 * not the form the stacked row count would select; so the ordered chunks are cut where their lengths cross that threshold and each side is
 * a lock-step call of its own: at most two calls (one when all lengths lie on one side — the node's total_time * 50 + 128 reaches 256 from
 * 2.56 s of audio on).  Each chunk's encoder attention likewise splits its keys as its own pass does (the activation quantiser behind it
 * amplifies what another summation order changes), so the encoder values of a chunk are its one-chunk pass's in the default mode too.
 * Calls whose chunks all have one length (audio_ctx == NULL, equal entries) choose by their stacked row count, as ever.
 * With the two-launch cross-attention (WMI_XATTN_TWO_PASS) the rows carry ONE length per launch: there the ordered chunks are cut into
 * sets of equal length, each a lock-step call of its own — same results, launches shared within a set only.
 * wmi_get_batch_timings reports the sums over the calls made; wmi_batch_enc_dims describes the last of them.
 * Any entry above the model's n_audio_ctx: -5 (whisper_full's message); a negative entry: -1; both before any device work. */
WHISPER_API int wmi_full_batch_ctx(struct whisper_context * ctx, struct whisper_full_params params, const float * const * pcm,
                                   const int * n_samples, const int * audio_ctx, int n_chunks, int pcm_on_device);
/* The plan of wmi_full_batch_ctx for n chunks with the encoder lengths audio_ctx[0 .. n) (0 = n_audio_ctx) on a model with that n_audio_ctx,
 * block-quantised or not (host only, no device, no context): order[i] = the chunk at position i of the order the call gives its chunks
 * (longest first, stable; the caller's order when all lengths are equal), set_of[i] = the lock-step call (0, 1, ...) position i lands in.
 * wmi_full_batch_ctx plans with the same function.  Returns the number of calls; -1 on a bad argument (NULL, n < 1, n_audio_ctx < 1, an
 * entry below 0 or above n_audio_ctx). */
WHISPER_API int wmi_selftest_lockstep_sets(const int * audio_ctx, int n, int n_audio_ctx, int quantised, int * order, int * set_of);
/* Layout of the last batched encoder pass, for the stage tests: rows, the row period of "batch_enc_x" / "batch_cross_k" / "batch_cross_v"
 * (rows between consecutive chunks; = the common T for a uniform call), and each row's own encoder length into row_T[0 .. rows).
 * Any pointer may be NULL.  -1 when there has been no such pass. */
WHISPER_API int wmi_batch_enc_dims(struct whisper_context * ctx, int * rows, int * row_period, int * row_T);
/* Lock-step projections run on the matrix cores by default (f32 sums in MFMA order), and a one-chunk encoder splits
 * the attention keys over two wavefront groups (partial sums added at the end).  on != 0 keeps the projections on the
 * weight-streaming VALU kernel and the attention on one group for every batch size: wmi_full_batch and whisper_full
 * then agree bit for bit (used by the parity tests; process-wide debug switch, set it before both calls). */
WHISPER_API void wmi_set_lockstep_exact(int on);
/* Make the whisper_full_n_segments / whisper_full_get_* accessors (W/whisper.h:541-575) read chunk `chunk` of the
 * last wmi_full_batch call; whisper_full_lang_id(ctx) is that chunk's language id from then on.  Returns its segment count, -1 for a
 * bad index. */
WHISPER_API int wmi_batch_select(struct whisper_context * ctx, int chunk);
/* 0: chunk `chunk` was decoded in lock-step; 1: it was run alone (fallback, see above); -1: bad index. */
WHISPER_API int wmi_batch_chunk_mode(struct whisper_context * ctx, int chunk);
/* Language of chunk `chunk` of the last wmi_full_batch call: the id whisper_full_lang_id would report after whisper_full on that chunk
 * (detected, or params.language's; a chunk that left lock-step reports what its own whisper_full run detected).  -1: bad index. */
WHISPER_API int wmi_batch_lang_id(struct whisper_context * ctx, int chunk);
/* The 100 language probabilities of that chunk's detection (whisper_lang_auto_detect's lang_probs) into probs100.  0, or -1 for a bad
 * index / a chunk whose language was not detected (known language, English-only model). */
WHISPER_API int wmi_batch_lang_probs(struct whisper_context * ctx, int chunk, float * probs100);

/* whisper_lang_auto_detect (W/whisper.cpp:3569-3650) through the language head: the encoder at offset_ms, <sot> through the decoder
 * layers, then the final LayerNorm and the 100 token-embedding rows behind <sot> only (k_lang_head) instead of the vocabulary
 * projection — 400 bytes cross PCIe instead of the logits.  Same ids, same probabilities (the 100 logits equal the projection's entries
 * bit for bit and both routes share the host soft-max), same return codes (-1 offset before the audio, -2 past its end, -6 encode, -7
 * decode); lang_probs may be NULL.  Unlike after whisper_lang_auto_detect, whisper_get_logits is NOT defined afterwards.  whisper_full
 * detects this way ("auto"), and skips its first encoder pass when the detection has encoded that window.
 * How the 400 bytes arrive: the kernel stores them straight into pinned host memory and the host takes them behind ONE stream
 * synchronisation at the end of the step — not by polling a tag as the greedy step's SampleOut is polled (100 floats are 25 separate
 * 16-byte stores; a tag per piece was not built).  There is no separate wait behind the log-mel / encoder either way. */
WHISPER_API int wmi_lang_detect(struct whisper_context * ctx, int offset_ms, float * lang_probs);
/* Lock-step calls in GROUPS side by side: wmi_full_batch deals its lock-step chunks to `n` contiguous ranges, each a lock-step call of its
 * own — range 0 on this context, the others on replica contexts (own state, stream and work set; the weights are borrowed) on host threads
 * of their own.
 * n = 0: the default (two groups from 16 chunks on — measured: 16 chunks 9.1 -> 8.3 ms per call, 8 chunks level; WMI_LOCKSTEP_GROUPS
 * overrides), 1: one chain.  A chunk's result does not depend on the grouping in the
 * exact mode (wmi_set_lockstep_exact); in the default mode the usual last-bit differences between chunk counts apply.
 * Returns the previous setting, -2 for a null context. */
WHISPER_API int wmi_set_lockstep_groups(struct whisper_context * ctx, int n);

/* Chunks that cannot advance in lock-step (beam search, temperature > 0, quantised beams ...) are run through the whisper_full
 * driver, up to 1 + n of them at a time: n replica contexts (own whisper_state and stream, the weight arena shared read-only with
 * `ctx`, ~0.15 GB of state each for base.en, ~0.6 GB for large-v3) work beside `ctx`, chunk c on worker c mod (1 + n).
 * replaces: the worker threads of whisper_full_parallel (W/whisper.cpp:5837-5913: one shared model, one whisper_state per worker).
 * Results do not depend on n (every chunk is whisper_full on a fresh state).  n = 0: one chunk at a time; n < 0: the default (3, or
 * WMI_BATCH_REPLICAS).  Not used when params carry user callbacks or print_realtime.  Lowering n releases the surplus replicas at once
 * (their state memory and streams).  With n > 0 whisper_log_set's callback and the print_progress lines can be invoked from the
 * library's worker threads (one call at a time: the library serialises them).  Returns the previous setting (-1 = default), -2 for a
 * null context. */
WHISPER_API int wmi_set_batch_replicas(struct whisper_context * ctx, int n);

/* Wall-clock buckets of the last wmi_full_batch call, microseconds: mel + envelope, encoder, decoder steps,
 * segment emission + token timestamps; n_steps = lock-step decode steps.  (cf. whisper_timings, W/whisper.cpp:3672) */
WHISPER_API void wmi_get_batch_timings(struct whisper_context * ctx, int64_t * t4, int32_t * n_steps);

/* Encoder length override for the bare whisper_encode / whisper_decode calls, i.e. what whisper_full
 * does with params.audio_ctx (W/whisper.cpp:5098-5102); 0 = model default.  Returns -5 if too large. */
WHISPER_API int wmi_set_audio_ctx(struct whisper_context * ctx, int n_audio_ctx);

/* Copy an internal tensor out as f32 (f16 tensors are widened).  Returns the element count, or -1 for
 * an unknown name; with dst == NULL only reports the count.  Names and layouts (row-major):
 *   "mel"        [n_mel][n_len]                 log-mel (W/whisper.cpp:2779)
 *   "embd_conv"  [n_ctx][n_state]               conv front-end output (reference holds the transpose)
 *   "embd_enc"   [n_ctx][n_state]               encoder output
 *   "cross_k"    [n_text_layer][n_ctx][n_state] cross-attention keys (pre-scaled by d^-1/4)
 *   "cross_v"    [n_text_layer][n_ctx][n_state] cross-attention values (reference holds [state][ctx])
 *   "self_k" / "self_v"  [n_text_layer][3*n_text_ctx][n_state]
 *   "enc_x"      [n_ctx][n_state]               residual stream after the last encoder block
 *   "dec_cross_q" [rows][n_state]               the last text layer's scaled cross query of the last whisper_decode / prompt batch (f16)
 *   "dtw_matrix" / "dtw_q" / "dtw_jumps"        the last aligned window (wmi_set_token_dtw below)
 */
WHISPER_API int wmi_get_tensor(struct whisper_context * ctx, const char * name, float * dst, int n);
WHISPER_API int wmi_mel_dims(struct whisper_context * ctx, int * n_len, int * n_len_org, int * n_mel);

/* Stage timers in microseconds, the reference's counters (W/whisper.cpp:770-783):
 * t[0..5] = mel, encode, decode, batchd, prompt, sample ; n[0..4] = n_encode, n_decode, n_batchd, n_prompt, n_sample
 * What a timer measures: whisper_full on an f16 model does not wait behind the log-mel and the encoder (the decoder's launches queue up
 * behind them on the stream); their timers are then the GPU time of each phase, taken from stream events when the first decode step's
 * sample arrives, and the decode timer is the host's wall time minus what spilled over from those phases.  Every other path (the stage
 * calls whisper_pcm_to_mel / whisper_encode / whisper_decode, block-quantised models, lock-step calls, WMI_PHASE_SYNC=1) waits behind each
 * phase and records host wall time.  A consequence for errors: a device fault inside the deferred encoder surfaces at the first decode
 * step's wait, i.e. as whisper_full's "failed to decode" (-7 / -8) rather than "failed to encode" (-6); a faulted device fails every later
 * call either way.
 * n_encode counts the encoder passes that actually ran: whisper_full with language "auto" on one window reports ONE (the detection's pass
 * is the first window's when offset_ms is 0 and the audio context in effect at detection time — the previous call's, 0 on a fresh
 * state — is the one the call asks for), two otherwise. */
WHISPER_API void wmi_get_timings(struct whisper_context * ctx, int64_t * t6, int32_t * n5);

/* The context's HIP stream (as void*), so a caller can order its own work / events against the hot path. */
WHISPER_API void * wmi_stream(struct whisper_context * ctx);

/* Draws of beam search and temperature > 0 (whisper_sample_token / _topk, W/whisper.cpp:4777-4909) run on the device by default: the
 * host keeps each decoder's mt19937 and ships its uniform numbers, the device searches the cumulative distribution in double over
 * block sums (k_prob_blocks / k_draw).  CONTRACT: not bit-exact with std::discrete_distribution on the host — the partial sums are
 * associated differently and exp() is the device's, so a uniform number that falls within ~1e-7 of a cell boundary may select the
 * neighbouring token, after which that stream diverges like any sampled stream would (tests: test_device_draws_equal_host_draws
 * pins equality on its fixtures, not in general).  WMI_HOST_DRAWS=1 (environment, read per window) keeps the reference's definition:
 * logits come back to the host, whisper_process_logits + std::discrete_distribution run there, bit-exact given equal logits.
 * In device-draw mode the per-step logits stay in HBM: whisper_get_logits() is only defined after whisper_decode() / with
 * WMI_HOST_DRAWS=1 (greedy whisper_full also keeps them on the device).
 *
 * Host-logic probes used by the parity tests (same decisions as the reference given the same logits). */
WHISPER_API int wmi_process_logits(struct whisper_context * ctx, struct whisper_full_params params, const float * raw_logits,
                                   const whisper_token * hist, int n_hist, int has_ts, int seek_delta, float temperature,
                                   float * out_logits, float * out_logprobs, float * out_probs);
WHISPER_API int wmi_sample_draws(struct whisper_context * ctx, const float * probs, const float * logprobs, int n_draw,
                                 int reseed, whisper_token_data * out);

/* Kernel-level cross-check of the two decoder projection implementations (weight-streaming GEMV vs
 * MFMA GEMM) on identical random inputs; op: 0 self q|k|v, 1 self out, 2 cross q, 4 mlp.0, 5 mlp.2.
 * Returns the largest absolute difference over all outputs (negative on error). */
WHISPER_API double wmi_selftest_proj(struct whisper_context * ctx, int op, int n, int layer);

/* Test hook for the step whisper_full's greedy path runs (temperature 0, one decoder, no callbacks): decodes `token` at position `pos` of
 * the context's own state with that step, exactly as whisper_full would after two text tokens without timestamps (the default greedy
 * parameters' filters, the state counted busy).  The cache before `pos` is whatever whisper_decode / earlier steps left there; the step's
 * slot bookkeeping is whisper_decode's, so both may be mixed.  logits (optional): the step's raw logits, n_vocab floats; out: the token
 * the device picked (id, tid, p, plog, pt, ptsum); forms (optional): the launch form the step took, a bit set —
 *   1 cache longer than 64 cells, 2 chained onto the previous step's pick, 4 replayed from a captured graph, 8 both MLP projections as
 *   one launch, 16 the front of each layer as one launch (together with 1: that launch's long-cache form), 32 the cross-attention back
 *   as one launch, 64 re-run after a failed in-launch hand-off, 128 a slow hand-off was reported, 256 the block-quantised step,
 *   512 the front and the cross-attention back of each layer as ONE launch (only with 16 and 32, caches of <= 64 cells; WMI_NO_JOIN=1,
 *   WMI_NO_FRONT=1 or WMI_NO_XBACK=1 turns it off).
 * Returns 0, or a negative value on error. */
WHISPER_API int wmi_selftest_greedy_step(struct whisper_context * ctx, whisper_token token, int pos, float * logits, whisper_token_data * out,
                                         int * forms);

/* Test hook for the device logit filters, the greedy pick and the draws (csrc/k_sample.hip, the fused epilogue of the vocabulary projection
 * in csrc/k_dec.hip) on caller logits.  The static ban is uploaded from `params` exactly as whisper_full does; row r's step record is built
 * as whisper_full / wmi_full_batch build it from `params`, the row's token history (hist: the histories one after the other, n_hist[r]
 * tokens each), has_ts[r] and seek_delta[r]; `temperature` (> 0: the logits are divided by it) is written into every record.
 *   mode 0  the statistics pass + the pick (k_filter_stats, k_filter_pick) on logits [n_rows][n_vocab], 1 <= n_rows <= 16 (n_rows > 1: the
 *           lock-step form, the row on grid.y); out [n_rows]
 *   mode 1  the fused form of ONE row: the vocabulary projection with the statistics in its epilogue, then the pick.  The caller supplies
 *           the projection: W f16 [n_vocab][K] and an f32 row x [K]; logits = W . LayerNorm(x) with gain 1 and bias 0.  logits_out
 *           [n_vocab] receives the logits the launch wrote (`logits` is ignored).  -4 when these arguments do not take the fused path
 *           (K not a multiple of 8 or above 1536, a vocabulary below 16384); out [1]
 *   mode 2  k draws per row (k_filter_stats, k_prob_blocks, k_draw) with the caller's uniform numbers u [n_rows][k], 1 <= n_rows <= 8,
 *           1 <= k <= 8; tid_default: the tid reported when every timestamp probability underflows; out [n_rows][k]
 * out: id, tid, p, plog, pt, ptsum of every pick / draw.  The hook allocates and frees its own device memory.
 * Returns 0; -1 bad arguments, -2 the context cannot compute (host-only, weights pending), -3 device error, -4 see mode 1.  Every
 * argument error returns before the device is touched. */
WHISPER_API int wmi_selftest_filters(struct whisper_context * ctx, struct whisper_full_params params, int mode, int n_rows,
                                     const float * logits, const whisper_token * hist, const int * n_hist, const int * has_ts,
                                     const int * seek_delta, float temperature, const void * W, const float * x, int K, float * logits_out,
                                     const double * u, int k, int tid_default, whisper_token_data * out);

/* Host half of wmi_resample on its own (no device needed; CPU-side tests): the frame counts src_simple reports for n_frames
 * mono frames at src_rate -> dst_rate (output capacity int(n_frames * ratio) as the host passes it), and the first n_pos output
 * positions (integer sample, fraction) the kernel would use.  converter: 1 - 4 as for wmi_resample.  Returns 0, or the converter error as
 * wmi_resample logs it (-6 ratio, -10 no such converter or table, -31 SRC_LINEAR on one frame at a ratio above 1).
 * closed_form: 1 when the positions come from the exact 128-bit product, 0 when the host ran the double recurrence. */
/* Test hook for the device form of the token timestamps' envelope side (csrc/k_mel.hip k_ts_refine; opt-in, WMI_TS_DEVICE=1):
 * `envelope` [n] is a host array standing in for the |x| envelope; for each of the n_tok tokens, s0s1[2 t] / s0s1[2 t + 1] are its start / end
 * sample.  Writes per token sums[t] = the sequential f32 sum of envelope[max(s0 - 2000, 0) .. min(s1 + 2000, n)), thold[t], and
 * walks[6 t ..] = { en[s0] > thold, en[s1] > thold, walk_down_while_above(s0), walk_up_while_below(s0, s1), walk_up_while_above(s1, n - 1),
 * walk_down_while_below(s1, 0) } — the loops of W/whisper.cpp:6540-6590.  Returns 0, or < 0 on argument / device errors. */
WHISPER_API int wmi_selftest_ts_refine(struct whisper_context * ctx, const float * envelope, int n, const int * s0s1, int n_tok,
                                       float * sums, float * thold, int * walks);
WHISPER_API int wmi_selftest_resample_plan(int n_frames, int src_rate, int dst_rate, int converter, long long * frames_gen,
                                           long long * frames_used, int * closed_form, int n_pos, long long * pos, double * frac);

/* Block-quantised kernels on caller data (parity tests, no context needed): w_blocks = the ggml blocks of an [N][K] matrix of
 * type `qtype` (ggml_type id: 2 q4_0, 3 q4_1, 6 q5_0, 7 q5_1, 8 q8_0; W/ggml-quants.h:10-47) exactly as a model file holds them,
 * x = f32 activation rows [M][K], all host pointers.  The rows are quantised to q8 blocks as the reference's mul_mat does
 * (W/ggml-quants.c:837-870) and multiplied with the integer-dot kernels:
 *   mode 0  weight-streaming row kernel (M <= 32)        mode 1  tiled GEMM (N % 128 == 0)
 *   mode 2  x ignored; M token ids in `tokens`: out[M][K] = dequantised rows `tokens[i]` of the matrix (get_rows)
 *   mode 3  the large-M form of mode 1 (N % 128 == 0): the same q8 rows as f16(d_a q_a) against the blocks as f16(d_w q_w + m_w) on the
 *           f16 MFMA GEMM, f32 accumulation (what encode uses from 256 activation rows on; WMI_QGEMM_F16_ROWS=0 keeps mode 1's kernel)
 *   mode 4  mode 3 through the product's own route: the row quantiser's launch also expands the weight blocks, then the projection
 *           (M >= 256; fails with -3 when that route is not taken)
 * out [M][N] f32 (mode 2: [M][K]); out_qs [M][K] int8 and out_ds [M][K/32][2] {d, s} receive the quantised rows when non-NULL.
 * Returns 0, or a negative value on a bad argument / device error. */
WHISPER_API int wmi_selftest_quant(int device, int qtype, int mode, const void * w_blocks, const float * x, const int32_t * tokens,
                                   int M, int N, int K, float * out, int8_t * out_qs, float * out_ds);

/* The encoder self-attention kernels on caller operands (parity tests, no context needed; tests/test_gpu_attn_encoder.py).  All host
 * pointers; q, k [B][qk_rows][S] and v [B][Tpad][S] (time-major) are f16 bit patterns.  The hook lays v out as the V^T image
 * [B][S][Tpad] the kernels read (time index with bits 2 and 3 swapped, the order the q|k|v epilogue writes), fills `out` — [B][out_rows][S],
 * f16 or, with want_f32, f32 — with `sentinel` (its low 16 bits for f16), launches once and copies all of `out` back.
 *   T        the launch's (largest) length; row_T (NULL, or B entries in [1, T]): a length per chunk, as lock-step chunks have (used from B = 2 on)
 *   form     2 one sweep with a running maximum, 1 exact maximum first, 0 the first kernel (16-row wavefronts) — WMI_ATTN_FORM's values
 *   groups   0 one key group, 1 the keys split over wave groups (four; form 0: two), -1 what the product decides for this launch
 * Returns 0; -1 for what the product never launches (S != 64 H, Tpad % 64, Tpad / qk_rows / out_rows < T, B > 16, a row_T entry outside
 * [1, T], groups = 1 below T = 512 (form 0: 256)) — decided before the device is touched; -2 / -3 on a device error. */
WHISPER_API int wmi_selftest_attn_encoder(int device, int B, int T, int Tpad, int S, int H, int qk_rows, int out_rows, const int32_t * row_T,
                                          int want_f32, int form, int groups, const uint16_t * q, const uint16_t * k, const uint16_t * v,
                                          uint32_t sentinel, void * out);
/* The encoder's q|k|v projection with its split epilogue on caller operands: xn [M][S] and W [3 S][S] as f16 bit patterns, bias [3 S] f32.
 * rows_per_chunk = 0: one chunk of M rows; else M = chunks x rows_per_chunk (<= 16 chunks), each chunk with its own V^T image.  The
 * arguments of the launch are the encoder's (ldaux2 = Tpad, chunk_stride_aux2 = S * Tpad).  q, k [out_rows][S] (out_rows >= M) and the raw
 * V^T image vt [chunks][S][Tpad] are filled with `sentinel` first and come back whole.  Returns 0; -1 bad argument (before the device is
 * touched: S % 64, Tpad % 64, rows_per_chunk > Tpad or not dividing M, out_rows < M); -2 / -3 on a device error. */
WHISPER_API int wmi_selftest_qkv_encoder(int device, int M, int S, int Tpad, int rows_per_chunk, const uint16_t * xn, const uint16_t * W,
                                         const float * bias, uint32_t sentinel, int out_rows, uint16_t * q, uint16_t * k, uint16_t * vt);
/* The decoder's self-attention kernels on caller operands (tests/test_gpu_attn_decoder.py; no context).  All host pointers; q [n][S] and the
 * caches kc, vc [cache_rows][cap][S] are f16 bit patterns, uploaded as given.  `out` — [out_rows][S], f16 or, with want_f32, f32 — is filled
 * with `sentinel` (its low 16 bits for f16) first, one launch on one stream, all of `out` comes back.
 *   form 0   attn_decoder: n rows against ONE cache (cache_rows = 1) of n_kv[0] cells with the additive mask [n][n_kv[0]] (f32, as given);
 *            via_dev: n_kv travels through device memory with n_kv_max = cap (the graph-replay route)
 *   form 1   self_attn_rows: row r against its own cache (cache_rows = n <= 16, cache_row_stride = cap S) with n_kv[r] cells, read from
 *            step records sizeof(DecStep) apart; long_cache: the four-wavefront form (some row must have more than 64 cells)
 *   form 2   gemv with the sa_* prologue and EPI_F32_BIAS_RESID as the out projection is set up (one row: device.cpp; n rows: `lanes`, where
 *            gemv_rows_take_self_attention says yes), W_o = identity, no bias, a zero residual: the f32 result (want_f32 must be set) IS
 *            the f16 attention row
 * Returns 0; -1 for what the product never launches (S != 64 H, S > 1280, cap > 448, a cell count outside [1, cap], form 0: n > cap or
 * n_kv < n; forms 1, 2: n > 16, ...) — decided before the device is touched; -2 / -3 on a device error. */
WHISPER_API int wmi_selftest_attn_decoder(int device, int form, int n, int S, int H, int cap, int cache_rows, const int32_t * n_kv, const float * mask,
                                          int via_dev, int long_cache, int want_f32, const uint16_t * q, const uint16_t * kc, const uint16_t * vc,
                                          uint32_t sentinel, int out_rows, void * out);
/* The decoder's cross-attention on caller operands: kc, vc [kv_rows][T][S] f16 (kv_rows = 1, or n with kv_row_stride = T S), `out` as above.
 *   form 0   attn_cross_split (q [n][S] f16)
 *   form 1   attn_cross_split_partials, then consumer 0 = attn_cross_combine, 1 = gemv with comb_* and an identity out projection as above
 *            (want_f32; lanes = 0: one row takes k_gemv1, 2 .. 8 rows k_gemv; lanes = 1: lock-step rows — the one-row kernel per row up to
 *            S = 512, k_rows_mfma above)
 *   form 2   attn_cross_qsplit_partials with LN gain 0, W_cq = 0 and q [S] f32 as the projection's bias — every row's query is
 *            f16(q * qscale) — then attn_cross_combine
 * row_lens (forms 1, 2; NULL or n entries in [1, T], the largest equal to T, kv_rows = n): a length per row, as lock-step chunks have.  The
 * scratch starts as f32 NaNs (0x7FC5A5A5), whatever `sentinel` and the output type.  pmax, part_l [n][H][ns] and part_o [n][H][ns][64] (forms 1, 2; room for ns = 16) take the raw partials,
 * info[2] = {ns, 1 one-launch form / 0 two launches (WMI_XATTN_TWO_PASS)}.  Returns as above (T <= 1500, n <= 16, per-row lengths need the
 * one-launch form, ...). */
WHISPER_API int wmi_selftest_attn_cross(int device, int form, int consumer, int n, int S, int H, int T, int kv_rows, const int32_t * row_lens,
                                        int want_f32, int lanes, const void * q, float qscale, const uint16_t * kc, const uint16_t * vc,
                                        uint32_t sentinel, int out_rows, void * out, float * pmax, float * part_l, float * part_o, int * info);
/* gemm()'s decision without a launch (host only, no device): the plan for epilogue `epi` (kernels.h Epi: 0 F16_BIAS, 1 F16_BIAS_GELU,
 * 2 F32_BIAS_RESID, 3 CONV2, 4 QKV_ENC, 5 QKV_DEC, 6 CROSS_KV, 7 Q_SCALED) at (M, N, K), split width S, on a device of n_cu compute units,
 * with none of the WMI_GEMM_* lab switches.  out[10] = {kernel (1 k_gemm, 8 k_gemm8), BM, BN, wavefronts, ring depth (k_gemm8: of the A
 * image), ring depth of the W image, 1 DMA ring / 0 register-staged loop, orientation rule (0 first, 1 transposed, 2 per tile: q and k
 * transposed, V^T first), k extent of a slot, epi}.  Returns 0; -1 bad argument. */
WHISPER_API int wmi_selftest_gemm_plan(int epi, int M, int N, int K, int S, int n_cu, int * out);
/* One f16 GEMM with its epilogue on caller operands, through gemm() — or, with force8_bm in {128, 192, 288}, through gemm8() directly.  No
 * context, no model.  A: f16 bit patterns, exactly (M - 1) lda + K elements (lda < K: the convolutions' implicit GEMM); W [N][K]; bias [N]
 * f32 (NULL: none, for the epilogues that allow it); resid f32: [M][N] for F32_BIAS_RESID (in_place = 1: placed in C and passed as
 * resid == C, as the product does), the positional rows [rows_per_chunk - 4 or M][N] for CONV2.  The arguments are filled as encode(),
 * encode_rows() and the decoder's projections fill them, with leading dimensions ld = (S for the split epilogues, else N) + ld_pad:
 *   C     [out_rows][ld] f16 or f32 (CROSS_KV: [n_layers][out_rows][ld], layer stride out_rows x ld)
 *   aux   CONV2 [out_rows][ld] f32 (NULL: not written) | QKV_ENC, QKV_DEC k [out_rows][ld] | CROSS_KV v [n_layers][out_rows][ld]
 *   aux2  QKV_ENC the raw V^T image [chunks][S][Tpad] | QKV_DEC v [out_rows][ld]
 * every one filled with `sentinel` (its low 16 bits for f16) first and copied back whole; out_rows >= M + 16.  plan_out[11]: the plan that
 * served the call, as wmi_selftest_gemm_plan reports it, and in [10] the device's CU count the dispatch used.  Returns 0; -1 for a bad argument or a shape whose launch could leave its
 * buffers — decided before the device is touched; -2 / -3 on a device error. */
WHISPER_API int wmi_selftest_gemm(int device, int epi, int M, int N, int K, int lda, int S, float scale, int n_layers, int rows_per_chunk,
                                  int conv2_out_rows, int Tpad, int ld_pad, int in_place, int force8_bm, const uint16_t * A,
                                  const uint16_t * W, const float * bias, const float * resid, uint32_t sentinel, int out_rows, void * C,
                                  void * aux, void * aux2, int * plan_out);
/* Its block-quantised twin: the block-dot GEMM's q|k|v split epilogue (what a quantised encoder pass launches below the f16 threshold, and a
 * stacked pass of short chunks at any row count).  x [M][S] f32 rows, quantised to q8 blocks as wmi_selftest_quant does; w_blocks = the ggml
 * blocks of the [3 S][S] matrix of type `qtype` as a model file holds them; the rest as wmi_selftest_qkv_encoder.  No context.  Returns 0;
 * -1 bad argument, before the device is touched (an unknown qtype, S % 128, Tpad % 64, rows_per_chunk > Tpad or not dividing M, more than 16
 * chunks, out_rows < M, a NULL pointer); -2 / -3 on a device error. */
WHISPER_API int wmi_selftest_qkv_encoder_q(int device, int qtype, int M, int S, int Tpad, int rows_per_chunk, const float * x,
                                           const void * w_blocks, const float * bias, uint32_t sentinel, int out_rows, uint16_t * q,
                                           uint16_t * k, uint16_t * vt);

/* Kernel micro-benchmarks on synthetic operands (used by bench.py for the roofline line):
 * runs `iters` launches on the context stream between two HIP events, returns average microseconds.
 *   which = 0  encoder MLP-0 GEMM  [T x 4S x S] f16 MFMA   (flops = 2*T*4S*S)
 *   which = 1  logits GEMV         [n_vocab x S] weight stream (bytes = n_vocab*S*2)
 *   which = 2  encoder attention   one layer
 *   which = 3  full encode (conv + L blocks + cross) — same as whisper_encode without the host sync per call
 *   which = 4  encoder MLP-0 GEMM over the lock-step work buffers [chunks*T x 4S x S] (after a wmi_full_batch call)
 *   which = 5  encoder attention, all lock-step chunks, one layer
 *   which = 6  the logits projection over a rotating set of copies of the matrix (> 256 MiB in total): an HBM figure, where
 *              which = 1 re-streams one matrix that the 256 MiB Infinity Cache holds
 *   which = 10..12  chains of trivial dependent kernels on 1 / 32 / 256 workgroups (launch floor)
 *   which = 13  the language head (k_lang_head: final LayerNorm + the 100 language rows of the token embedding) on the row which = 1
 *               projects — what a detection step runs instead of which = 1 (f16 models; -1 on a block-quantised model, whose
 *               language head is the row kernel over a slice of the matrix)
 *   which = 20  the kernels of the last greedy decode step back to back, no host in the loop (microseconds per step);
 *               the environment variable WMI_STEP_MASK selects kernel kinds (bit 0 embed, 1 q|k|v, 2 self-attention + out,
 *               3 cross scores, 4 cross combine + out, 5 mlp.0, 6 mlp.2, 7 logits, 8 filters)
 *   which = 21..36  the same for the lock-step step of (which - 20) chunks
 */
WHISPER_API double wmi_bench_kernel(struct whisper_context * ctx, int which, int iters);

/* The A/B switches that the launch paths read from the environment (WMI_NO_MLP_PAIR, WMI_SA_WPB, WMI_GEMV1_WIDE_GENERIC,
 * WMI_HOST_DRAWS, WMI_DEBUG_SYNC, WMI_PAIR_WITHHOLD, WMI_PAIR_SPIN_CAP, WMI_NO_FRONT, WMI_FRONT_WITHHOLD, WMI_NO_XBACK, WMI_XBACK_WITHHOLD) are read ONCE per process; a lab script that flips them between
 * probe calls of one process calls this afterwards.  Not while a transcription runs on another thread. */
WHISPER_API void wmi_reload_knobs(void);

/* Status of the one-launch forms of the greedy step (k_mlp_pair, k_front, k_xback: their workgroups hand rows to each other INSIDE the launch; one status word).  A
 * hand-off that does not complete is reported by the kernel, the step is run again in the two-launch form and the state keeps that form;
 * a slow hand-off (the device is shared with work this process does not count) switches to two launches for the next 512 steps.
 * out3 = { steps re-run, slow hand-offs seen, bit 0: the one-launch form is off for good, bit 1: off for now, bit 2: the lock-step rows'
 * one-launch front (k_front with the row on grid.y, wmi_full_batch) is off; its re-run steps are counted in out3[0] }.  rearm != 0 allows the
 * one-launch forms again (tests).  Returns 0, -1 without a context / state.  Reference behaviour matched: a decode either succeeds or
 * reports, W/whisper.cpp:2517-2595. */
WHISPER_API int wmi_pair_status(struct whisper_context * ctx, int32_t * out3, int rearm);

/* Probe: body / boundary split of the last greedy decode step's dependent launches, from time stamps taken INSIDE the kernels
 * (s_memrealtime at a wavefront's first instruction and behind its last store).  The step is captured as a graph with stamping on
 * and replayed; per launch i, out[6 i + 0..5] = first wavefront start, last wavefront start, last wavefront end (microseconds
 * from the step's first start), the number of wavefront records, and two optional mid points (one-row projections: activation
 * row ready, first row tile reduced; -1 where a kernel has none).  `out` holds 6 * cap doubles.  chained = 1: the form whose first kernel is the q|k|v
 * projection (the pick kernel of the previous step prepared token, position and activation row on the device).
 * Returns the number of launches written (<= cap), -1 when no greedy step has run on this context (or the model is quantised). */
WHISPER_API int wmi_step_stamps(struct whisper_context * ctx, double * out, int cap, int chained);

/* Probe: in-situ duration of every f16 encoder GEMM (conv front-end as implicit GEMMs, q|k|v, out, mlp.0, mlp.2, cross K/V) of ONE encoder
 * pass, from wall-clock stamps the kernels' workgroups take themselves (first workgroup entered -> last workgroup done, stores drained):
 * the cache state is the pass's own, not a back-to-back loop's.  chunks = 1: the context's last mel spectrogram (after whisper_full /
 * whisper_pcm_to_mel); chunks > 1: the rows of the last wmi_full_batch call.  out[6 i + 0..5] = {epilogue id, M, N, K, microseconds,
 * workgroups}; returns the number of launches written (<= cap), -1 when there is nothing to replay or the model is block-quantised.
 * bench.py builds SURVEY section 8(d)'s "MFMA utilisation on encoder GEMMs" from it (sum of 2 M N K / sum of microseconds). */
WHISPER_API int wmi_encoder_gemm_stamps(struct whisper_context * ctx, int chunks, double * out, int cap);

/* Host arithmetic self-test (no device needed): the window sums of the token timestamps are the reference's left-to-right f32 sums
 * (W/whisper.cpp:6506-6515), evaluated in blocks as integer additions wherever that is exact (csrc/full.cpp: seq_sum_f32).
 * out_blocked = that routine's result for x[0..n), out_plain = the plain loop's; they must have the same bits.  Returns 0. */
WHISPER_API int wmi_selftest_seqsum(const float * x, int n, float * out_blocked, float * out_plain);
/* Test hook, host only: the soft-max and tie order every language detection route ends in (100 f32 logits -> probs100, optional;
 * returns the language id: sorted by language code, stable-sorted by logit, exp in double relative to the maximum, summed in that order
 * — W/whisper.cpp:3600-3641).  -1: logits100 is NULL. */
WHISPER_API int wmi_selftest_lang_probs(const float * logits100, float * probs100);

/* The no-speech probability (OpenAI's no_speech_prob) and params.no_speech_thold.
 * For every 30 s window: the decoder's RAW logits l at the prompt row that carries <sot> — no temperature, no filter, no ban; the row
 * attends to whatever [prev ...] tokens precede it — and p = exp(l[nosp] - m) / sum_i exp(l[i] - m), m = max l, over the whole vocabulary.
 * Computed on the device (csrc/k_nospeech.hip) with a fixed arithmetic: the l are the f32 logits of the vocabulary projection; the
 * vocabulary is cut into blocks of 128 entries; a block keeps m_b = max l and s_b = sum exp(l - m_b), the difference in f32, exp and sums
 * in double; the blocks are combined in ascending order, S = sum_b s_b exp(m_b - M) with M = max m_b (difference in f32 again),
 * p = exp(l[nosp] - M) / S rounded to f32 once; an entry of -inf adds 0.  The same call twice gives the same bits.
 *   wmi_set_no_speech   the context's mode, read at the START of every whisper_full* / wmi_full_* / wmi_capture_full* / wmi_pool_full call
 *                       on it (wmi_pool_full: each pool context's own mode).  Returns the previous mode, -2 for a NULL context.
 *     0  off (the default): nothing is launched, nothing is stored, every result is what it was without this interface
 *     1  report: p is computed and stored; results otherwise as mode 0
 *     2  drop (OpenAI's rule): at a window with p > params.no_speech_thold the temperature fallback is not taken, and the window is
 *        dropped when its decoder failed or avg_logprobs < params.logprob_thold — no segments, seek += 3000, prompt_past untouched;
 *        otherwise it is emitted as decoded
 *     3  gate: a window with p > params.no_speech_thold ends right behind its <sot> step, with no sampling step — no segments, the same
 *        seek advance, prompt_past untouched
 *   wmi_full_n_windows / wmi_full_get_window   the windows of the last call (none in mode 0), in order; after wmi_batch_select /
 *        wmi_pool_select those of that chunk.  wmi_full_get_window returns 0, -1 for a bad index.
 *   wmi_full_get_segment_no_speech_prob        p of the window that emitted segment i_segment; -1.0f in mode 0 or for a bad index
 * p is taken once per window (at the first temperature), also where the window falls back to higher temperatures. */
struct wmi_window {
    int32_t seek;            /* start of the window, 10 ms frames */
    float   no_speech_prob;
    int32_t outcome;         /* 0 emitted, 1 dropped, 2 gated */
    int32_t i_segment;       /* its first segment (the segment count so far for a window without segments) */
    int32_t n_segments;
};
WHISPER_API int   wmi_set_no_speech(struct whisper_context * ctx, int mode);
WHISPER_API int   wmi_full_n_windows(struct whisper_context * ctx);
WHISPER_API int   wmi_full_get_window(struct whisper_context * ctx, int i, struct wmi_window * out);
WHISPER_API float wmi_full_get_segment_no_speech_prob(struct whisper_context * ctx, int i_segment);
WHISPER_API int   wmi_full_n_windows_from_state(struct whisper_state * state);
WHISPER_API int   wmi_full_get_window_from_state(struct whisper_state * state, int i, struct wmi_window * out);
WHISPER_API float wmi_full_get_segment_no_speech_prob_from_state(struct whisper_state * state, int i_segment);
/* The driver's rule on its own (host only, no device): what becomes of a window in `mode` whose <sot> row said p, given the best
 * decoder's failed flag and avg_logprob.  0 emit, 1 fall back to the next temperature (where one is left), 2 drop, 3 gate. */
WHISPER_API int   wmi_selftest_no_speech_rule(int mode, float p, float thold, int failed, double avg_logprob, float logprob_thold);
/* The no-speech kernels on caller data (no context; all host pointers).  rows in 1 .. 16 share one launch (the row on grid.y).
 *   form 1  logits [rows][n_vocab] f32
 *   form 0  the fused head: W f16 bit patterns [n_vocab][K], x f32 [rows][K]; logits = W . LayerNorm(x) with gain 1, bias 0, eps 1e-5,
 *           made and reduced inside the launch, never written.  K % 8 == 0, 8 <= K <= 1536.  logits_out (optional, [rows][n_vocab])
 *           receives the product's own one-row vocabulary projection (EPI_LOGITS) of the same rows — the same bits.
 * p_out [rows].  Returns 0; -1 bad argument, before the device is touched; -2 / -3 device errors. */
WHISPER_API int   wmi_selftest_no_speech(int device, int form, int rows, int n_vocab, int nosp, const float * logits, const uint16_t * W,
                                         const float * x, int K, float * logits_out, float * p_out);

/* Token times by dynamic time warping over the cross-attention of alignment heads (OpenAI's word_timestamps, whisper.cpp's t_dtw).
 * For every window that emitted segments and has a text token: x = [sot, (language, task), notimestamps, text tokens .., eot] — the best
 * decoder's result tokens with id < eot, no timestamp tokens, no [prev ..] context — is decoded once more, teacher-forced, as one batch on a
 * cleared self cache.  n = len(x), n_sot = 1 or 3, R = n - n_sot - 1 rows enter the path (the rows that PREDICT text_0 .. text_{N-1}, eot),
 * M = clamp(min(3000, seek_end - seek, seek_delta) / 2, 1, audio_ctx in effect) key frames.  Per (layer, head) pair the cross-attention
 * weights w = soft-max over exactly the first M keys of q . k (f16 operands as stored, f32 sums) are normalised per key frame over all n
 * rows (population sigma; sigma == 0 gives 0), median-filtered along time (width 7, reflect padding; none for M <= 3) and averaged over
 * the pairs in ascending (layer, head) order: A [R][M].  The path is the DTW of -A in f32 with OpenAI's tie rule (csrc/k_align.hip,
 * DESIGN.md section 5); text token r gets t_dtw = seek + 2 * (first frame of row r), in 10 ms units.
 *   wmi_set_token_dtw   mode 0 off (default: every result, counter and launch as without this interface), 1 on; layer_head = n_pairs
 *                       {layer, head} pairs, n_pairs = 0: every head of the upper half of the text layers (OpenAI's default mask).  Per-model
 *                       presets are not shipped.  Read at the START of every transcription call.  Returns the previous mode; -2 NULL context;
 *                       -1, nothing changed: a layer or head out of range, a duplicate pair, a NULL list with n_pairs > 0.  Needs the
 *                       hyper-parameters only: works on a host-only context.
 *   wmi_token_dtw_heads the pairs in effect (the default resolved), ascending, up to cap pairs into layer_head; returns their count
 *   wmi_full_get_token_dtw   t_dtw of token i_token of segment i_segment; -1 in mode 0, for a token that is no text, a bad index, or a
 *                       window that was not aligned.  Follows wmi_batch_select / wmi_pool_select like the other accessors.  t0 / t1 of
 *                       whisper_token_data stay the reference's.
 *   wmi_token_dtw_dims  the last window aligned on the context's state; returns 0, -1 when there is none
 *   wmi_get_tensor      "dtw_matrix" A [R][M], "dtw_q" [n_pairs][n][64] the query rows the pass used, "dtw_jumps" [R], of that window
 *   wmi_get_token_dtw_timings   the alignment's own timer (pass + matrix + path + the window's one wait; not part of wmi_get_timings)
 * While the mode is on, the chunks of wmi_full_batch* / wmi_capture_full_batch / wmi_pool_full take the general driver (chunk mode 1), and
 * the self cache after a call holds the alignment pass's rows, not the last decoding step's. */
WHISPER_API int     wmi_set_token_dtw(struct whisper_context * ctx, int mode, const int32_t * layer_head, int n_pairs);
WHISPER_API int     wmi_token_dtw_heads(struct whisper_context * ctx, int32_t * layer_head, int cap);
WHISPER_API int64_t wmi_full_get_token_dtw(struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API int64_t wmi_full_get_token_dtw_from_state(struct whisper_state * state, int i_segment, int i_token);
WHISPER_API int     wmi_token_dtw_dims(struct whisper_context * ctx, int * n, int * n_sot, int * R, int * M, int * n_pairs);
WHISPER_API void    wmi_get_token_dtw_timings(struct whisper_context * ctx, int64_t * us, int32_t * n_windows);
/* The alignment kernels on caller data (no context; all host pointers; f16 as bit patterns), in the product's layouts.
 *   wmi_selftest_dtw_matrix  q [L][n][S], k [L][T][S] (only the first M keys of a layer may be read), layer_head n_pairs pairs in ascending
 *                       order without duplicates, layers < L, heads < H; S = 64 H, H <= 32, 1 <= M <= T <= 1500, R = n - n_sot - 1 in
 *                       1 .. 511.  A_out [R][M].
 *   wmi_selftest_dtw_path    A [R][M] -> jumps [R], path [(R + M)][2] {row, frame} from the first point on, *n_path points.  device = -1: the
 *                       sequential host restatement (the definition; no GPU needed, any R >= 1); device >= 0: the kernel (R <= 511).
 * Return 0; -1 bad argument, before the device is touched; -2 / -3 device errors. */
WHISPER_API int     wmi_selftest_dtw_matrix(int device, int L, int S, int H, int n, int n_sot, int M, int T, const uint16_t * q, const uint16_t * k,
                                            const int32_t * layer_head, int n_pairs, float * A_out);
WHISPER_API int     wmi_selftest_dtw_path(int device, int R, int M, const float * A, int32_t * jumps, int32_t * path, int * n_path);

/* Grammar-constrained decoding on the device (whisper_full_params.grammar_rules; csrc/grammar_eval.h, csrc/k_grammar.hip).
 * By default a call with a grammar copies every step's logits to the host, filters them there and walks the grammar's pushdown stacks over
 * the whole vocabulary (csrc/grammar.cpp).  In mode 1 the general driver keeps the logits in HBM: after the host has advanced a decoder's
 * grammar by the one sampled token, its stacks and partial UTF-8 state go up (2 KB per decoder), k_grammar_reject evaluates every token id
 * below <eot> against them — one thread per id, the same text the host library compiles — into a reject byte mask beside the static ban,
 * and the penalised second pass of W/whisper.cpp:4657-4709 (unless the timestamp mass beats every text token: every rejected, allowed,
 * finite text logit loses grammar_penalty behind the temperature division, the log-soft-max is taken again) feeds the greedy pick, the
 * t > 0 draws and the beam draws there; 32 bytes per pick come back.
 * CONTRACT: the reject set is EXACT — the set grammar_penalise computes.  A decoder state above the compiled capacities (cap_stacks stacks
 * of cap_depth positions, 65535 grammar elements, a malformed grammar) or a token whose working set outgrows cap_words 16-bit words is never
 * guessed: that row's set is computed by the host's own logic for that step and uploaded, and the event is counted (rows_host).
 * Probabilities carry the device sums' ~1e-6 relative, as on every device sampling path (see above); a pick at a near-tie may differ.
 * whisper_get_logits() is undefined in the mode, as for device draws.  WMI_HOST_DRAWS=1 and a logits_filter_callback keep the whole host
 * path.  Lock-step calls send grammar chunks to the general driver as before; that driver takes this route.  The one-row greedy step of
 * grammar-free calls is not involved.
 *   wmi_set_grammar_device   mode 0 off (default: nothing is allocated or launched, every result is byte for byte what it was without this
 *                            interface), 1 on; read per window.  Returns the previous mode, -2 for a NULL context.
 *   wmi_grammar_status       counters since the start of the last whisper_full* call on the context's state, and the compiled capacities.
 *                            Returns 0, -2 for a NULL argument.
 * Not measured here: transcription quality under a grammar on real models — only synthetic weights exist in this repository. */
struct wmi_grammar_status {
    int32_t steps_device;    /* sampling steps whose reject masks the kernel wrote */
    int32_t rows_host;       /* decoder rows whose reject set the host computed instead (capacity fallback) */
    int32_t cap_stacks;      /* stacks of a decoder's uploaded state */
    int32_t cap_depth;       /* positions of one stack */
    int32_t cap_words;       /* 16-bit words of one of the two runs of a token's working set (a stack takes 1 + its depth) */
    float   reject_us;       /* GPU time of the last wmi_selftest_grammar(where = 1) launch of k_grammar_reject, by events (0: none yet) */
};
WHISPER_API int wmi_set_grammar_device(struct whisper_context * ctx, int mode);
WHISPER_API int wmi_grammar_status(struct whisper_context * ctx, struct wmi_grammar_status * out);
/* Test hooks.  Row r's grammar state is built from `params` (grammar_rules, n_grammar_rules, i_start_rule) and its token history exactly
 * as wmi_process_logits builds it (hist: the histories one after the other, n_hist[r] tokens each); 1 <= n_rows <= 8.
 *   wmi_selftest_grammar          reject_out [n_rows][n_vocab]: 1 rejected, 0 not; overflow_out [n_rows]: 1 where the row's state or a token's
 *                                 working set exceeded a capacity (the row's bytes are then 0).  where = 0: csrc/grammar_eval.h on the host —
 *                                 needs no device and touches none (works on a host-only context); where = 1: k_grammar_reject, the rows
 *                                 on grid.y of one launch.
 *   wmi_selftest_grammar_sample   modelled on wmi_selftest_filters (the same step records): caller logits [n_rows][n_vocab] go where the
 *                                 decoder leaves them, then the driver's own route runs — reject masks, penalised second pass, and
 *                                 mode 0 the pick (out [n_rows]) / mode 2 k draws per row with the uniform numbers u [n_rows][k]
 *                                 (out [n_rows][k]).  The counters of wmi_grammar_status advance as in a transcription call.
 * Return 0; -1 bad arguments (before the device is touched), -2 the context cannot compute, -3 device error. */
WHISPER_API int wmi_selftest_grammar(struct whisper_context * ctx, struct whisper_full_params params, int where, int n_rows,
                                     const whisper_token * hist, const int * n_hist, uint8_t * reject_out, uint32_t * overflow_out);
WHISPER_API int wmi_selftest_grammar_sample(struct whisper_context * ctx, struct whisper_full_params params, int mode, int n_rows,
                                            const float * logits, const whisper_token * hist, const int * n_hist, const int * has_ts,
                                            const int * seek_delta, float temperature, const double * u, int k, int tid_default,
                                            whisper_token_data * out);

/* Long recordings: cut at silences on the device, decode the pieces in lock-step.
 * whisper_full walks a long signal window by window (each seek comes from the previous window's timestamps); whisper_full_parallel cuts it
 * into equal pieces wherever the arithmetic lands.  wmi_full_long looks at the signal first:
 *   energies  e[f] = sum over i in [160 f, min(160 f + 160, n)) of | x[i] - x[i-1] |, x[-1] := 0, for every 10 ms frame f < F = ceil(n / 160):
 *             f32 throughout, the sum left to right from 0.0f (csrc/k_segment.hip; the first difference stands in for the node's freq_thold
 *             high-pass without its serial chain).  They come back in one copy behind one wait.
 *   plan      host only, deterministic, all in frames (csrc/segment.cpp; DESIGN.md section 5 has the rules in full): frames below
 *             thold x the mean level or below floor per sample are quiet; quiet runs of >= min_silence_ms are gaps, the runs between
 *             them islands; islands are widened by pad_ms, never past the midpoint of the gap to the neighbouring island; pieces absorb
 *             islands left to right while the gap in front is shorter than max_gap_ms and the piece stays within max_piece_ms; an island
 *             longer than max_piece_ms is cut at the frame of least energy in the last third of that length; pieces below 1 s are
 *             extended to 1 s where the neighbours leave room.  Gaps of max_gap_ms and more are decoded by no piece.
 *   decoding  the pieces go to wmi_full_batch (fit_audio_ctx: wmi_full_batch_ctx with min(n_audio_ctx, (frames + 1) / 2 + 128) per piece, the
 *             node's total_time * 50 + 128) as device pointers into the ONE PCM buffer: host PCM is uploaded once, device PCM not copied.
 *             Every piece is whisper_full on a fresh context with offset_ms = duration_ms = 0 and no_context, as every lock-step chunk;
 *             params.offset_ms / duration_ms restrict the frames the plan sees ([offset_ms / 10, + duration_ms / 10) clipped to F).
 *   result    the pieces' segments in order with t0 / t1, the tokens' t0 / t1 (where set: >= 0), every t_dtw >= 0 and every wmi_window.seek
 *             shifted by the piece's frame0, every window's i_segment rebased.  Pieces are disjoint: nothing is clamped.  The call leaves the
 *             merged result selected; wmi_long_select(piece) shows one piece with piece-relative times as wmi_batch_select does,
 *             wmi_long_select(-1) the merged result again.  whisper_full_lang_id of the merged view is the FIRST piece's; with "auto" every
 *             piece is detected on its own, as wmi_full_batch does (wmi_batch_lang_id(piece) has each).  The no-speech and token-DTW modes
 *             pass through untouched.  The piece views stay valid until the next transcription call on the context.
 * The defaults below are starting values: they have been tried on synthetic signals only.  Embedders tune them.
 * Returns wmi_full_batch's codes; 0 with no piece and no segment for a signal without an island (nothing is decoded).  -1 before any device
 * work: a NULL context / pcm, n_samples < 0, a field of wmi_long_params out of range (thold or floor negative or not finite,
 * min_silence_ms < 10, pad_ms < 0, max_gap_ms < 0, max_piece_ms outside 1000 .. 30000), or new_segment_callback, progress_callback,
 * encoder_begin_callback or logits_filter_callback set (their times and indices would be piece-relative: out of scope).  n_samples == 0: -3, as
 * whisper_full.  Host-only and weights-pending contexts: -2, as wmi_full_batch.
 * wmi_get_batch_timings keeps its meaning (the decoding of the pieces); wmi_get_long_timings has the front's own times, microseconds:
 * us3 = { upload of host PCM, energies (kernel + copy + the wait), plan }, n2 = { frames, pieces }. */
struct wmi_long_params {
    float   thold;            /* 0.25   a frame is quiet below this multiple of the mean level */
    float   floor;            /* 1e-4   or below this absolute level per sample (the node's 0.0001) */
    int32_t min_silence_ms;   /* 300    a quiet run this long is a gap */
    int32_t pad_ms;           /* 100    speech is widened by this much into the gaps */
    int32_t max_gap_ms;       /* 2000   gaps at least this long are left out of the pieces */
    int32_t max_piece_ms;     /* 30000  in 1000 .. 30000 */
    int32_t fit_audio_ctx;    /* 0      1: an encoder length per piece */
};
struct wmi_long_piece {
    int32_t frame0, frame1;   /* the piece is the samples [160 frame0, min(160 frame1, n_samples)) */
    int32_t audio_ctx;        /* its encoder length (0 = the model's n_audio_ctx); without fit_audio_ctx: params.audio_ctx (the plan hook: 0) */
    int32_t mode;             /* wmi_batch_chunk_mode of the piece */
    int32_t i_segment;        /* its first segment in the merged result */
    int32_t n_segments;
};
WHISPER_API struct wmi_long_params wmi_long_default_params(void);
WHISPER_API int  wmi_full_long(struct whisper_context * ctx, struct whisper_full_params params, const float * pcm, int n_samples,
                               int pcm_on_device, const struct wmi_long_params * long_params);      /* NULL: the defaults */
WHISPER_API int  wmi_long_n_pieces(struct whisper_context * ctx);                                   /* of the last wmi_full_long; -1 without a context */
WHISPER_API int  wmi_long_get_piece(struct whisper_context * ctx, int i, struct wmi_long_piece * out);   /* 0, -1 for a bad index */
WHISPER_API int  wmi_long_select(struct whisper_context * ctx, int piece);     /* -1: the merged result; returns the segment count, -1 for a bad index / no result */
WHISPER_API void wmi_get_long_timings(struct whisper_context * ctx, int64_t * us3, int32_t * n2);
/* Test hooks (no context; host pointers; argument errors are decided before the device is touched).
 *   wmi_selftest_frame_energy  the energies of x [n] into e_out [F = ceil(n / 160)]; device = -1: the sequential host restatement (the definition).
 *                              device >= 0: e_out holds F + 64 floats; all of them go to the device as the caller filled them (a sentinel), the
 *                              kernel runs once, all of them come back — the 64 behind F as they were unless the kernel wrote there.
 *                              Returns 0; -1 bad argument (NULL, n < 1, device < -1); -2 / -3 device errors.
 *   wmi_long_stage_samples     the kernel's staging extent in samples (a workgroup's run of frames): where its hand-over between workgroups lies
 *   wmi_selftest_long_window   the frames [*f0, *f1) of an n_samples signal that offset_ms / duration_ms leave to the plan, and in *n_sub the
 *                              samples they hold.  Returns 0; -1 bad argument (n_samples < 1, negative times, NULL).
 *   wmi_selftest_long_plan     the plan for the energies e [F] of an n_samples signal (F = ceil(n_samples / 160)) on a model with that
 *                              n_audio_ctx: up to cap pieces into out (frame0, frame1, audio_ctx; the other fields 0); returns the piece count
 *                              (which may exceed cap), -1 on a bad argument.  wmi_full_long plans with the same function, on the frames the
 *                              window leaves: e + f0, f1 - f0 frames, n_sub samples, frame numbers shifted back by f0. */
WHISPER_API int  wmi_selftest_frame_energy(int device, const float * x, int n, float * e_out);
WHISPER_API int  wmi_long_stage_samples(void);
WHISPER_API int  wmi_selftest_long_window(int n_samples, int offset_ms, int duration_ms, int * f0, int * f1, int * n_sub);
WHISPER_API int  wmi_selftest_long_plan(const float * e, int F, int n_samples, const struct wmi_long_params * long_params, int n_audio_ctx,
                                        struct wmi_long_piece * out, int cap);

/* Score candidate texts against the audio in one teacher-forced pass: "which of my N commands was said?", N-best rescoring, or a
 * confidence for a transcript the caller already has.  Given the encoder result in the state and n_texts token sequences, per text the
 * log-probability of every token and of the whole text, and the posterior over the call's texts — two decoder batches (the prefix, then all
 * texts side by side as sequences of the unified self cache) and ONE host wait, whatever the texts' lengths.
 * Prefix, as whisper_full builds a window's prompt: [<|startofprev|>, the last n_text_ctx / 2 - 1 prompt tokens] only when prompt tokens are
 * passed, <sot>, on multilingual models the language and the task token, <|notimestamps|>: P rows at positions 0 .. P - 1.
 * A text y_0 .. y_{n-1} (every id < eot, n >= 0) has n + 1 scored rows with with_eot (the default), n without: the prefix's last row predicts
 * y_0, input y_i at position P + i predicts y_{i+1}, input y_{n-1} predicts <eot>; n = 0 is legal only with with_eot and scores <eot> at the
 * prefix row.  Per scored row, on the RAW f32 logits l of the vocabulary projection (no temperature, no filter, no ban) with target t: the
 * no-speech head's block pass (blocks of 128 entries: m_b = max l, s_b = sum exp(l - m_b), the difference in f32, exp and sums in double,
 * an entry of -inf adds 0), the blocks combined in ascending order, M = max m_b, S = sum_b s_b exp(m_b - M), and
 * lp = f32(double(f32(l[t] - M)) - log(S)), rounded to f32 once; l[t] = -inf gives -inf.  Per text: sum_logprob = the sum of its lp in double
 * in ascending row order, avg_logprob = sum / count, posterior = exp(v_c - max v) / sum_c exp(v_c - max v) in double, the texts in ascending
 * order, rounded to f32, v = sum_logprob or (length_norm) sum / count; a text with v = -inf has posterior 0, and so has every text when all are -inf.
 * The same call twice gives the same bits (csrc/k_score.hip).
 *   wmi_score_texts    tokens: the texts' ids one text after the other, n_tokens [n_texts].  out [n_texts]; token_logprobs (may be NULL) holds
 *                      the sum of the texts' n_scored values, text c's from out[c].first on.  Needs an encoder result in the state: from
 *                      whisper_encode, any whisper_full*, or wmi_score_pcm.  Texts are split over several candidate passes, each text whole,
 *                      when their rows exceed n_text_ctx.  Afterwards the self cache holds the scoring rows, not a decoding step's (as after an
 *                      alignment pass), and whisper_get_logits() is what it was.
 *   wmi_score_pcm      log-mel and encoder of the window at seek 0 of pcm (audio_ctx = 0: the model's), then wmi_score_texts.
 *   wmi_get_score_timings   the scorer's own timer: us (plan, batches, kernels and the one wait), calls, launches of its kernels — not part
 *                      of wmi_get_timings, to which a scoring call adds nothing beyond wmi_score_pcm's log-mel and encoder pass.
 * Off unless called: a context that never scores allocates and launches nothing for it.
 * Returns 0; -1 no context / state, or a bad argument, nothing launched: NULL lists, n_texts < 1 or > 4096, an id < 0 or >= eot, a negative
 * length, an empty text without with_eot, a text longer than n_text_ctx - P, a language id out of range, a prompt id outside the vocabulary;
 * -2 no compute path (host-only context) or no encoder result in the state; -3 device error.
 * Not measured here: ranking quality on real models — only synthetic weights exist in this repository. */
struct wmi_score_params {
    int32_t lang_id;                       /* multilingual models: the language token's index (whisper_lang_id) */
    int32_t translate;                     /* multilingual models: the task token */
    const whisper_token * prompt_tokens;   /* NULL: no [<|startofprev|> ...] context */
    int32_t prompt_n_tokens;
    int32_t with_eot;                      /* score <eot> behind the last token (default 1) */
    int32_t length_norm;                   /* the posterior over avg_logprob instead of sum_logprob (default 0) */
};
struct wmi_text_score {
    double  sum_logprob;
    float   avg_logprob;
    float   posterior;
    int32_t n_scored;                      /* entries of token_logprobs that belong to the text */
    int32_t first;                         /* index of the first of them */
};
WHISPER_API struct wmi_score_params wmi_score_default_params(void);
WHISPER_API int  wmi_score_texts(struct whisper_context * ctx, struct wmi_score_params params, const whisper_token * tokens, const int32_t * n_tokens,
                                 int n_texts, struct wmi_text_score * out, float * token_logprobs);
/* the same on a caller-owned state (NULL: the context's own), under that state's lock; logits_out (tests, may be NULL): [sum of n_scored][n_vocab], the logits row
 * every entry of token_logprobs was taken from */
WHISPER_API int  wmi_score_texts_with_state(struct whisper_context * ctx, struct whisper_state * state, struct wmi_score_params params,
                                            const whisper_token * tokens, const int32_t * n_tokens, int n_texts, struct wmi_text_score * out,
                                            float * token_logprobs, float * logits_out);
WHISPER_API int  wmi_score_pcm(struct whisper_context * ctx, struct wmi_score_params params, const float * pcm, int n_samples, int pcm_on_device,
                               int audio_ctx, const whisper_token * tokens, const int32_t * n_tokens, int n_texts, struct wmi_text_score * out,
                               float * token_logprobs);
WHISPER_API void wmi_get_score_timings(struct whisper_context * ctx, int64_t * us, int32_t * n_calls, int32_t * n_launches);
/* Test hooks.
 *   wmi_selftest_score_rows   the scoring kernels on caller data (no context; host pointers): logits [rows][n_vocab] f32, targets [rows] in
 *                             [0, n_vocab), lp_out [rows]; rows >= 1 in groups of 8 as decode() groups its flagged rows, 1 <= n_vocab <= 65536.
 *                             Returns 0; -1 bad argument, before the device is touched; -2 / -3 device errors.
 *   wmi_selftest_score_plan   the plan of a call (host only: works on a wmi_init_host_only context).  prefix: up to cap_prefix ids, *n_prefix
 *                             their count; first [n_texts + 1]; prefix_target [n_texts]: the targets on the prefix's last row (text c's at
 *                             place first[c]); rows [cap_rows][7]: {pass, token, position, sequence id, flag, target, place} of every batch
 *                             row of every pass in order (target = place = -1 for a row that predicts nothing), *n_rows their count (which
 *                             may exceed cap_rows); pass_text0 [n_passes + 1 <= cap_passes]: the first text of every pass.  Returns the
 *                             number of passes, -1 for a bad argument (wmi_score_texts' list). */
WHISPER_API int  wmi_selftest_score_rows(int device, int rows, int n_vocab, const float * logits, const int32_t * targets, float * lp_out);
WHISPER_API int  wmi_selftest_score_plan(struct whisper_context * ctx, struct wmi_score_params params, const whisper_token * tokens,
                                         const int32_t * n_tokens, int n_texts, int32_t * prefix, int cap_prefix, int * n_prefix, int32_t * first,
                                         int32_t * prefix_target, int32_t * rows, int cap_rows, int * n_rows, int32_t * pass_text0, int cap_passes);

/* Verify a draft transcript in one decoder pass and decode only what differs.  The caller often has a good guess of a window's tokens — the
 * streaming node's previous result, a smaller model's output, a transcript re-checked after a parameter change.  An armed draft is fed
 * teacher-forced behind the prompt as ONE decoder batch; the filtered greedy pick of every row is taken on the device where its logits lie;
 * the longest prefix of the draft that IS the greedy decode is accepted together with the one token the pass gives for free behind it, and
 * the ordinary one-row step goes on from there.  The result is a greedy decode, never an approximation of one: a wrong draft costs one
 * batch.  DESIGN.md section 5 has the rule; the short form:
 *   honoured only in the first window of a call, at the first temperature, on whisper_full's device greedy path (greedy, temperature 0,
 *   best_of 1 there, no logits_filter_callback, no grammar, weights loaded); P = the window's prompt length, n_max = n_text_ctx / 2 - 4,
 *   n = min(n_offered, n_max - 1, max_tokens > 0 ? max_tokens + 1 : inf, n_text_ctx - P - 1); n <= 0: clipped to nothing.
 *   wmi_set_draft         arms the state's NEXT transcription call (whisper_full*, wmi_full_device_pcm, wmi_capture_full, wmi_full_wav); the
 *                         tokens are copied; the call consumes the draft whether it could use it or not; n = 0 clears it.  Returns 0; -1 for
 *                         n < 0, a NULL list with n > 0, or an id < 0 or >= n_vocab — nothing is armed (an earlier draft stays), no device
 *                         is touched.  Calls that cannot carry a draft (wmi_full_batch*, wmi_full_long*, wmi_pool_full,
 *                         whisper_full_parallel, wmi_capture_full_batch) clear it and report reason 2, whatever they return (an
 *                         argument error included; only a NULL context or a context without a state touches nothing).  A call that
 *                         can carry one takes it where its transcription starts: one that returns before that (wmi_full_wav on a
 *                         clip it cannot plan, wmi_capture_full on a failed resample) leaves the draft armed.
 *   wmi_draft_status      what became of the last transcription call's draft: n_offered tokens were armed, n_rows draft tokens were fed
 *                         (n above), n_accepted of them were the greedy decode, n_emitted_from_draft window tokens were taken from the
 *                         pass (at most n_accepted + 1; fewer where one of them completed or failed the decoder); reason 0 used,
 *                         1 nothing armed, 2 call not eligible, 3 clipped to nothing.
 *   wmi_capture_set_draft mode 1: every wmi_capture_full arms the token ids of the session's previous successful result (all tokens of all
 *                         its segments, in order) before it runs; wmi_capture_keep_last and a failed call forget them.  Mode 0 (default):
 *                         off.  Returns the previous mode, -1 for a NULL session.
 * wmi_get_timings of a drafted call shows fewer n_decode steps and more n_prompt (or n_batchd) rows: the draft's rows are batch rows.
 * Off unless armed: a context that never arms a draft allocates and launches nothing for it. */
struct wmi_draft_status { int32_t n_offered, n_rows, n_accepted, n_emitted_from_draft, reason; };
WHISPER_API int wmi_set_draft(struct whisper_context * ctx, const whisper_token * tokens, int n);
WHISPER_API int wmi_set_draft_with_state(struct whisper_context * ctx, struct whisper_state * state, const whisper_token * tokens, int n);
WHISPER_API int wmi_draft_status(struct whisper_context * ctx, struct wmi_draft_status * out);
WHISPER_API int wmi_draft_status_from_state(struct whisper_state * state, struct wmi_draft_status * out);
WHISPER_API int wmi_capture_set_draft(struct wmi_capture * cap, int mode);
/* Test hooks.
 *   wmi_selftest_draft_plan   the plan of the rule with no device (works on a wmi_init_host_only context): the window at
 *                             seek = offset_ms / 10 that ends at seek + (duration_ms > 0 ? duration_ms / 10 : 3000), a prompt of n_prompt
 *                             tokens.  *n_rows = n + 1 logits rows (1: clipped to nothing), logit_rows [n + 1] their batch rows
 *                             (n_prompt - 1 + j), steps [n + 1][16]: the DecStep words of every row (flags, space_id, eot, beg, n_vocab,
 *                             ts_floor_end, ts_initial_start filled; the rest 0).  The arrays hold n_max rows.  Returns 0, -1 bad argument.
 *   wmi_selftest_draft_rows   crafted logits [n_rows][n_vocab] through filter_stats + k_draft_pick per group of 8 + k_draft_finish on
 *                             `device` (no context; host pointers): ban [n_vocab] bytes, steps [n_rows][16] DecStep words, targets
 *                             [n_rows - 1]; out [n_rows][8] the records' words, *accepted.  Returns 0; -1 bad argument before the device
 *                             is touched; -2 / -3 device errors.
 *   wmi_selftest_draft_logits the next drafted call of the context's state also hands back the logits rows the verifier saw:
 *                             buf [cap_rows][n_vocab] (rows beyond cap_rows are not copied); taken with the draft.  NULL: off. */
WHISPER_API int wmi_selftest_draft_plan(struct whisper_context * ctx, struct whisper_full_params params, const whisper_token * prompt, int n_prompt,
                                        const whisper_token * draft, int n_draft, int32_t * n_rows, int32_t * logit_rows, int32_t * steps);
WHISPER_API int wmi_selftest_draft_rows(int device, int n_rows, int n_vocab, const float * logits, const uint8_t * ban, const int32_t * steps,
                                        const int32_t * targets, int32_t * out, int32_t * accepted);
WHISPER_API int wmi_selftest_draft_logits(struct whisper_context * ctx, float * buf, int cap_rows);

/* Transcribe what an AudioStreamWAV holds: its `data` bytes as they are — 8 or 16 bit, mono or stereo, at the asset's own mix rate.
 *   replaces: the per-sample loop of AudioStreamToText.get_text (bin/addons/godot_whisper/audio_stream_to_text.gd:31-48), which turns
 *             the bytes into floats one `append` at a time and transcribes them as 16 kHz mono whatever the asset is (INTEGRATION.md,
 *             host quirks: a stereo asset is read as interleaved mono, another rate at the wrong speed, an 8-bit asset every second byte).
 * The definition, held bit for bit (tests/wav_ref.py):
 *   sample   WMI_WAV_S16: float(v) / 32768, little-endian; WMI_WAV_S8: float(v) / 128, v signed; WMI_WAV_F32: as is — exact in f32
 *   frame    mono: the sample; stereo: (float(l + r) as f32, then / 2 through double), wmi_downmix_stereo's fold
 *   tails    a trailing incomplete sample (an odd byte at 16 bit) or frame (an odd sample in stereo) is ignored
 *   rate     mix_rate == 16000: the frames are the result.  Else wmi_resample(frames, mix_rate -> 16000, converter) on them, bit for bit:
 *            the result count is its plan's, within int(uint32(frames) * 16000.0 / mix_rate).  converter 1 - 4 as there (0: -10); it is
 *            not looked at when mix_rate == 16000
 * On the device this is ONE launch per clip: at 16 kHz k_wav_decode writes the f32 samples where the log-mel reads them; at any other rate
 * the resampler reads the packed frames itself (csrc/k_resample.hip in_frame) — no f32 image of the input is written, no separate decode
 * runs.  Host bytes are uploaded once, as bytes (2 or 1 per sample instead of 4), into a grow-only buffer of the context; upload, conversion
 * and log-mel are queued on one stream without a host wait between them.  `on_device` != 0: data is a device pointer on the context's
 * device, aligned to its sample size (any sample offset into an allocation will do).
 *   wmi_wav_to_pcm      the mono 16 kHz f32 samples into dst (a host pointer, or a device pointer with dst_on_device != 0); returns the
 *                       samples written.  Waits for them.
 *   wmi_full_wav        wmi_full_device_pcm on those samples (token timestamps take their envelope from the staged samples); waits where
 *                       whisper_full waits.  Results through the whisper_full_* accessors.
 *   wmi_full_long_wav   the whole recording into a device buffer of the context, then wmi_full_long on it (pcm_on_device)
 *   wmi_full_batch_wav  n clips, each with a format, channel count and rate of its own: every conversion is queued before the one wait,
 *                       then wmi_full_batch on the device samples.  Results through wmi_batch_select & co.
 *   wmi_selftest_wav_plan   host only, no context: the frame count and the result count of a clip.  Returns 0 or a conversion error.
 *   wmi_wav_stats       of the last of these calls on the context: out5 = { bytes copied host -> device (the clip's bytes, and the position
 *                       table at rates without a closed form, e.g. 22.05 kHz), frames read, samples written, kernel launches of the
 *                       conversion (one per non-empty clip), microseconds on the device from the first upload to the last conversion
 *                       launch (by stream events; this call waits for them) }.  All zero on a context that never made such a call.
 * Conversion errors, every one decided before the device is touched: -1 a NULL pointer, an unknown format, stereo outside 0 / 1, a
 * non-positive rate, negative bytes, more frames than an int holds, a device pointer that is not sample-aligned, a converter outside
 * 0 - 4; -11 formats 2 and 3 (IMA-ADPCM unless wmi_set_wav_adpcm turns it on, QOA: decoded on the host; logged); -10 converter 0; -2 the context cannot
 * compute; -3 a device error; -4 dst_capacity below the result count.  A converter error of the plan (ratio outside [1/256, 256],
 * SRC_LINEAR upsampling one frame) gives 0 samples, as wmi_resample.  The wmi_full_*_wav calls return a conversion error e as -100 + e,
 * and otherwise exactly what whisper_full / wmi_full_long / wmi_full_batch return for the converted samples (an empty clip included).
 * The no-speech, token-DTW and grammar-device modes apply as in those calls; each call takes the locks the call it ends in takes;
 * wmi_get_timings gains nothing (the conversion's time is in wmi_wav_stats, and, being queued in front of the log-mel, inside the wall
 * time of the transcription).  Off unless called: a context that never makes one of these calls allocates and launches nothing for them.
 * Not served: QOA, IMA-ADPCM outside wmi_set_wav_adpcm's mode 1, RIFF headers (Godot hands over the data chunk), more than two channels, SRC_SINC_BEST_QUALITY. */
enum { WMI_WAV_S8 = 0, WMI_WAV_S16 = 1, WMI_WAV_F32 = 32 };   /* 0 / 1 = AudioStreamWAV.FORMAT_8_BITS / FORMAT_16_BITS */
struct wmi_wav {
    const void * data;
    long long    n_bytes;
    int          format;
    int          stereo;
    int          mix_rate;
    int          on_device;
};
WHISPER_API int wmi_wav_to_pcm(struct whisper_context * ctx, const struct wmi_wav * wav, int converter, float * dst, int dst_capacity,
                               int dst_on_device);
WHISPER_API int wmi_full_wav(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wav, int converter);
WHISPER_API int wmi_full_long_wav(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wav, int converter,
                                  const struct wmi_long_params * long_params);
WHISPER_API int wmi_full_batch_wav(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wavs, int n,
                                   int converter);
WHISPER_API int wmi_selftest_wav_plan(const struct wmi_wav * wav, int converter, long long * frames, long long * n_out);
WHISPER_API int wmi_wav_stats(struct whisper_context * ctx, int64_t * out5);

/* Stereo clips: a speaker per segment and token from the channel energies (one voice per channel: two local microphones, a dialogue
 * recorded left and right).
 *   replaces: whisper.cpp's --diarize (examples/main/main.cpp:41-43 timestamp_to_sample, :237-268 estimate_diarization_speaker; the same in
 *             examples/server/server.cpp): per segment a host loop over an f32 copy of both channels — a copy the WAV calls never make.
 * The definition (tests/speaker_ref.py), for a stereo clip of n frames at `rate` Hz (frames as the WAV calls count them) and times in
 * centiseconds:
 *   is(t)    = max(0, min(n - 1, (t * rate) / 100)), 64-bit, truncating: the reference's clamp, at the asset's own rate, on the asset's own
 *              frames (before any fold, before any resampling).  The clamp makes a range that reaches the end exclude the last frame.
 *   e_c      = the sum of |x_c| over frames [is(t0), is(t1)), c = 0 left, 1 right, in double; s16 as v / 32768, s8 as v / 128
 *   speaker  = 0 if e0 > ratio * e1, else 1 if e1 > ratio * e0, else -1 (the reference's "?"); an empty range or clip: -1, energies 0
 * For s16 and s8 clips e0 / e1 equal the reference's sequential double loop bit for bit (ties included); for f32 clips they are within
 * 2 (is1 - is0) 2^-53 of it, relatively, in an order that is the same from run to run.
 * On the device this is ONE launch per stereo clip (csrc/k_speaker.hip): the packed frames are read where they lie (the uploaded bytes, a
 * device-resident clip, a capture session's frames) into a table of channel sums per centisecond, which one copy brings to pinned host
 * memory — queued behind the conversion, complete at a wait the call makes anyway; no wait is added.  Segment and token records are
 * formed from the table when they are asked for; no sample is read on the host.
 *   wmi_set_speaker   the context's mode, read at the START of wmi_full_wav / wmi_full_long_wav / wmi_full_batch_wav / wmi_capture_full:
 *                     0 (default) nothing is allocated, launched or stored and every result is byte for byte what it is without this
 *                     interface; 1 every segment of the result has a record over its [t0, t1); 2 every token too, over its own t0 / t1
 *                     (with params.token_timestamps; without it the token accessor answers -2).  ratio <= 0 (or NaN) selects 1.1.
 *                     Returns the previous mode, -2 for a NULL context, -1 for a mode outside 0 - 2.  Modes 1 and 2 change no token,
 *                     segment, time or counter of a result; the no-speech, token-DTW, grammar and draft modes pass through unchanged.
 *   wmi_full_get_segment_speaker / wmi_full_get_token_speaker   of the selected result: they follow wmi_batch_select (a table per stereo
 *                     clip) and wmi_long_select (the merged view's times are absolute; a selected piece shows the same records for its
 *                     segments, its piece-relative times shifted back).  0 ok; -1 a bad index or NULL; -2 the result carries no table:
 *                     mode 0, a mono clip, token records outside mode 2, or the result of any other call family (whisper_full*,
 *                     wmi_full_device_pcm, wmi_full_batch*, wmi_full_long on caller-made mono, wmi_pool_full, whisper_full_parallel,
 *                     wmi_capture_full_batch: out of scope — there is no stereo source, or no table per lane yet).  Every transcription
 *                     call on the context drops the tables of the one before it.
 *   wmi_wav_speaker   ranges of the caller's own (words built from wmi_full_get_token_dtw, say), no transcription: uploads, launches,
 *                     copies, waits once, and fills out[n].  Its argument errors are the WAV conversion errors, decided before the device
 *                     is touched (-1 also for n < 0 or NULL t0 / t1 / out with n > 0); -12 a mono clip; -2 / -3 as there.  Any positive rate.
 *   wmi_speaker_stats out4 = { tables made by the last call that took a mode, bins, bytes copied device -> host, kernel launches }
 *   wmi_selftest_channel_bins   the kernel alone on `device`: bins [cap_bins][2] and last2 [2] of 8 bytes each (uint64 sums of |v| for the
 *                     integer formats, doubles for WMI_WAV_F32); bin b covers frames [B(b), min(B(b + 1), n - 1)), B(b) = (b * rate) / 100,
 *                     *n_bins = the smallest b with B(b) >= n; last2 = the magnitudes of frame n - 1, which no range counts.  What lies
 *                     behind the n_bins pairs in `bins` is left as it was.  -4: cap_bins below the count (n_bins is still written); -5: the
 *                     launch wrote into the guard the hook keeps behind the device table.
 *   wmi_bench_channel_bins   the launch alone, `iters` times on a stream of its own, each between two device events: ms[iters]
 *   wmi_selftest_speaker_ranges   host only: csrc/speaker_ranges.h on a caller-made table.  kind = the format (WMI_WAV_*).  last2 is
 *                     not read (see above).  Returns 0, -1 for a bad argument. */
struct wmi_speaker { int speaker; int reserved; long long is0, is1; double e0, e1; };   /* speaker: 0, 1, -1 undecided */
WHISPER_API int wmi_set_speaker(struct whisper_context * ctx, int mode, double ratio);
WHISPER_API int wmi_full_get_segment_speaker(struct whisper_context * ctx, int i_segment, struct wmi_speaker * out);
WHISPER_API int wmi_full_get_token_speaker(struct whisper_context * ctx, int i_segment, int i_token, struct wmi_speaker * out);
WHISPER_API int wmi_wav_speaker(struct whisper_context * ctx, const struct wmi_wav * wav, const int64_t * t0, const int64_t * t1, int n,
                                double ratio, struct wmi_speaker * out);
WHISPER_API int wmi_speaker_stats(struct whisper_context * ctx, int64_t * out4);
WHISPER_API int wmi_selftest_channel_bins(int device, const struct wmi_wav * wav, void * bins, long long cap_bins, long long * n_bins,
                                          void * last2);
WHISPER_API int wmi_bench_channel_bins(int device, const struct wmi_wav * wav, int iters, float * ms);
WHISPER_API int wmi_selftest_speaker_ranges(const void * bins, long long n_bins, const void * last2, int kind, long long n_frames, int rate,
                                            double ratio, const int64_t * t0, const int64_t * t1, int n_ranges, struct wmi_speaker * out);

/* Stereo dialogues: the two channels of a stereo clip transcribed apart, in one lock-step call (one voice per channel — where both talk at
 * once the fold of wmi_full_wav hands the decoder a mixture, and the energy rule above can only answer "?").
 *   replaces: de-interleaving the asset on the host (in the node a GDScript loop per sample), two mono clips, wmi_full_batch_wav: two
 *             conversion launches and no joint result.
 * The definition, held bit for bit (tests/channels_ref.py), for a stereo clip of `frames` frames as the WAV calls count them:
 *   ch[c][f]   the sample of channel c (0 left, 1 right) of frame f: s16 v / 32768, s8 signed v / 128, f32 as is — no fold
 *   pcm[c]     mix_rate == 16000: ch[c].  Else wmi_resample(ch[c], mix_rate -> 16000, converter), bit for bit; both channels have the
 *              count of that plan, the count wmi_wav_to_pcm reports for the clip
 *   result     wmi_full_batch(ctx, params, { pcm[0], pcm[1] }, { n, n }, 2, on_device): chunk c is channel c
 * On the device the bytes are uploaded once and ONE launch reads every frame once and writes both channels (csrc/k_wav.hip k_wav_split at
 * 16 kHz; csrc/k_resample.hip k_resample_split otherwise: position, tap walk and interpolated coefficients computed once per output, two
 * accumulator pairs).
 *   wmi_wav_to_pcm_channels   the two channels' mono 16 kHz samples into dst0 / dst1 (host pointers, or device pointers with dst_on_device
 *                       != 0; room for dst_capacity samples EACH); returns the count per channel.  Waits for the samples.  Errors as
 *                       wmi_wav_to_pcm (also -1 for a NULL dst0 / dst1); -12 a mono clip (wmi_wav_speaker's code), decided behind the others.
 *   wmi_full_wav_channels   the one split launch into two slices of a device buffer of the context, one wait, then wmi_full_batch on the
 *                       two device pointers.  A conversion error e is returned as -100 + e (a mono clip: -112), otherwise exactly what
 *                       wmi_full_batch returns for the definition's samples.  It takes the locks of wmi_full_batch_wav and, like it,
 *                       carries no draft (an armed one is dropped).  The no-speech, token-DTW and grammar-device modes pass through as in
 *                       wmi_full_batch.  wmi_set_speaker modes 1 and 2 are NOT served: the result carries no table, the speaker accessors
 *                       answer -2 (each channel IS a speaker).  wmi_wav_stats afterwards: { n_bytes (+ the position table, once),
 *                       frames, 2 n, 1 launch, microseconds }.  When the call returns 0 the dialogue view is selected.
 *   wmi_channels_select   c = 0 / 1: the accessors read that channel, exactly as wmi_batch_select(ctx, c) (wmi_batch_chunk_mode,
 *                       wmi_batch_lang_id and the windows per channel as there); c = -1: the dialogue view — copies of both channels'
 *                       segments (text, tokens, times, DTW times untouched; nothing is shifted) in the order of a stable two-way merge by
 *                       start time: while both channels have segments left, channel 0's next if its t0 <= channel 1's next's t0, else
 *                       channel 1's; then the rest (csrc/channel_merge.h).  Its language id is channel 0's; it carries no window records
 *                       (wmi_full_n_windows 0) and no speaker table.  Returns the segment count; -1 for another index, or when the last
 *                       transcription call on the context was not wmi_full_wav_channels (every transcription call drops the view).
 *   wmi_channels_get_segment   segment i of the dialogue view: { its channel, its index in that channel's result }.  0; -1 for a bad index
 *                       or when the selected result is not the dialogue view.
 *   wmi_selftest_channels_merge   host only, no context: the merge rule on two lists of start times; out_channel / out_index hold
 *                       n_a + n_b entries, which is what it returns (-1: a negative count or a NULL pointer that is needed).
 * Off unless called.  Not served: the capture session's frames, the long and the batch form per channel, more than two channels,
 * suppressing what both microphones heard, energy tables on a channels result, interleaving below segment granularity. */
struct wmi_channel_segment { int channel; int index; };
WHISPER_API int wmi_wav_to_pcm_channels(struct whisper_context * ctx, const struct wmi_wav * wav, int converter, float * dst0, float * dst1,
                                        int dst_capacity, int dst_on_device);
WHISPER_API int wmi_full_wav_channels(struct whisper_context * ctx, struct whisper_full_params params, const struct wmi_wav * wav,
                                      int converter);
WHISPER_API int wmi_channels_select(struct whisper_context * ctx, int channel);
WHISPER_API int wmi_channels_get_segment(struct whisper_context * ctx, int i, struct wmi_channel_segment * out);
WHISPER_API int wmi_selftest_channels_merge(const int64_t * t0_a, int n_a, const int64_t * t0_b, int n_b, int * out_channel, int * out_index);

/* IMA-ADPCM clips (AudioStreamWAV.FORMAT_IMA_ADPCM, format value 2) decoded on the device: the compressed bytes go up as they are, half a
 * byte per sample, and every WAV call above serves them.
 *   replaces: decoding the clip on the host (in the node a GDScript loop per nibble) and handing over two or four bytes per sample.
 * The definition, held bit for bit (tests/adpcm_ref.py; csrc/adpcm_map.h):
 *   tables   the standard IMA ones: STEP[89] = 7, 8, 9, .. 29794, 32767; INDEX[16] = {-1, -1, -1, -1, 2, 4, 6, 8} twice
 *   state    per channel (predictor, step_index), (0, 0) in front of the clip; there are no block headers: a channel is ONE stream
 *   nibble n step = STEP[step_index]; step_index = clamp(step_index + INDEX[n], 0, 88);
 *            diff = step >> 3 (+ step >> 2 if n & 1) (+ step >> 1 if n & 2) (+ step if n & 4), negated if n & 8 — in at least 32 bits;
 *            predictor = clamp(predictor + diff, -32768, 32767); the sample is the predictor
 *   layout   the low nibble of a byte first.  Mono: byte k = frames 2k, 2k + 1; frames = 2 * n_bytes.  Stereo: byte 2k + c = frames 2k,
 *            2k + 1 of channel c; frames = 2 * (n_bytes / 2), a trailing odd byte is ignored
 *   result   the decoded clip is interleaved s16; a format-2 clip gives exactly what the same call gives for WMI_WAV_S16 data equal to
 *            the decoded samples, with the same stereo and mix_rate — nothing new is defined behind the decode
 * NOT verified (Godot's source is not part of this repository): the layout and the initial state are written from knowledge of Godot
 * 4.1's audio_stream_wav.cpp; and Godot may hold `diff` in an int16_t, which wraps where step >= 18500 meets n & 7 == 7 — an encoder
 * corner.  Here diff has 32 bits, as Godot's own encoder assumes; a clip that reaches that corner may decode differently there.
 * On the device (csrc/k_adpcm.hip): both recurrences are chains of clamped additions x -> min(max(x + a, lo), hi), which compose exactly
 * (csrc/adpcm_map.h), so each is a prefix scan over chunks of 32 nibbles: five launches per clip (reduce, walk of the
 * partials, apply — the index's apply is the predictor's reduce), queued on the conversion's stream between the upload and the existing
 * conversion with no host wait; no workgroup waits for another.  The s16 image lands in a grow-only buffer of the context and the call goes
 * on as for a device-resident WMI_WAV_S16 clip: the conversion, the resampler's readers, the channel split and the speaker bins are the
 * existing launches.
 *   wmi_set_wav_adpcm   the context's mode, read where a WAV call plans its clips.  0 (default): format 2 is -11 (-111) everywhere, as
 *                       without this interface, and nothing is allocated or launched for it.  on != 0: format 2 is served by wmi_wav_to_pcm,
 *                       wmi_wav_to_pcm_channels, wmi_full_wav, wmi_full_long_wav, wmi_full_batch_wav (clips of mixed formats in one call),
 *                       wmi_full_wav_channels (a mono clip: -12 as ever), wmi_wav_speaker, with the speaker modes.  Returns the previous
 *                       mode, -2 for a NULL context.  Format 3 (QOA) stays -11 in both modes.  Argument errors are decided on the host
 *                       as before: more frames than an int holds (mono: 2 * n_bytes > INT_MAX) is -1; a device source (on_device) may lie
 *                       at any byte address.  wmi_selftest_wav_plan has no context and keeps answering -11.  wmi_wav_stats: the bytes
 *                       copied count the ADPCM bytes, the launches count the five decode launches too.
 *   wmi_selftest_adpcm_plan    host only: wmi_selftest_wav_plan as mode 1 plans (format 2: the decoded clip's frames and result count)
 *   wmi_selftest_adpcm_shape   out5 = { nibbles per chunk (one chunk per thread and channel), lanes per wavefront, chunks per workgroup,
 *                       partials per tile of the cross-workgroup walk, launches per clip }
 *   wmi_selftest_adpcm_decode  the kernels alone on `device`: the bytes are placed src_byte_offset (0 - 4096) bytes into a device
 *                       allocation; out_s16 gets frames * channels interleaved samples.  *frames is written first; -4: cap_frames below
 *                       it; -5: a byte outside the image (the guard the hook keeps around it) was written; -1 / -2 / -3 as above
 *   wmi_selftest_adpcm_host    host only: the sequential loop in C++ — the definition, and the baseline for timing.  Returns the frames,
 *                       -4: cap_frames below them
 *   wmi_selftest_adpcm_maps    host only: csrc/adpcm_map.h's compose and apply over n caller-made nibbles (one per byte, 0 - 15) of one
 *                       channel cut into chunks of `chunk`: the kernels' plan with sequential scans.  out_predictor / out_index [chunks + 1]:
 *                       every chunk's entry state and, last, the state behind the stream.  Returns the chunk count; -4: cap below chunks + 1
 *   wmi_bench_adpcm_decode     the decode launches alone, `iters` times, each between two device events: ms[iters] */
WHISPER_API int wmi_set_wav_adpcm(struct whisper_context * ctx, int on);
WHISPER_API int wmi_selftest_adpcm_plan(const struct wmi_wav * wav, int converter, long long * frames, long long * n_out);
WHISPER_API int wmi_selftest_adpcm_shape(int * out5);
WHISPER_API int wmi_selftest_adpcm_decode(int device, const unsigned char * bytes, long long n_bytes, int stereo, int src_byte_offset,
                                          int16_t * out_s16, long long cap_frames, long long * frames);
WHISPER_API int wmi_selftest_adpcm_host(const unsigned char * bytes, long long n_bytes, int stereo, int16_t * out_s16, long long cap_frames);
WHISPER_API int wmi_selftest_adpcm_maps(const unsigned char * nibbles, long long n, int chunk, int32_t * out_predictor, int32_t * out_index,
                                        long long cap);
WHISPER_API int wmi_bench_adpcm_decode(int device, const unsigned char * bytes, long long n_bytes, int stereo, int src_byte_offset, int iters,
                                       float * ms);

/* Host worker pool self-test (no device needed): `reps` jobs of `n_tasks` tasks; returns reps * n_tasks * (n_tasks + 1) / 2
 * when every task of every job ran exactly once. */
WHISPER_API int64_t wmi_selftest_pool(int n_tasks, int reps);

#ifdef __cplusplus
}
#endif
#endif /* WMI_DEVICE_H */

// The combine of a row's partial filter statistics (kernels.h: FsPartial) into the filtered greedy pick and its record — the arithmetic of
// k_filter_pick (k_sample.hip), shared with k_draft_pick (k_draft.hip) so that both give the same bits on the same partials: the maxima by
// the 64-lane xor butterfly with first-index tie-break, the local sums rescaled to the global maximum (online soft-max identity) and added
// by the same butterfly, "the timestamp mass beats every text token" (W/whisper.cpp:4659-4683), the record of W/whisper.cpp:4793-4809.
// One wavefront; every lane ends with the same values.
//
// The two halves are statement blocks, not functions: as inlined functions (partials by reference, results in a struct) the same arithmetic
// compiled to other code for k_filter_pick — the partials' loads were split differently and the argument loads scheduled elsewhere — and
// the greedy step's pick kernel is to stay instruction for instruction what it was.  A block is the text both kernels compile.
#pragma once

#include "kernels.h"
#include "wave_ops.h"

namespace wmi { namespace k {

namespace {

using MaxIdx = FsMaxIdx;
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) {      // larger value, then smaller index (first occurrence)
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ MaxIdx wave_max(MaxIdx m) {
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) { MaxIdx t; t.v = WMI_SHX(m.v, o); t.i = WMI_SHX(m.i, o); m = better(m, t); }
    return m;
}
__device__ __forceinline__ float wave_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += WMI_SHX(v, o); return v; }

} // namespace

}} // namespace wmi::k

// In scope: FsPartial pq[PPL] (the partials lane, lane + 64, .. of the row, loaded), int nparts, int lane.  Declares a, t, z (the maxima over
// all / text / timestamp tokens), M, sum, sum_ts, lse, ts_logprob, max_text, force_ts, pick, id.
#define WMI_FS_COMBINE(PPL) \
    MaxIdx la = {-INFINITY, 0x7fffffff}, lt = la, lz = la; \
    _Pragma("unroll") \
    for (int q = 0; q < PPL; ++q) { \
        if (lane + 64 * q >= nparts) { pq[q].all = MaxIdx{-INFINITY, 0x7fffffff}; pq[q].txt = pq[q].all; pq[q].ts = pq[q].all; pq[q].sum = 0.0f; pq[q].sum_ts = 0.0f; } \
        la = better(la, pq[q].all); lt = better(lt, pq[q].txt); lz = better(lz, pq[q].ts); \
    } \
    const MaxIdx a = wave_max(la), t = wave_max(lt), z = wave_max(lz); \
    const float M = a.v; \
    float lsum = 0.0f, lsum_ts = 0.0f; \
    _Pragma("unroll") \
    for (int q = 0; q < PPL; ++q) { \
        const float w = pq[q].all.v > -INFINITY ? expf(pq[q].all.v - M) : 0.0f;      /* rescale the local sums to the global max */ \
        if (q == 0) { lsum = pq[q].sum * w; lsum_ts = pq[q].sum_ts * w; } else { lsum += pq[q].sum * w; lsum_ts += pq[q].sum_ts * w; } \
    } \
    const float sum = wave_sum(lsum), sum_ts = wave_sum(lsum_ts); \
    /* every lane evaluates the pick (uniform values): no broadcast between the decision and what follows it */ \
    const float lse = logf(sum) + M; \
    /* timestamp log-mass vs best text token (W/whisper.cpp:4659-4683) */ \
    const float ts_logprob = sum_ts > 0.0f ? logf(sum_ts) + M - lse : -INFINITY; \
    const float max_text = t.v > -INFINITY ? t.v - lse : -INFINITY; \
    const bool force_ts = ts_logprob > max_text; \
    const MaxIdx pick = force_ts ? z : a; \
    const int id = pick.i;

// Behind WMI_FS_COMBINE, in scope: int beg, int seqv (the tag of both halves).  Declares SampleOut r, the pick's record.
#define WMI_FS_RECORD() \
        SampleOut r; \
        r.id = id; r.plog = pick.v - lse; r.p = expf(r.plog); r.seq0 = seqv; r.seq = seqv; \
        /* timestamp statistics over the post-filter probabilities (W/whisper.cpp:4793-4809) */ \
        const float p_ts_max = z.v > -INFINITY ? expf(z.v - lse) : 0.0f; \
        const double sum_ts_p = (double) sum_ts * (double) expf(M - lse); \
        r.tid = p_ts_max > 0.0f ? z.i : 0; \
        r.pt = (float) ((double) p_ts_max / (sum_ts_p + 1e-10)); \
        r.ptsum = (float) sum_ts_p; \
        if (r.id >= beg) { r.tid = r.id; r.pt = r.p; }

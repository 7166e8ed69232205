// The draft verifier's picks for gfx950 (kernels.h has the contract): behind the vocabulary projection of a group of <= 8
// teacher-forced decoder rows and k_filter_stats on them, k_draft_pick turns every row's 64 partial statistics into the filtered greedy
// pick with k_filter_pick's arithmetic (filter_combine.h: the same statements in the same order, so the same bits), stores the pick's
// record into pinned host memory and one word "the pick is the draft's token" into device memory; k_draft_finish, one launch behind the
// last group, counts the leading matches.  Workgroups are independent inside both launches: plain loads, wave reductions, vector stores —
// no atomics, no spinning, no hand-off inside a launch, no scratch.

#include "kernels.h"
#include "wave_ops.h"
#include "filter_combine.h"

#include <cmath>

namespace wmi { namespace k {

namespace {

// grid = the group's rows, one wavefront each (row = row0 + blockIdx.x of the call; part, stp: the group's).  20 VGPRs, no LDS.
// out_host[row] gets the record as two 16-byte stores, each tagged with the row's DecStep::seq; match[row] = 1 where row < n_targets and
// the pick is targets[row], else 0 (a row without a target: "no match").
__global__ __launch_bounds__(64) void k_draft_pick(const FsPartial * __restrict__ part, const DecStep * __restrict__ stp,
                                                   const int32_t * __restrict__ targets, int row0, int n_targets,
                                                   SampleOut * __restrict__ out_host, int32_t * __restrict__ match) {
    const int lane = threadIdx.x, row = row0 + (int) blockIdx.x;
    constexpr int nparts = 64;
    part += (size_t) blockIdx.x * nparts; stp += blockIdx.x;
    // the record's fields, the target and the partials are requested together
    const int beg = stp->beg;
    const int seqv = stp->seq & SAMPLE_SEQ_MASK;
    const int target = targets[row < n_targets ? row : 0];
    FsPartial pq[1];
    pq[0] = part[lane];
    WMI_FS_COMBINE(1)
    if (lane == 0) {
        WMI_FS_RECORD()
        const int4 * h = (const int4 *) &r;
        ((int4 *) (out_host + row))[0] = h[0];
        ((int4 *) (out_host + row))[1] = h[1];
        match[row] = (row < n_targets && id == target) ? 1 : 0;
    }
}

// one wavefront: lane L looks at rows L, L + 64, ..; per 64 rows one __ballot of "matched", the first clear bit ends the accepted run
// (a row at or behind n_rows counts as a mismatch, so accepted <= n_rows).  {accepted, tag} is ONE 8-byte store.  4 VGPRs, no LDS.
__global__ __launch_bounds__(64) void k_draft_finish(const int32_t * __restrict__ match, int n_rows, int32_t tag, DraftOut * __restrict__ out) {
    const int lane = threadIdx.x;
    int accepted = n_rows;
    for (int base = 0; base < n_rows; base += 64) {
        const int i = base + lane;
        const bool ok = i < n_rows && match[i < n_rows ? i : 0] != 0;
        const unsigned long long miss = ~__ballot(ok);
        if (miss != 0ull) { accepted = base + (int) __ffsll(miss) - 1; break; }
    }
    if (lane == 0) *(int2 *) out = make_int2(accepted, tag);
}

} // namespace

void draft_pick(const FsPartial * part, const DecStep * steps, const int32_t * targets, int row0, int n_group, int n_targets,
                SampleOut * out_host, int32_t * match, hipStream_t st) {
    hipLaunchKernelGGL(k_draft_pick, dim3(n_group), dim3(64), 0, st, part, steps, targets, row0, n_targets, out_host, match);
}

void draft_finish(const int32_t * match, int n_rows, int32_t tag, DraftOut * out, hipStream_t st) {
    hipLaunchKernelGGL(k_draft_finish, dim3(1), dim3(64), 0, st, match, n_rows, tag, out);
}

}} // namespace wmi::k

// The dialogue view of a two-channel transcription (include/wmi_device.h wmi_full_wav_channels, wmi_channels_select): in which order the
// segments of the two channels' results are shown.  Plain C++ without a device: compiled into the library (wav.cpp) and into a stand-alone
// sanitizer program (scratch/lab/channel_merge_asan.cpp).
//
// The rule: a stable two-way merge by the segments' start times.  While both channels have segments left, channel 0's head is taken if
// its t0 <= channel 1's head's t0, else channel 1's head; then the rest of whichever channel has some.  A channel's own order is never
// changed — whether or not its start times ascend —, and equal start times put channel 0 first.
#pragma once
#include <cstdint>

namespace wmi { namespace chm {

// entry i of the merged order: segment out_index[i] of channel out_channel[i]; both arrays hold n_a + n_b entries, which is what is returned
inline int merge(const int64_t * t0_a, int n_a, const int64_t * t0_b, int n_b, int * out_channel, int * out_index) {
    int a = 0, b = 0, n = 0;
    while (a < n_a && b < n_b) {
        if (t0_a[a] <= t0_b[b]) { out_channel[n] = 0; out_index[n] = a++; }
        else                    { out_channel[n] = 1; out_index[n] = b++; }
        ++n;
    }
    for (; a < n_a; ++n) { out_channel[n] = 0; out_index[n] = a++; }
    for (; b < n_b; ++n) { out_channel[n] = 1; out_index[n] = b++; }
    return n;
}

}}  // namespace wmi::chm

// Stand-alone host check of csrc/channel_merge.h under AddressSanitizer / UBSan: the dialogue view's merge rule on exactly sized heap
// blocks (a read or a write one entry too far is a report), against the rule restated below as a sort: the entries of both sides ordered
// by (t0, channel, index) — which is what a stable two-way merge with "channel 0 first on a tie" gives for sides whose start times do not
// fall.  For a side whose times do fall, only the properties are checked: each side keeps its order, n_a + n_b entries, every one once.
// Nothing runs on a GPU.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scratch/lab/channel_merge_asan.cpp \
//       -o /tmp/channel_merge_asan && /tmp/channel_merge_asan
//   (prints the number of merges compared; exit status 0 = every one held and no sanitizer report)
#include "../../godot-whisper_amd/csrc/channel_merge.h"

#include <algorithm>
#include <cstdio>
#include <memory>
#include <tuple>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (rng_state >> 33); }

int main() {
    long compared = 0;
    for (int round = 0; round < 20000; ++round) {
        const int n_a = (int) (rnd() % 13), n_b = (int) (rnd() % 13);
        const bool sorted = round % 5 != 4;
        const int64_t span = round % 3 == 0 ? 4 : 3000;                      // a narrow span: many ties
        // exactly n entries on the heap (n = 0: a block of no entries)
        std::unique_ptr<int64_t[]> a(new int64_t[(size_t) n_a]), b(new int64_t[(size_t) n_b]);
        for (int i = 0; i < n_a; ++i) a[i] = (int64_t) (rnd() % span) - (round % 7 == 0 ? 2 : 0);
        for (int i = 0; i < n_b; ++i) b[i] = (int64_t) (rnd() % span);
        if (round % 11 == 0 && n_a) a[n_a - 1] = INT64_MAX;
        if (round % 13 == 0 && n_b) b[0] = INT64_MIN;
        if (sorted) { std::sort(a.get(), a.get() + n_a); std::sort(b.get(), b.get() + n_b); }
        const int n = n_a + n_b;
        std::unique_ptr<int[]> ch(new int[(size_t) n]), ix(new int[(size_t) n]);
        if (wmi::chm::merge(a.get(), n_a, b.get(), n_b, ch.get(), ix.get()) != n) { std::printf("MISMATCH count, round %d\n", round); return 1; }
        // each side in its own order, every entry once
        int na = 0, nb = 0;
        for (int i = 0; i < n; ++i) {
            const bool ok = ch[i] == 0 ? ix[i] == na++ : ch[i] == 1 ? ix[i] == nb++ : false;
            if (!ok) { std::printf("MISMATCH order, round %d entry %d: channel %d index %d\n", round, i, ch[i], ix[i]); return 1; }
        }
        if (na != n_a || nb != n_b) { std::printf("MISMATCH sides, round %d\n", round); return 1; }
        if (sorted) {
            std::vector<std::tuple<int64_t, int, int>> want;
            for (int i = 0; i < n_a; ++i) want.emplace_back(a[i], 0, i);
            for (int i = 0; i < n_b; ++i) want.emplace_back(b[i], 1, i);
            std::sort(want.begin(), want.end());
            for (int i = 0; i < n; ++i)
                if (std::get<1>(want[i]) != ch[i] || std::get<2>(want[i]) != ix[i]) {
                    std::printf("MISMATCH rule, round %d entry %d: got (%d, %d), want (%d, %d)\n", round, i, ch[i], ix[i], std::get<1>(want[i]), std::get<2>(want[i]));
                    return 1;
                }
        } else {
            // the rule itself, step by step: the head taken is channel 0's unless channel 1's starts strictly earlier
            int pa = 0, pb = 0;
            for (int i = 0; i < n; ++i) {
                const int want = pa < n_a && (pb >= n_b || a[pa] <= b[pb]) ? 0 : 1;
                if (ch[i] != want) { std::printf("MISMATCH step, round %d entry %d\n", round, i); return 1; }
                (want == 0 ? pa : pb)++;
            }
        }
        ++compared;
    }
    std::printf("%ld merges compared\n", compared);
    return 0;
}

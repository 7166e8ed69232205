// Stand-alone host check of csrc/speaker_ranges.h under AddressSanitizer / UBSan: the range arithmetic of the speaker labels on tables
// built here from pseudo-random stereo clips (exactly sized heap blocks, so a read one bin too far is a report), against main.cpp's
// straight loop over the samples restated below.  s16 and s8 must be equal bit for bit; f32 within 2 m 2^-53.  Nothing runs on a GPU.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scratch/lab/speaker_ranges_asan.cpp \
//       -o /tmp/speaker_ranges_asan && /tmp/speaker_ranges_asan
//   (prints the number of ranges compared; exit status 0 = every one held and no sanitizer report)
#include "../../godot-whisper_amd/csrc/speaker_ranges.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace wmi::spk;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (rng_state >> 33); }

// the definition: timestamp_to_sample with the asset's rate, then the sequential double loop
static long long is_of(long long t, long long n, long long rate) {
    if (t < 0) return 0;
    const __int128 s = (__int128) t * rate / 100;
    const long long c = s < (__int128) (n - 1) ? (long long) s : n - 1;
    return c < 0 ? 0 : c;
}

int main() {
    const long long rates[] = { 16000, 44100, 22050, 11025, 150, 63, 4096000, 1, 100, 2147483647 };
    const long long counts[] = { 0, 1, 2, 159, 160, 161, 4097, 48001 };
    const int kinds[] = { KIND_S16, KIND_S8, KIND_F32 };
    long compared = 0;
    for (int kind : kinds) for (long long rate : rates) for (long long n : counts) {
        // the channels as f32 (what the reference holds) and as magnitudes
        std::vector<float> x((size_t) (2 * n));
        std::vector<uint64_t> mag((size_t) (2 * n));
        for (long long i = 0; i < 2 * n; ++i) {
            if (kind == KIND_F32) { x[i] = (float) ((int) (rnd() % 2001) - 1000) * ((i & 1) ? 1e-3f : 7e-3f); if (i == 4) x[i] = 1e30f; if (i == 7) x[i] = -1e-30f; }
            else {
                const int hi = kind == KIND_S16 ? 32768 : 128;
                int v = (int) (rnd() % (2 * hi)) - hi; if (i < 4) v = -hi;
                mag[i] = (uint64_t) (v < 0 ? -v : v); x[i] = (float) v / (float) hi;
            }
        }
        const long long nb = n_bins(n, rate);
        if (nb > 6000000) continue;
        // exactly nb pairs on the heap
        std::unique_ptr<uint64_t[]> ib(new uint64_t[(size_t) (2 * nb) + 1]);
        double * db = (double *) ib.get();
        for (long long b = 0; b < nb; ++b) {
            long long f0 = (long long) ((__int128) b * rate / 100), f1 = (long long) ((__int128) (b + 1) * rate / 100);
            if (f1 > n - 1) f1 = n - 1;
            for (int c = 0; c < 2; ++c) {
                if (kind == KIND_F32) { double e = 0.0; for (long long j = f0; j < f1; ++j) e += std::fabs(x[2 * j + c]); db[2 * b + c] = e; }
                else { uint64_t s = 0; for (long long j = f0; j < f1; ++j) s += mag[2 * j + c]; ib[2 * b + c] = s; }
            }
        }
        const long long big = (long long) 1 << 40;
        const long long ts[][2] = { {0, 0}, {0, 1}, {1, 0}, {0, nb}, {0, nb - 1}, {nb - 1, nb}, {nb, nb + 5}, {0, nb + 100}, {nb / 3, 2 * nb / 3},
                                    {-5, 3}, {3, -5}, {0, big}, {big, 2 * big}, {0, (long long) 1 << 62}, {nb / 2, 9223372036854775807ll} };
        for (const auto & t : ts) {
            const Range r = range_eval(nb ? (const void *) ib.get() : nullptr, nb, kind, n, rate, 1.1, t[0], t[1]);
            const long long is0 = n ? is_of(t[0], n, rate) : 0, is1 = n ? is_of(t[1], n, rate) : 0;
            double e[2] = { 0.0, 0.0 };
            for (int c = 0; c < 2; ++c) for (long long j = is0; j < is1; ++j) e[c] += std::fabs(x[2 * j + c]);
            const int want = e[0] > 1.1 * e[1] ? 0 : e[1] > 1.1 * e[0] ? 1 : -1;
            bool ok = r.is0 == is0 && r.is1 == is1;
            if (kind == KIND_F32) {
                const double m = (double) (is1 > is0 ? is1 - is0 : 0);
                ok = ok && std::fabs(r.e0 - e[0]) <= 2.0 * m * std::ldexp(1.0, -53) * e[0] && std::fabs(r.e1 - e[1]) <= 2.0 * m * std::ldexp(1.0, -53) * e[1];
            } else ok = ok && r.e0 == e[0] && r.e1 == e[1] && r.speaker == want;
            if (!ok) {
                std::printf("MISMATCH kind %d rate %lld n %lld t [%lld, %lld): got %d %lld %lld %.17g %.17g, want %d %lld %lld %.17g %.17g\n", kind, rate, n,
                            t[0], t[1], r.speaker, r.is0, r.is1, r.e0, r.e1, want, is0, is1, e[0], e[1]);
                return 1;
            }
            ++compared;
        }
    }
    std::printf("%ld ranges compared\n", compared);
    return 0;
}

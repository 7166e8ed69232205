// Stand-alone host check of csrc/adpcm_map.h under AddressSanitizer / UBSan: the map algebra of the IMA-ADPCM decode and the sequential
// decoder built from the same header, on exactly sized heap blocks (a read one byte too far is a report; a signed overflow in a composed
// map's additive term is a report).  For every stream and chunk size the chunked plan — index maps composed per chunk, their prefix
// applied to 0, predictor maps from every chunk's entry index, their prefix applied to 0 — must give the sequential decoder's state at
// every chunk edge.  Nothing runs on a GPU.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined scratch/lab/adpcm_map_asan.cpp \
//       -o /tmp/adpcm_map_asan && /tmp/adpcm_map_asan
//   (prints the number of chunk edges compared; exit status 0 = every one held and no sanitizer report)
#include "../../godot-whisper_amd/csrc/adpcm_map.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace wmi::adpcm;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (rng_state >> 33); }

// the stream's nibbles in AudioStreamWAV bytes of one channel, exactly n / 2 bytes on the heap
static std::unique_ptr<unsigned char[]> pack(const std::vector<int> & nib) {
    std::unique_ptr<unsigned char[]> b(new unsigned char[nib.size() / 2 + (nib.empty() ? 1 : 0)]);
    for (size_t k = 0; k < nib.size() / 2; ++k) b[k] = (unsigned char) (nib[2 * k] | (nib[2 * k + 1] << 4));
    return b;
}

static long check(const std::vector<int> & nib, long long chunk) {
    const long long n = (long long) nib.size();
    const auto bytes = pack(nib);
    // the sequential decoder, reading the bytes through the header's layout
    std::vector<int> sp((size_t) n + 1), si((size_t) n + 1);
    int pred = 0, index = 0;
    for (long long i = 0; i < n; ++i) {
        sp[(size_t) i] = pred; si[(size_t) i] = index;
        const int x = nibble_at(bytes.get(), 1, 0, i);
        if (x != nib[(size_t) i]) { std::printf("MISMATCH nibble_at %lld\n", i); std::exit(1); }
        decode_nibble(x, pred, index);
    }
    sp[(size_t) n] = pred; si[(size_t) n] = index;
    // the chunked plan
    const long long chunks = (n + chunk - 1) / chunk;
    std::unique_ptr<IdxMap[]> im(new IdxMap[(size_t) chunks + 1]);
    std::unique_ptr<int[]> entry((new int[(size_t) chunks + 1]));
    for (long long j = 0; j < chunks; ++j) {
        IdxMap m = idx_identity();
        for (long long i = j * chunk; i < n && i < (j + 1) * chunk; ++i) m = compose(m, idx_nibble(nib[(size_t) i]));
        im[(size_t) j] = m;
    }
    IdxMap pi = idx_identity();
    for (long long j = 0; j <= chunks; ++j) { entry[(size_t) j] = apply(pi, 0); if (j < chunks) pi = compose(pi, im[(size_t) j]); }
    PredMap pp = pred_identity();
    long compared = 0;
    for (long long j = 0; j <= chunks; ++j) {
        const long long at = j * chunk < n ? j * chunk : n;
        const int p = apply(pp, 0);
        if (p != sp[(size_t) at] || entry[(size_t) j] != si[(size_t) at]) {
            std::printf("MISMATCH n %lld chunk %lld edge %lld: got (%d, %d), want (%d, %d)\n", n, chunk, j, p, entry[(size_t) j], sp[(size_t) at], si[(size_t) at]);
            std::exit(1);
        }
        ++compared;
        if (j == chunks) break;
        PredMap m = pred_identity();
        int idx = entry[(size_t) j];
        for (long long i = at; i < n && i < (j + 1) * chunk; ++i) {
            m = compose(m, pred_nibble(idx, nib[(size_t) i]));
            idx = apply(idx_nibble(nib[(size_t) i]), idx);
        }
        // a map is a function of the whole domain: both ends through the chunk against the sequential loop
        for (int x0 : { PRED_MIN, PRED_MAX, 0 }) {
            int q = x0, qi = entry[(size_t) j];
            for (long long i = at; i < n && i < (j + 1) * chunk; ++i) decode_nibble(nib[(size_t) i], q, qi);
            if (apply(m, x0) != q) { std::printf("MISMATCH map of chunk %lld from %d\n", j, x0); std::exit(1); }
        }
        pp = compose(pp, m);
    }
    return compared;
}

int main() {
    long compared = 0;
    const long long sizes[] = { 0, 2, 4, 30, 32, 34, 64, 514, 4000 };
    const long long chunkings[] = { 1, 2, 8, 32, 64, 1000 };
    for (long long n : sizes) for (int kind = 0; kind < 6; ++kind) {
        std::vector<int> nib((size_t) n);
        for (long long i = 0; i < n; ++i)
            nib[(size_t) i] = kind == 0 ? (int) (rnd() & 15) : kind == 1 ? 7 : kind == 2 ? 15 : kind == 3 ? 0 : kind == 4 ? (((i / 37) & 1) ? 15 : 7) : (int) (rnd() & 3) | (int) (rnd() & 8);
        for (long long chunk : chunkings) compared += check(nib, chunk);
    }
    // 70 000 nibbles of 7, then 70 000 of 15: the additive term passes 2^31 twice
    std::vector<int> sat(140000);
    for (size_t i = 0; i < sat.size(); ++i) sat[i] = i < 70000 ? 7 : 15;
    for (long long chunk : { 32ll, 35000ll, 70000ll, 140000ll }) compared += check(sat, chunk);
    PredMap m = pred_identity();
    for (int i = 0; i < 70000; ++i) m = compose(m, pred_nibble(88, 7));
    if (m.a <= (1ll << 31) || apply(m, PRED_MIN) != PRED_MAX) { std::printf("MISMATCH saturation map\n"); return 1; }
    // the stereo layout: byte 2k + c holds frames 2k, 2k + 1 of channel c; exactly sized block
    std::unique_ptr<unsigned char[]> st(new unsigned char[6]);
    for (int i = 0; i < 6; ++i) st[(size_t) i] = (unsigned char) (0x10 * (2 * i + 1) + 2 * i);
    for (int c = 0; c < 2; ++c) for (long long i = 0; i < frames_of(6, true); ++i)
        if (nibble_at(st.get(), 2, c, i) != (int) (2 * ((i >> 1) * 2 + c) + (i & 1))) { std::printf("MISMATCH stereo layout\n"); return 1; }
    if (frames_of(7, true) != 6 || frames_of(7, false) != 14) { std::printf("MISMATCH frames_of\n"); return 1; }
    std::printf("%ld chunk edges compared\n", compared);
    return 0;
}

// The front of wmi_full_long, host side: the sequential restatement of the frame energies (the definition k_segment.hip is held to) and
// the plan that turns the energies into pieces (include/wmi_device.h has the interface, DESIGN.md section 5 the rules by number).
// Everything here is integer arithmetic in 10 ms frames, except rule 1's comparisons, which are evaluated in double.  No device.

#include "wmi.h"

#include <algorithm>
#include <cmath>

namespace wmi {

void frame_energy_host(const float * x, int n, float * e) {
    float prev = 0.0f;
    for (int f = 0, F = (n + 159) / 160; f < F; ++f) {
        const int i1 = std::min(160 * f + 160, n);
        float acc = 0.0f;
        for (int i = 160 * f; i < i1; ++i) { const float v = x[i]; acc += fabsf(v - prev); prev = v; }
        e[f] = acc;
    }
}

wmi_long_params long_default_params() {
    wmi_long_params p{};
    p.thold = 0.25f; p.floor = 1e-4f; p.min_silence_ms = 300; p.pad_ms = 100; p.max_gap_ms = 2000; p.max_piece_ms = 30000; p.fit_audio_ctx = 0;
    return p;
}

bool long_params_ok(const wmi_long_params & p) {
    return std::isfinite(p.thold) && p.thold >= 0.0f && std::isfinite(p.floor) && p.floor >= 0.0f && p.min_silence_ms >= 10 && p.pad_ms >= 0 &&
           p.max_gap_ms >= 0 && p.max_piece_ms >= 1000 && p.max_piece_ms <= 30000;
}

// the frames params.offset_ms / duration_ms leave to the plan (whisper_full's seek_start / seek_end, clipped to the signal)
int long_window(int n_samples, int offset_ms, int duration_ms, int * f0, int * f1, int * n_sub) {
    if (n_samples < 1 || offset_ms < 0 || duration_ms < 0 || !f0 || !f1 || !n_sub) return -1;
    const int F = (n_samples + 159) / 160;
    const int a = std::min(offset_ms / 10, F);
    const int b = duration_ms == 0 ? F : (int) std::min<int64_t>((int64_t) a + duration_ms / 10, F);
    *f0 = a; *f1 = std::max(a, b);
    *n_sub = *f1 > a ? std::min(160 * *f1, n_samples) - 160 * a : 0;
    return 0;
}

// e [F]: the energies of a signal of n samples, F = ceil(n / 160).  Pieces in order into `out` (frame0, frame1, audio_ctx).
int long_plan(const float * e, int F, int n, const wmi_long_params & lp, int n_audio_ctx, std::vector<wmi_long_piece> & out) {
    out.clear();
    if (!e || F < 1 || n < 1 || F != (n + 159) / 160 || n_audio_ctx < 1 || !long_params_ok(lp)) return -1;
    const int G = lp.min_silence_ms / 10, P = lp.pad_ms / 10, Gmax = lp.max_gap_ms / 10, Lmax = lp.max_piece_ms / 10;
    // rule 1: the mean level per sample, and the quiet frames
    double sum = 0.0;
    for (int f = 0; f < F; ++f) sum += (double) e[f];
    const double E = sum / (double) n;
    std::vector<char> quiet(F);
    for (int f = 0; f < F; ++f) {
        const double len = (double) std::min(160, n - 160 * f), ef = (double) e[f];
        quiet[f] = ef < (double) lp.thold * E * len || ef < (double) lp.floor * len;
    }
    // rule 2: gaps = maximal quiet runs of at least G frames; islands = the maximal runs of frames in no gap
    struct Island { int a, b, gap; };            // [a, b) (widened below); gap: frames of the gap in front of it (the first island: none, 0)
    std::vector<Island> isl;
    std::vector<int> gs, ge;                     // the gap in front of island i: [gs[i], ge[i]) (the first island: an empty one at 0 unless the signal starts with a gap)
    {
        int a = 0, g0 = 0, g1 = 0;               // start of the island being built, the gap in front of it
        for (int f = 0; f < F; ) {
            if (!quiet[f]) { ++f; continue; }
            int r = f;
            while (r < F && quiet[r]) ++r;
            if (r - f >= G) {
                if (f > a) { isl.push_back({a, f, g1 - g0}); gs.push_back(g0); ge.push_back(g1); }
                a = r; g0 = f; g1 = r;
            }
            f = r;
        }
        if (F > a) { isl.push_back({a, F, g1 - g0}); gs.push_back(g0); ge.push_back(g1); }
    }
    if (isl.empty()) return 0;
    // rule 3: widen by P, never past the midpoint of the gap to the neighbouring island; no neighbour: the end of the signal
    {
        const int ni = (int) isl.size();
        std::vector<int> lo(ni), hi(ni);
        for (int i = 0; i < ni; ++i) {
            const int m_prev = i == 0 ? 0 : (gs[i] + ge[i]) / 2;
            const int m_next = i == ni - 1 ? F : (gs[i + 1] + ge[i + 1]) / 2;
            lo[i] = std::max(isl[i].a - P, m_prev); hi[i] = std::min(isl[i].b + P, m_next);
        }
        for (int i = 0; i < ni; ++i) { isl[i].a = lo[i]; isl[i].b = hi[i]; }
        isl[0].gap = 0;
    }
    // rules 4 and 5: pack left to right; an island longer than Lmax on its own is cut at its quietest frame in the last third of Lmax
    std::vector<std::pair<int, int>> pieces;
    for (size_t i = 0; i < isl.size(); ) {
        const int s = isl[i].a;
        if (isl[i].b - s > Lmax) {
            int c = s + Lmax - Lmax / 3;
            for (int f = c + 1; f <= s + Lmax; ++f) if (e[f] < e[c]) c = f;        // earliest on ties
            pieces.push_back({s, c});
            isl[i].a = c; isl[i].gap = 0;                                          // the rest: a new island at c, no padding there
            continue;
        }
        int end = isl[i].b;
        ++i;
        while (i < isl.size() && isl[i].gap < Gmax && isl[i].b - s <= Lmax) { end = isl[i].b; ++i; }
        pieces.push_back({s, end});
    }
    // rule 6: pieces below 100 frames take what their neighbours leave, the end first
    for (size_t i = 0; i < pieces.size(); ++i) {
        auto & pc = pieces[i];
        if (pc.second - pc.first >= 100) continue;
        pc.second = std::min(pc.first + 100, i + 1 < pieces.size() ? pieces[i + 1].first : F);
        if (pc.second - pc.first >= 100) continue;
        pc.first = std::max(pc.second - 100, i > 0 ? pieces[i - 1].second : 0);
    }
    // rule 7
    for (const auto & pc : pieces) {
        wmi_long_piece o{};
        o.frame0 = pc.first; o.frame1 = pc.second;
        o.audio_ctx = lp.fit_audio_ctx ? std::min(n_audio_ctx, (pc.second - pc.first + 1) / 2 + 128) : 0;
        out.push_back(o);
    }
    return (int) out.size();
}

} // namespace wmi

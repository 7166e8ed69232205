// One evaluator of "does the grammar reject this token?" for the host library and for k_grammar_reject (k_grammar.hip), compiled
// from this text on both sides.  The definition is grammar_penalise's reject set (grammar.cpp; W/whisper.cpp:4114-4176):
//   1. the token's bytes are decoded from the row's partial UTF-8 state as decode_utf8 does — an invalid byte gives the single code
//      point 0 with n_remain = -1, a decoded code point 0 ends the token like the terminator it is in the reference's arrays;
//   2. a token is ACCEPTED iff some stack can consume all of its complete code points and then either there is no trailing partial
//      sequence, or the surviving stack is non-empty and match_partial_char holds at its top;
//   3. an empty stack accepts only an exhausted token with n_remain == 0;
//   4. everything else is REJECTED.
// The grammar is flat: one array of (type, value) elements, every rule closed by an END element, plus the rules' offsets; a position is
// an index into that array (16 bits).  A set of stacks is a run of 16-bit words, stack after stack: {length, position * length}, the
// top last.  No containers, no allocation, no recursion: a token's working set is two such runs of WS_WORDS words that the caller
// supplies (word i of a run at ws[i * stride]: the kernel interleaves the threads of a workgroup in LDS).  Duplicate stacks are
// dropped — only existence matters.  A stack deeper than MAX_DEPTH or a run longer than WS_WORDS yields OVERFLOW, never a guess.
//
// Well-formed grammars only: the flattening (grammar.cpp: grammar_flatten) refuses anything else, and such rows take the host's
// grammar_penalise logic.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define WMI_GE_HD __host__ __device__ inline
#else
#define WMI_GE_HD inline
#endif

namespace wmi { namespace ge {

constexpr int MAX_STACKS = 64, MAX_DEPTH = 16;                 // a row's state: what the host uploads per decoder and step
constexpr int STATE_WORDS = MAX_STACKS * (MAX_DEPTH + 1);
constexpr int WS_WORDS = 120;                                  // one of the two runs of a token's working set
constexpr int MAX_ELEMS = 65535;                               // positions are 16 bits
enum : uint8_t { ACCEPTED = 0, REJECTED = 1, OVERFLOW = 2 };
enum : uint32_t { T_END = 0, T_ALT = 1, T_RULE_REF = 2, T_CHAR = 3, T_CHAR_NOT = 4, T_CHAR_RNG_UPPER = 5, T_CHAR_ALT = 6 };   // W/whisper.h:117-140
constexpr uint16_t DEAD = 0x8000;                              // length word of a stack that has been expanded into others

struct Elem  { uint32_t type, value; };                        // whisper_grammar_element's layout
struct Rules { const Elem * e; const uint32_t * rule_off; int n_rules; };           // rule_off [n_rules + 1]
// texts up to their first NUL (the reference walks C strings), one after the other; off [n + 1], bit 31 of off[id]: never a candidate (an
// empty text); ids >= n (= eot) are never candidates either
struct Vocab { const uint8_t * bytes; const uint32_t * off; int n; };
constexpr uint32_t OFF_MASK = 0x7fffffffu;
// n_stacks = 0: the grammar has no stack left and rejects nothing; < 0: the row's mask comes from the host (capacity exceeded)
struct RowState { uint32_t partial_value; int32_t partial_n_remain; int32_t n_stacks; int32_t n_words; uint16_t words[STATE_WORDS]; };

WMI_GE_HD bool ends_alternative(uint32_t type) { return type == T_END || type == T_ALT; }

// does chr satisfy the (possibly negated) character class starting at p?  *after = the element behind the class
WMI_GE_HD bool match_char(const Rules & R, uint32_t p, uint32_t chr, uint32_t * after) {
    const bool positive = R.e[p].type == T_CHAR;
    bool found = false;
    do {
        if (R.e[p + 1].type == T_CHAR_RNG_UPPER) { found = found || (R.e[p].value <= chr && chr <= R.e[p + 1].value); p += 2; }
        else                                     { found = found || R.e[p].value == chr; p += 1; }
    } while (R.e[p].type == T_CHAR_ALT);
    *after = p;
    return found == positive;
}

// could some completion of the partial sequence satisfy the class at p?  (W/whisper.cpp:3975-4019)
WMI_GE_HD bool match_partial_char(const Rules & R, uint32_t p, uint32_t value, int n_remain) {
    const bool positive = R.e[p].type == T_CHAR;
    if (n_remain < 0 || (n_remain == 1 && value < 2)) return false;       // invalid, or an overlong 7-bit char
    uint32_t low = value << (n_remain * 6);
    const uint32_t high = low | ((1u << (n_remain * 6)) - 1);
    if (low == 0) { if (n_remain == 2) low = 1u << 11; else if (n_remain == 3) low = 1u << 16; }
    do {
        if (R.e[p + 1].type == T_CHAR_RNG_UPPER) { if (R.e[p].value <= high && low <= R.e[p + 1].value) return positive; p += 2; }
        else                                     { if (low <= R.e[p].value && R.e[p].value <= high) return positive; p += 1; }
    } while (R.e[p].type == T_CHAR_ALT);
    return !positive;
}

// a run of stacks: word i at w[i * stride]
struct Run { uint16_t * w; int stride; int used; };
WMI_GE_HD uint16_t run_get(const Run & r, int i) { return r.w[(long) i * r.stride]; }
WMI_GE_HD void run_set(const Run & r, int i, uint16_t v) { r.w[(long) i * r.stride] = v; }

// append the stack {src[s0 .. s0 + n_keep), extra[0 .. n_extra)} to dst unless dst holds it already (alive or expanded).
// 1 appended, 0 already there, -1 over a capacity
WMI_GE_HD int run_append(Run & dst, const Run & src, int s0, int n_keep, int n_extra, uint16_t x0, uint16_t x1) {
    const int len = n_keep + n_extra;
    if (len > MAX_DEPTH) return -1;
    for (int p = 0; p < dst.used;) {
        const int l = run_get(dst, p) & ~DEAD;
        if (l == len) {
            bool same = true;
            for (int j = 0; j < n_keep && same; ++j) same = run_get(dst, p + 1 + j) == run_get(src, s0 + j);
            if (same && n_extra > 0) same = run_get(dst, p + 1 + n_keep) == x0;
            if (same && n_extra > 1) same = run_get(dst, p + 2 + n_keep) == x1;
            if (same) return 0;
        }
        p += 1 + l;
    }
    if (dst.used + 1 + len > WS_WORDS) return -1;
    const int p = dst.used;
    run_set(dst, p, (uint16_t) len);
    for (int j = 0; j < n_keep; ++j) run_set(dst, p + 1 + j, run_get(src, s0 + j));
    if (n_extra > 0) run_set(dst, p + 1 + n_keep, x0);
    if (n_extra > 1) run_set(dst, p + 2 + n_keep, x1);
    dst.used = p + 1 + len;
    return 1;
}

// advance_stack without recursion: every stack of dst from word `from` on whose top is a rule reference is replaced — marked DEAD, its
// expansions appended behind — by one stack per alternative of the referenced rule, until every live stack is empty or rests on a
// character class.  false: over a capacity
WMI_GE_HD bool run_expand(const Rules & R, Run & dst, int from) {
    for (int p = from; p < dst.used;) {
        const uint16_t hdr = run_get(dst, p);
        const int len = hdr & ~DEAD;
        if (!(hdr & DEAD) && len > 0) {
            const uint32_t top = run_get(dst, p + len);
            const uint32_t type = R.e[top].type;
            if (type != T_CHAR && type != T_CHAR_NOT) {
                run_set(dst, p, (uint16_t) (hdr | DEAD));
                if (type == T_RULE_REF && R.e[top].value < (uint32_t) R.n_rules) {
                    const bool has_next = !ends_alternative(R.e[top + 1].type);          // what follows the reference
                    uint32_t sub = R.rule_off[R.e[top].value];
                    for (;;) {                                                           // one new stack per alternative
                        const bool has_sub = !ends_alternative(R.e[sub].type);           // a non-empty alternative
                        const uint16_t x0 = has_next ? (uint16_t) (top + 1) : (uint16_t) sub;
                        if (run_append(dst, dst, p + 1, len - 1, (has_next ? 1 : 0) + (has_sub ? 1 : 0), x0, (uint16_t) sub) < 0) return false;
                        while (!ends_alternative(R.e[sub].type)) ++sub;
                        if (R.e[sub].type != T_ALT) break;
                        ++sub;
                    }
                }
            }
        }
        p += 1 + len;
    }
    return true;
}

// ws: 2 * WS_WORDS words at ws[i * stride]
WMI_GE_HD uint8_t eval_token(const Rules & R, const Vocab & V, const RowState & st, int id, uint16_t * ws, int stride) {
    if (id < 0 || id >= V.n || st.n_stacks <= 0) return ACCEPTED;
    const uint32_t o0 = V.off[id];
    if (o0 >> 31) return ACCEPTED;
    const uint8_t * t = V.bytes + o0;
    const int n = (int) ((V.off[id + 1] & OFF_MASK) - o0);

    Run cur = { const_cast<uint16_t *>(st.words), 1, st.n_words };
    int which = 0;                                        // which of the two runs the next set goes to
    bool ended = false;                                   // a decoded 0: the reference's arrays end there, the tail is still the whole text's

    // one code point: cur -> the stacks that took it.  false: none did
    auto take = [&](uint32_t chr, uint8_t * verdict) {
        Run nx = { ws + (long) which * WS_WORDS * stride, stride, 0 };
        for (int p = 0; p < cur.used;) {
            const uint16_t hdr = run_get(cur, p);
            const int len = hdr & ~DEAD;
            uint32_t after;
            if (!(hdr & DEAD) && len > 0 && match_char(R, run_get(cur, p + len), chr, &after)) {
                const int from = nx.used;
                const bool has_after = !ends_alternative(R.e[after].type);
                const int r = run_append(nx, cur, p + 1, len - 1, has_after ? 1 : 0, (uint16_t) after, 0);
                if (r < 0 || (r > 0 && !run_expand(R, nx, from))) { *verdict = OVERFLOW; return false; }
            }
            p += 1 + len;
        }
        if (nx.used == 0) { *verdict = REJECTED; return false; }
        cur = nx; which ^= 1;
        return true;
    };

    // decode_utf8 (W/whisper.cpp:3878-3935), a code point at a time
    uint8_t verdict = REJECTED;
    uint32_t value = st.partial_value;
    int n_remain = st.partial_n_remain;
    int i = 0;
    for (; i < n && n_remain > 0; ++i, --n_remain) {
        const uint8_t b = t[i];
        if ((b >> 6) != 2) return REJECTED;               // invalid: one code point 0, n_remain = -1 — no stack takes that
        value = (value << 6) + (b & 0x3F);
    }
    if (st.partial_n_remain > 0 && n_remain == 0) {
        if (value == 0) ended = true; else if (!take(value, &verdict)) return verdict;
    }
    while (i < n) {
        const uint8_t first = t[i];
        const int hi = first >> 4;
        n_remain = (hi < 8 ? 1 : hi < 12 ? 0 : hi < 14 ? 2 : hi == 14 ? 3 : 4) - 1;
        if (n_remain < 0) return REJECTED;
        value = first & ((1u << (7 - n_remain)) - 1);
        ++i;
        for (; i < n && n_remain > 0; ++i, --n_remain) value = (value << 6) + (t[i] & 0x3F);
        if (n_remain == 0 && !ended) {
            if (value == 0) ended = true; else if (!take(value, &verdict)) return verdict;
        }
    }
    // exhausted: the tail {value, n_remain} against the survivors
    for (int p = 0; p < cur.used;) {
        const uint16_t hdr = run_get(cur, p);
        const int len = hdr & ~DEAD;
        if (!(hdr & DEAD)) {
            if (len == 0) { if (n_remain == 0) return ACCEPTED; }
            else if (n_remain == 0 || match_partial_char(R, run_get(cur, p + len), value, n_remain)) return ACCEPTED;
        }
        p += 1 + len;
    }
    return REJECTED;
}

}} // namespace wmi::ge

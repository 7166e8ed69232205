// Stand-alone host check of csrc/grammar_eval.h under AddressSanitizer / UBSan: the evaluator k_grammar_reject compiles, run on the host
// over three grammars (the colour list, the negated class and the unicode grammar of tests/golden_util.py) and a synthetic vocabulary with
// truncated, overlong and invalid UTF-8, against grammar.cpp's own reject set (grammar_reject_mask).  Nothing runs on a GPU.
//
//   cd godot-whisper_amd/csrc && hipcc -O1 -g -std=c++17 -x hip --offload-host-only -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined ../../scratch/lab/grammar_eval_asan.cpp -o /tmp/grammar_eval_asan
//   /tmp/grammar_eval_asan          (prints the number of comparisons; exit status 0 = every mask equal and no sanitizer report)
#include "../../godot-whisper_amd/csrc/grammar.cpp"

#include <cstdio>

using namespace wmi;

typedef std::vector<std::vector<whisper_grammar_element>> RuleSet;
static whisper_grammar_element E(whisper_gretype t, uint32_t v) { return whisper_grammar_element{ t, v }; }
static void lit(std::vector<whisper_grammar_element> & r, std::initializer_list<uint32_t> cps) { for (uint32_t c : cps) r.push_back(E(WHISPER_GRETYPE_CHAR, c)); }
static void lits(std::vector<whisper_grammar_element> & r, const char * s) { for (; *s; ++s) r.push_back(E(WHISPER_GRETYPE_CHAR, (uint8_t) *s)); }

static RuleSet colours() {
    RuleSet R(6);
    const auto ref = [](uint32_t i) { return E(WHISPER_GRETYPE_RULE_REF, i); };
    const auto ALT = E(WHISPER_GRETYPE_ALT, 0);
    const auto digit = [](std::vector<whisper_grammar_element> & r) { r.push_back(E(WHISPER_GRETYPE_CHAR, '0')); r.push_back(E(WHISPER_GRETYPE_CHAR_RNG_UPPER, '9')); };
    R[0] = { ref(3), ref(1), ref(2) }; lits(R[0], ".");
    lits(R[1], "red"); R[1].push_back(ALT); lits(R[1], "green"); R[1].push_back(ALT); lits(R[1], "blue"); R[1].push_back(ALT); R[1].push_back(ref(4));
    lits(R[2], ", "); R[2].push_back(ref(1)); R[2].push_back(ref(2)); R[2].push_back(ALT);
    lits(R[3], " "); R[3].push_back(ALT);
    digit(R[4]); R[4].push_back(ref(5));
    digit(R[5]); R[5].push_back(ref(5)); R[5].push_back(ALT);
    return R;
}
static RuleSet negated() {
    std::vector<whisper_grammar_element> cls = { E(WHISPER_GRETYPE_CHAR_NOT, '0'), E(WHISPER_GRETYPE_CHAR_RNG_UPPER, '9'), E(WHISPER_GRETYPE_CHAR_ALT, ','),
                                                 E(WHISPER_GRETYPE_CHAR_ALT, 'x'), E(WHISPER_GRETYPE_CHAR_RNG_UPPER, 'z') };
    RuleSet R(3);
    R[0] = { E(WHISPER_GRETYPE_RULE_REF, 1) };
    R[1] = cls; R[1].push_back(E(WHISPER_GRETYPE_RULE_REF, 2));
    R[2] = cls; R[2].push_back(E(WHISPER_GRETYPE_RULE_REF, 2)); R[2].push_back(E(WHISPER_GRETYPE_ALT, 0));
    return R;
}
static RuleSet unicode() {
    RuleSet R(3);
    R[0] = { E(WHISPER_GRETYPE_RULE_REF, 1), E(WHISPER_GRETYPE_RULE_REF, 2) }; lits(R[0], "!");
    lit(R[1], { 0xE9 }); R[1].push_back(E(WHISPER_GRETYPE_ALT, 0));
    R[1].push_back(E(WHISPER_GRETYPE_CHAR, 0x3B1)); R[1].push_back(E(WHISPER_GRETYPE_CHAR_RNG_UPPER, 0x3C9)); R[1].push_back(E(WHISPER_GRETYPE_ALT, 0));
    lit(R[1], { 0x65E5, 0x672C });
    R[2] = { E(WHISPER_GRETYPE_RULE_REF, 1), E(WHISPER_GRETYPE_RULE_REF, 2), E(WHISPER_GRETYPE_ALT, 0) };
    return R;
}

int main() {
    whisper_context ctx;
    Vocab & v = ctx.model.vocab;
    const std::vector<std::string> texts = {
        "", " ", "red", " red", "re", "d", ",", ", ", ", g", "green", "blue", ".", "blue.", "12", "7,", " 1", "x", "hello", " world", "a,b", "!",
        "\xC3\xA9", "\xC3", "\xA9", "\xA9!", "\xCE\xB2", "\xCE", "\xB2\xCF\x89", "\xE6\x97\xA5", "\xE6", "\xE6\x97", "\x97\xA5", "\xA5\xE6\x9C\xAC", "\xE6\x97\xA5\xE6\x9C",
        "\xE6\x97\xA5\xE6\x9C\xAC", "\xC3\xA9\xCE\xB2!", "\xF0\x9F\x98\x80", "\xF0\x9F", "\x9F\x98\x80",
        "\xFF", "\x80" "abc", "a\xC3", "a\xC3" "b", "\xC0\x80", "\xC0\x80" "red", "\xC1\xBF", std::string("a\0b", 3), std::string("\0red", 4), "\xED\xA0\x80", "\xF8\x88\x80\x80\x80",
        "caf\xC3\xA9", "caf\xC3", "red, green, blue.", " red, 12", "\xCE\xB1\xCF\x89\xC3\xA9\xE6\x97\xA5\xE6\x9C\xAC!",
    };
    v.id_to_token = texts;
    v.id_to_token.push_back("[_EOT_]"); v.id_to_token.push_back("[_SOT_]"); v.id_to_token.push_back("[_TT_1]");
    v.eot = (int32_t) texts.size(); v.sot = v.eot + 1; v.beg = v.eot + 2; v.n_vocab = (int) v.id_to_token.size();
    for (int i = 0; i < v.n_vocab; ++i) v.token_to_id[v.id_to_token[i]] = i;
    const auto id = [&](const std::string & s) { return v.token_to_id.at(s); };

    std::vector<uint8_t> bytes; std::vector<uint32_t> off;
    grammar_vocab_flat(v, bytes, off);

    struct Set { const char * name; RuleSet rules; std::vector<std::vector<std::string>> hists; };
    std::vector<Set> sets = {
        { "colours", colours(), { {}, { " red" }, { " red", "," }, { "re" }, { "re", "d", ", g" }, { "blue." }, { "hello" }, { " 1" }, { "[_TT_1]", "red" }, { " red", ", ", "12", ", " } } },
        { "negated", negated(), { {}, { "hello" }, { "caf\xC3" }, { "caf\xC3", "\xA9" }, { "12" }, { "\xE6\x97" }, { "\xFF" } } },
        { "unicode", unicode(), { {}, { "\xC3" }, { "\xC3\xA9" }, { "\xCE" }, { "\xE6" }, { "\xE6\x97" }, { "\xE6\x97\xA5" }, { "\xE6\x97\xA5\xE6\x9C" }, { "\xE6\x97\xA5\xE6\x9C\xAC", "\xCE\xB2" },
                                    { "\xC3\xA9", "!" }, { "x" }, { "\xF0\x9F" } } },
    };
    int n_cmp = 0, n_bad = 0, n_rej = 0;
    for (const Set & s : sets) {
        std::vector<const whisper_grammar_element *> ptrs;
        RuleSet closed = s.rules;
        for (auto & r : closed) { r.push_back(E(WHISPER_GRETYPE_END, 0)); ptrs.push_back(r.data()); }
        for (const auto & h : s.hists) {
            Grammar g = grammar_init(ptrs.data(), ptrs.size(), 0);
            for (const std::string & t : h) grammar_accept_token(ctx, g, id(t));
            const GrammarFlat f = grammar_flatten(g);
            ge::RowState st;
            if (!f.ok || !grammar_row_state(g, f, st)) { fprintf(stderr, "%s: the state does not fit\n", s.name); return 2; }
            std::vector<uint8_t> got(v.n_vocab, 9), want(v.n_vocab, 9);
            if (!grammar_eval_host(f, bytes, off, st, got.data(), v.n_vocab)) { fprintf(stderr, "%s: overflow\n", s.name); return 2; }
            grammar_reject_mask(ctx, g, want.data());
            ++n_cmp;
            for (int i = 0; i < v.n_vocab; ++i) {
                n_rej += want[i];
                if (got[i] != want[i]) { ++n_bad; fprintf(stderr, "%s, history of %zu: token %d evaluator %d definition %d\n", s.name, h.size(), i, got[i], want[i]); }
            }
        }
    }
    // the capacities: more stacks than a state holds, and a malformed grammar, are refused by the flattening — never evaluated
    {
        RuleSet many(1);
        for (int i = 0; i < ge::MAX_STACKS + 6; ++i) { if (i) many[0].push_back(E(WHISPER_GRETYPE_ALT, 0)); lit(many[0], { 0x4E00u + i, 'x' }); }
        many[0].push_back(E(WHISPER_GRETYPE_END, 0));
        const whisper_grammar_element * p = many[0].data();
        const Grammar g = grammar_init(&p, 1, 0);
        ge::RowState st;
        if (grammar_row_state(g, grammar_flatten(g), st) || st.n_stacks != -1) { fprintf(stderr, "a state over the capacity was accepted\n"); return 2; }
        Grammar bad; bad.rules = { { E(WHISPER_GRETYPE_CHAR_RNG_UPPER, 'a'), E(WHISPER_GRETYPE_END, 0) } }; bad.stacks = { { GrammarPos{ 0, 0 } } };
        if (grammar_flatten(bad).ok) { fprintf(stderr, "a malformed grammar was flattened\n"); return 2; }
    }
    printf("%d states compared over %d tokens, %d rejections in all, %d differences\n", n_cmp, v.n_vocab, n_rej, n_bad);
    return n_bad ? 1 : 0;
}

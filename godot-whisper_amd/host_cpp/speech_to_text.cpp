// see speech_to_text.h.  Reference lines are cited per function.
#include "speech_to_text.h"
#include <algorithm>

#include <cmath>
#include <cstdio>
#include <cstring>

namespace godot_whisper {

SpeechToText::SpeechToText(const TranscribeSettings & s) : settings(s) {}

SpeechToText::~SpeechToText() {                                        // src/speech_to_text.cpp:348-351
    whisper_free(context_instance);
    context_instance = nullptr;
}

const char * SpeechToText::language_to_code(int lang) const {           // src/speech_to_text.cpp:117-324
    if (lang == Auto) return "auto";
    if (lang >= 1 && lang - 1 <= whisper_lang_max_id()) return whisper_lang_str(lang - 1);   // the enum follows whisper.cpp's table
    return "en";                                                         // "Default to English if unknown language"
}

void SpeechToText::set_language_model(const uint8_t * data, size_t size) {   // src/speech_to_text.cpp:326-346
    whisper_free(context_instance);
    context_instance = nullptr;
    fprintf(stderr, "%s\n", whisper_print_system_info());
    if (data == nullptr || size == 0) return;
    const whisper_context_params context_params{ settings.use_gpu };
    context_instance = whisper_init_from_buffer_with_params((void *) data, size, context_params);
    if (context_instance && no_speech != 0) (void) wmi_set_no_speech(context_instance, no_speech);
    if (context_instance && token_dtw) (void) wmi_set_token_dtw(context_instance, 1, token_dtw_pairs.data(), (int) token_dtw_pairs.size() / 2);
    if (context_instance && grammar_device) (void) wmi_set_grammar_device(context_instance, 1);
    if (context_instance && speaker_mode) (void) wmi_set_speaker(context_instance, speaker_mode, speaker_ratio);
    if (context_instance && wav_adpcm) (void) wmi_set_wav_adpcm(context_instance, 1);
}

bool SpeechToText::set_wav_adpcm(bool on) {
    const bool prev = wav_adpcm;
    wav_adpcm = on;
    if (context_instance) (void) wmi_set_wav_adpcm(context_instance, on ? 1 : 0);
    return prev;
}

int SpeechToText::set_speaker_labels(int mode, double ratio) {
    const int prev = speaker_mode;
    speaker_mode = mode < 0 ? 0 : (mode > 2 ? 2 : mode); speaker_ratio = ratio;
    if (context_instance) (void) wmi_set_speaker(context_instance, speaker_mode, speaker_ratio);
    return prev;
}

std::vector<SegmentSpeaker> SpeechToText::speakers() const {
    std::vector<SegmentSpeaker> out;
    if (!context_instance || !speaker_mode) return out;
    const int n_segments = whisper_full_n_segments(context_instance);
    for (int i = 0; i < n_segments; ++i) {
        struct wmi_speaker rec;
        if (wmi_full_get_segment_speaker(context_instance, i, &rec) != 0) return std::vector<SegmentSpeaker>();
        SegmentSpeaker s;
        s.t0 = whisper_full_get_segment_t0(context_instance, i); s.t1 = whisper_full_get_segment_t1(context_instance, i);
        s.text = whisper_full_get_segment_text(context_instance, i);
        s.speaker = rec.speaker; s.e0 = rec.e0; s.e1 = rec.e1;
        out.push_back(std::move(s));
    }
    return out;
}

std::string SpeechToText::diarized_text() const {                    // examples/main/main.cpp:262-265 in front of every segment
    std::string out;
    for (const SegmentSpeaker & s : speakers())
        out += std::string("(speaker ") + (s.speaker < 0 ? "?" : s.speaker == 0 ? "0" : "1") + ") " + s.text;
    return out;
}

void SpeechToText::set_grammar(const std::vector<std::vector<whisper_grammar_element>> & rules, float penalty) {
    grammar_rules = rules; grammar_penalty = penalty;
    grammar_ptrs.clear();
    for (auto & r : grammar_rules) { r.push_back(whisper_grammar_element{ WHISPER_GRETYPE_END, 0 }); grammar_ptrs.push_back(r.data()); }
}

int SpeechToText::set_grammar_device(bool on) {
    grammar_device = on;
    return context_instance ? wmi_set_grammar_device(context_instance, on ? 1 : 0) : 0;
}

int SpeechToText::set_token_dtw(bool on, const std::vector<int32_t> & layer_head) {
    token_dtw = on; token_dtw_pairs = layer_head;
    if (!context_instance) return 0;
    return wmi_set_token_dtw(context_instance, on ? 1 : 0, token_dtw_pairs.data(), (int) token_dtw_pairs.size() / 2);
}

int SpeechToText::set_draft(const std::vector<int32_t> & tokens) {
    if (!context_instance) return -1;
    return wmi_set_draft(context_instance, tokens.empty() ? nullptr : tokens.data(), (int) tokens.size());
}

struct wmi_draft_status SpeechToText::draft_status() const {
    struct wmi_draft_status s = { 0, 0, 0, 0, 1 };
    if (context_instance) (void) wmi_draft_status(context_instance, &s);
    return s;
}

int SpeechToText::set_no_speech(int mode) {
    const int prev = no_speech;
    no_speech = mode < 0 ? 0 : (mode > 3 ? 3 : mode);
    if (context_instance) (void) wmi_set_no_speech(context_instance, no_speech);
    return prev;
}

std::vector<float> SpeechToText::resample(const std::vector<float> & interleaved_xy, InterpolatorType interpolator_type, int mix_rate) {   // src/speech_to_text.cpp:353-376
    last_resample_error.clear();
    const int64_t buffer_len = (int64_t) (interleaved_xy.size() / 2);
    const uint32_t expected_size = (uint32_t) (buffer_len * WHISPER_SAMPLE_RATE / mix_rate);
    if (!context_instance || buffer_len == 0) return {};
    std::vector<float> buffer_float((size_t) buffer_len);
    if (wmi_downmix_stereo(context_instance, interleaved_xy.data(), (int) buffer_len, 0, buffer_float.data()) != 0) return {};   // _vector2_array_to_float_array
    std::vector<float> resampled_float((size_t) std::max<int64_t>(expected_size, mix_rate == WHISPER_SAMPLE_RATE ? buffer_len : 0) + 1);
    int result_size = wmi_resample(context_instance, buffer_float.data(), (int) buffer_len, mix_rate, WHISPER_SAMPLE_RATE, (int) interpolator_type, 0,
                                   resampled_float.data(), (int) resampled_float.size());                                        // _resample_audio_buffer
    if (result_size < 0) result_size = 0;                                                                                      // converter error: 0 frames
    if ((uint32_t) result_size != expected_size)
        last_resample_error = "size differ exp: " + std::to_string(expected_size) + " res: " + std::to_string(result_size);
    resampled_float.resize((size_t) result_size);
    return resampled_float;
}

bool SpeechToText::voice_activity_detection(const std::vector<float> & buffer) const {     // src/speech_to_text.cpp:378-399
    const int n_samples_vad_window = WHISPER_SAMPLE_RATE * 3;            // the most recent 3 s
    const int vad_last_ms = 500;                                         // energy of the last 500 ms vs the whole window
    if ((int) buffer.size() >= n_samples_vad_window) {
        std::vector<float> window(buffer.end() - n_samples_vad_window, buffer.end());
        return vad_simple(window, WHISPER_SAMPLE_RATE, vad_last_ms, settings.vad_treshold, settings.freq_treshold);
    }
    return false;
}

whisper_full_params SpeechToText::make_params(const std::string & initial_prompt, int audio_ctx) const {   // :402-413
    whisper_full_params p = whisper_full_default_params(WHISPER_SAMPLING_GREEDY);
    p.language = language_to_code(language);
    p.audio_ctx = audio_ctx;
    p.speed_up = settings.speed_up_2x;
    p.split_on_word = true;
    p.token_timestamps = true;
    p.suppress_non_speech_tokens = true;
    p.single_segment = true;
    p.max_tokens = settings.max_tokens;
    p.entropy_thold = settings.entropy_treshold;
    p.initial_prompt = initial_prompt.c_str();          // the caller's string outlives the call (the reference lets it dangle, :413)
    if (!grammar_ptrs.empty()) {
        p.grammar_rules = const_cast<const whisper_grammar_element **>(grammar_ptrs.data()); p.n_grammar_rules = grammar_ptrs.size();
        p.i_start_rule = 0; p.grammar_penalty = grammar_penalty;
    }
    return p;
}

Transcription SpeechToText::collect() const {                            // src/speech_to_text.cpp:424-447
    Transcription out;
    out.ok = true;
    const int n_segments = whisper_full_n_segments(context_instance);
    for (int i = 0; i < n_segments; ++i) {
        const int n_tokens = whisper_full_n_tokens(context_instance, i);
        out.full_text += whisper_full_get_segment_text(context_instance, i);
        const float no_speech_prob = wmi_full_get_segment_no_speech_prob(context_instance, i);
        for (int j = 0; j < n_tokens; ++j) {
            const whisper_token_data token = whisper_full_get_token_data(context_instance, i, j);
            Token t;
            t.text = whisper_full_get_token_text(context_instance, i, j);
            t.id = token.id; t.p = token.p; t.plog = token.plog; t.pt = token.pt; t.ptsum = token.ptsum;
            t.t0 = token.t0; t.t1 = token.t1; t.tid = token.tid; t.vlen = token.vlen;
            t.no_speech_prob = no_speech_prob;
            t.t_dtw = wmi_full_get_token_dtw(context_instance, i, j);
            out.tokens.push_back(std::move(t));
        }
    }
    return out;
}

std::vector<SpeechToText::TextScore> SpeechToText::score_texts(const std::vector<float> & buffer, const std::vector<std::string> & texts,
                                                               const std::string & prompt, bool length_norm, int audio_ctx) {
    std::vector<TextScore> res;
    if (!context_instance) {
        fprintf(stderr, "ERROR: Context instance is null\n");
        return res;
    }
    auto tokenize = [&](const std::string & t) {
        std::vector<whisper_token> ids(t.size() + 8);
        const int n = whisper_tokenize(context_instance, t.c_str(), ids.data(), (int) ids.size());
        ids.resize(n > 0 ? n : 0);
        return ids;
    };
    std::vector<TextScore> all(texts.size());
    std::vector<whisper_token> flat;
    std::vector<int32_t> n_tokens;
    for (size_t c = 0; c < texts.size(); ++c) {
        all[c].text = texts[c];
        const auto ids = tokenize(" " + texts[c]);
        all[c].tokens.assign(ids.begin(), ids.end());
        flat.insert(flat.end(), ids.begin(), ids.end());
        n_tokens.push_back((int32_t) ids.size());
    }
    wmi_score_params p = wmi_score_default_params();
    p.length_norm = length_norm ? 1 : 0;
    if (whisper_is_multilingual(context_instance)) {
        const int id = whisper_lang_id(language_to_code(language));
        p.lang_id = id > 0 ? id : 0;                                      // ("auto": English, nothing is detected here)
    }
    const std::vector<whisper_token> pt = prompt.empty() ? std::vector<whisper_token>() : tokenize(prompt);
    if (!pt.empty()) { p.prompt_tokens = pt.data(); p.prompt_n_tokens = (int32_t) pt.size(); }
    std::vector<wmi_text_score> out(texts.size() ? texts.size() : 1);
    std::vector<float> lp(flat.size() + texts.size() + 1);
    last_return = wmi_score_pcm(context_instance, p, buffer.data(), (int) buffer.size(), 0, audio_ctx, flat.empty() ? nullptr : flat.data(),
                                n_tokens.data(), (int) texts.size(), out.data(), lp.data());
    if (last_return != 0) {
        fprintf(stderr, "ERROR: Failed to score the texts, returned %d\n", last_return);
        return res;
    }
    for (size_t c = 0; c < texts.size(); ++c) {
        all[c].token_logprobs.assign(lp.begin() + out[c].first, lp.begin() + out[c].first + out[c].n_scored);
        all[c].sum_logprob = out[c].sum_logprob; all[c].avg_logprob = out[c].avg_logprob; all[c].posterior = out[c].posterior;
    }
    return all;
}

Transcription SpeechToText::transcribe(const std::vector<float> & buffer, const std::string & initial_prompt, int audio_ctx) {
    const whisper_full_params whisper_params = make_params(initial_prompt, audio_ctx);
    if (!context_instance) {
        fprintf(stderr, "ERROR: Context instance is null\n");
        return Transcription();
    }
    const int ret = whisper_full(context_instance, whisper_params, buffer.data(), (int) buffer.size());
    last_return = ret;
    if (ret != 0) {
        fprintf(stderr, "ERROR: Failed to process audio, returned %d\n", ret);
        return Transcription();
    }
    return collect();
}

Transcription SpeechToText::transcribe_wav(const std::vector<uint8_t> & data, int format, bool stereo, int mix_rate,
                                           const std::string & initial_prompt, int audio_ctx, InterpolatorType interpolator_type) {
    const whisper_full_params whisper_params = make_params(initial_prompt, audio_ctx);
    if (!context_instance) {
        fprintf(stderr, "ERROR: Context instance is null\n");
        return Transcription();
    }
    static const uint8_t none = 0;                                   // an empty PackedByteArray still hands over a pointer
    const wmi_wav wav = { data.empty() ? &none : data.data(), (long long) data.size(), format, stereo ? 1 : 0, mix_rate, 0 };
    const int ret = wmi_full_wav(context_instance, whisper_params, &wav, (int) interpolator_type);
    last_return = ret;
    if (ret != 0) {
        fprintf(stderr, "ERROR: Failed to process audio, returned %d\n", ret);
        return Transcription();
    }
    return collect();
}

std::vector<SpeechToText::DialogueSegment> SpeechToText::transcribe_wav_channels(const std::vector<uint8_t> & data, int format, int mix_rate,
                                                                                const std::string & initial_prompt, int audio_ctx,
                                                                                InterpolatorType interpolator_type) {
    std::vector<DialogueSegment> out;
    last_channels.clear();
    const whisper_full_params whisper_params = make_params(initial_prompt, audio_ctx);
    if (!context_instance) {
        fprintf(stderr, "ERROR: Context instance is null\n");
        return out;
    }
    static const uint8_t none = 0;
    const wmi_wav wav = { data.empty() ? &none : data.data(), (long long) data.size(), format, 1, mix_rate, 0 };
    const int ret = wmi_full_wav_channels(context_instance, whisper_params, &wav, (int) interpolator_type);
    last_return = ret;
    if (ret != 0) {
        fprintf(stderr, "ERROR: Failed to process audio, returned %d\n", ret);
        return out;
    }
    for (int c = 0; c < 2; ++c) {
        if (wmi_channels_select(context_instance, c) < 0) return out;
        last_channels.push_back(collect());
    }
    const int n = wmi_channels_select(context_instance, -1);         // the dialogue view stays selected
    for (int i = 0; i < n; ++i) {
        struct wmi_channel_segment rec;
        if (wmi_channels_get_segment(context_instance, i, &rec) != 0) return std::vector<DialogueSegment>();
        DialogueSegment s;
        s.channel = rec.channel; s.index = rec.index;
        s.t0 = whisper_full_get_segment_t0(context_instance, i); s.t1 = whisper_full_get_segment_t1(context_instance, i);
        s.text = whisper_full_get_segment_text(context_instance, i);
        out.push_back(std::move(s));
    }
    return out;
}

std::string SpeechToText::dialogue_text(const std::vector<DialogueSegment> & dialogue) {
    std::string out;
    for (const DialogueSegment & s : dialogue) out += std::string("(speaker ") + (s.channel == 0 ? "0" : "1") + ") " + s.text;
    return out;
}

std::vector<Transcription> SpeechToText::transcribe_batch(const std::vector<std::vector<float>> & buffers,
                                                          const std::string & initial_prompt, int audio_ctx) {
    std::vector<Transcription> out;
    const whisper_full_params whisper_params = make_params(initial_prompt, audio_ctx);
    if (!context_instance) {
        fprintf(stderr, "ERROR: Context instance is null\n");
        return out;
    }
    last_langs.clear();
    std::vector<const float *> ptrs; std::vector<int> lens;
    for (const auto & b : buffers) { ptrs.push_back(b.data()); lens.push_back((int) b.size()); }
    const int ret = wmi_full_batch(context_instance, whisper_params, ptrs.data(), lens.data(), (int) buffers.size(), 0);
    last_return = ret;
    if (ret != 0) {
        fprintf(stderr, "ERROR: Failed to process audio, returned %d\n", ret);
        return out;
    }
    for (int c = 0; c < (int) buffers.size(); ++c) {
        wmi_batch_select(context_instance, c);
        last_langs.push_back(wmi_batch_lang_id(context_instance, c));
        out.push_back(collect());
    }
    return out;
}

Transcription SpeechToText::transcribe_long(const std::vector<float> & buffer, const std::string & initial_prompt,
                                            const wmi_long_params * long_params) {
    const whisper_full_params whisper_params = make_params(initial_prompt, 0);
    last_pieces.clear();
    if (!context_instance) {
        fprintf(stderr, "ERROR: Context instance is null\n");
        return Transcription();
    }
    const int ret = wmi_full_long(context_instance, whisper_params, buffer.data(), (int) buffer.size(), 0, long_params);
    last_return = ret;
    if (ret != 0) {
        fprintf(stderr, "ERROR: Failed to process audio, returned %d\n", ret);
        return Transcription();
    }
    for (int i = 0; i < wmi_long_n_pieces(context_instance); ++i) {
        wmi_long_piece pc{};
        if (wmi_long_get_piece(context_instance, i, &pc) == 0) last_pieces.push_back(pc);
    }
    return collect();                                  // the call leaves the merged result selected
}

// ------------------------------------------------------------------------------------------------ VAD
void high_pass_filter(std::vector<float> & data, float cutoff, float sample_rate) {          // src/speech_to_text.cpp:53-66
    const float rc = 1.0f / (2.0f * 3.14159265358979323846 * cutoff);      // Math_PI is a double in the reference: double arithmetic, rounded to float
    const float dt = 1.0f / sample_rate;
    const float alpha = dt / (rc + dt);
    float y = data[0];
    for (size_t i = 1; i < data.size(); i++) {
        y = alpha * (y + data[i] - data[i - 1]);
        data[i] = y;
    }
}

bool vad_simple(std::vector<float> & pcmf32, int sample_rate, int last_ms, float vad_thold, float freq_thold) {   // :69-104
    const int n_samples = (int) pcmf32.size();
    const int n_samples_last = (sample_rate * last_ms) / 1000;
    if (n_samples_last >= n_samples) return false;                        // not enough samples
    if (freq_thold > 0.0f) high_pass_filter(pcmf32, freq_thold, (float) sample_rate);
    float energy_all = 0.0f, energy_last = 0.0f;
    for (int i = 0; i < n_samples; i++) {
        energy_all += fabsf(pcmf32[i]);
        if (i >= n_samples - n_samples_last) energy_last += fabsf(pcmf32[i]);
    }
    energy_all /= n_samples;
    energy_last /= n_samples_last;
    // the host's extra "both energies tiny" clause on top of upstream vad_simple
    if (!(energy_all < 0.0001f && energy_last < 0.0001f) || energy_last > vad_thold * energy_all) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------ GDScript nodes
std::string remove_special_characters(std::string message) {            // addon/audio_stream_to_text.gd:64-88
    const char * pairs[2][2] = { {"[", "]"}, {"<", ">"} };
    for (auto & pr : pairs) {
        while (true) {
            const size_t i = message.find(pr[0]), j = message.find(pr[1]);
            if (i == std::string::npos || j == std::string::npos || j < i) break;
            message.erase(i, j + 1 - i);
        }
    }
    const std::string hallucination = ". you.";
    if (message.size() >= hallucination.size() && message.compare(message.size() - hallucination.size(), hallucination.size(), hallucination) == 0)
        message.replace(message.size() - hallucination.size(), hallucination.size(), ".");
    return message;
}

std::string AudioStreamToText::get_text(const std::vector<float> & pcm16k, const std::string & initial_prompt) {   // :31-62
    const Transcription t = transcribe(pcm16k, initial_prompt, 0);
    if (!t.ok) return std::string();
    return remove_special_characters(t.full_text);
}

static bool ends_with_any_codepoint(const std::string & text, const std::string & set) {
    if (text.empty()) return false;
    size_t i = text.size() - 1;                                           // start of the last UTF-8 code point
    while (i > 0 && ((unsigned char) text[i] & 0xC0) == 0x80) --i;
    const std::string last = text.substr(i);
    for (size_t k = 0; k < set.size();) {
        size_t n = 1;
        const unsigned char c = (unsigned char) set[k];
        if (c >= 0xF0) n = 4; else if (c >= 0xE0) n = 3; else if (c >= 0xC0) n = 2;
        if (set.compare(k, n, last) == 0) return true;
        k += n;
    }
    return false;
}

std::vector<CaptureStreamToText::Update> CaptureStreamToText::stream(const std::vector<float> & pcm16k, int max_calls) {
    // addon/capture_stream_to_text.gd:65-120 — every `transcribe_interval` seconds the WHOLE accumulated buffer is
    // transcribed again with audio_ctx = total_s * 50 + 128 (:84)
    std::vector<Update> out;
    const int sr = WHISPER_SAMPLE_RATE;
    const size_t step = (size_t) std::lround(transcribe_interval * sr);
    size_t start = 0, pos = 0; int calls = 0; int last_tokens = -1;
    while (pos < pcm16k.size()) {
        pos = std::min(pos + step, pcm16k.size());
        const std::vector<float> acc(pcm16k.begin() + start, pcm16k.begin() + pos);
        const double total_s = (double) acc.size() / sr;
        if (total_s < 1.0) continue;
        const bool no_activity = voice_activity_detection(acc);
        const int audio_ctx = std::min((int) (total_s * 50 + 128), 1500);
        const Transcription t = transcribe(acc, "", audio_ctx);
        ++calls;
        if (!t.ok) continue;
        const std::string text = remove_special_characters(t.full_text);
        const int n_tok = (int) t.tokens.size();
        bool finish = false;
        const double total_ms = total_s * 1000;
        if (total_ms > minimum_sentence_ms) {
            if ((ends_with_any_codepoint(text, punctuation_characters) || no_activity) && std::abs(n_tok - last_tokens) <= 1) finish = true;
            if (total_ms > maximum_sentence_ms) finish = true;
        }
        last_tokens = n_tok;
        out.push_back(Update{finish, text, acc.size(), audio_ctx, t.tokens});
        if (finish) {
            start = pos > (size_t) (0.2 * sr) ? pos - (size_t) (0.2 * sr) : 0;    // keep only the last 0.2 s (:111)
            last_tokens = -1;
        }
        if (max_calls >= 0 && calls >= max_calls) break;
    }
    return out;
}

static bool contains_any_codepoint(const std::string & text, const std::string & set) {     // _has_terminating_characters (:124-128)
    for (size_t k = 0; k < set.size();) {
        size_t n = 1;
        const unsigned char c = (unsigned char) set[k];
        if (c >= 0xF0) n = 4; else if (c >= 0xE0) n = 3; else if (c >= 0xC0) n = 2;
        if (text.find(set.substr(k, n)) != std::string::npos) return true;
        k += n;
    }
    return false;
}

std::vector<CaptureStreamToText::Update> CaptureStreamToText::stream_capture(const std::vector<float> & interleaved_xy, int mix_rate,
                                                                             InterpolatorType interpolator_type, int max_calls, bool use_session) {
    std::vector<Update> out;
    if (!context_instance || mix_rate <= 0) return out;
    const int sr = WHISPER_SAMPLE_RATE;
    const size_t n_frames = interleaved_xy.size() / 2;
    const size_t step = std::max<size_t>((size_t) std::lround(transcribe_interval * mix_rate), 1);
    wmi_capture * cap = use_session ? wmi_capture_init(context_instance, mix_rate, (int) interpolator_type, (int) (maximum_sentence_ms / 1000.0 * mix_rate)) : nullptr;
    if (use_session && !cap) { fprintf(stderr, "ERROR: wmi_capture_init failed\n"); return out; }
    if (cap && draft_reuse) (void) wmi_capture_set_draft(cap, 1);   // every step offers the previous step's tokens as a draft
    size_t start = 0, pos = 0; int calls = 0, last_token_count = 0;
    std::vector<float> resampled;
    while (pos < n_frames) {
        const size_t take = std::min(step, n_frames - pos);
        int size = 0;
        if (cap) {
            if (wmi_capture_push(cap, interleaved_xy.data() + 2 * pos, (int) take, 0) < 0) break;      // _accumulated_frames.append_array(...) (:73)
            pos += take;
            size = wmi_capture_resample(cap, nullptr);
        } else {
            pos += take;
            resampled = resample(std::vector<float>(interleaved_xy.begin() + 2 * start, interleaved_xy.begin() + 2 * pos), interpolator_type, mix_rate);
            size = (int) resampled.size();
        }
        if (size <= 0) continue;
        const bool no_activity = cap ? wmi_capture_vad(cap, settings.vad_treshold, settings.freq_treshold, nullptr) > 0 : voice_activity_detection(resampled);
        const double total_time = (double) size / sr;
        const int audio_ctx = std::min((int) (total_time * 1500 / 30 + 128), 1500);                    // :84
        Transcription t;
        if (cap) {
            const std::string prompt;
            last_return = wmi_capture_full(cap, make_params(prompt, audio_ctx));
            if (last_return == 0) t = collect();
            else fprintf(stderr, "ERROR: Failed to process audio, returned %d\n", last_return);
        } else t = transcribe(resampled, "", audio_ctx);
        ++calls;
        if (!t.ok) break;                                                                              // "No tokens generated" (:88-90)
        bool finish = total_time * 1000 > maximum_sentence_ms;
        std::string text;
        for (const Token & tok : t.tokens) text += tok.text;
        text = remove_special_characters(text);
        if (contains_any_codepoint(text, punctuation_characters) || no_activity) finish = true;
        if (total_time * 1000 < minimum_sentence_ms || std::abs((int) t.tokens.size() - last_token_count) > hallucinating_count) finish = false;
        out.push_back(Update{finish, t.full_text, (size_t) size, audio_ctx, t.tokens, no_activity});
        if (!no_activity) {                                                                            // `if no_activity: continue` (:108-109)
            if (finish) {                                                                              // :110-113
                const size_t keep = (size_t) (0.2 * mix_rate);
                if (cap) wmi_capture_keep_last(cap, (int) keep);
                else start = std::max(start, pos > keep ? pos - keep : 0);
            }
            last_token_count = (int) t.tokens.size();
        }
        if (max_calls >= 0 && calls >= max_calls) break;
    }
    wmi_capture_free(cap);
    return out;
}

} // namespace godot_whisper

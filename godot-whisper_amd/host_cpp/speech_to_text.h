// Host side of the boundary in the reference's own language: the SpeechToText node (src/speech_to_text.h:20-172,
// src/speech_to_text.cpp:106-450) and the two GDScript call patterns (addon/audio_stream_to_text.gd:31-88,
// addon/capture_stream_to_text.gd:65-120) restated over the C ABI of include/whisper_mi355.h, with std:: types where
// the reference uses Godot's (PackedFloat32Array -> std::vector<float>, String -> std::string, Array of Dictionary ->
// Transcription).  Godot, godot-cpp and SCons are not in this image, so this is what the GDExtension would compile
// to once its Variant plumbing is removed: same methods, same argument meaning, same error behaviour (empty result +
// a message on stderr where the reference ERR_PRINTs).  godot-whisper_amd/host.py is the same mirror in Python and is
// what the parity tests drive; tests/test_host_cpp.py checks that both give identical results.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/whisper_mi355.h"
#include "../../include/wmi_device.h"

namespace godot_whisper {

// ProjectSettings "audio/input/transcribe/*" (src/register_types.cpp:64-69; spelling is the reference's)
struct TranscribeSettings {
    float entropy_treshold = 2.8f;
    float freq_treshold = 200.0f;
    int   max_tokens = 16;
    float vad_treshold = 2.0f;
    bool  use_gpu = true;
    bool  speed_up_2x = false;
};

// one element of the Array transcribe() returns (src/speech_to_text.cpp:431-443)
struct Token {
    std::string text;
    int32_t id = 0, tid = 0;
    float   p = 0, plog = 0, pt = 0, ptsum = 0, vlen = 0;
    int64_t t0 = 0, t1 = 0;
    float   no_speech_prob = -1.0f;   // not in the reference: of the token's segment (wmi_full_get_segment_no_speech_prob; -1 with set_no_speech(0))
    int64_t t_dtw = -1;               // not in the reference: the token's DTW time in 10 ms units (wmi_full_get_token_dtw; -1 without set_token_dtw, or for a token that is no text)
};
// not in the reference node: one segment's speaker from the two channels of a stereo asset (include/wmi_device.h wmi_speaker; whisper.cpp's
// --diarize, examples/main/main.cpp:237-268).  speaker: 0 left, 1 right, -1 the reference's "?"
struct SegmentSpeaker {
    int64_t t0 = 0, t1 = 0;
    std::string text;
    int speaker = -1;
    double e0 = 0.0, e1 = 0.0;
};
// the Array itself: element 0 is the full text, the rest are the token dictionaries (:447)
struct Transcription {
    bool ok = false;              // false <=> the reference returns an empty Array
    std::string full_text;
    std::vector<Token> tokens;
};

class SpeechToText {
public:
    // src/speech_to_text.h:22-128: Auto = 0, then whisper.cpp's language table in its own order
    enum Language { Auto = 0, English = 1 };

    explicit SpeechToText(const TranscribeSettings & settings = TranscribeSettings());
    ~SpeechToText();
    SpeechToText(const SpeechToText &) = delete;
    SpeechToText & operator=(const SpeechToText &) = delete;

    void set_language(int p_language) { language = p_language; }
    int  get_language() const { return language; }
    // set_language_model(Ref<WhisperResource>) + _load_model(): the resource's bytes (src/resource_whisper.h)
    void set_language_model(const uint8_t * data, size_t size);
    // not in the reference: the context's no-speech mode (include/wmi_device.h wmi_set_no_speech: 0 off, 1 report, 2 drop, 3 gate), kept
    // across set_language_model.  Returns the previous mode.
    int  set_no_speech(int mode);
    int  get_no_speech() const { return no_speech; }
    // not in the reference: DTW token times (include/wmi_device.h wmi_set_token_dtw) over the default alignment heads, or over the
    // given {layer, head, layer, head, ..} list; kept across set_language_model.  Returns what wmi_set_token_dtw does (0 without a context).
    int  set_token_dtw(bool on, const std::vector<int32_t> & layer_head = {});
    bool get_token_dtw() const { return token_dtw; }
    // not in the reference: speaker labels for the stereo assets of transcribe_wav (include/wmi_device.h wmi_set_speaker: 0 off, 1 per
    // segment, 2 per token too); kept across set_language_model.  Returns the previous mode.  speakers(): a record per segment of the last
    // result, empty where it carries none (mode 0, a mono asset, another call); diarized_text(): main.cpp's "(speaker 0) text" lines joined.
    int  set_speaker_labels(int mode, double ratio = 1.1);
    std::vector<SegmentSpeaker> speakers() const;
    // not in the reference: AudioStreamWAV.FORMAT_IMA_ADPCM (format 2) for transcribe_wav / transcribe_wav_channels, decoded on the device
    // (include/wmi_device.h wmi_set_wav_adpcm); off: format 2 is refused (last_return -111).  Kept across set_language_model.  Returns the
    // previous setting.
    bool set_wav_adpcm(bool on);
    std::string diarized_text() const;
    // not in the reference: a grammar for every later transcription (whisper_full_params.grammar_rules: rule 0 is the start rule, each rule
    // without its closing END element; an empty list: none), and where it is evaluated (include/wmi_device.h wmi_set_grammar_device:
    // true — reject masks and penalised sampling on the device); both kept across set_language_model.  set_grammar_device returns the
    // previous mode (0 without a context).
    void set_grammar(const std::vector<std::vector<whisper_grammar_element>> & rules, float penalty = 100.0f);
    int  set_grammar_device(bool on);
    bool get_grammar_device() const { return grammar_device; }
    // not in the reference: a draft for the NEXT transcription call (include/wmi_device.h wmi_set_draft): token ids the call verifies in one
    // decoder pass and decodes on from where they stop being the greedy decode — the result is the undrafted call's.  An empty list clears
    // it.  Returns what wmi_set_draft does (-1 without a context); draft_status(): what became of the last call's draft.
    int  set_draft(const std::vector<int32_t> & tokens);
    struct wmi_draft_status draft_status() const;

    // src/speech_to_text.h:151-156, :162 — resample(PackedVector2Array buffer, InterpolatorType): stereo capture frames at the mix rate
    // -> mono 16 kHz.  The reference folds on the CPU and calls libsamplerate's src_simple; here both steps run on the device
    // (wmi_downmix_stereo, wmi_resample: the same arithmetic frame for frame).  `mix_rate` stands in for AudioServer::get_mix_rate().
    enum InterpolatorType { SRC_SINC_BEST_QUALITY = 0, SRC_SINC_MEDIUM_QUALITY = 1, SRC_SINC_FASTEST = 2, SRC_ZERO_ORDER_HOLD = 3, SRC_LINEAR = 4 };
    std::vector<float> resample(const std::vector<float> & interleaved_xy, InterpolatorType interpolator_type, int mix_rate);
    std::string last_resample_error;      // what the reference ERR_PRINTs ("size differ exp: ... res: ...")

    bool voice_activity_detection(const std::vector<float> & buffer) const;
    Transcription transcribe(const std::vector<float> & buffer, const std::string & initial_prompt, int audio_ctx);
    // not in the reference: an AudioStreamWAV as it is (include/wmi_device.h: wmi_full_wav) — `data` = audio_stream.data, format =
    // audio_stream.format (0 = FORMAT_8_BITS, 1 = FORMAT_16_BITS), stereo, mix_rate.  Every sample is decoded, a stereo asset folded
    // and another rate resampled to 16 kHz on the device; the node's own GDScript loop (addon/audio_stream_to_text.gd:40-46) does none of it.
    Transcription transcribe_wav(const std::vector<uint8_t> & data, int format, bool stereo, int mix_rate, const std::string & initial_prompt = "",
                                 int audio_ctx = 0, InterpolatorType interpolator_type = SRC_SINC_FASTEST);
    // not in the reference: a STEREO AudioStreamWAV with one voice per channel (include/wmi_device.h: wmi_full_wav_channels) — the two
    // channels transcribed apart in one lock-step call.  Returns the dialogue: a record per segment in the merged view's order (by start
    // time, the left channel first on a tie), the channel being the speaker; last_channels has the two per-channel results.
    // dialogue_text(): "(speaker 0) text" per segment joined, in diarized_text()'s format.
    struct DialogueSegment { int channel = 0, index = 0; int64_t t0 = 0, t1 = 0; std::string text; };
    std::vector<DialogueSegment> transcribe_wav_channels(const std::vector<uint8_t> & data, int format, int mix_rate,
                                                         const std::string & initial_prompt = "", int audio_ctx = 0,
                                                         InterpolatorType interpolator_type = SRC_SINC_FASTEST);
    std::vector<Transcription> last_channels;
    static std::string dialogue_text(const std::vector<DialogueSegment> & dialogue);
    // not in the reference: several buffers in lock-step on one GPU (include/wmi_device.h: wmi_full_batch); element c is
    // what transcribe(buffers[c], initial_prompt, audio_ctx) returns on a fresh context
    std::vector<Transcription> transcribe_batch(const std::vector<std::vector<float>> & buffers, const std::string & initial_prompt,
                                                int audio_ctx);
    // not in the reference: a whole recording cut at its silences on the device, the pieces decoded in lock-step (include/wmi_device.h:
    // wmi_full_long); one merged result, times relative to the recording.  long_params = nullptr: the library's defaults.
    // last_pieces has the plan of the call.
    Transcription transcribe_long(const std::vector<float> & buffer, const std::string & initial_prompt = "",
                                  const wmi_long_params * long_params = nullptr);
    std::vector<wmi_long_piece> last_pieces;

    // not in the reference: candidate texts scored against the audio in one teacher-forced pass (include/wmi_device.h: wmi_score_pcm) — per
    // text the log-probability of every token and of the whole text, and the posterior over the texts.  Every text is tokenized with a
    // leading space (examples/command/command.cpp:276).  An empty result: an error, its code in last_return.
    struct TextScore { std::string text; std::vector<int32_t> tokens; std::vector<float> token_logprobs; double sum_logprob = 0.0; float avg_logprob = 0.0f, posterior = 0.0f; };
    std::vector<TextScore> score_texts(const std::vector<float> & buffer, const std::vector<std::string> & texts, const std::string & prompt = "",
                                       bool length_norm = false, int audio_ctx = 0);

    whisper_context * context() { return context_instance; }
    int last_return = 0;          // whisper_full's code of the last transcribe()
    std::vector<int> last_langs;  // transcribe_batch: per chunk the language id whisper_full would report (the detected one with Language "auto")

protected:
    whisper_full_params make_params(const std::string & initial_prompt, int audio_ctx) const;
    Transcription collect() const;
    const char * language_to_code(int language) const;

    TranscribeSettings settings;
    int language = English;
    int no_speech = 0;
    bool token_dtw = false; std::vector<int32_t> token_dtw_pairs;
    int speaker_mode = 0; double speaker_ratio = 1.1;
    bool wav_adpcm = false;
    bool grammar_device = false; float grammar_penalty = 100.0f;
    std::vector<std::vector<whisper_grammar_element>> grammar_rules;     // each closed by an END element
    std::vector<const whisper_grammar_element *> grammar_ptrs;
    whisper_context * context_instance = nullptr;
};

// addon/audio_stream_to_text.gd
class AudioStreamToText : public SpeechToText {
public:
    using SpeechToText::SpeechToText;
    std::string get_text(const std::vector<float> & pcm16k, const std::string & initial_prompt = "");
};
std::string remove_special_characters(std::string message);          // addon/audio_stream_to_text.gd:64-88

// addon/capture_stream_to_text.gd: the streaming loop — stream() over a pre-recorded 16 kHz buffer, stream_capture() the node's own loop
// over stereo capture frames at the mix rate
class CaptureStreamToText : public SpeechToText {
public:
    using SpeechToText::SpeechToText;
    float transcribe_interval = 0.3f;
    bool  draft_reuse = false;       // not in the reference: stream_capture on a session offers every step the previous step's tokens as a draft (wmi_capture_set_draft)
    int   minimum_sentence_ms = 3000, maximum_sentence_ms = 15000;
    int   hallucinating_count = 1;
    std::string punctuation_characters = ".!?;\xe3\x80\x82\xef\xbc\x9b\xef\xbc\x9f\xef\xbc\x81";
    struct Update { bool finish; std::string text; size_t n_samples; int audio_ctx; std::vector<Token> tokens; bool no_activity = false; };
    std::vector<Update> stream(const std::vector<float> & pcm16k, int max_calls = -1);
    // transcribe_thread (addon/capture_stream_to_text.gd:69-120) over pre-recorded capture frames: every pass appends transcribe_interval
    // seconds of frames, resamples the whole accumulation, runs the VAD and transcribes with audio_ctx = total_time * 1500 / 30 + 128; a
    // pass with no_activity neither ends the sentence nor updates the token count, a finished sentence keeps the last 0.2 * mix_rate frames.
    // use_session: on a capture session (include/wmi_device.h wmi_capture_*: frames and PCM stay on the device), else the same loop over
    // resample() / voice_activity_detection() / transcribe() on host vectors — the same updates either way.
    std::vector<Update> stream_capture(const std::vector<float> & interleaved_xy, int mix_rate, InterpolatorType interpolator_type = SRC_SINC_FASTEST,
                                       int max_calls = -1, bool use_session = true);
};

// src/speech_to_text.cpp:53-104
void high_pass_filter(std::vector<float> & data, float cutoff, float sample_rate);
bool vad_simple(std::vector<float> & pcmf32, int sample_rate, int last_ms, float vad_thold, float freq_thold);

} // namespace godot_whisper

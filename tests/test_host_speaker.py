"""-m gpu: the host mirrors of the speaker labels — host.py's speaker_labels dictionaries, the "(speaker N) " prefix of get_text_wav and the
batch's dictionaries against the judge (tests/speaker_ref.py), and godot_whisper::SpeechToText::set_speaker_labels through
wmi_host_demo --wav-bytes .. --diarize against the Python mirror."""
import numpy as np
import pytest

import speaker_ref as sr
import wav_ref as wr
from godot_whisper_amd import host, synth
from test_host_cpp import run_demo

pytestmark = pytest.mark.gpu

SR = 16000


@pytest.fixture(scope="module")
def model():
    return synth.make_model("micro.en", seed=8)


def _clip(fmt, rate, seconds, seed, gains):
    n = int(seconds * rate)
    chans = [gains[c] * synth.make_pcm(n / SR, seed=seed + (c if gains[0] != gains[1] else 0))[:n] for c in range(2)]   # equal gains: one signal twice
    return wr.pack(np.stack(chans, axis=1).reshape(-1).astype(np.float32), fmt)


def _want(s, x, rate, ratio=sr.RATIO):
    j = sr.speaker(x, rate, s["t0"], s["t1"], ratio)
    return {"t0": s["t0"], "t1": s["t1"], "text": s["text"], "speaker": j["speaker"] if j["speaker"] >= 0 else None,
            "channel_energy": (j["e0"], j["e1"]), "samples": (j["is0"], j["is1"])}


def test_dictionaries_and_prefix_equal_the_judge(product_lib, model):
    plain = host.AudioStreamToText(product_lib); plain.set_language_model(model)
    node = host.AudioStreamToText(product_lib, speaker_labels="tokens"); node.set_language_model(model)
    try:
        for gains, rate, fmt in (((1.0, 0.2), 44100, wr.S16), ((0.2, 1.0), 22050, wr.S8), ((0.5, 0.5), 16000, wr.S16)):
            data = _clip(fmt, rate, 3.0, 5, gains)
            x = sr.channels(data, fmt)
            got = node.transcribe_wav(data, fmt, True, rate)
            assert node.last_ret == 0 and len(got) > 1 and node.last_speakers
            assert node.last_speakers == [_want(s, x, rate) for s in node.last_speakers]
            # the transcription itself is the plain node's, the token dictionaries gain "speaker" and nothing else
            base = plain.transcribe_wav(data, fmt, True, rate)
            assert plain.last_speakers == [] and got[0] == base[0] and len(got) == len(base)
            for a, b in zip(got[1:], base[1:]):
                assert {k: v for k, v in a.items() if k != "speaker"} == b and "speaker" not in b
                j = sr.speaker(x, rate, a["t0"], a["t1"])
                assert a["speaker"] == (j["speaker"] if j["speaker"] >= 0 else None)
            # main.cpp's prefix in front of every segment's text
            text = node.get_text_wav(data, fmt, True, rate, speaker_prefix=True)
            want = "".join("(speaker %s) " % ("?" if s["speaker"] is None else s["speaker"]) +
                           host.remove_special_characters(s["text"].decode("utf-8", errors="replace")) for s in node.last_speakers)
            assert text == want and text.startswith("(speaker ")
            assert plain.get_text_wav(data, fmt, True, rate, speaker_prefix=True) == plain.get_text_wav(data, fmt, True, rate)
        # equal channels: the reference's "?"
        assert all(s["speaker"] is None for s in node.last_speakers) and "(speaker ?) " in text
        # a batch: per clip, [] for the mono one
        clips = [(_clip(wr.S16, 48000, 2.5, 7, (1.0, 0.3)), wr.S16, 1, 48000), (wr.pack(synth.make_pcm(2.0, seed=9), wr.S16), wr.S16, 0, 16000)]
        node.transcribe_wav_batch(clips)
        assert node.last_ret == 0 and len(node.last_batch_speakers) == 2 and node.last_batch_speakers[1] == []
        x0 = sr.channels(clips[0][0], wr.S16)
        assert node.last_batch_speakers[0] and node.last_batch_speakers[0] == [_want(s, x0, 48000) for s in node.last_batch_speakers[0]]
        # turning the labels off again
        assert node.set_speaker_labels(False) == 2
        node.transcribe_wav(clips[0][0], wr.S16, True, 48000)
        assert node.last_speakers == []
    finally:
        node.close(); plain.close()


def test_cpp_diarize_equals_the_python_mirror(product_lib, model, tmp_path):
    data = _clip(wr.S16, 44100, 3.0, 5, (1.0, 0.2))
    node = host.AudioStreamToText(product_lib, speaker_labels=True); node.set_language_model(model)
    try:
        node.transcribe_wav(data, wr.S16, True, 44100)
        want = node.last_speakers
        assert want
        text = node.get_text_wav(data, wr.S16, True, 44100, speaker_prefix=True)
    finally:
        node.close()
    out = run_demo(tmp_path, model, data, "--wav-bytes", wr.S16, "1,44100,2", 0, "--diarize")
    assert out["ret"] == 0
    assert [(s["t0"], s["t1"], s["speaker"] if s["speaker"] >= 0 else None, (s["e0"], s["e1"])) for s in out["speakers"]] == \
           [(s["t0"], s["t1"], s["speaker"], s["channel_energy"]) for s in want]
    assert out["diarized"].startswith("(speaker ")
    plain = run_demo(tmp_path, model, data, "--wav-bytes", wr.S16, "1,44100,2", 0)
    assert "speakers" not in plain and plain["transcription"] == out["transcription"]

"""-m gpu: the host mirrors of the two-channel WAV call — host.py's transcribe_wav_channels / get_text_wav(channels=True) against the C
calls they wrap (wmi_full_wav_channels, wmi_channels_select, wmi_channels_get_segment), and
godot_whisper::SpeechToText::transcribe_wav_channels through wmi_host_demo --wav-bytes ... --channels against the Python mirror, in the
manner of tests/test_host_wav.py."""
import ctypes as C

import numpy as np
import pytest

import channels_ref as cr
import golden_util as gu
import wav_ref as wr
from godot_whisper_amd import abi, host, synth
from test_host_cpp import _as_rows, run_demo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    return synth.make_model("micro.en", seed=8)


@pytest.fixture
def node(product_lib, model):
    n = host.AudioStreamToText(product_lib); n.set_language_model(model)
    yield n
    n.close()


def _clip(fmt, rate, seconds, seed):
    n = int(seconds * rate)
    chans = [synth.make_pcm(n / 16000, seed=seed + c)[:n] for c in range(2)]
    return wr.pack(np.stack(chans, axis=1).reshape(-1), fmt)


def _c_wav(data, fmt, stereo, rate):
    buf = C.create_string_buffer(data, max(len(data), 1))
    w = abi.wmi_wav(C.cast(buf, C.c_void_p), len(data), fmt, stereo, rate, 0)
    w._keep = buf
    return w


def test_python_mirror_equals_the_c_calls(product_lib, node):
    lib, ctx = product_lib, node.ctx
    a = _clip(wr.S16, 44100, 4.0, seed=5)
    dialogue = node.transcribe_wav_channels(a, abi.WMI_WAV_S16, 44100, initial_prompt=" Hello", audio_ctx=328, interpolator_type=1)
    assert node.last_ret == 0 and len(dialogue) >= 2 and len(node.last_channels) == 2
    channels = list(node.last_channels)
    # = wmi_full_wav_channels with the node's parameters + the accessors
    assert lib.wmi_full_wav_channels(ctx, node.full_params(" Hello", 328), C.byref(_c_wav(a, wr.S16, 1, 44100)), 1) == 0
    assert node.segments() == [(d["t0"], d["t1"], d["text"]) for d in dialogue]        # the call leaves the dialogue view selected
    assert node.collect_batch(2) == channels
    # each channel is transcribe_batch on the judge's samples, the dialogue the judge's merge of the two
    pcms = cr.convert_channels(a, wr.S16, 44100, 1)
    assert channels == node.transcribe_batch(list(pcms), " Hello", 328)
    segs = []
    for c in range(2):
        assert lib.wmi_batch_select(ctx, c) >= 0
        segs.append(node.segments())
    order = cr.merge([s[0] for s in segs[0]], [s[0] for s in segs[1]])
    assert [(d["channel"], d["index"]) for d in dialogue] == order
    assert [(d["t0"], d["t1"], d["text"]) for d in dialogue] == [segs[c][i] for c, i in order]
    assert {d["channel"] for d in dialogue} == {0, 1}
    # get_text_wav(channels=True): the dialogue joined with the speaker prefix of speaker_prefix=True
    text = node.get_text_wav(a, wr.S16, 1, 44100, interpolator_type=1, channels=True)
    plain = node.transcribe_wav_channels(a, wr.S16, 44100, interpolator_type=1)
    assert text == "".join("(speaker %d) " % d["channel"] + host.remove_special_characters(d["text"].decode("utf-8", errors="replace")) for d in plain)
    assert text.startswith("(speaker ") and text.count("(speaker ") == len(plain)
    # a refused clip leaves the code and an empty answer
    assert node.transcribe_wav_channels(a, 2, 44100) == [] and node.last_ret == -111 and node.last_channels == []
    assert node.get_text_wav(a, wr.S16, 1, 0, channels=True) == "" and node.last_ret == -101
    assert lib.wmi_full_wav_channels(ctx, node.full_params("", 0), C.byref(_c_wav(a, wr.S16, 0, 44100)), 2) == -112


@pytest.mark.parametrize("fmt,rate,interp", [(wr.S16, 44100, 2), (wr.S8, 16000, 2)], ids=["s16x2-44k1", "s8x2-16k"])
def test_cpp_host_equals_python_mirror(product_lib, model, node, tmp_path, fmt, rate, interp):
    data = _clip(fmt, rate, 5.0, seed=30)
    want = node.transcribe_wav_channels(data, fmt, rate, "", 0, interp)
    assert node.last_ret == 0 and len(want) >= 2
    got = run_demo(tmp_path, model, data, "--wav-bytes", fmt, f"1,{rate},{interp}", 0, "--channels")
    assert got["ret"] == 0
    assert [(d["channel"], d["index"], d["t0"], d["t1"], d["text"].encode("latin-1")) for d in got["dialogue"]] == \
           [(d["channel"], d["index"], d["t0"], d["t1"], bytes(d["text"])) for d in want]
    assert got["text"].encode("latin-1") == b"".join(b"(speaker %d) " % d["channel"] + bytes(d["text"]) for d in want)
    assert len(got["channels"]) == 2
    for tr, w_list in zip(got["channels"], node.last_channels):
        assert tr["ok"] and tr["full_text"].encode("latin-1") == bytes(w_list[0])
        w = gu.tokens_array(w_list); g = _as_rows(tr)
        assert g.shape == w.shape and np.array_equal(g[:, [0, 1, 6, 7]], w[:, [0, 1, 6, 7]])
        assert np.abs(g - w).max() <= 1e-6                  # same library, same kernels: float text round trip only
    # a refused format comes back as the call's code
    bad = run_demo(tmp_path, model, data, "--wav-bytes", 2, f"1,{rate},{interp}", 0, "--channels")
    assert bad["ret"] == -111 and bad["dialogue"] == [] and bad["channels"] == []

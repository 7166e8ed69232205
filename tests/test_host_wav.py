"""-m gpu: the host mirrors of the AudioStreamWAV calls — host.py's transcribe_wav / transcribe_wav_batch / get_text_wav against the C
calls they wrap (wmi_full_wav, wmi_full_batch_wav, wmi_full_long_wav), and godot_whisper::SpeechToText::transcribe_wav through
wmi_host_demo --wav-bytes against the Python mirror, as tests/test_host_cpp.py does for the other calls."""
import ctypes as C

import numpy as np
import pytest

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


def _clip(fmt, stereo, rate, seconds, seed):
    n = int(seconds * rate)
    chans = [synth.make_pcm(n / 16000, seed=seed + c)[:n] for c in range(2 if stereo else 1)]
    return wr.pack(np.stack(chans, axis=1).reshape(-1), fmt)


def _c_wav(data, fmt, stereo, rate):
    buf = C.create_string_buffer(data, max(len(data), 1))
    w = abi.wmi_wav(C.cast(buf, C.c_void_p), len(data), fmt, stereo, rate, 0)
    w._keep = buf
    return w


def test_python_mirrors_equal_the_c_calls(product_lib, node):
    lib, ctx = product_lib, node.ctx
    a = _clip(wr.S16, 1, 44100, 3.0, seed=5); b = _clip(wr.S8, 0, 22050, 2.0, seed=6)
    # transcribe_wav = wmi_full_wav with the node's parameters + collect()
    got = node.transcribe_wav(a, abi.WMI_WAV_S16, True, 44100, initial_prompt=" Hello", audio_ctx=328, interpolator_type=1)
    assert node.last_ret == 0 and len(got) > 1
    assert lib.wmi_full_wav(ctx, node.full_params(" Hello", 328), C.byref(_c_wav(a, wr.S16, 1, 44100)), 1) == 0
    assert node.collect() == got
    # and it is transcribe() on the judge's samples
    assert got == node.transcribe(wr.convert(a, wr.S16, 1, 44100, 1), " Hello", 328)
    # transcribe_wav_batch = wmi_full_batch_wav + the batch accessors
    clips = [(a, wr.S16, 1, 44100), (b, wr.S8, 0, 22050)]
    got = node.transcribe_wav_batch(clips, interpolator_type=4)
    assert node.last_ret == 0 and len(got) == 2
    keep = [_c_wav(*c) for c in clips]
    wavs = (abi.wmi_wav * 2)(*keep)
    assert lib.wmi_full_batch_wav(ctx, node.full_params("", 0), wavs, 2, 4) == 0
    assert node.collect_batch(2) == got
    assert got == node.transcribe_batch([wr.convert(d, f, st, r, 4) for d, f, st, r in clips])
    # get_text_wav: the one-shot node's call, both forms
    pcm = wr.convert(a, wr.S16, 1, 44100, 2)
    assert node.get_text_wav(a, wr.S16, 1, 44100) == node.get_text(pcm) != ""
    assert node.get_text_wav(a, wr.S16, 1, 44100, long_form=True) == node.get_text(pcm, long_form=True)
    # a refused clip leaves the code and an empty answer
    assert node.transcribe_wav(a, 2, False, 44100) == [] and node.last_ret == -111
    assert node.get_text_wav(a, wr.S16, 1, 0) == "" and node.last_ret == -101
    assert node.transcribe_wav_batch([(a, wr.S16, 1, 44100), (b, 3, 0, 22050)]) == [] and node.last_ret == -111


@pytest.mark.parametrize("fmt,stereo,rate,interp", [(wr.S16, 0, 16000, 2), (wr.S16, 1, 44100, 2), (wr.S8, 1, 48000, 3)], ids=["s16-16k", "s16x2-44k1", "s8x2-48k"])
def test_cpp_host_equals_python_mirror(product_lib, model, node, tmp_path, fmt, stereo, rate, interp):
    data = _clip(fmt, stereo, rate, 5.0, seed=30)
    want = node.transcribe_wav(data, fmt, stereo, rate, "", 0, interp)
    assert node.last_ret == 0 and len(want) > 1
    got = run_demo(tmp_path, model, data, "--wav-bytes", fmt, f"{stereo},{rate},{interp}", 0)
    tr = got["transcription"]
    assert got["ret"] == 0 and tr["ok"] and tr["full_text"].encode("latin-1") == bytes(want[0])
    w = gu.tokens_array(want); g = _as_rows(tr)
    assert g.shape == w.shape and np.array_equal(g[:, [0, 1, 6, 7]], w[:, [0, 1, 6, 7]])
    assert np.abs(g - w).max() <= 1e-6                      # same library, same kernels: float text round trip only
    # a refused format comes back as the call's code
    bad = run_demo(tmp_path, model, data, "--wav-bytes", 2, f"{stereo},{rate},{interp}", 0)
    assert bad["ret"] == -111 and not bad["transcription"]["ok"]

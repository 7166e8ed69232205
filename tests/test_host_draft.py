"""host.SpeechToText.transcribe(draft=...) arms what the C call arms and leaves the status the C call reports; host.CaptureStreamToText's
draft_reuse turns the session's mode on."""
import ctypes as C

import numpy as np
import pytest

from godot_whisper_amd import abi, host, synth


def test_transcribe_without_a_context_is_empty():
    node = host.SpeechToText(lib=None)
    assert node.transcribe(np.zeros(16000, np.float32), draft=[1, 2, 3]) == [] and node.last_draft_status == {}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["micro.en", "micro"])
def test_draft_equals_the_c_call(product_lib, shape):
    lib = product_lib
    model = synth.make_model(shape, seed=8); pcm = synth.make_pcm(4.0, seed=8)
    node = host.SpeechToText(lib); node.set_language_model(model)
    try:
        p = node.full_params("", 160); p.temperature_inc = 0.0; p.max_tokens = 10
        plain = node.transcribe(pcm, params=p)
        assert node.last_ret == 0 and node.last_draft_status["reason"] == abi.DRAFT_NONE
        ids = [t["id"] for t in plain[1:]]
        got = node.transcribe(pcm, params=p, draft=ids)
        st = node.last_draft_status
        assert node.last_ret == 0 and st["reason"] == abi.DRAFT_USED and st["n_offered"] == len(ids) and st["n_rows"] == len(ids)
        # the C calls on the same tokens
        arr = np.asarray(ids, np.int32)
        assert lib.wmi_set_draft(node.ctx, arr.ctypes.data_as(C.c_void_p), arr.size) == 0
        assert lib.whisper_full(node.ctx, p, pcm.ctypes.data_as(C.POINTER(C.c_float)), pcm.size) == 0
        c = abi.wmi_draft_status()
        assert lib.wmi_draft_status(node.ctx, C.byref(c)) == 0
        assert {k: getattr(c, k) for k, _ in c._fields_} == st
        assert [t["id"] for t in node.collect()[1:]] == [t["id"] for t in got[1:]]
        with pytest.raises(ValueError):
            node.transcribe(pcm, params=p, draft=[lib.whisper_n_vocab(node.ctx)])
    finally:
        node.close()

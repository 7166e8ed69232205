"""host.SpeechToText.score returns what the C call returns for the same tokens, and the C++ mirror (host_cpp: SpeechToText::score_texts,
through the demo of tests/test_host_cpp.py) returns the same again."""
import ctypes as C
import math

import numpy as np
import pytest

import score_f64 as sf
from godot_whisper_amd import abi, host, synth
from test_host_cpp import run_demo

TEXTS = ["turn left", "turn right", "stop", "go forward now"]


def test_score_without_a_context_is_empty():
    node = host.SpeechToText(lib=None)
    assert node.score(np.zeros(16000, np.float32), TEXTS) == [] and node.last_scores == []


@pytest.mark.gpu
@pytest.mark.parametrize("shape,language", [("micro.en", "en"), ("micro", "de")])
def test_score_equals_the_c_call_and_the_cpp_mirror(product_lib, tmp_path, shape, language):
    lib = product_lib
    model = synth.make_model(shape, seed=8); pcm = synth.make_pcm(5.0, seed=8)
    node = host.SpeechToText(lib); node.set_language_model(model)
    node.language = language
    try:
        got = node.score(pcm, TEXTS)
        assert node.last_ret == 0 and got is node.last_scores and [g["text"] for g in got] == TEXTS
        toks = [node.tokenize(" " + t) for t in TEXTS]
        assert [g["tokens"] for g in got] == toks and all(len(y) >= 1 for y in toks)
        # the C call on the same tokens
        p = lib.wmi_score_default_params()
        p.lang_id = lib.whisper_lang_id(language.encode()) if lib.whisper_is_multilingual(node.ctx) else 0
        flat = np.asarray([t for y in toks for t in y], np.int32); nt = np.asarray([len(y) for y in toks], np.int32)
        out = (abi.wmi_text_score * len(TEXTS))(); lp = np.zeros(int(nt.sum()) + len(TEXTS), np.float32)
        assert lib.wmi_score_pcm(node.ctx, p, pcm.ctypes.data_as(C.c_void_p), pcm.size, 0, 0, flat.ctypes.data_as(C.c_void_p),
                                 nt.ctypes.data_as(C.c_void_p), len(TEXTS), out, lp.ctypes.data_as(C.c_void_p)) == 0
        for g, o in zip(got, out):
            assert g["token_logprobs"] == lp[o.first:o.first + o.n_scored].tolist()
            assert (g["sum_logprob"], g["avg_logprob"], g["posterior"]) == (o.sum_logprob, o.avg_logprob, o.posterior)
        first = [0] + np.cumsum(nt + 1).tolist()
        recs = [(o.sum_logprob, o.avg_logprob, o.posterior, o.n_scored, o.first) for o in out]
        assert sf.judge_texts(recs, lp, first) and math.isclose(sum(g["posterior"] for g in got), 1.0, abs_tol=1e-5)
        # length_norm and a prompt reach the call
        ln = node.score(pcm, TEXTS, length_norm=True)
        assert [g["token_logprobs"] for g in ln] == [g["token_logprobs"] for g in got] and sf.judge_texts(
            [(g["sum_logprob"], g["avg_logprob"], g["posterior"], len(g["token_logprobs"]), f) for g, f in zip(ln, first)], lp, first, True)
        assert [g["token_logprobs"] for g in node.score(pcm, TEXTS, prompt=" previously said")] != [g["token_logprobs"] for g in got]
    finally:
        node.close()
    # the C++ mirror: the same library and kernels, a float text round trip only
    lang_enum = 1 + lib.whisper_lang_id(language.encode())
    cpp = run_demo(tmp_path, model, pcm.astype("<f4").tobytes(), "score", lang_enum, "|".join(TEXTS), 0)
    assert cpp["ret"] == 0 and len(cpp["scores"]) == len(TEXTS)
    for c, g in zip(cpp["scores"], got):
        assert c["text"] == g["text"] and c["tokens"] == g["tokens"]
        assert np.array_equal(np.asarray(c["token_logprobs"], np.float32), np.asarray(g["token_logprobs"], np.float32))
        assert c["sum_logprob"] == g["sum_logprob"] and np.float32(c["avg_logprob"]) == np.float32(g["avg_logprob"])
        assert np.float32(c["posterior"]) == np.float32(g["posterior"])

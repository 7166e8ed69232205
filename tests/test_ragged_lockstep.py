"""Lock-step chunks with an encoder length each (include/wmi_device.h wmi_full_batch_ctx, wmi_capture_full_batch, wmi_batch_enc_dims):
the part that needs no GPU — the header declares the three functions, the loader binds them, and a host-only context answers the
argument errors before it is asked whether it can compute."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import golden_util as gu
from godot_whisper_amd import runtime

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAMES = ("wmi_full_batch_ctx", "wmi_capture_full_batch", "wmi_batch_enc_dims")


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


def test_header_declares_and_loader_binds_the_three_functions(lib):
    text = (ROOT / "include" / "wmi_device.h").read_text()
    bound = {name: (res, args) for name, res, args in runtime.DEVICE_API}
    for n in NAMES:
        assert re.search(r"WHISPER_API\s+int\s+%s\s*\(" % n, text), n
        assert n in bound and bound[n][0] is C.c_int, n
        assert getattr(lib, n).argtypes == bound[n][1], n
    assert len(bound["wmi_full_batch_ctx"][1]) == 7 and len(bound["wmi_capture_full_batch"][1]) == 4 and len(bound["wmi_batch_enc_dims"][1]) == 4


def test_argument_errors_need_no_device(lib):
    model, _, _ = gu.case_inputs("en30")
    buf = C.create_string_buffer(model, len(model))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(model))
    assert ctx
    try:
        n_ctx = lib.whisper_n_audio_ctx(ctx)
        pcm = np.zeros(16000 * 2, np.float32)
        ptrs = (C.c_void_p * 2)(pcm.ctypes.data, pcm.ctypes.data); lens = (C.c_int * 2)(pcm.size, pcm.size)
        p = lib.whisper_full_default_params(0)

        def call(a, b):
            return lib.wmi_full_batch_ctx(ctx, p, ptrs, lens, (C.c_int * 2)(a, b), 2, 0)
        assert call(0, n_ctx + 1) == -5                     # above the model's n_audio_ctx: whisper_full's code
        assert call(-1, 100) == -1
        assert call(n_ctx + 1, -1) == -1                    # a negative entry is a bad argument whatever else the array holds
        assert call(0, n_ctx) == -2                         # valid lengths: the host-only context's loud failure, as wmi_full_batch
        assert lib.wmi_full_batch_ctx(ctx, p, ptrs, lens, None, 2, 0) == lib.wmi_full_batch(ctx, p, ptrs, lens, 2, 0) == -2
        assert lib.wmi_full_batch_ctx(None, p, ptrs, lens, (C.c_int * 2)(0, 0), 2, 0) == -1
        # no batched encoder pass yet
        rows, period = C.c_int(-7), C.c_int(-7)
        assert lib.wmi_batch_enc_dims(ctx, C.byref(rows), C.byref(period), None) == -1 and rows.value == -7
        assert lib.wmi_batch_enc_dims(None, None, None, None) == -1
        # sessions: nothing to transcribe, a NULL session
        assert lib.wmi_capture_full_batch(None, 0, p, None) == -1
        caps = (C.c_void_p * 2)(None, None)
        assert lib.wmi_capture_full_batch(caps, 0, p, None) == -1
        assert lib.wmi_capture_full_batch(caps, 2, p, None) == -1
        assert lib.wmi_capture_full_batch(caps, -3, p, (C.c_int * 2)(0, 0)) == -1
    finally:
        lib.whisper_free(ctx)

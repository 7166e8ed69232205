"""The plan of a lock-step call with an encoder length per chunk (include/wmi_device.h wmi_selftest_lockstep_sets; wmi_full_batch_ctx plans
with the same function), no GPU: the order — longest first, stable — and the lock-step calls the ordered chunks are cut into.  A
block-quantised model cuts where the lengths cross the threshold between the block-dot and the f16 form of its projections (256 rows: the
stacked pass runs every projection in the form each chunk's own pass takes), an f16 model does not cut at all."""
import ctypes as C
import pathlib
import re

import pytest

from godot_whisper_amd import runtime

ROOT = pathlib.Path(__file__).resolve().parent.parent
CTX8 = [0, 428, 278, 129, 64, 1500, 50, 777]


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


def _plan(lib, ctxs, quantised, n_audio_ctx=1500):
    n = len(ctxs)
    order, set_of = (C.c_int * n)(*([-7] * n)), (C.c_int * n)(*([-7] * n))
    rc = lib.wmi_selftest_lockstep_sets((C.c_int * n)(*ctxs), n, n_audio_ctx, quantised, order, set_of)
    return rc, list(order), list(set_of)


def test_header_declares_and_loader_binds_the_hooks(lib):
    text = (ROOT / "include" / "wmi_device.h").read_text()
    bound = {name: (res, args) for name, res, args in runtime.DEVICE_API}
    for n, n_args in (("wmi_selftest_lockstep_sets", 6), ("wmi_selftest_qkv_encoder_q", 14)):
        assert re.search(r"WHISPER_API\s+int\s+%s\s*\(" % n, text), n
        assert n in bound and bound[n][0] is C.c_int and len(bound[n][1]) == n_args, n
        assert getattr(lib, n).argtypes == bound[n][1], n


def test_quantised_model_two_sets_split_at_the_threshold(lib):
    rc, order, set_of = _plan(lib, CTX8, 1)
    # effective lengths 1500 428 278 129 64 1500 50 777: longest first, the two 1500s in the caller's order
    assert order == [0, 5, 7, 1, 2, 3, 4, 6]
    assert rc == 2 and set_of == [0, 0, 0, 0, 0, 1, 1, 1]           # >= 256 | < 256
    # exactly at the threshold: 256 is the f16 side, 255 the block-dot side
    rc, order, set_of = _plan(lib, [255, 256, 300, 17], 1)
    assert rc == 2 and order == [2, 1, 0, 3] and set_of == [0, 0, 1, 1]
    # all on one side: one set
    assert _plan(lib, [129, 64, 50, 200], 1) == (1, [3, 0, 1, 2], [0, 0, 0, 0])
    assert _plan(lib, [777, 428, 278, 256], 1) == (1, [0, 1, 2, 3], [0, 0, 0, 0])
    assert _plan(lib, [428, 129, 278, 64], 1) == (2, [0, 2, 1, 3], [0, 0, 1, 1])


def test_f16_model_one_set(lib):
    rc, order, set_of = _plan(lib, CTX8, 0)
    assert rc == 1 and order == [0, 5, 7, 1, 2, 3, 4, 6] and set_of == [0] * 8


@pytest.mark.parametrize("quantised", [0, 1])
def test_uniform_lengths_keep_the_callers_order(lib, quantised):
    assert _plan(lib, [428] * 5, quantised) == (1, [0, 1, 2, 3, 4], [0] * 5)
    assert _plan(lib, [0, 1500, 0], quantised) == (1, [0, 1, 2], [0] * 3)          # 0 = the model's length
    assert _plan(lib, [64, 64], quantised) == (1, [0, 1], [0, 0])


@pytest.mark.parametrize("quantised", [0, 1])
def test_one_chunk(lib, quantised):
    for a in (0, 64, 255, 256, 1500):
        assert _plan(lib, [a], quantised) == (1, [0], [0])


def test_other_model_length(lib):
    # 0 means n_audio_ctx: 300 rows here, the f16 side; 100 the block-dot side
    assert _plan(lib, [100, 0, 300], 1, n_audio_ctx=300) == (2, [1, 2, 0], [0, 0, 1])


def test_epilogue_hook_decides_argument_errors_before_the_device(lib):
    import numpy as np
    S, Tpad, M = 128, 64, 96
    x = np.zeros((M, S), np.float32); w = np.zeros(3 * S * (S // 32) * 24, np.uint8); b = np.zeros(3 * S, np.float32)
    q = np.zeros((M, S), np.uint16); k = np.zeros((M, S), np.uint16); vt = np.zeros((2, S, Tpad), np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(qtype=7, M=M, S=S, Tpad=Tpad, rpc=48, out_rows=M, x=x, w=w, b=b, q=q, k=k, vt=vt):
        return lib.wmi_selftest_qkv_encoder_q(0, qtype, M, S, Tpad, rpc, p(x) if x is not None else None, p(w) if w is not None else None,
                                              p(b) if b is not None else None, 0x7B7B, out_rows, p(q) if q is not None else None,
                                              p(k) if k is not None else None, p(vt) if vt is not None else None)
    assert call(qtype=5) == -1 and call(qtype=0) == -1              # not a block type this project loads
    assert call(M=0) == -1 and call(S=64) == -1 and call(S=192) == -1 and call(Tpad=48) == -1 and call(Tpad=0) == -1
    assert call(rpc=-1) == -1 and call(rpc=80) == -1 and call(rpc=36) == -1 and call(out_rows=M - 1) == -1
    assert call(M=17 * 4, rpc=4, out_rows=68) == -1                  # more than 16 chunks
    for name in ("x", "w", "b", "q", "k", "vt"):
        assert call(**{name: None}) == -1, name


def test_bad_arguments(lib):
    two = (C.c_int * 2)(100, 200)
    o, s = (C.c_int * 2)(-7, -7), (C.c_int * 2)(-7, -7)
    f = lib.wmi_selftest_lockstep_sets
    assert f(None, 2, 1500, 1, o, s) == -1
    assert f(two, 0, 1500, 1, o, s) == -1 and f(two, -1, 1500, 1, o, s) == -1
    assert f(two, 2, 0, 1, o, s) == -1
    assert f(two, 2, 1500, 1, None, s) == -1 and f(two, 2, 1500, 1, o, None) == -1
    assert f((C.c_int * 2)(100, -1), 2, 1500, 1, o, s) == -1
    assert f((C.c_int * 2)(100, 1501), 2, 1500, 1, o, s) == -1
    assert f(two, 2, 150, 0, o, s) == -1                             # 200 > n_audio_ctx
    assert list(o) == [-7, -7] and list(s) == [-7, -7]               # nothing written by a refused call
    assert f(two, 2, 1500, 1, o, s) == 1 and list(o) == [1, 0] and list(s) == [0, 0]

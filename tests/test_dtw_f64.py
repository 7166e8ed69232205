"""The judge of the token alignment (tests/dtw_f64.py) on the CPU: it accepts its own f32 restatement, proves the closed form of the band
family, and REFUSES the wrong restatements a kernel or a driver could be — so that the GPU tests, which hold the kernels to it, would see
them.  Then the host form of the path (wmi_selftest_dtw_path with device = -1) against the NumPy loop on every family, and
wmi_set_token_dtw on host-only contexts."""
import ctypes as C

import numpy as np
import pytest

import dtw_f64 as dj
from godot_whisper_amd import runtime, synth


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


@pytest.fixture(scope="module")
def rnd():
    """a random case with more keys than frames, two layers, start rows: every wrong restatement has something to get wrong"""
    return dj.random_case("rnd", 384, 6, 23, 3, 50, 87, [(0, 1), (0, 4), (1, 0), (1, 5)], seed=11, L=2)


def host_path(lib, A):
    A = np.ascontiguousarray(A, np.float32)
    R, M = A.shape
    jumps = np.full(R, -7, np.int32); path = np.full((R + M, 2), -7, np.int32); n_path = C.c_int(-1)
    assert lib.wmi_selftest_dtw_path(-1, R, M, A.ctypes.data, jumps.ctypes.data, path.ctypes.data, C.byref(n_path)) == 0
    assert (path[n_path.value:] == -7).all()
    return jumps, path[:n_path.value]


def test_f32_restatement_within_bound(rnd):
    """the bound is a worst case over summation orders; one f32 order sits far inside it (the docstring of dtw_f64 quotes the figure)"""
    worst = 0.0
    cases = [rnd, dj.random_case("m1", 384, 6, 9, 1, 1, 38, [(0, 0)], 1), dj.random_case("m3", 384, 6, 9, 3, 3, 3, [(0, 2), (0, 3)], 2),
             dj.random_case("m4", 384, 6, 5, 3, 4, 41, [(0, 5)], 3), dj.random_case("m77", 1280, 20, 65, 1, 77, 114, [(1, 19), (0, 7)][::-1], 4)]
    for c in cases:
        A64, bound = c.expected()
        worst = max(worst, dj.hold_matrix(dj.matrix_f32(*c.operands(), c.n_sot), A64, bound, c.name))
    print(f"f32 restatement: largest |d| / bound = {worst:.4f}")
    assert worst <= 0.5                                       # (twice the restatement's own distance still fits the bound)


@pytest.mark.parametrize("wrong", ["softmax_T", "sample_sigma", "edge_pad", "median5", "no_shift", "wrong_layer"])
def test_judge_refuses_wrong_matrices(rnd, wrong):
    A64, bound = rnd.expected()
    qp, kp = rnd.operands()
    if wrong == "wrong_layer":
        swapped = [(1 - l, h) for l, h in rnd.pairs]
        A = dj.matrix_f32(*rnd.operands(pairs=swapped), rnd.n_sot)
    elif wrong == "softmax_T":
        A = dj.matrix_f32(qp, kp, rnd.n_sot, wrong, k_all=rnd.operands(keys=rnd.T)[1])
    else:
        A = dj.matrix_f32(qp, kp, rnd.n_sot, wrong)
    with pytest.raises(AssertionError):
        dj.hold_matrix(A, A64, bound, wrong)


def test_judge_refuses_wrong_paths():
    refused = {"tie_le": 0, "transposed": 0}
    for name, A in dj.tie_matrices():
        j, p = dj.dtw_f32(A)
        dj.hold_path(A, j, p, name)
        for wrong in refused:
            wj, wp = dj.dtw_f32(A, wrong)
            if wp.shape == p.shape and (wp == p).all() and (wj == j).all():
                continue                                      # (a 1 x 1 matrix has one path)
            with pytest.raises(AssertionError):
                dj.hold_path(A, wj, wp, (name, wrong))
            refused[wrong] += 1
    assert min(refused.values()) >= 10, refused
    Z = np.zeros((4, 9), np.float32)                          # all zeros: every comparison is a tie, the rule says "left", then "up" at the border
    j, p = dj.dtw_f32(Z)
    assert list(j) == [0, 0, 0, 0] and [tuple(x) for x in p] == [(0, 0), (1, 0), (2, 0), (3, 0)] + [(3, t) for t in range(1, 9)]


def test_band_family_has_its_closed_form():
    for n_sot, R, M, S, H, pairs in ((1, 5, 50, 384, 6, [(0, 2)]), (3, 11, 77, 384, 6, [(0, 0), (0, 5), (1, 3)]), (3, 60, 1500, 128, 2, [(1, 1)])):
        c = dj.band_case("bands", S, H, n_sot + R + 1, n_sot, M, M + 37, pairs, seed=R)
        A64, bound = c.expected()
        band = np.searchsorted(np.array(c.starts), np.arange(M), side="right") - 1
        inside = band[None, :] == np.arange(R)[:, None]
        assert (A64[inside] > 1.0).all() and (A64[~inside] < 0.0).all()
        for r in range(R):                                    # a staircase: constant on every band, for every row
            for b in range(R):
                seg = A64[r, c.starts[b]:(c.starts[b + 1] if b + 1 < R else M)]
                assert np.ptp(seg) <= 1e-9, (r, b)
        assert bound.max() < 0.25 * (A64[inside].min() - A64[~inside].max())       # the bound leaves the staircase its steps
        for A in (A64.astype(np.float32), dj.matrix_f32(*c.operands(), c.n_sot)):
            j, _ = dj.dtw_f32(A)
            assert list(j) == list(c.starts)


def test_sweep_order_does_not_matter():
    for name, A in dj.tie_matrices() + [("rnd", dj.path_matrix("random", 17, 29)), ("rnd2", dj.path_matrix("random", 29, 17))]:
        a, b = dj.dtw_scalar(A), dj.dtw_f32(A)
        assert (a[0] == b[0]).all() and a[1].shape == b[1].shape and (a[1] == b[1]).all(), name


@pytest.mark.parametrize("family", ["ties", "bands", "random"])
def test_host_path_is_the_numpy_loop(lib, family):
    for R, M in ((1, 1), (1, 2), (2, 1), (2, 50), (63, 50), (64, 2), (65, 50), (225, 50), (50, 225), (448, 1500), (448, 50)):
        A = dj.path_matrix(family, R, M)
        j, p = host_path(lib, A)
        dj.hold_path(A, j, p, (family, R, M))
        if family == "bands" and M >= R:
            assert list(j) == list(dj.staircase_jumps(R, M))
    if family == "ties":
        for name, A in dj.tie_matrices():
            dj.hold_path(A, *host_path(lib, A), name)


def test_path_hook_argument_errors(lib):
    A = np.zeros((2, 2), np.float32); j = np.zeros(2, np.int32); p = np.zeros((4, 2), np.int32); n = C.c_int()
    ok = (A.ctypes.data, j.ctypes.data, p.ctypes.data, C.byref(n))
    for dev in (-1, 0):                                       # decided before the device is touched: the same answers without a GPU
        assert lib.wmi_selftest_dtw_path(dev, 0, 2, *ok) == -1 and lib.wmi_selftest_dtw_path(dev, 2, 0, *ok) == -1
        assert lib.wmi_selftest_dtw_path(dev, 2, 2, None, *ok[1:]) == -1 and lib.wmi_selftest_dtw_path(dev, 2, 2, ok[0], None, *ok[2:]) == -1
    assert lib.wmi_selftest_dtw_path(0, 512, 2, *ok) == -1
    q = np.zeros((1, 4, 384), np.float16); k = np.zeros((1, 8, 384), np.float16); lh = np.array([0, 0], np.int32); out = np.zeros((2, 8), np.float32)

    def matrix(L=1, S=384, H=6, n=4, n_sot=1, M=8, T=8, pairs=lh, n_pairs=1, qq=q):
        return lib.wmi_selftest_dtw_matrix(0, L, S, H, n, n_sot, M, T, qq.ctypes.data if qq is not None else None, k.ctypes.data,
                                           pairs.ctypes.data, n_pairs, out.ctypes.data)
    assert matrix(S=380) == -1 and matrix(M=9) == -1 and matrix(M=0) == -1 and matrix(T=1501, M=8) == -1 and matrix(n=2) == -1
    assert matrix(n_sot=0) == -1 and matrix(n_pairs=0) == -1 and matrix(qq=None) == -1 and matrix(H=33, S=64 * 33) == -1
    assert matrix(pairs=np.array([1, 0], np.int32)) == -1 and matrix(pairs=np.array([0, 6], np.int32)) == -1
    assert matrix(pairs=np.array([0, 1, 0, 1], np.int32), n_pairs=2) == -1 and matrix(pairs=np.array([0, 1, 0, 0], np.int32), n_pairs=2) == -1


def header_and_zeros(shape):
    """a model image of the shape with every tensor zero (the hyper-parameters are all wmi_set_token_dtw reads; synth.make_model would draw
    1.5 G normal numbers for large-v3)"""
    import struct
    hp = list(synth.SHAPES[shape])
    parts = [struct.pack("<I", synth.GGML_MAGIC), struct.pack("<11i", *hp, 1), struct.pack("<2i", hp[9], 201),
             np.ascontiguousarray(synth.mel_filters(hp[9]), dtype="<f4").tobytes(), synth.vocab_blob(hp[0] >= 51865)]
    for name, ne, kind in synth.tensor_specs(hp):
        f32 = kind in ("pe", "ln_w", "ln_b", "bias")
        nm = name.encode()
        parts += [struct.pack("<3i", len(ne), len(nm), synth.GGML_TYPE_F32 if f32 else synth.GGML_TYPE_F16), struct.pack(f"<{len(ne)}i", *ne), nm,
                  bytes(int(np.prod(ne)) * (4 if f32 else 2))]
    return b"".join(parts)


@pytest.mark.parametrize("shape,layers,heads", [("tiny", 4, 6), ("base", 6, 8), ("large-v3", 32, 20)])
def test_set_token_dtw_on_a_host_only_context(lib, shape, layers, heads):
    mb = header_and_zeros(shape)
    ctx = lib.wmi_init_host_only(C.cast(C.c_char_p(mb), C.c_void_p), len(mb))      # (the loader only borrows the buffer during the call)
    assert ctx
    del mb
    try:
        def heads_now():
            n = lib.wmi_token_dtw_heads(ctx, None, 0)
            a = (C.c_int32 * (2 * n))()
            assert lib.wmi_token_dtw_heads(ctx, a, n) == n
            return [(a[2 * i], a[2 * i + 1]) for i in range(n)]

        def set_(mode, pairs):
            flat = [v for lh in pairs for v in lh]
            a = (C.c_int32 * max(1, len(flat)))(*flat)
            return lib.wmi_set_token_dtw(ctx, mode, a, len(pairs))
        default = [(l, h) for l in range(layers // 2, layers) for h in range(heads)]
        assert heads_now() == default and len(default) == (layers - layers // 2) * heads
        assert lib.wmi_set_token_dtw(None, 1, None, 0) == -2
        assert lib.wmi_set_token_dtw(ctx, 1, None, 0) == 0 and heads_now() == default       # previous mode 0
        assert set_(1, [(layers - 1, 2), (0, 1), (0, 0)]) == 1 and heads_now() == [(0, 0), (0, 1), (layers - 1, 2)]
        for bad in ([(layers, 0)], [(0, heads)], [(-1, 0)], [(0, -1)], [(1, 1), (0, 0), (1, 1)]):
            assert set_(0, bad) == -1
        assert lib.wmi_set_token_dtw(ctx, 1, None, 1) == -1 and lib.wmi_set_token_dtw(ctx, 1, None, -1) == -1
        assert heads_now() == [(0, 0), (0, 1), (layers - 1, 2)]                              # nothing changed
        assert lib.wmi_set_token_dtw(ctx, 0, None, 0) == 1 and lib.wmi_set_token_dtw(ctx, 0, None, 0) == 0 and heads_now() == default
        # a context that has never transcribed: the accessors answer "nothing"
        assert lib.wmi_full_get_token_dtw(ctx, 0, 0) == -1 and lib.wmi_token_dtw_dims(ctx, None, None, None, None, None) == -1
        us, nw = C.c_int64(-1), C.c_int32(-1)
        lib.wmi_get_token_dtw_timings(ctx, C.byref(us), C.byref(nw))
        assert (us.value, nw.value) == (0, 0)
    finally:
        lib.whisper_free(ctx)

"""The judge of the long-recording front (tests/segment_f64.py) on the CPU: the library's plan equals the restatement piece for piece on
energy arrays that hit every rule, the judge REFUSES the wrong plans a driver could make, the host restatement of the energies
(wmi_selftest_frame_energy with device = -1) equals the NumPy definition on the GPU test's inputs, and the argument errors and struct
layouts of the interface."""
import ctypes as C

import numpy as np
import pytest

import segment_f64 as sj
from godot_whisper_amd import abi, runtime, synth


@pytest.fixture(scope="module")
def lib():
    lib = runtime.load_library()
    runtime.silence_logs(lib)
    return lib


CASES = sj.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_equals_the_restatement(lib, case):
    got = sj.lib_plan(lib, case["e"], case["n"], case["lp"], case["n_audio_ctx"], case.get("offset_ms", 0), case.get("duration_ms", 0))
    want = sj.hold_plan(got, case)
    F = case["e"].size
    for i, (a, b, _) in enumerate(want):                        # pieces are in order, disjoint, inside the signal
        assert 0 <= a < b <= F and (i == 0 or want[i - 1][1] <= a), want


def test_the_cases_hit_the_rules():
    """what each crafted array is there for, stated on the restatement's own plan"""
    by = {c["name"]: sj.plan(c["e"], c["n"], c["lp"], c["n_audio_ctx"], None, c.get("offset_ms", 0), c.get("duration_ms", 0)) for c in CASES}
    assert by["no island"] == [] and by["offset behind the signal"] == []
    assert by["one island fills the signal"] == [(0, 500, 0)]
    assert by["gap of G and of G - 1"] == [(0, 659, 0)]                            # the gap of 30 is bridged (< max_gap), the run of 29 is no gap at all
    assert by["pad clipped at a midpoint and at both ends"] == [(0, 205, 0), (205, 407, 0)]       # 0 | midpoint 205 | F
    assert by["absorption stopped by max_gap"] == [(0, 460, 0), (640, 1149, 0)]    # 150 and 199 are bridged, 200 is not
    assert by["absorption stopped by Lmax"] == [(90, 310, 0), (340, 755, 0)]
    assert by["absorption just fits Lmax"] == [(90, 590, 0)]                       # exactly Lmax
    assert [p[:2] for p in by["island of 2.5 Lmax, unique minima"]] == [(40, 450), (450, 870), (870, 1310)]
    assert [p[:2] for p in by["island of 2.5 Lmax, ties"]][0] == (40, 430)
    assert [p[:2] for p in by["island of 2.5 Lmax, flat"]] == [(0, 334), (334, 668), (668, 1002), (1002, 1250)]
    assert by["40-frame island between long gaps"][1][:2] == (540, 640)            # the end moved
    assert by["40-frame island squeezed on both sides"][1][:2] == (310, 390)       # the end to the next piece, then the start to the previous: still short, kept
    assert by["40-frame island at the end"][1][:2] == (525, 625)                   # the end to F, then the start
    assert by["shorter than 1 s"] == [(0, 60, 0)]
    assert [p[2] for p in by["fit_audio_ctx against a small n_audio_ctx"]] == [200, 188, 178]
    assert [p[2] for p in by["fit_audio_ctx"]] == [(310 + 1) // 2 + 128, (121 + 1) // 2 + 128]
    assert by["offset and duration"][0][0] == 290 and by["offset and duration"][-1][1] <= 853


@pytest.mark.parametrize("wrong", sj.WRONG_PLANS)
def test_judge_refuses_wrong_plans(wrong):
    case = next(c for c in CASES if c["name"] == sj.WRONG_ON[wrong])
    bad = sj.plan(case["e"], case["n"], case["lp"], case["n_audio_ctx"], wrong)
    with pytest.raises(AssertionError):
        sj.hold_plan(bad, case, wrong)
    refused = 0
    for c in CASES:                                             # and none of them is accepted across the whole set
        if c.get("offset_ms") or c.get("duration_ms"):
            continue
        try:
            sj.hold_plan(sj.plan(c["e"], c["n"], c["lp"], c["n_audio_ctx"], wrong), c, wrong)
        except AssertionError:
            refused += 1
    assert refused >= 1, wrong


def test_plan_on_random_energies(lib):
    """seeded gated noise levels: runs of random length at random levels, every parameter drawn"""
    rng = np.random.default_rng(5)
    for k in range(200):
        runs = [(int(rng.integers(1, 400)), float(rng.choice([0.0, 0.001, 0.5, 4.0, 16.0, 40.0]))) for _ in range(int(rng.integers(1, 14)))]
        e, n = sj._e(runs, tail=int(rng.integers(1, 161)))
        e = (e * rng.uniform(0.9, 1.1, e.size)).astype(np.float32)
        lp = sj.params(thold=float(rng.choice([0.1, 0.25, 0.6])), min_silence_ms=int(rng.choice([10, 100, 300, 505])),
                       pad_ms=int(rng.choice([0, 100, 250, 1000])), max_gap_ms=int(rng.choice([0, 300, 2000])),
                       max_piece_ms=int(rng.choice([1000, 2000, 5000, 30000])), fit_audio_ctx=int(rng.integers(0, 2)))
        off, dur = (int(rng.integers(0, 3000)), int(rng.integers(0, 20000))) if k % 3 == 0 else (0, 0)
        case = dict(name=("random", k), e=e, n=n, lp=lp, n_audio_ctx=int(rng.choice([300, 1500])), offset_ms=off, duration_ms=dur)
        sj.hold_plan(sj.lib_plan(lib, e, n, lp, case["n_audio_ctx"], off, dur, cap=2048), case)


def test_window(lib):
    for n, off, dur in ((1, 0, 0), (160, 0, 0), (161, 0, 0), (16000, 250, 0), (16000, 0, 250), (16000, 995, 10), (16000, 2000, 5), (16077, 990, 0),
                        (16077, 1000, 0), (16077, 1010, 0), (48000, 1234, 567)):
        assert sj.lib_window(lib, n, off, dur) == sj.window(n, off, dur), (n, off, dur)
    z = C.c_int(0)
    assert lib.wmi_selftest_long_window(0, 0, 0, C.byref(z), C.byref(z), C.byref(z)) == -1
    assert lib.wmi_selftest_long_window(100, -1, 0, C.byref(z), C.byref(z), C.byref(z)) == -1
    assert lib.wmi_selftest_long_window(100, 0, -1, C.byref(z), C.byref(z), C.byref(z)) == -1
    assert lib.wmi_selftest_long_window(100, 0, 0, None, C.byref(z), C.byref(z)) == -1


def test_host_energies_equal_the_definition(lib):
    stage = lib.wmi_long_stage_samples()
    assert stage > 0 and stage % sj.FRAME == 0
    for fam in sj.FAMILIES:
        for n in sj.sizes(stage):
            x = sj.make_input(fam, n, seed=n % 1000 + 7)
            F = (n + sj.FRAME - 1) // sj.FRAME
            e = np.full(F + 3, -7.0, np.float32)
            assert lib.wmi_selftest_frame_energy(-1, x.ctypes.data, n, e.ctypes.data) == 0
            want = sj.energies(x)
            assert e[:F].tobytes() == want.tobytes(), (fam, n)
            assert (e[F:] == -7.0).all()


def test_the_definition_is_the_plain_loop():
    """the vectorised NumPy form against the one-by-one loop it stands for"""
    x = sj.make_input("special", 1000, 3)
    x = np.concatenate([x, sj.make_input("seqsum", 487, 4)])
    want = []
    prev = np.float32(0.0)
    for f in range((x.size + 159) // 160):
        acc = np.float32(0.0)
        for v in x[160 * f:160 * f + 160]:
            acc = np.float32(acc + np.abs(np.float32(v - prev)))
            prev = v
        want.append(acc)
    assert np.array(want, np.float32).tobytes() == sj.energies(x).tobytes()


def test_input_guards():
    """conditions on the INPUTS of the GPU test: a tree or butterfly reduction of a frame's terms, and a kernel that reads x[160 f - 1]
    as 0 at frame edges, each give other bits than the definition — so neither can pass there"""
    stage = 10240
    for n in [m for m in sj.sizes(stage) if m >= 159]:
        x = sj.make_input("seqsum", n, seed=n % 1000 + 7)
        e = sj.energies(x)
        assert (sj.energies_tree(x).view(np.uint32) != e.view(np.uint32)).any(), n
        assert (sj.energies_tree(x, butterfly=True).view(np.uint32) != e.view(np.uint32)).any(), n
    for fam in sj.FAMILIES:
        for n in sj.sizes(stage):
            if n <= sj.FRAME:
                continue
            x = sj.make_input(fam, n, seed=n % 1000 + 7)
            e, z = sj.energies(x).view(np.uint32), sj.energies(x, edge_zero=True).view(np.uint32)
            assert (e[1:] != z[1:]).any(), (fam, n)
            if n > stage:                                       # and at the hand-over between two workgroups in particular
                assert e[stage // sj.FRAME] != z[stage // sj.FRAME], (fam, n)


def test_struct_layouts_and_defaults(lib):
    assert C.sizeof(abi.wmi_long_params) == 28 and C.sizeof(abi.wmi_long_piece) == 24
    assert [getattr(abi.wmi_long_params, f).offset for f, _ in abi.wmi_long_params._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert [getattr(abi.wmi_long_piece, f).offset for f, _ in abi.wmi_long_piece._fields_] == [0, 4, 8, 12, 16, 20]
    d = lib.wmi_long_default_params()
    assert (d.min_silence_ms, d.pad_ms, d.max_gap_ms, d.max_piece_ms, d.fit_audio_ctx) == (300, 100, 2000, 30000, 0)
    assert d.thold == np.float32(0.25) and d.floor == np.float32(1e-4)
    assert bytes(d) == bytes(sj.params())
    # the header declares what the tables bind
    import pathlib
    text = (pathlib.Path(__file__).resolve().parent.parent / "include" / "wmi_device.h").read_text()
    for name in ("wmi_full_long", "wmi_long_n_pieces", "wmi_long_get_piece", "wmi_long_select", "wmi_selftest_frame_energy",
                 "wmi_selftest_long_plan", "wmi_get_long_timings"):
        assert name + "(" in text and hasattr(lib, name)
    # NULL parameters are the defaults
    c = CASES[2]
    assert sj.lib_plan(lib, c["e"], c["n"], None, 1500) == sj.lib_plan(lib, c["e"], c["n"], sj.params(), 1500)


def test_hook_argument_errors(lib):
    x = np.zeros(320, np.float32); e = np.zeros(66, np.float32)
    assert lib.wmi_selftest_frame_energy(-1, None, 320, e.ctypes.data) == -1
    assert lib.wmi_selftest_frame_energy(-1, x.ctypes.data, 0, e.ctypes.data) == -1
    assert lib.wmi_selftest_frame_energy(-1, x.ctypes.data, -5, e.ctypes.data) == -1
    assert lib.wmi_selftest_frame_energy(-1, x.ctypes.data, 320, None) == -1
    assert lib.wmi_selftest_frame_energy(-2, x.ctypes.data, 320, e.ctypes.data) == -1
    assert lib.wmi_selftest_frame_energy(0, None, 320, e.ctypes.data) == -1          # before the device is touched
    en = np.full(10, 16.0, np.float32); out = (abi.wmi_long_piece * 4)()
    ok = sj.params()

    def call(e_ptr=en.ctypes.data, F=10, n=1600, lp=ok, nac=1500, o=out, cap=4):
        return lib.wmi_selftest_long_plan(e_ptr, F, n, C.byref(lp) if lp is not None else None, nac, o, cap)
    assert call() == 1
    assert call(e_ptr=None) == -1 and call(F=0) == -1 and call(n=0) == -1 and call(nac=0) == -1 and call(cap=-1) == -1 and call(o=None) == -1
    assert call(n=1441) == 1 and call(n=1440) == -1 and call(n=1601) == -1            # F must be ceil(n / 160)
    assert call(o=None, cap=0) == 1                                                   # counting only
    for bad in (dict(max_piece_ms=999), dict(max_piece_ms=30001), dict(min_silence_ms=9), dict(pad_ms=-1), dict(max_gap_ms=-1),
                dict(thold=-0.5), dict(floor=float("nan")), dict(thold=float("inf"))):
        assert call(lp=sj.params(**bad)) == -1, bad
    assert call(lp=sj.params(max_piece_ms=1000)) == 1 and call(lp=sj.params(max_piece_ms=30000)) == 1
    many = np.tile(np.concatenate([np.full(120, 16.0, np.float32), np.zeros(250, np.float32)]), 6)
    two = (abi.wmi_long_piece * 2)()
    assert lib.wmi_selftest_long_plan(many.ctypes.data, many.size, many.size * 160, None, 1500, two, 2) == 6      # the count may exceed cap
    assert (two[1].frame0, two[1].frame1) == (360, 500)


def test_full_long_argument_errors_without_a_device(lib):
    p = lib.whisper_full_default_params(0)
    pcm = np.zeros(16000, np.float32)
    assert lib.wmi_full_long(None, p, pcm.ctypes.data, pcm.size, 0, None) == -1
    assert lib.wmi_long_n_pieces(None) == -1 and lib.wmi_long_select(None, -1) == -1
    assert lib.wmi_long_get_piece(None, 0, C.byref(abi.wmi_long_piece())) == -1
    us, n2 = (C.c_int64 * 3)(5, 5, 5), (C.c_int32 * 2)(5, 5)
    lib.wmi_get_long_timings(None, us, n2)
    assert list(us) == [0, 0, 0] and list(n2) == [0, 0]
    mb = synth.make_model("micro.en", seed=1)
    buf = C.create_string_buffer(mb, len(mb))
    ctx = lib.wmi_init_host_only(C.cast(buf, C.c_void_p), len(mb))
    try:
        assert lib.wmi_full_long(ctx, p, None, pcm.size, 0, None) == -1
        assert lib.wmi_full_long(ctx, p, pcm.ctypes.data, -1, 0, None) == -1
        assert lib.wmi_full_long(ctx, p, pcm.ctypes.data, pcm.size, 0, C.byref(sj.params(max_piece_ms=999))) == -1
        assert lib.wmi_full_long(ctx, p, pcm.ctypes.data, pcm.size, 0, C.byref(sj.params(max_piece_ms=30001))) == -1
        assert lib.wmi_full_long(ctx, p, pcm.ctypes.data, 0, 0, None) == -3                # as whisper_full: no signal
        assert lib.wmi_full_long(ctx, p, pcm.ctypes.data, pcm.size, 0, None) == -2         # no compute path, as the other compute calls
        cb = C.CFUNCTYPE(None)(lambda: None)
        for field in ("new_segment_callback", "progress_callback", "encoder_begin_callback", "logits_filter_callback"):
            q = lib.whisper_full_default_params(0)
            setattr(q, field, C.cast(cb, C.c_void_p).value)
            assert lib.wmi_full_long(ctx, q, pcm.ctypes.data, pcm.size, 0, None) == -1, field
        assert lib.wmi_long_n_pieces(ctx) == 0 and lib.wmi_long_select(ctx, -1) == -1 and lib.wmi_long_select(ctx, 0) == -1
        assert lib.wmi_long_get_piece(ctx, 0, C.byref(abi.wmi_long_piece())) == -1
    finally:
        lib.whisper_free(ctx)

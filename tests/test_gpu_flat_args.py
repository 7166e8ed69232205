"""-m gpu: the operands of the kernels whose leading arguments are plain parameters (kernarg preload; csrc/k_dec.hip k_front, k_mlp_pair,
k_gemv1; csrc/k_attn.hip k_xback; csrc/k_gemm.hip, csrc/k_gemm8.hip) are wired to the right places.

Each of those kernels rebuilds its argument struct from the leading parameters, a packed word of dimensions and the trailing by-value
struct; a swapped pointer or a dimension cut at the wrong bit gives wrong numbers, not a crash.  So:

  1. one-row greedy steps (wmi_selftest_greedy_step) on synthetic two-layer decoders of width 384 and 512 at self-cache lengths 1, 64, 65
     and 130: the one-launch forms (front, cross-attention back, MLP pair: three launches per layer) give the bits of the plain chain of
     the same build (WMI_NO_FRONT, WMI_NO_XBACK, WMI_NO_MLP_PAIR), and both are within test_gpu_parity.py's logits tolerance of the oracle
     port.  The encoder is short (audio_ctx 64).  At 64 frames the cross-attention has one key slice and k_xback needs four: the same
     steps also run at audio_ctx 768, the shortest multiple of 64 at which the step takes k_xback.
  2. the same models with 2 and 3 lock-step rows (the rows' shifts on blockIdx.y / blockIdx.z): rows of different encoder lengths (64,
     768 — k_front, k_gemv1) and rows of one encoder length with audio of different lengths (k_xback takes uniform rows only), each row
     bit for bit what whisper_full gives for it alone (the exact mode).
  3. every GEMM epilogue through wmi_selftest_gemm at the smallest shapes of tests/gemm_f64.py's table that reach k_gemm and k_gemm8, on
     the two exact operand families: bit-identical to the float64 judge, the sentinels around the output untouched (gemm_f64.hold_gemm).
"""
import ctypes as C
import os

import numpy as np
import pytest

import gemm_f64 as gf
import stage_compare as sc
from godot_whisper_amd import abi, host, synth
from oracle import port
from test_gpu_gemm import run as run_gemm_case
from test_gpu_parity import _assert_same_transcription, assert_logits

pytestmark = pytest.mark.gpu

# forms of the greedy step (include/wmi_device.h: wmi_selftest_greedy_step)
LONG, CHAINED, GRAPH, PAIRED, FRONTED, BACKED, RERUN, SLOW, QUANT = 1, 2, 4, 8, 16, 32, 64, 128, 256
# (n_vocab, n_audio_ctx, S, H, L_audio, n_text_ctx, S_text, H_text, L_text, n_mels): two encoder and two decoder layers
SHAPES = {384: (51864, 1500, 384, 6, 2, 448, 384, 6, 2, 80), 512: (51864, 1500, 512, 8, 2, 448, 512, 8, 2, 80)}
LENGTHS = (1, 64, 65, 130)            # cells of the self cache the step attends (its own included)
CTX_SHORT, CTX_BACK = 64, 768         # encoder frames: one key slice of the cross-attention; four (the fewest k_xback takes)
PLAIN = ("WMI_NO_FRONT", "WMI_NO_XBACK", "WMI_NO_MLP_PAIR")

_MODELS, _RUNS = {}, {}


def _model(width):
    if width not in _MODELS:
        _MODELS[width] = synth.make_model(SHAPES[width], seed=384512)
    return _MODELS[width]


def _tokens(lib, ctx):
    rng = np.random.default_rng(20240)
    return [lib.whisper_token_sot(ctx)] + [int(t) for t in rng.integers(0, lib.whisper_token_eot(ctx), max(LENGTHS) - 1)]


def _product_steps(lib, model, actx):
    """-> the tokens and [(logits, pick, forms)] for LENGTHS: the cells before the step's own written by whisper_decode"""
    prod = sc.ProductSide(lib, model)
    try:
        prod.mel(synth.make_pcm(30.0, seed=77)); prod.encode(0, actx)
        toks = _tokens(lib, prod.ctx); out = []
        for n in LENGTHS:
            if n > 1 and n - 1 != LENGTHS[LENGTHS.index(n) - 1]:      # (65 follows 64 directly: a step onto the step's cell)
                prod.decode(toks[:n - 1], 0)
            lg = np.empty(prod.NV, np.float32); td = abi.whisper_token_data(); fm = C.c_int(0)
            rc = lib.wmi_selftest_greedy_step(prod.ctx, toks[n - 1], n - 1, sc._fptr(lg), C.byref(td), C.byref(fm))
            assert rc == 0, (n, rc)
            if fm.value & SLOW:                                        # the device is shared: allow the one-launch forms again
                assert lib.wmi_pair_status(prod.ctx, None, 1) == 0
            out.append((lg, td.id, fm.value))
        return toks, out
    finally:
        prod.close()


def _runs(lib, width, actx):
    """the default build's steps, the plain chain's and the oracle port's logits, once per (width, encoder length)"""
    key = (width, actx)
    if key not in _RUNS:
        model = _model(width)
        toks, default = _product_steps(lib, model, actx)
        saved = {k: os.environ.get(k) for k in PLAIN}
        try:
            for k in PLAIN:
                os.environ[k] = "1"
            lib.wmi_reload_knobs()                                     # (the switches are read once per process)
            toks0, plain = _product_steps(lib, model, actx)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            lib.wmi_reload_knobs()
        chk = port.PortSide(model, n_threads=16)
        try:
            chk.mel(synth.make_pcm(30.0, seed=77)); chk.encode(0, actx)
            assert toks0 == toks
            want = [chk.decode(toks[:n], 0) for n in LENGTHS]
        finally:
            chk.close()
        _RUNS[key] = (default, plain, want)
    return _RUNS[key]


CASES = [(w, a) for w in SHAPES for a in (CTX_SHORT, CTX_BACK)]


@pytest.mark.parametrize("width,actx", CASES)
def test_one_launch_forms_are_taken(product_lib, width, actx):
    default, plain, _ = _runs(product_lib, width, actx)
    slow = [n for n, (_, _, fm) in zip(LENGTHS, default) if fm & SLOW]
    assert len(slow) <= 1, (width, actx, slow)                        # (a slow hand-off: the device is busy with someone else's work)
    for n, (_, _, fm) in zip(LENGTHS, default):
        assert not fm & (RERUN | QUANT), (width, actx, n, hex(fm))
        if slow:
            continue
        want = PAIRED | FRONTED | (LONG if n > 64 else 0) | (BACKED if actx == CTX_BACK else 0)
        assert fm & (PAIRED | FRONTED | BACKED | LONG) == want, (width, actx, n, hex(fm), hex(want))
    for n, (_, _, fm) in zip(LENGTHS, plain):
        assert not fm & (PAIRED | FRONTED | BACKED | RERUN), (width, actx, n, hex(fm))


@pytest.mark.parametrize("width,actx", CASES)
def test_one_launch_forms_equal_the_plain_chain(product_lib, width, actx):
    default, plain, _ = _runs(product_lib, width, actx)
    for n, (lg, pick, fm), (lg0, pick0, fm0) in zip(LENGTHS, default, plain):
        if not np.array_equal(lg, lg0):
            d = np.abs(lg.astype(np.float64) - lg0.astype(np.float64))
            pytest.fail(f"width {width}, {actx} frames, {n} cells: forms {hex(fm)} against {hex(fm0)}, max |d| {d.max():.3e} in {int((d > 0).sum())} logits")
        assert pick == pick0, (width, actx, n)


@pytest.mark.parametrize("width,actx", CASES)
def test_steps_agree_with_the_oracle_port(product_lib, width, actx):
    default, plain, want = _runs(product_lib, width, actx)
    for n, (lg, _, fm), (lg0, _, fm0), lr in zip(LENGTHS, default, plain, want):
        assert_logits(lg, lr, (width, actx, n, hex(fm)))
        assert_logits(lg0, lr, (width, actx, n, hex(fm0)))


@pytest.mark.parametrize("width", list(SHAPES))
def test_stamped_launches_take_the_same_operands(product_lib, width):
    """The probe's launches (wmi_step_stamps: the chained step captured with in-kernel time stamps on, replayed three times) carry the stamp
    switch as a bit of the packed dimension word: the fields beside it must come out as they went in — the launches of the replay are the
    step's, every one left its records, and the step gives the same logits after the replays as before them."""
    lib = product_lib
    prod = sc.ProductSide(lib, _model(width))
    try:
        prod.mel(synth.make_pcm(30.0, seed=77)); prod.encode(0, CTX_BACK)
        toks = _tokens(lib, prod.ctx)[:17]

        def step():
            prod.decode(toks[:16], 0)
            lg = np.empty(prod.NV, np.float32); td = abi.whisper_token_data(); fm = C.c_int(0)
            assert lib.wmi_selftest_greedy_step(prod.ctx, toks[16], 16, sc._fptr(lg), C.byref(td), C.byref(fm)) == 0
            return lg, fm.value

        before, fm = step()
        cap = 64; buf = (C.c_double * (6 * cap))()
        n = lib.wmi_step_stamps(prod.ctx, buf, cap, 1)
        assert n > 0
        stamped = [(buf[6 * i], buf[6 * i + 2]) for i in range(n) if buf[6 * i + 3] > 0]      # (first wavefront's start, last wavefront's end) of the launches with records
        if not fm & SLOW:
            assert fm & (PAIRED | FRONTED | BACKED) == PAIRED | FRONTED | BACKED, hex(fm)
            assert len(stamped) in (3 * prod.L + 2, 3 * prod.L + 3), (n, len(stamped))      # three launches per layer, the vocabulary projection, the pick (+ the embedding)
        assert all(first >= 0 and end > first for first, end in stamped), stamped
        after, _ = step()
        assert np.array_equal(before, after)
    finally:
        prod.close()


# ------------------------------------------------------------------------------------------------ 2. lock-step rows
@pytest.fixture
def exact(product_lib):
    product_lib.wmi_set_lockstep_exact(1)
    yield
    product_lib.wmi_set_lockstep_exact(0)


@pytest.mark.parametrize("rows", [2, 3])
@pytest.mark.parametrize("kind", ["own encoder lengths", "one encoder length"])
@pytest.mark.parametrize("width", list(SHAPES))
def test_lockstep_rows_equal_one_row_at_a_time(product_lib, exact, width, kind, rows):
    secs = [9.0, 1.3, 15.0][:rows]
    ctxs = [CTX_BACK, CTX_SHORT, CTX_BACK][:rows] if kind == "own encoder lengths" else [CTX_BACK] * rows
    pcms = [synth.make_pcm(s, seed=310 + i) for i, s in enumerate(secs)]
    model = _model(width)

    def params(node):
        # no fallback: no row may leave lock-step; no timestamps: a two-layer decoder counts as a distilled checkpoint, which whisper_full
        # forces to no_timestamps and the lock-step call hands back to whisper_full unless the caller has said so itself
        p = node.full_params("", 0); p.temperature_inc = 0.0; p.no_timestamps = True
        return p

    want = []
    for b, a in zip(pcms, ctxs):                          # whisper_full per row with its own audio_ctx, each on a fresh context
        node = host.SpeechToText(product_lib); node.set_language_model(model)
        try:
            p = params(node); p.audio_ctx = int(a)
            want.append(node.transcribe(b, params=p))
            assert node.last_ret == 0
        finally:
            node.close()
    node = host.SpeechToText(product_lib); node.set_language_model(model)
    try:
        got = node.transcribe_batch(pcms, params=params(node), audio_ctxs=ctxs)
        assert node.last_ret == 0 and len(got) == rows
        assert list(node.last_modes) == [0] * rows, node.last_modes          # every row stayed in lock-step
        for c, (g, w) in enumerate(zip(got, want)):
            _assert_same_transcription(g, w, (width, kind, rows, c, ctxs[c]), True)
    finally:
        node.close()
    assert any(len(g) > 1 for g in got), [len(g) for g in got]


# ------------------------------------------------------------------------------------------------ 3. the GEMMs' operands
def _smallest(epi, kernel):
    specs = [s for s in gf.TABLE if s.epi == epi and s.plan[0] == kernel and not s.force8]
    return min(specs, key=lambda s: (s.M * s.N * s.K, s.M)) if specs else None


GEMM_CASES = [(gf.EPI_NAMES[e], k, _smallest(e, k)) for e in range(len(gf.EPI_NAMES)) for k in (1, 8) if _smallest(e, k) is not None]


def test_every_epilogue_has_a_k_gemm_case_and_k_gemm8_its_own():
    assert {n for n, k, _ in GEMM_CASES if k == 1} == set(gf.EPI_NAMES)
    # k_gemm8 by the product's dispatch serves these epilogues (tests/gemm_f64.py: the table of plans)
    assert {n for n, k, _ in GEMM_CASES if k == 8} == {gf.EPI_NAMES[s.epi] for s in gf.TABLE if s.plan[0] == 8 and not s.force8}


@pytest.mark.parametrize("family", ["sparse", "dense"])
@pytest.mark.parametrize("name,kernel,spec", GEMM_CASES, ids=[f"{n}-k_gemm{'8' if k == 8 else ''}" for n, k, _ in GEMM_CASES])
def test_gemm_epilogues_are_exact(product_lib, name, kernel, spec, family):
    run_gemm_case(product_lib, spec, family)

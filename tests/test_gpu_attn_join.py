"""-m gpu: the front of a decoder layer and the back of its cross-attention as ONE launch (csrc/k_dec.hip: k_attn_join).

The joined launch runs k_front's body on its first 3 S / 16 workgroups and k_xback's on the H x ns behind them; the residual row crosses
from the first role's out projection to the second's LayerNorm as S granules {f32, tag} inside the launch.  Per value the operations
are the two launches', so everything here is held bit for bit:

  1. one-row greedy steps (wmi_selftest_greedy_step) on the two-layer decoders of width 384 and 512 of tests/test_gpu_flat_args.py, at
     encoder lengths 768 (four key slices, the fewest k_xback takes) and 1500 (eight) and self-cache lengths 1, 2 and 64 (the long-cache
     form of the front keeps its own launch): default = WMI_NO_JOIN = the plain chain, and within test_gpu_parity.py's logits tolerance
     of the oracle port.  Width 384: S / 2 = 192 polling threads, six heads — every index that is a power of two only at 512 shows.
  2. the two roles' stamp records of a replay overlap in time: it IS one launch; three records per layer as before.
  3. whisper_full on the width-512 model with the host's parameters: the same token array with and without WMI_NO_JOIN.
  4. a front-role wavefront that never publishes its granules of the row (WMI_JOIN_WITHHOLD): the bounded polls give up, the status word
     says so, the step is re-run in the plain form with the plain chain's result and the state stays on that form.
"""
import ctypes as C
import os

import numpy as np
import pytest

import golden_util as gu
import stage_compare as sc
from godot_whisper_amd import abi, host, synth
from oracle import port
from test_gpu_flat_args import BACKED, FRONTED, LONG, PAIRED, PLAIN, QUANT, RERUN, SHAPES, SLOW, _model
from test_gpu_parity import assert_logits

pytestmark = pytest.mark.gpu

JOINED = 512                          # include/wmi_device.h: wmi_selftest_greedy_step
LENGTHS = (1, 2, 64)                  # cells of the self cache the step attends (its own included)
CTXS = (768, 1500)                    # encoder frames: four and eight key slices of the cross-attention
CASES = [(w, a) for w in SHAPES for a in CTXS]

_RUNS = {}


class _knobs:
    """environment switches of the launch paths for the duration of a block (read once per process: wmi_reload_knobs)"""

    def __init__(self, lib, **env):
        self.lib, self.env = lib, env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        self.lib.wmi_reload_knobs()

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        self.lib.wmi_reload_knobs()


def _tokens(lib, ctx):
    rng = np.random.default_rng(20250)
    return [lib.whisper_token_sot(ctx)] + [int(t) for t in rng.integers(0, lib.whisper_token_eot(ctx), max(LENGTHS) - 1)]


def _step(lib, prod, token, pos):
    lg = np.empty(prod.NV, np.float32); td = abi.whisper_token_data(); fm = C.c_int(0)
    rc = lib.wmi_selftest_greedy_step(prod.ctx, token, pos, sc._fptr(lg), C.byref(td), C.byref(fm))
    assert rc == 0, (pos, rc)
    return lg, td.id, fm.value


def _product_steps(lib, model, actx):
    """-> the tokens and [(logits, pick, forms)] for LENGTHS: the cells before the step's own written by whisper_decode"""
    prod = sc.ProductSide(lib, model)
    try:
        prod.mel(synth.make_pcm(30.0, seed=77)); prod.encode(0, actx)
        toks = _tokens(lib, prod.ctx); out = []
        for n in LENGTHS:
            if n > 2:                                                  # (2 follows 1 directly: a step onto the step's cell)
                prod.decode(toks[:n - 1], 0)
            out.append(_step(lib, prod, toks[n - 1], n - 1))
            if out[-1][2] & SLOW:                                      # the device is shared: allow the one-launch forms again
                assert lib.wmi_pair_status(prod.ctx, None, 1) == 0
        return toks, out
    finally:
        prod.close()


def _runs(lib, width, actx):
    """the default build's steps, the two-launch form's (WMI_NO_JOIN), the plain chain's and the oracle port's logits, once per case"""
    key = (width, actx)
    if key not in _RUNS:
        model = _model(width)
        toks, default = _product_steps(lib, model, actx)
        with _knobs(lib, WMI_NO_JOIN="1"):
            toks1, apart = _product_steps(lib, model, actx)
        with _knobs(lib, **{k: "1" for k in PLAIN}):
            toks0, plain = _product_steps(lib, model, actx)
        assert toks0 == toks and toks1 == toks
        chk = port.PortSide(model, n_threads=16)
        try:
            chk.mel(synth.make_pcm(30.0, seed=77)); chk.encode(0, actx)
            want = [chk.decode(toks[:n], 0) for n in LENGTHS]
        finally:
            chk.close()
        _RUNS[key] = (default, apart, plain, want)
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ 1. same bits
@pytest.mark.parametrize("width,actx", CASES)
def test_the_joined_form_is_taken_and_the_switch_turns_it_off(product_lib, width, actx):
    default, apart, plain, _ = _runs(product_lib, width, actx)
    slow = [n for n, (_, _, fm) in zip(LENGTHS, default) if fm & SLOW]
    assert len(slow) <= 1, (width, actx, slow)                        # (a slow hand-off: the device is busy with someone else's work)
    for n, (_, _, fm) in zip(LENGTHS, default):
        assert not fm & (RERUN | QUANT | LONG), (width, actx, n, hex(fm))
        if not slow:
            assert fm & (JOINED | FRONTED | BACKED | PAIRED) == JOINED | FRONTED | BACKED | PAIRED, (width, actx, n, hex(fm))
    if not any(fm & SLOW for _, _, fm in apart):
        for n, (_, _, fm) in zip(LENGTHS, apart):
            assert fm & (JOINED | FRONTED | BACKED | PAIRED | RERUN) == FRONTED | BACKED | PAIRED, (width, actx, n, hex(fm))
    for n, (_, _, fm) in zip(LENGTHS, plain):
        assert not fm & (JOINED | PAIRED | FRONTED | BACKED | RERUN), (width, actx, n, hex(fm))


@pytest.mark.parametrize("width,actx", CASES)
def test_the_joined_form_equals_two_launches_and_the_plain_chain(product_lib, width, actx):
    default, apart, plain, _ = _runs(product_lib, width, actx)
    for name, other in (("WMI_NO_JOIN", apart), ("the plain chain", plain)):
        for n, (lg, pick, fm), (lg0, pick0, fm0) in zip(LENGTHS, default, other):
            if not np.array_equal(lg, lg0):
                d = np.abs(lg.astype(np.float64) - lg0.astype(np.float64))
                pytest.fail(f"width {width}, {actx} frames, {n} cells, against {name}: forms {hex(fm)} / {hex(fm0)}, max |d| {d.max():.3e} in {int((d > 0).sum())} logits")
            assert pick == pick0, (width, actx, n, name)


@pytest.mark.parametrize("width,actx", CASES)
def test_both_forms_agree_with_the_oracle_port(product_lib, width, actx):
    default, apart, _, want = _runs(product_lib, width, actx)
    for n, (lg, _, fm), (lg1, _, fm1), lr in zip(LENGTHS, default, apart, want):
        assert_logits(lg, lr, (width, actx, n, hex(fm)))
        assert_logits(lg1, lr, (width, actx, n, hex(fm1)))


# ------------------------------------------------------------------------------------------------ 2. one launch
@pytest.mark.parametrize("width", list(SHAPES))
def test_the_two_roles_of_a_layer_run_in_one_launch(product_lib, width):
    """wmi_step_stamps: per layer the records are front, cross-attention back, MLP pair.  Two launches of a stream follow each other —
    the second's first wavefront starts after the first's last has ended; the roles of the joined launch start together."""
    lib = product_lib
    prod = sc.ProductSide(lib, _model(width))
    try:
        prod.mel(synth.make_pcm(30.0, seed=77)); prod.encode(0, CTXS[0])
        toks = _tokens(lib, prod.ctx)[:18]
        prod.decode(toks[:16], 0)
        _, _, fm = _step(lib, prod, toks[16], 16)
        if fm & SLOW:                                                   # the device is shared: allow the one-launch forms again, once
            assert lib.wmi_pair_status(prod.ctx, None, 1) == 0
            _, _, fm = _step(lib, prod, toks[17], 17)
        assert fm & JOINED and not fm & (SLOW | RERUN), hex(fm)
        cap = 64; buf = (C.c_double * (6 * cap))()
        n = lib.wmi_step_stamps(prod.ctx, buf, cap, 1)
        assert n > 0
        stamped = [(buf[6 * i], buf[6 * i + 2]) for i in range(n) if buf[6 * i + 3] > 0]      # (first start, last end) of the launches with records
        assert len(stamped) in (3 * prod.L + 2, 3 * prod.L + 3), (n, len(stamped))
        base = len(stamped) - (3 * prod.L + 2)                          # (+ the embedding launch in front)
        for il in range(prod.L):
            (f0, f1), (x0, x1), (m0, m1) = stamped[base + 3 * il: base + 3 * il + 3]
            assert x0 < f1, (width, il, stamped)                       # the back's first wavefront runs while the front's still do
            assert x1 > f1 and m0 > x1, (width, il, stamped)           # ... it ends behind them, and the MLP pair is the next launch
    finally:
        prod.close()


# ------------------------------------------------------------------------------------------------ 3. a whole call
def test_whisper_full_gives_the_same_tokens_with_and_without_the_join(product_lib):
    lib = product_lib
    pcm = synth.make_pcm(11.0, seed=512)

    def call():
        node = host.SpeechToText(lib); node.set_language_model(_model(512))
        try:
            got = node.transcribe(pcm, params=node.full_params("", 0))
            assert node.last_ret == 0
            return got
        finally:
            node.close()

    a = call()
    with _knobs(lib, WMI_NO_JOIN="1"):
        b = call()
    ga, gb = gu.tokens_array(a), gu.tokens_array(b)
    assert len(ga) > 1, ga.shape
    assert ga.shape == gb.shape and np.array_equal(ga, gb), (ga, gb)   # every field of every token
    assert bytes(a[0]) == bytes(b[0])


# ------------------------------------------------------------------------------------------------ 4. the hop's fall-back
@pytest.mark.parametrize("width", list(SHAPES))
def test_a_failed_hop_is_reported_and_the_step_rerun(product_lib, width):
    """WMI_JOIN_WITHHOLD=2: wavefront 1 of the front role never publishes its four granules of the row; every reader of the row gives
    up after WMI_PAIR_SPIN_CAP polls (a few milliseconds) and says so in the status word.  The pick kernel reports it, the host runs the
    step again in the plain form — whose result this must be — and the state keeps that form."""
    lib = product_lib
    _, _, plain, _ = _runs(lib, width, CTXS[0])
    prod = sc.ProductSide(lib, _model(width))
    try:
        prod.mel(synth.make_pcm(30.0, seed=77)); prod.encode(0, CTXS[0])
        toks = _tokens(lib, prod.ctx)
        st = (C.c_int32 * 3)()
        with _knobs(lib, WMI_JOIN_WITHHOLD="2", WMI_PAIR_SPIN_CAP="3000"):
            lg, pick, fm = _step(lib, prod, toks[0], 0)
            assert lib.wmi_pair_status(prod.ctx, st, 0) == 0
            lg2, pick2, fm2 = _step(lib, prod, toks[1], 1)             # the next step: no in-launch hand-off any more
        assert fm & RERUN and fm & JOINED, hex(fm)
        assert st[0] == 1 and st[2] & 1, list(st)                      # one fall-back, the one-launch forms off
        assert np.array_equal(lg, plain[0][0]) and pick == plain[0][1]
        assert not fm2 & (JOINED | FRONTED | BACKED | PAIRED | RERUN), hex(fm2)
        assert np.array_equal(lg2, plain[1][0]) and pick2 == plain[1][1]
        assert lib.wmi_pair_status(prod.ctx, None, 1) == 0
    finally:
        prod.close()

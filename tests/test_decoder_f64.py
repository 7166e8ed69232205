"""The float64 restatement of the decoder (tests/decoder_f64.py) against the CPU port (oracle/libwhisper_port.so, the reference's
arithmetic) on micro.en over all 448 positions of the text context — and what the logit bounds of the -m gpu tests can see.

The restatement is what test_gpu_decode_lengths.py holds the product to on micro.en / tiny.en: rms(product - f64) <= SWEEP_LIMIT (1.5)
x rms(checker - f64) over a sweep of every position.  Here it must agree with the port within F64_RMS / F64_ABS per position (measured worst 5.5e-4 /
1.6e-2: the port rounds its operands, the cache and the activations to f16, the restatement does not), and one-cell mistakes made on
purpose must stand out:

    mistake (one row of the causal pass)           rms-rel vs the port   x LOGIT_RMS (1e-3)
    cell 65 visible at n_kv = 65 (a future cell)   9.8e-3                9.8
    the last cell dropped at n_kv = 65             6.2e-3                6.2
    the last cell dropped at n_kv = 448            1.3e-3                1.3    <- under 3x: one-cell weight ~ 1 / n_kv
    the last cross key dropped at n_kv = 65        1.4e-3                1.4    <- under 3x: one of 1500 encoder frames
    the last cross key dropped at n_kv = 448       0.85e-3               0.85   <- not seen by the per-position bound

The per-position bounds therefore see a one-cell error in a SHORT cache only.  What catches the others is the float64 sweep: the same
mistake made at every position moves rms(mistake - f64) / rms(port - f64) to 26 (the last cell, n_kv > 64) and 2.9 (the last cross
key): 17x and 1.9x the sweep's limit.  (That limit was tightened from 2 to 1.5 for the cross key; the product measures 1.01.)  Both
numbers are asserted below; a single dropped cross key at one position stays under every bound here."""
import numpy as np
import pytest

import stage_compare as sc
from decoder_f64 import SWEEP_LIMIT, DecoderF64
from godot_whisper_amd import synth
from oracle import port

LOGIT_RMS = 1e-3                 # tests/test_gpu_parity.py (not imported: that module is -m gpu)
F64_RMS, F64_ABS = 7e-4, 2.5e-2  # port vs the restatement, per position


@pytest.fixture(scope="module")
def micro():
    if not port.available():
        pytest.fail("oracle/libwhisper_port.so not built (python __graft_entry__.py build)")
    model = synth.make_model("micro.en", seed=1234)
    chk = port.PortSide(model, n_threads=8)
    try:
        chk.mel(synth.make_pcm(30.0, seed=1234))
        enc = chk.encode(0, 0)
        rng = np.random.default_rng(7)
        toks = [chk.sot] + [int(t) for t in rng.integers(0, 50256, chk.n_text_ctx - 1)]
        lr = np.stack([chk.decode(toks[:1], 0)] + [chk.decode([toks[p]], p) for p in range(1, len(toks))]).astype(np.float64)
    finally:
        chk.close()
    dec = DecoderF64(model)
    return dec, toks, enc["cross_k"], enc["cross_v"], lr, dec.logits(toks, enc["cross_k"], enc["cross_v"])


def test_float64_decoder_agrees_with_the_port_at_every_position(micro):
    dec, toks, ck, cv, lr, lf = micro
    assert lf.shape == lr.shape == (448, dec.n_vocab)
    worst = (0.0, 0.0)
    for p in range(len(toks)):
        st = sc.err_stats(lr[p], lf[p])
        assert st["rms_rel"] <= F64_RMS and st["max_abs"] <= F64_ABS, (p, st)
        worst = (max(worst[0], st["rms_rel"]), max(worst[1], st["max_abs"]))
    print(f"\nport vs float64 over 448 positions: worst rms-rel {worst[0]:.2e}, worst max |d| {worst[1]:.2e}")
    # causal: a row does not depend on what comes after it (a shorter pass gives the same row, up to float64 summation order)
    np.testing.assert_allclose(dec.logits(toks[:100], ck, cv, rows=[99])[0], lf[99], rtol=0, atol=1e-11)


def _causal(n, row):
    return np.arange(n) <= row


@pytest.mark.parametrize("mistake,row,at_least", [
    ("future cell visible", 64, 3 * LOGIT_RMS),
    ("last cell dropped", 64, 3 * LOGIT_RMS),
    ("last cell dropped", 447, LOGIT_RMS),
    ("last cross key dropped", 64, LOGIT_RMS),
    ("last cross key dropped", 447, 0.5 * LOGIT_RMS),
])
def test_a_one_cell_mistake_stands_out_at_one_position(micro, mistake, row, at_least):
    dec, toks, ck, cv, lr, lf = micro
    n, T = len(toks), ck.shape[1]
    sv, xv = {}, {}
    if mistake == "future cell visible":
        m = _causal(n, row); m[row + 1] = True; sv[row] = m
    elif mistake == "last cell dropped":
        m = _causal(n, row); m[row] = False; sv[row] = m
    else:
        m = np.ones(T, bool); m[T - 1] = False; xv[row] = m
    bad = dec.logits(toks, ck, cv, rows=[row], self_visible=sv, cross_visible=xv)[0]
    st = sc.err_stats(bad, lr[row])
    print(f"\n{mistake} at n_kv = {row + 1}: rms-rel vs the port {st['rms_rel']:.2e} = {st['rms_rel'] / LOGIT_RMS:.2f} x LOGIT_RMS")
    assert st["rms_rel"] >= at_least, (mistake, row, st)


@pytest.mark.parametrize("mistake,at_least", [("last cell dropped, n_kv > 64", 3 * SWEEP_LIMIT), ("last cross key dropped", 1.5 * SWEEP_LIMIT)])
def test_a_systematic_one_cell_mistake_fails_the_float64_sweep(micro, mistake, at_least):
    dec, toks, ck, cv, lr, lf = micro
    n, T = len(toks), ck.shape[1]
    if mistake.startswith("last cell"):
        rows = range(64, n)
        bad = dec.logits(toks, ck, cv, self_visible={r: np.arange(n) < r for r in rows})
    else:
        rows = range(n)
        m = np.ones(T, bool); m[T - 1] = False
        bad = dec.logits(toks, ck, cv, cross_visible={r: m for r in rows})
    rows = list(rows)
    ratio = float(np.sqrt(np.mean((bad[rows] - lf[rows]) ** 2)) / np.sqrt(np.mean((lr[rows] - lf[rows]) ** 2)))
    print(f"\n{mistake} at every position: rms(mistake - f64) / rms(port - f64) = {ratio:.2f} (sweep limit {SWEEP_LIMIT})")
    assert ratio >= at_least, (mistake, ratio)

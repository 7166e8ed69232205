"""-m gpu: every hand-written form of the decoder's attention on crafted operands, against float64.

Cases, expectations and the one judge hold_case() come from tests/dec_attn_f64.py; tests/test_dec_attn_f64.py proves on the CPU that the judge
refuses the last valid cell dropped, cell n_kv counted, a slice's first key dropped, a slice's last key counted by the next slice too, a quarter
boundary key of the long form counted twice, slices combined with weight 1, a missing slice's stale partial, the next head's columns, the row stride ignored and the causal
mask off by one.  The launches go through wmi_selftest_attn_decoder / wmi_selftest_attn_cross (csrc/api.cpp), which call the launchers of
csrc/kernels.h and nothing below them:

  self-attention   self_attn_rows at 1 .. 448 cells (dec_attn_f64.SELF_CELLS: both pass counts of self_attn_wave, the barrier form behind 64
                   cells, k_self_attn_rows_long from 65 cells on with a partial last group in most quarters), 16 rows with a cache each, the selector over both
                   sides of every multiple of 8 and every quarter boundary; f16 and f32 (f16(out32) == out bit for bit); the out projection
                   with the sa_* prologue and an identity matrix (k_gemv1 per lock-step row and at one row) returns the same values; six (random:
                   twelve) lock-step rows of {1, 32, 33, 64, 65, 200} cells in one grid; full caches of 64 and 448 cells; 6, 8, 12, 16 and 20 heads
  k_attn_dec       one row at the same cell counts (n_kv by value and through device memory with n_kv_max = cap), 5 rows from n_past = 59, 60, 61,
                   200 and 448 rows from 0.  The random family needs 1024 elements per launch for its ratios: the one-row shapes run 8 rows under a
                   mask of zeros (2 cells: 2 rows of 8 heads), the 5-row prompts 4 heads; every k_attn_dec launch is ratio-judged
  cross-attention  T in dec_attn_f64.CROSS_T (1 .. 8 slices; 1344 / 1345: the last general combine and the first ns == 8 one; 768 and 1152
                   added for 4 and 6 slices), the selector over both sides of every slice and wavefront boundary: attn_cross_split, the
                   partials with k_xattn_combine, and with the comb_* prologue of k_gemv1 (one row, and per lock-step row), k_gemv (3 and 8
                   rows) and k_rows_mfma (S = 768, lock-step rows) — all bit-identical to each other; 6 and 8 heads at T = 1500; four lock-step rows
                   of {1500, 777, 193, 1} keys with a cache each: judged at their own length, bit-identical to the one-row launch at that
                   length, neutral partials in the slices a row does not have; the projection inside (S = 128, 768, 1280: NC = 1, 2, 3) with
                   a known query; the two-launch form (WMI_XATTN_TWO_PASS, read once per process) in a child process
Not covered: k_front and k_xback (held bit for bit to these launches by test_gpu_front_long.py / test_gpu_variants.py / test_gpu_flat_args.py)
and the block-quantised qattn_cross_qsplit_partials (k_quant.hip).

Worst measured ratios of the kernels' distance from float64 to attend_ref_points' own on the random family (MI355X; limits 1.5 rms, 2.0 max),
as (rms, max |d|):
    self_attn_wave (<= 64 cells)          1.026, 1.099     k_self_attn_rows barrier form   1.009, 1.000     k_self_attn_rows_long   1.009, 1.001
    sa_* prologue, lock-step rows         1.021, 1.000     sa_* prologue, one row (1 cell) 1.002, 1.000     k_attn_dec              1.010, 1.001
    cross: attn_cross_split / k_xattn_combine / comb_* of k_gemv and of k_gemv1 per lock-step row (bit-identical)      0.926, 1.015
    cross: lock-step rows with a length each  0.804, 0.799     comb_* of k_rows_mfma (S = 768)  0.804, 0.660
    cross: projection inside  0.872, 0.892 (lock-step rows 0.516, 0.729)     two launches  0.906, 1.000 (projection inside 0.800, 1.106)
(the self-attention forms and k_attn_dec ARE the reference's points up to the f32 summation order: ratios of 1; the cross forms round the
unnormalised numerator and never the normalised probability: one f16 rounding fewer).  No case missed a selector or a uniform bound and no
form measured above a limit: the cases found no kernel bug.

What is NOT ratio-judged on the random family: one-row launches of 128 elements — the one-row sa_* prologue and the one-row cross launches —
which are compared bit for bit with the same row of a judged launch of 8 rows instead (judge()); the rows of the lock-step launches taken
alone, likewise compared with the judged lock-step launch.  No test reads the reference checkout or oracle/_ref."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_f64 as af
import dec_attn_f64 as df
import stage_compare as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("selector", "uniform", "random")

self_cases = functools.lru_cache(maxsize=None)(lambda *a, **kw: tuple(df.self_cases(*a, **kw)))
dec_row_cases = functools.lru_cache(maxsize=None)(lambda *a, **kw: tuple(df.dec_row_cases(*a, **kw)))
dec_prompt_cases = functools.lru_cache(maxsize=None)(lambda *a, **kw: tuple(df.dec_prompt_cases(*a, **kw)))
cross_cases = functools.lru_cache(maxsize=None)(lambda *a, **kw: tuple(df.cross_cases(*a, **kw)))
cross_lockstep_cases = functools.lru_cache(maxsize=None)(lambda *a, **kw: tuple(df.cross_lockstep_cases(*a, **kw)))
self_lockstep_cases = functools.lru_cache(maxsize=None)(lambda *a, **kw: tuple(df.self_lockstep_cases(*a, **kw)))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def hold(kind, measured, limit, what=None):
    print(f"{measured:7.3f} of {limit:g}  {kind}  [{what}]")
    sc.hold(kind, measured, limit, what)


def judge(c, raw, want_f32, label, partials=None, tied=False):
    """hold_case().  The random family is ratio-judged on launches of at least 1024 elements (or of one key, where the result is exact), and a
    random launch with fewer that is not `tied` is an error of the test.  tied: the caller compares this ONE-ROW launch bit for bit with the
    same row of a judged launch of 8 rows; its own 128 elements are then held to the sentinel and finiteness only, because two heads are two
    draws of the rounding errors and the ratio of two such rms values scatters past any limit (the NumPy restatement of the one-launch
    cross form at T = 191, spread 1, gives 0.06 .. 1.92 over the eight rows taken alone and 0.35 pooled; the kernel measured 1.918 on the
    row where the restatement gives 1.9175).  Only two callers pass it: the one-row sa_* prologue in check_self() and the one-row cross
    launches of test_cross_attention().  Every k_attn_dec launch is ratio-judged."""
    few = c.family == "random" and c.n * c.S < 1024 and max(c.vis) > 1
    assert not few or (tied and c.n == 1), (c.name, "a random launch too small for its ratios, and tied to no judged launch")
    df.hold_case(c, raw, want_f32, label, (lambda *a, **kw: None) if few else hold, partials=partials)


# ---------------------------------------------------------------------------------------------- launches
def run_dec(lib, c, form, want_f32, via_dev=0):
    """form 0 attn_decoder, 1 self_attn_rows, 2 gemv with the sa_* prologue (f32)"""
    out = np.zeros((c.out_rows, c.S), np.uint32 if want_f32 else np.uint16)
    n_kv = np.asarray([c.n_past + c.n] if form == 0 else c.vis, np.int32)
    mask = c.mask() if form == 0 else None
    rc = lib.wmi_selftest_attn_decoder(0, form, c.n, c.S, c.H, c.cells, c.rows, _p(n_kv), _p(mask), via_dev, int(c.long_form and form == 1), int(want_f32),
                                       _p(c.q), _p(c.k), _p(c.v), af.SENTINEL32 if want_f32 else af.SENTINEL16, c.out_rows, _p(out))
    assert rc == 0, (rc, c.name, form, want_f32, via_dev)
    return out


def run_cross(lib, c, form, consumer=0, want_f32=False, lanes=0):
    """form 0 attn_cross_split, 1 partials + (consumer 0 k_xattn_combine, 1 gemv comb_*), 2 the projection inside + k_xattn_combine.
    Returns (out, (pmax, part_l, part_o, ns) or None, one-launch form?)"""
    out = np.zeros((c.out_rows, c.S), np.uint32 if want_f32 else np.uint16)
    pm = np.zeros((c.n, c.H, 16), np.float32); pl = np.zeros_like(pm); po = np.zeros((c.n, c.H, 16, 64), np.float32); info = np.zeros(2, np.int32)
    qscale = 1.0
    q = c.q
    if form == 2:
        qscale = 0.125
        q = c.q[0].astype(np.float32) * np.float32(8.0)          # the projection's bias; the effective query, computed the kernel's way:
        assert np.array_equal((q * np.float32(qscale)).astype(np.float16), c.q[0]) and all(np.array_equal(c.q[i], c.q[0]) for i in range(c.n))
    rl = np.asarray(c.vis, np.int32) if c.ragged else None
    rc = lib.wmi_selftest_attn_cross(0, form, consumer, c.n, c.S, c.H, c.cells, c.rows, _p(rl), int(want_f32), lanes, _p(q), C.c_float(qscale), _p(c.k), _p(c.v),
                                     af.SENTINEL32 if want_f32 else af.SENTINEL16, c.out_rows, _p(out), _p(pm), _p(pl), _p(po), _p(info))
    assert rc == 0, (rc, c.name, form, consumer, want_f32, lanes)
    ns = int(info[0])
    assert ns == df.xattn_plan(c.cells)[0]
    parts = None
    if form != 0:
        parts = (pm.reshape(-1)[:c.n * c.H * ns].reshape(c.n, c.H, ns), pl.reshape(-1)[:c.n * c.H * ns].reshape(c.n, c.H, ns),
                 po.reshape(-1)[:c.n * c.H * ns * 64].reshape(c.n, c.H, ns, 64), ns)
    return out, parts, bool(info[1])


def f16_image(raw32, n):
    """the f32 result of an identity out projection as the f16 image hold_case() takes: every value must BE an f16 value"""
    assert (raw32[n:] == af.SENTINEL32).all(), "rows behind the launch's rows were written"
    vals = raw32[:n].view(np.float32)
    assert np.isfinite(vals).all()
    h = vals.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), vals), "the identity out projection returned something that is no f16 value"
    out = np.full(raw32.shape, af.SENTINEL16, np.uint16)
    out[:n] = h.view(np.uint16)
    return out


def same_values(a16, b16, n, what):
    """two f16 images agree in every VALUE (the identity projection's sum turns -0 into +0)"""
    a, b = a16[:n].view(np.float16).astype(np.float32), b16[:n].view(np.float16).astype(np.float32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, (what, "first (row, column)", tuple(bad[0]), len(bad))


def rounds_to(out32, out16, n, what):
    r16 = out32[:n].view(np.float32).astype(np.float16).view(np.uint16)
    bad = np.argwhere(r16 != out16[:n])
    assert bad.size == 0, (what, "f16(out32) != out at (row, column)", tuple(bad[0]), len(bad))


# ---------------------------------------------------------------------------------------------- self-attention
def check_self(lib, c, label, prologue=True):
    o16 = run_dec(lib, c, 1, False); judge(c, o16, False, label)
    o32 = run_dec(lib, c, 1, True); judge(c, o32, True, label)
    rounds_to(o32, o16, c.n, (label, c.name))
    if prologue:                                             # the out projection with the attention in its prologue: the same values
        rows = f16_image(run_dec(lib, c, 2, True), c.n)
        judge(c, rows, False, "sa_* prologue, lock-step rows")
        same_values(rows, o16, c.n, (c.name, "sa_* prologue (lock-step rows) against self_attn_rows"))
        for i in sorted({0, c.n - 1}):
            one = c.one_row(i)
            alone = f16_image(run_dec(lib, one, 2, True), 1)
            judge(one, alone, False, "sa_* prologue, one row", tied=True)
            same_values(alone, o16[i:i + 1], 1, (c.name, f"sa_* prologue at one row against row {i} of self_attn_rows"))
    return o16


def form_label(c):
    return "k_self_attn_rows_long" if c.long_form else "self_attn_wave" if max(c.vis) <= 64 else "k_self_attn_rows barrier form" if min(c.vis) > 64 else "k_self_attn_rows mixed"


# the long form is launched where the host knows a row has more than 64 cells (kernels.h); rows of 64 cells or fewer meet it only beside such
# a row: the lock-step case below
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cells,long_form", [(c, False) for c in df.SELF_CELLS] + [(c, True) for c in df.SELF_CELLS if c > 64])
def test_self_attention_rows(product_lib, cells, long_form, family):
    for c in self_cases(family, cells, long_form=long_form):
        check_self(product_lib, c, form_label(c), prologue=not long_form)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("long_form", [False, True], ids=["short", "long"])
def test_self_attention_lockstep_rows_of_every_form_in_one_grid(product_lib, long_form, family):
    for c in self_lockstep_cases(family, long_form=long_form):
        o16 = check_self(product_lib, c, form_label(c), prologue=not long_form)
        for i in (0, 2, c.n - 1):                             # each row is what a launch of its own writes
            if long_form and c.vis[i] <= 64:
                continue                                      # (alone, such a row never takes the long form)
            same_values(run_dec(product_lib, c.one_row(i), 1, False), o16[i:i + 1], 1, (c.name, f"row {i} alone"))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cap,long_form", [(64, False), (448, False), (448, True)])
def test_self_attention_full_cache(product_lib, cap, long_form, family):
    for c in self_cases(family, cap, cap=cap, long_form=long_form):
        check_self(product_lib, c, form_label(c), prologue=not long_form)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cells", df.HEAD_CELLS)
@pytest.mark.parametrize("H", df.HEADS)
def test_self_attention_head_counts(product_lib, H, cells, family):
    """the wave routine's heads per wavefront (2, 2, 3, 4, 5) and its FAST / masked reductions change with H"""
    for c in self_cases(family, cells, H=H, rows=4, limit=2):
        check_self(product_lib, c, form_label(c))
    if cells > 64:
        for c in self_cases(family, cells, H=H, rows=4, limit=1, long_form=True):
            check_self(product_lib, c, form_label(c), prologue=False)


# ---------------------------------------------------------------------------------------------- k_attn_dec
def check_dec(lib, c):
    got = {}
    for via_dev in (0, 1):
        for want_f32 in (False, True):
            o = run_dec(lib, c, 0, want_f32, via_dev)
            judge(c, o, want_f32, "k_attn_dec")
            got[(via_dev, want_f32)] = o
    assert np.array_equal(got[(0, False)], got[(1, False)]) and np.array_equal(got[(0, True)], got[(1, True)]), (c.name, "n_kv by value and through device memory differ")
    rounds_to(got[(0, True)], got[(0, False)], c.n, c.name)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cells", df.SELF_CELLS)
def test_attn_dec_one_row(product_lib, cells, family):
    for c in dec_row_cases(family, cells):
        check_dec(product_lib, c)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,n_past", df.DEC_PROMPTS)
def test_attn_dec_prompt_rows(product_lib, n, n_past, family):
    for c in dec_prompt_cases(family, n, n_past, cap=448 if n < 448 else None):
        check_dec(product_lib, c)


# ---------------------------------------------------------------------------------------------- cross-attention
def check_cross(lib, c, consumers=True, tied=False):
    """attn_cross_split and the partials with every consumer the launch's shape reaches; returns the f16 image.  In the one-launch form all of
    them combine the same partials with the same operations: bit-identical.  tied: see judge() — the caller compares the returned image
    with a row of a judged launch."""
    o16, _, fused = run_cross(lib, c, 0, want_f32=False); judge(c, o16, False, "cross, attn_cross_split", tied=tied)
    o32, _, _ = run_cross(lib, c, 0, want_f32=True); judge(c, o32, True, "cross, attn_cross_split", tied=tied)
    rounds_to(o32, o16, c.n, c.name)
    p16, parts, _ = run_cross(lib, c, 1, 0, False); judge(c, p16, False, "cross, partials + k_xattn_combine", partials=parts, tied=tied)
    p32, _, _ = run_cross(lib, c, 1, 0, True); judge(c, p32, True, "cross, partials + k_xattn_combine", tied=tied)
    assert np.array_equal(p16, o16) and np.array_equal(p32, o32), (c.name, "the partials' combine differs from attn_cross_split")
    if consumers:
        kinds = [(0, "k_gemv1" if c.n == 1 else "k_gemv")] if c.n <= 8 else []
        if c.n >= 2:
            kinds.append((1, "k_gemv1 per lock-step row" if c.S <= 512 else "k_rows_mfma"))
        for lanes, name in kinds:
            g = f16_image(run_cross(lib, c, 1, 1, True, lanes=lanes)[0], c.n)
            judge(c, g, False, f"cross, comb_* prologue of {name}", tied=tied)
            same_values(g, o16, c.n, (c.name, f"comb_* prologue of {name} against k_xattn_combine"))
    return o16


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T", df.CROSS_T)
def test_cross_attention(product_lib, T, family):
    for c in cross_cases(family, T):                          # 8 rows: k_gemv, k_gemv1 per lock-step row
        o16 = check_cross(product_lib, c)
        one = c.one_row(0)                                    # one row: k_gemv1
        same_values(check_cross(product_lib, one, tied=True), o16[:1], 1, (c.name, "row 0 alone"))
    if family != "random":                                    # three rows: k_gemv<3> (the random family always takes 8 rows: the launches above)
        for c in cross_cases(family, T, n=3, limit=1):
            check_cross(product_lib, c)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("H", [6, 8])
def test_cross_attention_head_counts(product_lib, H, family):
    for c in cross_cases(family, 1500, n=3, H=H, limit=2):
        check_cross(product_lib, c)


@pytest.mark.parametrize("family", FAMILIES)
def test_cross_attention_lockstep_rows_with_a_length_each(product_lib, family):
    lib = product_lib
    for c in cross_lockstep_cases(family):
        assert c.ragged and c.rows == c.n
        p16, parts, fused = run_cross(lib, c, 1, 0, False)
        assert fused
        judge(c, p16, False, "cross, lock-step rows + k_xattn_combine", partials=parts)
        p32, parts32, _ = run_cross(lib, c, 1, 0, True)
        judge(c, p32, True, "cross, lock-step rows + k_xattn_combine", partials=parts32)
        g = f16_image(run_cross(lib, c, 1, 1, True, lanes=1)[0], c.n)
        same_values(g, p16, c.n, (c.name, "comb_* prologue of k_gemv1 per lock-step row"))
        if c.n <= 8:
            g = f16_image(run_cross(lib, c, 1, 1, True, lanes=0)[0], c.n)
            same_values(g, p16, c.n, (c.name, "comb_* prologue of k_gemv"))
        for i in range(min(c.n, 4)):                          # each row at its own length IS the one-row launch at that length
            one = c.one_row(i)
            a16, _, _ = run_cross(lib, one, 1, 0, False); a32, _, _ = run_cross(lib, one, 1, 0, True)
            assert np.array_equal(a16[:1], p16[i:i + 1]) and np.array_equal(a32[:1], p32[i:i + 1]), (c.name, f"row {i} differs from its one-row launch at T = {c.vis[i]}")


@pytest.mark.parametrize("family", FAMILIES)
def test_cross_attention_lockstep_rows_on_the_matrix_cores(product_lib, family):
    """S = 768: the lock-step out projection with the comb_* prologue is k_rows_mfma"""
    for c in df.cross_lockstep_cases(family, lens=(385, 193, 97, 1), H=12)[:3]:
        p16, parts, _ = run_cross(product_lib, c, 1, 0, False)
        judge(c, p16, False, "cross, lock-step rows + k_xattn_combine", partials=parts)
        g = f16_image(run_cross(product_lib, c, 1, 1, True, lanes=1)[0], c.n)
        judge(c, g, False, "cross, comb_* prologue of k_rows_mfma")
        same_values(g, p16, c.n, (c.name, "comb_* prologue of k_rows_mfma against k_xattn_combine"))
    for c in cross_cases(family, 1500, n=8, H=12, limit=1):   # ns == 8
        p16, _, _ = run_cross(product_lib, c, 1, 0, False)
        judge(c, p16, False, "cross, partials + k_xattn_combine")
        same_values(f16_image(run_cross(product_lib, c, 1, 1, True, lanes=1)[0], c.n), p16, c.n, (c.name, "k_rows_mfma, ns == 8"))
        same_values(f16_image(run_cross(product_lib, c, 1, 1, True, lanes=0)[0], c.n), p16, c.n, (c.name, "k_gemv, ns == 8"))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("H,T", [(2, 385), (2, 1500), (12, 385), (20, 193)])
def test_cross_attention_with_the_projection_inside(product_lib, H, T, family):
    """k_xattn_fused<NC, true> at NC = 1, 2, 3 with a known query (one for all rows; a cache per row): judged, and bit-identical to the launch
    that is handed the same query as f16"""
    for c in cross_cases(family, T, n=3, H=H, same_q=True, limit=2):
        for want_f32 in (False, True):
            o, parts, _ = run_cross(product_lib, c, 2, 0, want_f32)
            judge(c, o, want_f32, "cross, projection inside + k_xattn_combine", partials=parts)
            plain, pparts, _ = run_cross(product_lib, c, 1, 0, want_f32)
            assert np.array_equal(o, plain), (c.name, "differs from the launch with the query as f16")
            assert all(np.array_equal(a, b) for a, b in zip(parts[:3], pparts[:3]))
    if H == 2 and T == 1500:
        for c in df.cross_lockstep_cases(family, same_q=True)[:2]:
            o, parts, _ = run_cross(product_lib, c, 2, 0, True)
            judge(c, o, True, "cross, projection inside, lock-step rows", partials=parts)


# ---------------------------------------------------------------------------------------------- the two-launch form: a process of its own
_TWO_PASS = r"""
import json, sys
sys.path.insert(0, ROOT_PLACEHOLDER); sys.path.insert(0, ROOT_PLACEHOLDER + "/tests")
import __graft_entry__ as entry
entry.load_package()
import numpy as np
from godot_whisper_amd import runtime
import dec_attn_f64 as df
import test_gpu_attn_decoder as t
lib = runtime.require_gpu(); runtime.silence_logs(lib)
worst = {}
def hold(kind, measured, limit, what=None):
    assert measured <= limit, (kind, what, measured, limit)
    if measured >= worst.get(kind, (-1.0,))[0]: worst[kind] = (measured, limit, str(what)[:80])
t.hold = hold
outs = {}
for T in (193, 777, 1500):
    for family in t.FAMILIES:
        for j, c in enumerate(df.cross_cases(family, T)):
            o16, _, fused = t.run_cross(lib, c, 0, want_f32=False)
            assert not fused, "WMI_XATTN_TWO_PASS did not select the two-launch form"
            o32, _, _ = t.run_cross(lib, c, 0, want_f32=True)
            df.hold_case(c, o16, False, "cross, two launches", hold); df.hold_case(c, o32, True, "cross, two launches", hold)
            t.rounds_to(o32, o16, c.n, c.name)
            p32, parts, _ = t.run_cross(lib, c, 1, 0, True)
            assert np.array_equal(p32, o32)
            g = t.f16_image(t.run_cross(lib, c, 1, 1, True, lanes=0)[0], c.n)      # the ns == 8 and the general branch without slice maxima
            t.same_values(g, o16, c.n, (c.name, "comb_* prologue of k_gemv, two launches"))
            g = t.f16_image(t.run_cross(lib, c.one_row(0), 1, 1, True, lanes=0)[0], 1)
            t.same_values(g, o16[:1], 1, (c.name, "comb_* prologue of k_gemv1, two launches"))
            if family != "random": outs["%d/%s/%d" % (T, family, j)] = o32[:c.n].view(np.float32)
        for c in df.cross_cases(family, T, n=3, same_q=True, limit=1):             # k_xattn_qscores
            q32, _, fused = t.run_cross(lib, c, 2, 0, True)
            assert not fused
            df.hold_case(c, q32, True, "cross, two launches, projection inside", hold)
np.savez(sys.argv[1], **outs)
print("RESULT" + json.dumps(worst))
""".replace("ROOT_PLACEHOLDER", repr(ROOT))


def test_the_two_launch_form_in_a_process_of_its_own(product_lib, tmp_path):
    env = dict(os.environ); env["WMI_XATTN_TWO_PASS"] = "1"
    path = str(tmp_path / "two_pass.npz")
    r = subprocess.run([sys.executable, "-c", _TWO_PASS, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    worst = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][-1][len("RESULT"):])
    assert len(worst) == 4, worst
    for kind, (measured, limit, what) in worst.items():
        hold(kind, measured, limit, what)
    # selector and uniform: the two forms agree within the families' bounds (on the random family they are different arithmetics,
    # each judged against float64 on its own)
    two = np.load(path)
    for T in (193, 777, 1500):
        for family in ("selector", "uniform"):
            for j, c in enumerate(cross_cases(family, T)):
                one = run_cross(product_lib, c, 0, want_f32=True)[0][:c.n].view(np.float32).astype(np.float64)
                d = np.abs(one - two[f"{T}/{family}/{j}"].astype(np.float64))
                lim = 2 * (2.0 ** -30 if family == "selector" else c.uniform_bound(True))
                assert (d <= lim).all(), (c.name, float(d.max()))

"""-m gpu: the encoder self-attention kernels and the q|k|v projection's split epilogue on crafted operands, against float64.

The attention kernels — k_attn_enc2<4,1,*> and <2,4,*> (csrc/k_attn_enc.hip: one sweep with a running maximum = form 2, exact maximum first =
form 1; one or four key groups) and k_attn_enc<4,1> / <4,2> (csrc/k_attn.hip: form 0, one or two key groups) — run through
wmi_selftest_attn_encoder, which names the form and the key-group choice itself (attn_encoder_form; the product's attn_encoder() is that
function with the environment's form and its own rule's answer).  The EPI_QKV_ENC epilogue (csrc/gemm_epi.h, with epilogue_vt_wide) runs
through wmi_selftest_qkv_encoder.  Cases, expectations and the judge hold_case() / hold_qkv() come from tests/attn_f64.py;
tests/test_attn_f64.py proves on the CPU that hold_case() refuses a padded key counted, the last key dropped, the V^T order without its bit
swap, the next head's columns, the next chunk's rows and a row stored at a chunk's length.

  one chunk, one key group    forms 2, 1, 0 at T in {1, 33, 64, 65, 129, 200}: selector, uniform and random (three score spreads), f16 and f32
  one chunk, split            forms 2, 1 at T in {513 (fourth group empty, last tile one key), 563, 576 (no padding), 641 (a tile wholly
                              past T, its V^T start clamped)}; form 0 with two groups at {257, 563}
  T = 1500                    the product's own launch (groups = -1, form 2), selector and uniform
  the product's decision      groups = -1 at T = 200 / 563 is bit for bit the explicit choice the rule names
  a head count of 5           S = 320, one group at T = 200 and split at T = 563
  several chunks              B = 3 uniform (qk_rows 576, out_rows 570) and B = 4 with lengths {641, 513, 200, 80} (qk_rows 656, out_rows 650,
                              Tpad 704), one group and split: per chunk the family's expectation at the chunk's OWN length, rows
                              [T_chunk, out_rows) still the sentinel, and the bytes of the one-chunk launch of the same form and group choice
                              at that length — wherever such a launch exists: the split forms refuse a single chunk below 512 (form 0: 256)
                              frames, so chunks of 200 and 80 frames under the split kernels are held by their expectations alone
  f32 against f16             f16(out32) == out bit for bit on every random case above
  q|k|v epilogue              exact operands at one chunk (M = 563), three chunks and eight chunks (M = 4608: the other orientation and tile
                              choice) of 576 rows, and one chunk into a Tpad of 640: q, k bit for bit, V^T through vt_pos, padding columns
                              finite up to the 16-step block, the sentinel everywhere else; normal operands at three chunks within
                              ulp/2 + K 2^-24 sum|a||w|

The selector's f16 result is compared as VALUES (a zero of either sign): with the one-sweep form the numerators of the keys seen before the
match leave a remainder scaled by e^-40 or less, whose sign a rounding to zero keeps.

THE BUG THESE CASES FOUND (fixed in csrc/k_attn_enc.hip): the selector family's f32 bound |d| <= 2^-30 was missed by the one-sweep form
(form 2) at T = 129, 200, 513, 563, 576, 641 and 1500, with five heads and in the four-chunk launches: max |d| 2.38e-07 = 2^-22, 35 of
16 512 elements at T = 129, 111 of 25 600 at T = 200, every one of them exactly |d| = 2^-24 |v| at a POSITIVE power of two v.  Cause, found
by restating the sweep on the CPU (the set of wrong elements was predicted exactly, 35 / 35 and 111 / 111): the keys seen before the match
left a remainder r = o alpha, |r| ~ 1e-37 .. 1e-25, in the accumulator the P.V MFMA (v_mfma_f32_32x32x16_f16) then adds v to.  The matrix
pipe aligns its addends by an arithmetic shift: a NEGATIVE addend far below the sum's last bit counts as minus one internal unit instead of
zero, and v - unit rounds to the next f32 below v when v = +2^k (where the spacing below is half the spacing above).  The exact-maximum forms
(1, 0) add v to a zero accumulator and were exact.  The fix: when the running maximum rises by more than 17.5, every key seen so far has a
numerator below 2^-25 relative to the new maximum — zero in f16, dropped by the reference and by the two-sweep forms — and the one-sweep
form now drops them too (alpha = 0) instead of carrying e^-17.5 or less of them along.

Worst measured ratios of the kernels' distance from float64 to attend_ref_points' own on the random family (MI355X; limits 1.5 rms, 2.0 max),
as (rms, max |d|):
    form 2   one key group 0.852, 1.024     split (four key groups) 0.813, 0.980
    form 1   one key group 0.904, 1.024     split (four key groups) 0.904, 1.000
    form 0   one key group 0.904, 1.024     split (two key groups)  0.904, 1.000
(the kernels round the unnormalised numerator and never the normalised probability: one f16 rounding fewer than the reference)

No test reads the reference checkout or oracle/_ref."""
import ctypes as C
import functools

import numpy as np
import pytest

import attn_f64 as af
import stage_compare as sc

pytestmark = pytest.mark.gpu

FORMS = (2, 1, 0)
FAMILIES = (("selector", 1.0), ("uniform", 1.0), ("random", 0.25), ("random", 1.0), ("random", 4.0))


@functools.lru_cache(maxsize=None)
def case(family, lens, spread=1.0, H=2, Tpad=None, qk_rows=None, out_rows=None, ragged=None):
    return af.make_case(family, list(lens) if isinstance(lens, tuple) else lens, Tpad=Tpad, H=H, qk_rows=qk_rows, out_rows=out_rows,
                        ragged=ragged, spread=spread)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def launch(lib, c, form, groups, want_f32):
    out = np.zeros((c.B, c.out_rows, c.S), np.uint32 if want_f32 else np.uint16)
    rt = np.asarray(c.lens, np.int32) if c.ragged else None
    q, k, v = (np.ascontiguousarray(a) for a in (c.q, c.k, c.v))
    rc = lib.wmi_selftest_attn_encoder(0, c.B, c.T, c.Tpad, c.S, c.H, c.qk_rows, c.out_rows, _p(rt), int(want_f32), form, groups,
                                       _p(q), _p(k), _p(v), af.SENTINEL32 if want_f32 else af.SENTINEL16, _p(out))
    assert rc == 0, (rc, c.name, form, groups, want_f32)
    return out


def hold(kind, measured, limit, what=None):
    print(f"{measured:7.3f} of {limit:g}  {kind}  [{what}]")
    sc.hold(kind, measured, limit, what)


def check(lib, c, form, groups, before_f32=None):
    """both result types through hold_case(), the f16 one first; on the random family the f32 result rounds to the f16 one bit for bit"""
    label = f"form {form}, {'one key group' if groups == 0 else 'split' if groups == 1 else 'own decision'}"
    got = {want_f32: launch(lib, c, form, groups, want_f32) for want_f32 in (False, True)}
    af.hold_case(c, got[False], False, label, hold)
    if c.family == "random":
        for b, Tb in enumerate(c.lens):
            r16 = got[True][b, :Tb].view(np.float32).astype(np.float16).view(np.uint16)
            bad = np.argwhere(r16 != got[False][b, :Tb])
            assert bad.size == 0, (label, c.name, "f16(out32) != out at (row, column)", tuple(bad[0]), len(bad))
    if before_f32:
        before_f32(got)
    af.hold_case(c, got[True], True, label, hold)
    return got


def cases_of(family, T, H=2, **kw):
    return [case(f, T, spread=s, H=H, **kw) for f, s in FAMILIES if f == family]


FAMILY_NAMES = ("selector", "uniform", "random")


# ---------------------------------------------------------------------------------------------- one chunk
@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("T", [1, 33, 64, 65, 129, 200])
@pytest.mark.parametrize("form", FORMS)
def test_one_chunk_one_key_group(product_lib, form, T, family):
    for c in cases_of(family, T):
        check(product_lib, c, form, 0)


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("form,T", [(f, T) for f in (2, 1) for T in (513, 563, 576, 641)] + [(0, 257), (0, 563)])
def test_one_chunk_split(product_lib, form, T, family):
    for c in cases_of(family, T):
        check(product_lib, c, form, 1)


@pytest.mark.parametrize("family", ["selector", "uniform"])
def test_full_length_the_products_own_launch(product_lib, family):
    check(product_lib, case(family, 1500), 2, -1)


@pytest.mark.parametrize("T,split", [(200, {2: 0, 1: 0, 0: 0}), (563, {2: 1, 1: 1, 0: 1})])
@pytest.mark.parametrize("form", FORMS)
def test_own_decision_is_the_choice_the_rule_names(product_lib, form, T, split):
    """attn_encoder_splits: the second form splits when ceil(T / 128) H B < 512 and T >= 512, the first when ceil(T / 64) H B <= 512 and
    T >= 256: at H = 2, one chunk, T = 200 is one key group in every form and T = 563 is split in every form."""
    c = case("random", T)
    for want_f32 in (False, True):
        own = launch(product_lib, c, form, -1, want_f32)
        named = launch(product_lib, c, form, split[form], want_f32)
        other = launch(product_lib, c, form, 1 - split[form], want_f32) if T >= 512 else None
        assert np.array_equal(own, named), (form, T, want_f32)
        if other is not None and want_f32:
            assert not np.array_equal(own, other), "the two key-group choices do not differ on these operands: the comparison above says nothing"


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_five_heads(product_lib, form, family):
    for c in cases_of(family, 200, H=5):
        check(product_lib, c, form, 0)
    if family != "uniform":
        check(product_lib, case(family, 563, H=5), form, 1)


# ---------------------------------------------------------------------------------------------- several chunks
def chunks_check(lib, c, form, groups):
    floor = 0 if groups == 0 else 256 if form == 0 else 512

    def same_bytes_as_alone(got):
        compared = 0
        for b, Tb in enumerate(c.lens):
            if Tb < floor:
                continue                                      # no one-chunk launch of this form and group choice exists at this length
            one = c.one_chunk(b)
            for want_f32 in (False, True):
                alone = launch(lib, one, form, groups, want_f32)
                bad = np.argwhere(alone[0] != got[want_f32][b])
                assert bad.size == 0, (c.name, form, groups, want_f32, f"chunk {b} (T = {Tb}) differs from its one-chunk launch at (row, column)", tuple(bad[0]), len(bad))
            compared += 1
        assert compared >= (len(c.lens) if groups == 0 else 2)

    check(lib, c, form, groups, before_f32=same_bytes_as_alone)


@pytest.mark.parametrize("groups", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_three_chunks_of_one_length(product_lib, form, groups):
    chunks_check(product_lib, case("uniform", (563, 563, 563), qk_rows=576, out_rows=570), form, groups)


@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("groups", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_four_chunks_each_with_its_own_length(product_lib, form, groups, family):
    c = case(family, (641, 513, 200, 80), Tpad=704, qk_rows=656, out_rows=650)
    assert c.ragged
    chunks_check(product_lib, c, form, groups)


# ---------------------------------------------------------------------------------------------- the q|k|v epilogue
def run_qkv(lib, c):
    out_rows = c.M + 16
    q = np.zeros((out_rows, c.S), np.uint16); k = np.zeros_like(q); vt = np.zeros((c.chunks, c.S, c.Tpad), np.uint16)
    rc = lib.wmi_selftest_qkv_encoder(0, c.M, c.S, c.Tpad, c.rows_per_chunk, _p(c.xn.view(np.uint16)), _p(c.W.view(np.uint16)), _p(c.bias),
                                      af.SENTINEL16, out_rows, _p(q), _p(k), _p(vt))
    assert rc == 0, (rc, c.name)
    af.hold_qkv(c, q, k, vt, out_rows)


@pytest.mark.parametrize("chunks", [0, 3, 8])
def test_qkv_epilogue_exact_operands(product_lib, chunks):
    run_qkv(product_lib, af.make_qkv_case(chunks))


def test_qkv_epilogue_leaves_the_padding_behind_the_last_block_alone(product_lib):
    run_qkv(product_lib, af.make_qkv_case(0, Tpad=640))
    run_qkv(product_lib, af.make_qkv_case(2, Tpad=640))


def test_qkv_epilogue_normal_operands(product_lib):
    run_qkv(product_lib, af.make_qkv_case(3, exact=False))

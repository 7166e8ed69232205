"""-m gpu: the frame-energy kernel (csrc/k_segment.hip) against its definition (tests/segment_f64.py), bit for bit.

    e[f] = sum over i in [160 f, min(160 f + 160, n)) of | x[i] - x[i-1] |,  x[-1] := 0  — f32, the sum left to right from 0.0f

Sizes: one sample, both sides of one and two frames, both sides of the kernel's staging extent (where a frame's predecessor sample belongs
to the previous workgroup), three extents and a partial frame, and 480 007 samples.  Three input families: seeded noise; denormals, signed
zeros and unit steps; and one whose sequential f32 sum differs from any pairwise sum (one term of 4096 followed by 159 terms below half
an ulp of it).  tests/test_segment_f64.py::test_input_guards asserts on the CPU that these inputs separate a tree / butterfly reduction
and a zero read at a frame edge from the definition, and repeats it here for the inputs actually used.  The output is sentinel-filled; the
64 words behind the last frame must come back untouched."""
import numpy as np
import pytest

import segment_f64 as sj

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)


def _run(lib, x):
    n = x.size
    F = (n + sj.FRAME - 1) // sj.FRAME
    e = np.full(F + 64, SENTINEL, np.float32)
    assert lib.wmi_selftest_frame_energy(0, x.ctypes.data, n, e.ctypes.data) == 0
    assert (e[F:] == SENTINEL).all(), ("words behind the last frame were written", n)
    return e[:F]


@pytest.mark.parametrize("family", sj.FAMILIES)
def test_kernel_equals_the_definition(product_lib, family):
    stage = product_lib.wmi_long_stage_samples()
    assert stage % sj.FRAME == 0 and stage >= 2 * sj.FRAME
    for n in sj.sizes(stage):
        x = sj.make_input(family, n, seed=n % 1000 + 7)
        want = sj.energies(x)
        if family == "seqsum" and n >= 159:                  # a condition on the input: no tree reduction gives these bits
            assert (sj.energies_tree(x).view(np.uint32) != want.view(np.uint32)).any()
            assert (sj.energies_tree(x, butterfly=True).view(np.uint32) != want.view(np.uint32)).any()
        if n > stage:                                            # nor does a zero read at the hand-over between two workgroups
            k = stage // sj.FRAME
            assert sj.energies(x, edge_zero=True).view(np.uint32)[k] != want.view(np.uint32)[k]
        got = _run(product_lib, x)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (family, n, bad[:8], got[bad[:8]], want[bad[:8]])


def test_same_call_twice_and_argument_errors(product_lib):
    x = sj.make_input("noise", 48123, seed=3)
    assert _run(product_lib, x).tobytes() == _run(product_lib, x).tobytes()
    e = np.zeros(400, np.float32)
    assert product_lib.wmi_selftest_frame_energy(0, x.ctypes.data, 0, e.ctypes.data) == -1
    assert product_lib.wmi_selftest_frame_energy(0, None, 100, e.ctypes.data) == -1

"""Records what libsamplerate's src_simple returns for SRC_ZERO_ORDER_HOLD and SRC_LINEAR as DATA (resample_zoh_linear.npz):
per case the input's seed, length and rate, the converter, output_frames_gen, input_frames_used and the bits of the output frames.
Run where a checkout of the reference lies, never at test time:

    python tests/golden/make_resample_goldens.py <reference checkout>

It compiles thirdparty/libsamplerate/src/{samplerate.c, src_zoh.c, src_linear.c} of that checkout into a temporary directory
(cc -O2 -ffp-contract=off: every operation of the C source rounds on its own, as the product's build has it), with a stub of
three functions written here in place of src_sinc.c, whose best-quality table is a missing blob of the checkout, and calls
src_simple the way the host does (src/speech_to_text.cpp:16-43).  Nothing compiled is kept.  Cases and inputs:
tests/resample_ref.py (cases, make_input).
"""
import ctypes as C
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import resample_ref as rr  # noqa: E402

STUB = """
const char * sinc_get_name (int src_enum) { (void) src_enum ; return 0 ; }
const char * sinc_get_description (int src_enum) { (void) src_enum ; return 0 ; }
int sinc_set_converter (void * psrc, int src_enum) { (void) psrc ; (void) src_enum ; return 10 ; }   /* SRC_ERR_BAD_CONVERTER */
"""


class SRC_DATA(C.Structure):                                    # thirdparty/libsamplerate/src/samplerate.h:26-36
    _fields_ = [("data_in", C.c_void_p), ("data_out", C.c_void_p), ("input_frames", C.c_long), ("output_frames", C.c_long),
                ("input_frames_used", C.c_long), ("output_frames_gen", C.c_long), ("end_of_input", C.c_int), ("src_ratio", C.c_double)]


def build(ref: pathlib.Path, tmp: pathlib.Path):
    src = ref / "thirdparty" / "libsamplerate" / "src"
    stub = tmp / "sinc_stub.c"
    stub.write_text(STUB)
    so = tmp / "libsrc_simple.so"
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(src), "-DPACKAGE=\"libsamplerate\"", "-DVERSION=\"0\"",
                    "-DCPU_CLIPS_POSITIVE=0", "-DCPU_CLIPS_NEGATIVE=0", str(src / "samplerate.c"), str(src / "src_zoh.c"),
                    str(src / "src_linear.c"), str(stub), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.src_simple.restype = C.c_int
    lib.src_simple.argtypes = [C.POINTER(SRC_DATA), C.c_int, C.c_int]
    return lib


def run(lib, x, rate, converter):
    ratio, out_frames = rr.ratio_and_capacity(x.size, rate)
    guard = 16                                                   # a marked frame either side: the converter must leave them alone
    buf = np.full(out_frames + 2 * guard, np.float32(12345.0), np.float32)
    xin = np.ascontiguousarray(x, np.float32).copy()
    d = SRC_DATA(xin.ctypes.data if xin.size else None, buf[guard:].ctypes.data, xin.size, out_frames, 0, 0, 0, ratio)
    err = lib.src_simple(C.byref(d), converter, 1)
    assert err == 0, (x.size, rate, converter, err)
    gen, used = int(d.output_frames_gen), int(d.input_frames_used)
    assert 0 <= gen <= out_frames and np.all(buf[:guard] == 12345.0) and np.all(buf[guard + gen + (out_frames - gen):] == 12345.0)
    return buf[guard:guard + gen].copy(), used


def main():
    ref = pathlib.Path(sys.argv[1])
    with tempfile.TemporaryDirectory() as t:
        lib = build(ref, pathlib.Path(t))
        cols = {k: [] for k in ("seed", "length", "rate", "converter", "frames_gen", "frames_used")}
        outs, offset = [], [0]
        for seed, n, rate, conv in rr.cases():
            out, used = run(lib, rr.make_input(seed, n), rate, conv)
            for k, v in zip(cols, (seed, n, rate, conv, out.size, used)):
                cols[k].append(v)
            outs.append(out.view(np.uint32))
            offset.append(offset[-1] + out.size)
        del lib
    np.savez_compressed(rr.FIXTURE, out_bits=np.concatenate(outs).astype("<u4"), offset=np.asarray(offset, np.int64),
                        **{k: np.asarray(v, np.int64) for k, v in cols.items()})
    print(rr.FIXTURE.name, len(offset) - 1, "cases,", offset[-1], "frames,", rr.FIXTURE.stat().st_size, "bytes")


if __name__ == "__main__":
    main()

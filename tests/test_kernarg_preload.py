"""The hot path's kernels get their leading arguments in SGPRs at wavefront launch (csrc/Makefile: -amdgpu-kernarg-preload-count).

hipcc preloads leading pointer and scalar parameters only: a by-value struct in front gets nothing.  So the kernels of the decode step and
the f16 GEMMs take the operands of their first loads as plain leading parameters, followed by the by-value struct with the rest.  This
test reads the kernel descriptors of the gfx950 code objects inside the built library (the toolchain's llvm-readelf to find the fat binary,
llvm-objdump to decode the descriptors in .rodata; descriptor fields only, no instructions) and holds

  * every kernel of HOT (the launches of one whisper_full call on base.en, by the identifier in their mangled name) to a non-zero
    preload length, and
  * the flattened kernels (k_gemm8 is not among them: it keeps its by-value struct, csrc/gemm_epi.h) to the dwords of their leading parameters, padding included, capped at what the toolchain grants
    (GRANTED = 14 of the 16 user SGPRs: two hold the argument segment's address).

A pointer takes two dwords on an 8-byte boundary and is preloaded whole or not at all, which is why k_xattn_fused stops at 13.
The numbers below are this build's (hipcc 7.2)."""
import pathlib
import re
import shutil
import struct
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
LIB = ROOT / "godot-whisper_amd" / "libwhisper_mi355.so"
LLVM = pathlib.Path("/opt/rocm/llvm/bin")
GRANTED = 14

# identifier (as it stands in the mangled name, length prefix included) -> dwords of the leading parameters
FLAT = {
    # x, ln_g, ln_b, Wqkv, ck, cv (6 pointers = 12), dims = S | par << 15 | stamp bit, cap
    "7k_frontI": 14,
    # xio, ln_g, ln_b, W1, W2, epoch (12), dims = S | par << 15 | G << 16 | stamp bit
    "10k_mlp_pairI": 13,
    # x, ln_g, ln_b, wq, kc, vc (12), dims = S | par << 15 | ns << 16 | stamp bit, keys_tk = T | ks << 16
    "7k_xbackE": 14,
    # x32, ln_g, ln_b, a16, W, bias (12), dims = K | N << 13 | lock-step bit | stamp bit
    "7k_gemv1I": 13,
    # A, W, probe (6), lda, ldw, M, N, K, no_glds, S (7)
    "6k_gemmI": 13,
    # part (2), nparts, a hole, stp, out, out_host (6), the stamp's base (2) and slot — in front of the by-value ChainNext
    "13k_filter_pickI": 13,
}
# flat before this change: x32, ln_g, ln_b (6), eps, a hole, wq, bq (4), qscale = 13; q16 (a pointer behind a hole) would end at 16
ALREADY_FLAT = {"13k_xattn_fusedI": 13}
HOT = list(FLAT) + list(ALREADY_FLAT) + ["16k_dec_embed_stepE", "11k_layernormI", "10k_attn_encI",
                                          "9k_mel_padE", "12k_mel_framesE", "15k_mel_normalizeE", "11k_mel_sliceE"]


def _tools():
    readelf, objdump = LLVM / "llvm-readelf", LLVM / "llvm-objdump"
    if not (readelf.exists() and objdump.exists()):
        readelf, objdump = shutil.which("llvm-readelf"), shutil.which("llvm-objdump")
    if not (readelf and objdump):
        pytest.skip("llvm-readelf / llvm-objdump not found")
    return str(readelf), str(objdump)


def _code_objects(readelf, tmp_path):
    """the gfx950 entries of the clang offload bundles in .hip_fatbin, one file each"""
    out = subprocess.run([readelf, "-S", "--wide", str(LIB)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"\.hip_fatbin\s+PROGBITS\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)", out)
    assert m, "no .hip_fatbin section in the library"
    off, size = int(m.group(1), 16), int(m.group(2), 16)
    fat = LIB.read_bytes()[off:off + size]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    files, at = [], fat.find(magic)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", fat, at + len(magic))
        p = at + len(magic) + 8
        for _ in range(count):
            e_off, e_size, t_size = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24:p + 24 + t_size].decode()
            p += 24 + t_size
            if triple.endswith("gfx950") and e_size:
                f = tmp_path / f"co{len(files)}.elf"
                f.write_bytes(fat[at + e_off:at + e_off + e_size])
                files.append(f)
        at = fat.find(magic, at + len(magic))
    assert files, "no gfx950 code object in the library"
    return files


@pytest.fixture(scope="module")
def preload_lengths(tmp_path_factory):
    if not LIB.exists():
        pytest.skip("the library is not built")
    readelf, objdump = _tools()
    lengths = {}
    for f in _code_objects(readelf, tmp_path_factory.mktemp("co")):
        text = subprocess.run([objdump, "-D", "-j", ".rodata", str(f)], check=True, capture_output=True, text=True).stdout
        for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
            m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", body)
            lengths[name] = int(m.group(1)) if m else 0
    assert len(lengths) > 100, len(lengths)
    return lengths


def _of(lengths, ident):
    got = {n: v for n, v in lengths.items() if ident in n and not n.startswith("__")}
    assert got, f"no kernel with {ident} in its name"
    return got


@pytest.mark.parametrize("ident", HOT)
def test_hot_path_kernels_have_their_leading_arguments_preloaded(preload_lengths, ident):
    none = sorted(n for n, v in _of(preload_lengths, ident).items() if v == 0)
    assert not none, none


@pytest.mark.parametrize("ident,dwords", sorted({**FLAT, **ALREADY_FLAT}.items()))
def test_preload_length_is_the_flat_prefix(preload_lengths, ident, dwords):
    want = min(dwords, GRANTED)
    wrong = {n: v for n, v in _of(preload_lengths, ident).items() if v != want}
    assert not wrong, (want, wrong)

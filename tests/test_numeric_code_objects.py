"""What the tensor output's arithmetic contract rests on in the gfx950 code objects (no GPU needed): the pack_tensor and
resize_tensor kernels hold no fused or multiply-accumulate float instruction (every operation rounds on its own:
-ffp-contract=off reached the device pass), their kernel descriptors start every wave with float32 and float16
denormals kept and round-to-nearest-even, and the conversions are the instructions DESIGN.md 5.7 names."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "compeg_amd", "libcompeg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
DTYPES, KS = ("u8", "f16", "bf16", "f32"), (1, 2, 4, 8)
KERNELS = tuple(f"pack_tensor_{t}_k{k}_kernel" for t in DTYPES for k in KS) + \
    tuple(f"resize_tensor_{f}_{t}_k{k}_kernel" for f in ("nearest", "bilinear") for t in DTYPES for k in KS)
# float multiply-adds of any kind: fused (v_fma, v_fmac, v_pk_fma, v_dot), or unfused with modes of their own (v_mad_f32,
# v_mac_f32 flush denormals whatever the wave's mode says)
FUSED = re.compile(r"\bv_(?:pk_)?(?:fma|fmac|mac|mad|mad_legacy|mad_mix\w*|fma_mix\w*|dot\w*)_(?:legacy_)?(?:f16|f32|f64|bf16)\w*")


def _has(body, name):
    """The instruction, or its packed form (v_pk_mul_f32, v_cvt_pk_f16_f32), in any encoding (_e32, _e64, _sdwa, _dpp)."""
    packed = name.replace("v_cvt_", "v_cvt_pk_") if name.startswith("v_cvt_") else name.replace("v_", "v_pk_", 1)
    return re.search(r"\b(?:" + name + "|" + packed + r")(?:_e32|_e64|_sdwa|_dpp)?\b", body) is not None


def _kernel_of(symbol):
    return next((k for k in KERNELS if re.search(r"\d+" + k + "E", symbol)), None)


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """[(path, disassembly)] of the gfx950 code objects that hold tensor kernels."""
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or llvm-objdump not here")
    tmp = tmp_path_factory.mktemp("numeric_co")
    lib = shutil.copy(LIB, tmp / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp)
    found = []
    for p in sorted(tmp.iterdir()):
        if "gfx950" in p.name:
            asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", str(p)], check=True, capture_output=True, text=True).stdout
            if "pack_tensor_" in asm or "resize_tensor_" in asm:
                found.append((str(p), asm))
    return found


def _bodies(code_objects):
    for _, asm in code_objects:
        for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <\S+>:|\Z)", asm, re.S | re.M):
            kernel = _kernel_of(m.group(1))
            if kernel:
                yield kernel, m.group(2)


def test_no_tensor_kernel_fuses_or_accumulates_a_float_operation(code_objects):
    seen = set()
    for kernel, body in _bodies(code_objects):
        seen.add(kernel)
        fused = sorted({m.group(0) for m in FUSED.finditer(body)})
        assert not fused, f"{kernel}: {fused} -- the contract rounds every operation on its own"
        assert _has(body, "v_mul_f32") and _has(body, "v_add_f32"), f"{kernel}: no separate multiply and add"
    assert seen == set(KERNELS), f"kernels not found in the code objects: {sorted(set(KERNELS) - seen)}"


def test_conversions_are_the_instructions_the_design_names(code_objects):
    for kernel, body in _bodies(code_objects):
        if "_f16_" in kernel:
            assert _has(body, "v_cvt_f16_f32"), f"{kernel}: no v_cvt_f16_f32"
            assert not re.search(r"\bv_cvt_pkrtz", body), f"{kernel}: a round-towards-zero f16 conversion"
        if "_u8_" in kernel:
            assert _has(body, "v_rndne_f32") and _has(body, "v_med3_f32"), f"{kernel}: no v_rndne_f32 + v_med3_f32"
        # no instruction carries an output modifier or a clamp: they would flush denormals and saturate
        assert not re.search(r"\b(?:clamp|mul:[24]|div:2)\b", body), f"{kernel}: an output modifier"
        # nothing rewrites the wave's rounding or denormal mode (MODE is hardware register 1)
        assert not re.search(r"\bs_setreg\w*\s+hwreg\(HW_REG_MODE", body) and not re.search(r"\bs_(?:round|denorm)_mode\b", body), kernel


def test_kernel_descriptors_keep_denormals_and_round_to_nearest_even(code_objects):
    """compute_pgm_rsrc1 (bytes 48..51 of the 64-byte descriptor): bits 12-13 / 14-15 the rounding mode of f32 / f16 and
    f64 (0: nearest even), bits 16-17 / 18-19 their denormal mode (3: kept, sources and results)."""
    seen = set()
    for path, _ in code_objects:
        sections = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", path], check=True, capture_output=True, text=True).stdout
        symbols = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", path], check=True, capture_output=True, text=True).stdout
        layout = {}   # section index -> (address, file offset)
        for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sections, re.M):
            layout[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
        raw = open(path, "rb").read()
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+64\s+OBJECT\s+\S+\s+\S+\s+(\d+)\s+(\S+)\.kd$", symbols, re.M):
            kernel = _kernel_of(m.group(3))
            if not kernel:
                continue
            address, offset = layout[int(m.group(2))]
            at = int(m.group(1), 16) - address + offset
            rsrc1, = struct.unpack_from("<I", raw, at + 48)
            seen.add(kernel)
            assert (rsrc1 >> 12) & 0xf == 0, f"{kernel}: rounding modes {(rsrc1 >> 12) & 0xf:#x}, not nearest even"
            assert (rsrc1 >> 16) & 3 == 3, f"{kernel}: float32 denormal mode {(rsrc1 >> 16) & 3}: denormals are flushed"
            assert (rsrc1 >> 18) & 3 == 3, f"{kernel}: float16 / float64 denormal mode {(rsrc1 >> 18) & 3}: denormals are flushed"
    assert seen == set(KERNELS), f"kernel descriptors not found: {sorted(set(KERNELS) - seen)}"

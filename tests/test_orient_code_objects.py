"""What the compiler made of the orient_tensor kernels (no GPU needed), like test_filter_code_objects.py for its
kernels: every element type x downscale factor the dispatch table can launch is in the gfx950 code object; its memory
traffic is global_* instructions (a pointer that lost its address space would make it flat_*), nothing spills, no lane
has private memory -- the band's sums and the run that is put into output order are registers --, and every float
multiply and add is an instruction of its own (the pattern of tests/test_numeric_code_objects.py)."""
import os
import re
import shutil
import subprocess

import pytest

from test_numeric_code_objects import FUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "compeg_amd", "libcompeg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = tuple(f"orient_tensor_{t}_k{k}_kernel" for t in ("u8", "f16", "bf16", "f32") for k in (1, 2, 4, 8))


def _code_objects(tmp_path):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or llvm-objdump not here")
    lib = shutil.copy(LIB, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp_path)
    return [str(p) for p in tmp_path.iterdir() if "gfx950" in p.name]


def test_orient_kernels_are_there_unfused_without_flat_scratch_or_private_memory(tmp_path):
    seen, sized = set(), set()
    for co in _code_objects(tmp_path):
        asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <\S+>:|\Z)", asm, re.S | re.M):
            name, body = m.group(1), m.group(2)
            kernel = next((k for k in KERNELS if re.search(r"\d+" + k + "E", name)), None)
            if not kernel:
                continue
            seen.add(kernel)
            flat = len(re.findall(r"\bflat_(load|store|atomic)", body))
            scratch = len(re.findall(r"\bscratch_(load|store)", body))
            assert flat == 0, f"{kernel}: {flat} flat memory instructions (a global pointer lost its address space)"
            assert scratch == 0, f"{kernel}: {scratch} scratch instructions (register spills)"
            assert re.search(r"\bglobal_load_dword", body) and re.search(r"\bglobal_store_", body), f"{kernel}: no pixel loads or no stores"
            fused = sorted({f.group(0) for f in FUSED.finditer(body)})
            assert not fused, f"{kernel}: {fused} -- the contract rounds every operation on its own"
            assert re.search(r"\bv_mul_f32", body) and re.search(r"\bv_add_f32", body), f"{kernel}: no separate multiply and add"
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            size = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            kernel = name and next((k for k in KERNELS if re.search(r"\d+" + k + "E", name.group(1))), None)
            if kernel and size:
                sized.add(kernel)
                assert int(size.group(1)) == 0, f"{kernel}: {size.group(1)} bytes of private memory per lane"
    assert seen == set(KERNELS), f"kernels not found in the code objects: {sorted(set(KERNELS) - seen)}"
    assert sized == set(KERNELS), f"kernels without metadata: {sorted(set(KERNELS) - sized)}"

"""What the compiler made of the luma_tensor kernels (no GPU needed), like test_nhwc_code_objects.py for its kernels:
every element type x downscale factor the dispatch table can launch is in the library's gfx950 code objects; its memory
traffic is global_* instructions (a pointer that lost its address space would make it flat_*), nothing spills, no lane
has private memory, there is no LDS and no lane exchange, and every float multiply and add is an instruction of its own.
A luma kernel holds a third of the oriented kernel's sums: its VGPR count, read from the notes, is no larger than that
of the orient_tensor kernel of the same element type and factor in the same library (each family is a translation unit
and so a code object of its own; both are built by the same compiler with the same flags)."""
import os
import re
import subprocess

from test_numeric_code_objects import FUSED
from test_orient_code_objects import LLVM, _code_objects

NAMES = tuple(f"{t}_k{k}" for t in ("u8", "f16", "bf16", "f32") for k in (1, 2, 4, 8))
KERNELS = tuple(f"luma_tensor_{n}_kernel" for n in NAMES)
ORIENT = tuple(f"orient_tensor_{n}_kernel" for n in NAMES)


def test_luma_kernels_are_there_unfused_without_flat_scratch_lds_or_private_memory_and_no_wider_than_orient(tmp_path):
    seen, sized, vgprs = set(), set(), {}
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
            lds = len(re.findall(r"\bds_\w+", body))
            assert flat == 0, f"{kernel}: {flat} flat memory instructions (a global pointer lost its address space)"
            assert scratch == 0, f"{kernel}: {scratch} scratch instructions (register spills)"
            assert lds == 0, f"{kernel}: {lds} LDS or lane-exchange instructions"
            assert re.search(r"\bglobal_load_dword", body) and re.search(r"\bglobal_store_", body), f"{kernel}: no pixel loads or no stores"
            fused = sorted({f.group(0) for f in FUSED.finditer(body)})
            assert not fused, f"{kernel}: {fused} -- the contract rounds every operation on its own"
            assert re.search(r"\bv_mul_f32", body) and re.search(r"\bv_add_f32", body), f"{kernel}: no separate multiply and add"
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            size = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            group = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
            count = re.search(r"\.vgpr_count:\s+(\d+)", block)
            kernel = name and next((k for k in KERNELS + ORIENT if re.search(r"\d+" + k + "E", name.group(1))), None)
            if kernel and count:
                vgprs[kernel] = int(count.group(1))
            if kernel in KERNELS and size and group:
                sized.add(kernel)
                assert int(size.group(1)) == 0, f"{kernel}: {size.group(1)} bytes of private memory per lane"
                assert int(group.group(1)) == 0, f"{kernel}: {group.group(1)} bytes of LDS"
    assert seen == set(KERNELS), f"kernels not found in the code objects: {sorted(set(KERNELS) - seen)}"
    assert sized == set(KERNELS), f"kernels without metadata: {sorted(set(KERNELS) - sized)}"
    for n in NAMES:
        luma, orient = vgprs.get(f"luma_tensor_{n}_kernel"), vgprs.get(f"orient_tensor_{n}_kernel")
        print(f"{n}: luma {luma} VGPRs, orient {orient}")
        assert luma is not None and orient is not None, f"{n}: no VGPR count in the notes"
        assert luma <= orient, f"luma_tensor_{n}_kernel: {luma} VGPRs, more than orient_tensor_{n}_kernel's {orient}"

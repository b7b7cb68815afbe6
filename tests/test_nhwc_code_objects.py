"""What the compiler made of the nhwc_tensor kernels (no GPU needed), like test_orient_code_objects.py for its kernels:
every element type x downscale factor the dispatch table can launch is in the gfx950 code object (`channels` is a uniform
branch inside each, not a kernel of its own); its memory traffic is global_* instructions (a pointer that lost its address
space would make it flat_*), nothing spills, no lane has private memory -- the band's sums and the interleaved run of up
to 32 elements are registers --, there is no LDS and every float multiply and add is an instruction of its own."""
import os
import re
import subprocess

from test_numeric_code_objects import FUSED
from test_orient_code_objects import LLVM, _code_objects

KERNELS = tuple(f"nhwc_tensor_{t}_k{k}_kernel" for t in ("u8", "f16", "bf16", "f32") for k in (1, 2, 4, 8))


def test_nhwc_kernels_are_there_unfused_without_flat_scratch_lds_or_private_memory(tmp_path):
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
            lds = len(re.findall(r"\bds_\w+", body))
            assert flat == 0, f"{kernel}: {flat} flat memory instructions (a global pointer lost its address space)"
            assert scratch == 0, f"{kernel}: {scratch} scratch instructions (register spills)"
            assert lds == 0, f"{kernel}: {lds} LDS or lane-exchange instructions"
            assert re.search(r"\bglobal_load_dword", body) and re.search(r"\bglobal_store_", body), f"{kernel}: no pixel loads or no stores"
            # a whole pixel or a whole vector of the run leaves in one 16-byte store where its address allows it
            assert re.search(r"\bglobal_store_dwordx4", body), f"{kernel}: no 16-byte store"
            fused = sorted({f.group(0) for f in FUSED.finditer(body)})
            assert not fused, f"{kernel}: {fused} -- the contract rounds every operation on its own"
            assert re.search(r"\bv_mul_f32", body) and re.search(r"\bv_add_f32", body), f"{kernel}: no separate multiply and add"
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            size = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            group = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
            kernel = name and next((k for k in KERNELS if re.search(r"\d+" + k + "E", name.group(1))), None)
            if kernel and size and group:
                sized.add(kernel)
                assert int(size.group(1)) == 0, f"{kernel}: {size.group(1)} bytes of private memory per lane"
                assert int(group.group(1)) == 0, f"{kernel}: {group.group(1)} bytes of LDS"
    assert seen == set(KERNELS), f"kernels not found in the code objects: {sorted(set(KERNELS) - seen)}"
    assert sized == set(KERNELS), f"kernels without metadata: {sorted(set(KERNELS) - sized)}"

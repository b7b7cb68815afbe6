"""What the compiler made of the planes kernels (no GPU needed; the pattern of tests/test_gray_code_objects.py): all five
are in the gfx950 code object, their memory traffic is global_* instructions (a pointer that lost its address space would
make it flat_*), nothing spills, no lane has private memory, and their vector registers allow the waves per SIMD that
their launch bounds declare and the planner assumes (planes_wave_cap: 768 threads a workgroup on four SIMDs are three
waves, 512 / 3 registers each in the allocation's steps of 8; 512 threads two waves, 256 registers).  The counts
themselves are in DESIGN.md 5.16."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "compeg_amd", "libcompeg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (launch bounds, vector stores it must have)
KERNELS = {"decode_planes_422_kernel": (768, ("global_store_dwordx4", "global_store_dwordx2")),
           "decode_planes_444_kernel": (768, ("global_store_dwordx4", "global_store_dwordx2")),
           "decode_planes_440_kernel": (768, ("global_store_dwordx4", "global_store_dwordx2")),
           "decode_planes_420_kernel": (512, ("global_store_dwordx4", "global_store_dwordx2")),
           "decode_planes_gray_kernel": (768, ("global_store_dwordx2",))}


def _budget(threads):
    waves_per_simd = threads // 64 // 4
    return 512 // waves_per_simd // 8 * 8   # 168, 256


def _code_objects(tmp_path):
    assert os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump")), "library or llvm-objdump not here"
    lib = shutil.copy(LIB, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp_path)
    return [str(p) for p in tmp_path.iterdir() if "gfx950" in p.name]


def test_planes_kernels_are_there_without_flat_scratch_or_private_memory_within_their_registers(tmp_path):
    seen, sized = set(), {}
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
            for store in KERNELS[kernel][1]:
                assert re.search(r"\b" + store + r"\b", body), f"{kernel}: no {store} (the aligned path's vector stores)"
            assert re.search(r"\bglobal_store_byte\b", body), f"{kernel}: no byte stores (the path of cut and unaligned MCUs)"
            if kernel == "decode_planes_422_kernel":
                assert re.search(r"\bv_perm_b32\b", body) and re.search(r"\bv_lerp_u8\b", body), "the interleaves and the 4:2:0 average are packed byte operations"
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            kernel = name and next((k for k in KERNELS if re.search(r"\d+" + k + "E", name.group(1))), None)
            if not kernel:
                continue
            private = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            vgprs = re.search(r"\.vgpr_count:\s+(\d+)", block)
            agprs = re.match(r":?\s*(\d+)", block)
            threads = re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block)
            assert private and vgprs and agprs and threads, f"{kernel}: incomplete metadata"
            assert int(private.group(1)) == 0, f"{kernel}: {private.group(1)} bytes of private memory per lane"
            assert int(threads.group(1)) == KERNELS[kernel][0], f"{kernel}: launch bounds of {threads.group(1)} threads"
            sized[kernel] = int(vgprs.group(1)) + int(agprs.group(1))   # (one file of 512 on gfx950)
            print(f"{kernel}: {vgprs.group(1)} VGPRs + {agprs.group(1)} AGPRs")
            budget = _budget(KERNELS[kernel][0])
            assert sized[kernel] <= budget, f"{kernel}: {sized[kernel]} registers, its launch bounds' waves per SIMD need {budget} or fewer"
    assert seen == set(KERNELS), f"kernels not found in the code objects: {sorted(set(KERNELS) - seen)}"
    assert set(sized) == set(KERNELS), f"kernels without metadata: {sorted(set(KERNELS) - set(sized))}"

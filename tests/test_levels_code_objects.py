"""What the compiler made of the levels kernels (no GPU needed; the pattern of tests/test_reduced_code_objects.py): all
five are in the gfx950 code object's metadata, no lane has private memory (no scratch), nothing spills, none uses AGPRs,
and their launch bounds are the sixteen waves levels_wave_cap() lets the planner choose, whose four waves a SIMD the
vector registers must allow (512 / 4 = 128).  The counts are printed; DESIGN.md 5.20 has them."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "compeg_amd", "libcompeg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("decode_levels_422_kernel", "decode_levels_444_kernel", "decode_levels_440_kernel", "decode_levels_420_kernel",
           "decode_levels_gray_kernel")
THREADS, BUDGET = 1024, 128


def _code_objects(tmp_path):
    assert os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump")), "library or llvm-objdump not here"
    lib = shutil.copy(LIB, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp_path)
    return [str(p) for p in tmp_path.iterdir() if "gfx950" in p.name]


def test_levels_kernels_are_there_without_scratch_spills_or_agprs(tmp_path):
    sized = {}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            kernel = name and next((k for k in KERNELS if re.search(r"\d+" + k + "E", name.group(1))), None)
            if not kernel:
                continue
            field = {key: re.search(r"\." + key + r":\s+(\d+)", block) for key in
                     ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size")}
            agprs = re.match(r":?\s*(\d+)", block)
            assert agprs and all(field.values()), f"{kernel}: incomplete metadata"
            value = {key: int(m.group(1)) for key, m in field.items()}
            print(f"{kernel}: {value['vgpr_count']} VGPRs + {agprs.group(1)} AGPRs, launch bounds {value['max_flat_workgroup_size']}")
            assert value["private_segment_fixed_size"] == 0, f"{kernel}: {value['private_segment_fixed_size']} bytes of private memory per lane (scratch)"
            assert value["vgpr_spill_count"] == 0 and value["sgpr_spill_count"] == 0, f"{kernel}: spills ({value})"
            assert int(agprs.group(1)) == 0, f"{kernel}: {agprs.group(1)} AGPRs"
            assert value["max_flat_workgroup_size"] == THREADS, f"{kernel}: launch bounds of {value['max_flat_workgroup_size']} threads"
            assert value["vgpr_count"] <= BUDGET, f"{kernel}: {value['vgpr_count']} registers, four waves a SIMD need {BUDGET} or fewer"
            sized[kernel] = value["vgpr_count"]
    assert set(sized) == set(KERNELS), f"kernels not found in the code objects: {sorted(set(KERNELS) - set(sized))}"

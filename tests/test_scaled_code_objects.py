"""What the compiler made of the scaled kernels (no GPU needed; the pattern of tests/test_reduced_code_objects.py): all
ten -- five samplings, each at N = 4 and N = 2 -- are in the gfx950 code object's metadata, no lane has private memory (no
scratch: the samples a lane keeps per MCU must stay in registers), nothing spills, none uses AGPRs, and their launch bounds
are the waves scaled_wave_cap(hs, vs, n) lets the planner choose -- sixteen for both sizes -- whose four waves a SIMD the
vector registers must allow (512 / 4 = 128).  The counts are printed; DESIGN.md 5.19 has them.  Register counts and
metadata only: no instruction is looked for."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "compeg_amd", "libcompeg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
SAMPLINGS = ("422", "444", "440", "420", "gray")
WAVES = {4: 16, 2: 16}   # scaled_wave_cap (compeg_amd/csrc/scaled_kernels.hip), by N
KERNELS = {(s, n): f"decode_scaled_{s}_kernelILi{n}EE" for s in SAMPLINGS for n in WAVES}


def _code_objects(tmp_path):
    assert os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump")), "library or llvm-objdump not here"
    lib = shutil.copy(LIB, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp_path)
    return [str(p) for p in tmp_path.iterdir() if "gfx950" in p.name]


def test_wave_cap_in_the_source_is_what_this_test_assumes():
    src = open(os.path.join(ROOT, "compeg_amd", "csrc", "scaled_kernels.hip")).read()
    assert "constexpr uint32_t scaled_waves(int) { return 16u; }" in src
    assert src.count("__launch_bounds__(scaled_waves(N) * kWave)") == len(SAMPLINGS)


def test_scaled_kernels_are_there_without_scratch_spills_or_agprs(tmp_path):
    sized = {}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            key = name and next((k for k, v in KERNELS.items() if re.search(r"\d+" + v, name.group(1))), None)
            if not key:
                continue
            kernel, threads = KERNELS[key], 64 * WAVES[key[1]]
            budget = 512 // (WAVES[key[1]] // 4)   # (a CU has four SIMDs: the workgroup's waves a SIMD share its 512 registers)
            field = {k: re.search(r"\." + k + r":\s+(\d+)", block) for k in
                     ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size")}
            agprs = re.match(r":?\s*(\d+)", block)
            assert agprs and all(field.values()), f"{kernel}: incomplete metadata"
            value = {k: int(m.group(1)) for k, m in field.items()}
            print(f"{kernel}: {value['vgpr_count']} VGPRs + {agprs.group(1)} AGPRs, launch bounds {value['max_flat_workgroup_size']}")
            assert value["private_segment_fixed_size"] == 0, f"{kernel}: {value['private_segment_fixed_size']} bytes of private memory per lane (scratch)"
            assert value["vgpr_spill_count"] == 0 and value["sgpr_spill_count"] == 0, f"{kernel}: spills ({value})"
            assert int(agprs.group(1)) == 0, f"{kernel}: {agprs.group(1)} AGPRs"
            assert value["max_flat_workgroup_size"] == threads, f"{kernel}: launch bounds of {value['max_flat_workgroup_size']} threads"
            assert value["vgpr_count"] <= budget, f"{kernel}: {value['vgpr_count']} registers, {WAVES[key[1]] // 4} waves a SIMD need {budget} or fewer"
            sized[key] = value["vgpr_count"]
    assert set(sized) == set(KERNELS), f"kernels not found in the code objects: {sorted(set(KERNELS) - set(sized))}"

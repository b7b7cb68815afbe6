"""What the compiler made of the region-list cropped kernels (no GPU needed; the pattern of
tests/test_crop_code_objects.py): all five are in the gfx950 code object's metadata, no lane has private memory (no
scratch), nothing spills, none uses AGPRs, and their launch bounds are 64 x the waves crop_regions_wave_cap() lets the planner
choose -- the one-rectangle kernels' caps: twelve (4:2:0: eight), three (two) waves a SIMD, which the vector registers
must allow: 512 / 3 = 170 (512 / 2 = 256).  The counts are printed; DESIGN.md 5.21 has them."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "compeg_amd", "libcompeg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> waves a workgroup crop_regions_wave_cap(hs, vs) allows (compeg_amd/csrc/crop_regions_kernels.hip)
WAVE_CAP = {"decode_cropped_regions_422_kernel": 12, "decode_cropped_regions_444_kernel": 12, "decode_cropped_regions_440_kernel": 12,
            "decode_cropped_regions_420_kernel": 8, "decode_cropped_regions_gray_kernel": 12}


def _code_objects(tmp_path):
    assert os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump")), "library or llvm-objdump not here"
    lib = shutil.copy(LIB, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=tmp_path)
    return [str(p) for p in tmp_path.iterdir() if "gfx950" in p.name]


def test_the_wave_caps_are_the_one_rectangle_kernels():
    """crop_regions_wave_cap as crop_regions_kernels.hip has it, read from the source: it hands on crop_wave_cap, which the
    table above restates (tests/test_crop_code_objects.py reads that one from its source)."""
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    text = open(os.path.join(csrc, "crop_regions_kernels.hip")).read()
    assert re.search(r"uint32_t crop_regions_wave_cap\(uint32_t hs, uint32_t vs\) \{ return crop_wave_cap\(hs, vs\); \}", text), \
        "crop_regions_wave_cap has another form: restate it here"
    m = re.search(r"uint32_t crop_wave_cap\(uint32_t hs, uint32_t vs\) \{ return hs == 2 && vs == 2 \? (\d+)u : (\d+)u; \}",
                  open(os.path.join(csrc, "crop_kernels.hip")).read())
    assert m and {k: (int(m.group(1)) if "420" in k else int(m.group(2))) for k in WAVE_CAP} == WAVE_CAP
    for kernel, waves in WAVE_CAP.items():
        assert re.search(r"__launch_bounds__\(" + str(64 * waves) + r"\)\s+" + kernel + r"\(", text), f"{kernel}: launch bounds in the source"


def test_region_kernels_are_there_without_scratch_spills_or_agprs(tmp_path):
    sized = {}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            kernel = name and next((k for k in WAVE_CAP if re.search(r"\d+" + k + "E", name.group(1))), None)
            if not kernel:
                continue
            field = {key: re.search(r"\." + key + r":\s+(\d+)", block) for key in
                     ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size")}
            agprs = re.match(r":?\s*(\d+)", block)
            assert agprs and all(field.values()), f"{kernel}: incomplete metadata"
            value = {key: int(m.group(1)) for key, m in field.items()}
            waves = WAVE_CAP[kernel]
            per_simd = -(-waves // 4)
            budget = 512 // per_simd
            print(f"{kernel}: {value['vgpr_count']} VGPRs + {agprs.group(1)} AGPRs, {value['sgpr_count']} SGPRs, launch bounds "
                  f"{value['max_flat_workgroup_size']} ({waves} waves, {per_simd} a SIMD: {budget} registers)")
            assert value["private_segment_fixed_size"] == 0, f"{kernel}: {value['private_segment_fixed_size']} bytes of private memory per lane (scratch)"
            assert value["vgpr_spill_count"] == 0 and value["sgpr_spill_count"] == 0, f"{kernel}: spills ({value})"
            assert int(agprs.group(1)) == 0, f"{kernel}: {agprs.group(1)} AGPRs"
            assert value["max_flat_workgroup_size"] == 64 * waves, f"{kernel}: launch bounds of {value['max_flat_workgroup_size']} threads"
            assert value["vgpr_count"] <= budget, f"{kernel}: {value['vgpr_count']} registers, {per_simd} waves a SIMD need {budget} or fewer"
            sized[kernel] = value["vgpr_count"]
    assert set(sized) == set(WAVE_CAP), f"kernels not found in the code objects: {sorted(set(WAVE_CAP) - set(sized))}"

#!/usr/bin/env python3
"""VGPR / spill / LDS use of the gfx950 kernels in a built object (no GPU needed).

Usage: python tools/kernel_resources.py [alpenglow_amd/_lib/obj/rs_window.hip.o] [name-filter]
Unbundles the object's .hip_fatbin with the ROCm LLVM tools and reads the code-object notes.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def unbundle(obj, co):
    """The gfx950 code object of a host object's .hip_fatbin, written to `co`."""
    fat = co + ".fat"
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    os.remove(fat)


def kernel_notes(co):
    """{kernel name: {field: value}} from the code object's notes (FIELDS; "-" where absent)."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    out = {}
    for blk in notes.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: (re.search(r"\." + k + r":\s+(\d+)", blk) or [None, "-"])[1] for k in FIELDS}
    return out


def main():
    obj = sys.argv[1] if len(sys.argv) > 1 else "alpenglow_amd/_lib/obj/rs_window.hip.o"
    filt = sys.argv[2] if len(sys.argv) > 2 else ""
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "k.co")
        unbundle(obj, co)
        notes = kernel_notes(co)
    for name, g in notes.items():
        if filt not in name:
            continue
        print(f"{name[:100]:100s} vgpr {g['vgpr_count']:>4} spill {g['vgpr_spill_count']:>3} "
              f"sgpr_spill {g['sgpr_spill_count']:>3} scratch {g['private_segment_fixed_size']:>4} "
              f"lds {g['group_segment_fixed_size']:>6}")


if __name__ == "__main__":
    main()

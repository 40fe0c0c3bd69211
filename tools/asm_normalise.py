"""Normalise a device assembly file (hipcc -S --cuda-device-only) so that two compiles of sources that should give the same code
compare equal: the per-compile __hip_cuid_ symbol loses its hash, and every mangled name becomes SYM<k>, k by first appearance
(a type that changes its name or namespace changes the mangled names of the kernels that take it, not their order in the file).

  asm_normalise.py IN.s OUT.s [--table]     --table: print kernel, VGPRs, SGPR / VGPR spills, scratch and LDS bytes from the metadata"""
import re
import sys


def normalise(text):
    names = {}
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)
    return re.sub(r"_Z\w+", lambda m: names.setdefault(m.group(0), f"SYM{len(names)}"), text), names


def table(text, names):
    rows = []
    for block in text.split("  - .agpr_count:")[1:]:
        field = lambda key: re.search(rf"\.{key}:\s*(\S+)", block).group(1)
        rows.append((field("name"), field("vgpr_count"), field("sgpr_spill_count"), field("vgpr_spill_count"), field("private_segment_fixed_size"),
                     field("group_segment_fixed_size")))
    return rows


if __name__ == "__main__":
    src = open(sys.argv[1]).read()
    out, names = normalise(src)
    open(sys.argv[2], "w").write(out)
    if "--table" in sys.argv:
        print("kernel vgpr sgpr_spill vgpr_spill scratch_bytes lds_bytes")
        for row in table(src, names):
            print(" ".join(row))

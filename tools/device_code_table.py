#!/usr/bin/env python3
"""The gfx950 code object of one or two builds of libptgpu.so, function by function: vector and scalar registers, scratch
and LDS from the code object's notes, the number of instructions and the first 16 hex digits of a SHA-256 of the disassembly
(llvm-objdump -d, addresses, encodings and pc-relative distances to constant tables stripped).  With two libraries - parent, change - the kernels that are new, gone
or different are listed first, then the change's table.

    tools/device_code_table.py [parent.so] change.so > profiles/rNN_device_code.txt"""
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def table(lib):
    with tempfile.TemporaryDirectory() as tmp:
        fat, elf = Path(tmp) / "fat.bin", Path(tmp) / "gfx950.elf"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)], check=True)
        subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fat}", f"--output={elf}"], check=True)
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(elf)], check=True, capture_output=True, text=True).stdout
        asm = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", str(elf)], check=True,
                             capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                     for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    for m in re.finditer(r"^<([^>]+)>:\n(.*?)(?=^<|\Z)", asm, re.S | re.M):
        if m.group(1) not in out:
            continue
        lines = [re.sub(r"\s*//.*$", "", ln).strip() for ln in m.group(2).splitlines()]
        lines = [ln for ln in lines if ln and not ln.endswith(":")]
        # (the literal added to a program counter read just before is the distance to a constant table: it moves with the
        # layout of the code object, not with the kernel's code)
        for k in range(len(lines)):
            if lines[k].startswith("s_getpc_b64"):
                for j in (k + 1, k + 2):
                    if j < len(lines) and lines[j].startswith(("s_add_u32", "s_addc_u32")):
                        lines[j] = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", lines[j])
        out[m.group(1)].update(insns=len(lines), sha=hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16])
    return out


def row(name, k):
    return (f"  {name[:74]:74s}  vgpr {k['vgpr_count']:3d} sgpr {k['sgpr_count']:3d} scratch {k['private_segment_fixed_size']:4d} "
            f"lds {k['group_segment_fixed_size']:6d} insns {k.get('insns', 0):6d} {k.get('sha', '?')}")


def main():
    libs = sys.argv[1:]
    if len(libs) == 2:
        parent, change = table(libs[0]), table(libs[1])
        new, gone = sorted(set(change) - set(parent)), sorted(set(parent) - set(change))
        differ = sorted(n for n in set(parent) & set(change) if parent[n] != change[n])
        print(f"parent: {len(parent)} kernels, change: {len(change)} kernels; new: {len(new)}; gone: {len(gone)}")
        print(f"{len(set(parent) & set(change)) - len(differ)} functions identical (registers, scratch, LDS, instruction count, "
              f"SHA-256 of the disassembly), {len(differ)} differ")
        for n in differ:
            print("differs, parent:\n" + row(n, parent[n]) + "\ndiffers, change:\n" + row(n, change[n]))
        print("\nnew:")
        for n in new:
            print(row(n, change[n]))
        print("\nThe change's table:")
    else:
        change = table(libs[0])
    for n in sorted(change):
        print(row(n, change[n]))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Compare two gfx950 device code objects kernel by kernel.

Proof that a refactor of a kernel source left the machine code alone.  Build
the device code object of each tree with the project's flags (HIP_FLAGS in
native/build.py) plus -save-temps, in a scratch directory:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics \\
          -Inative/include -save-temps -c native/kernels/kmeans.hip -o kmeans.o

which writes kmeans-hip-amdgcn-amd-amdhsa-gfx950.out, then

    tools/kernel_isa_diff.py parent.out new.out [--allow NAME]... [--rename OLD=NEW]...

Each object is disassembled with ROCm's llvm-objdump and split per symbol;
addresses, the address/encoding comments, <sym+0x...> branch targets and the
alignment padding after a kernel ("...", and the s_nop run after the last
kernel of .text) are stripped, so a kernel that merely moved compares equal.
Names are demangled,
without "(anonymous namespace)::" and the parameter list, e.g.
"kmeans_assign_v2_kernel<64, 2>".  --rename pairs a kernel of the first object
whose template list shrank with its new name.  Prints REMOVED / ADDED / DIFF
names and "same N diff M"; exits 1 if a kernel not named by --allow differs.
"""
import argparse
import os
import re
import subprocess
import sys

OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")
_SYM = re.compile(r"^[0-9a-f]+ <(.*)>:$")


def kernel_name(sym: str) -> str:
    s = sym.replace("(anonymous namespace)::", "")
    s = s[5:] if s.startswith("void ") else s
    return s.split("(", 1)[0]


def normalise(disasm: str) -> dict:
    """{kernel name: [instruction text, ...]} of llvm-objdump -d -C output."""
    out, cur = {}, None
    for line in disasm.splitlines():
        m = _SYM.match(line)
        if m:
            cur = out.setdefault(kernel_name(m.group(1)), [])
        elif cur is not None and line.startswith(("\t", " ")):
            text = " ".join(line.split("//", 1)[0].split())
            if text and text != "...":      # "...": elided zero padding up to the next symbol
                cur.append(text)
    for ins in out.values():        # the s_nop run that closes .text lands in whichever kernel
        while ins and ins[-1] == "s_nop 0":     # is last; it follows s_endpgm and never runs
            ins.pop()
    return out


def disassemble(path: str) -> dict:
    r = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "-C", path], check=True,
                       capture_output=True, text=True)
    return normalise(r.stdout)


def compare(old: dict, new: dict, rename: dict, allow: set):
    """(removed, added, diff, same count, ok) between two normalise() results."""
    old = {rename.get(k, k): v for k, v in old.items()}
    removed = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    common = sorted(set(old) & set(new))
    diff = [k for k in common if old[k] != new[k]]
    return removed, added, diff, len(common) - len(diff), all(k in allow for k in diff)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", action="append", default=[], metavar="NAME",
                    help="kernel that may differ")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args(argv)
    rename = dict(r.split("=", 1) for r in a.rename)
    removed, added, diff, same, ok = compare(disassemble(a.old), disassemble(a.new), rename,
                                             set(a.allow))
    for tag, names in (("REMOVED", removed), ("ADDED", added), ("DIFF", diff)):
        for k in names:
            print(tag, k)
    print(f"same {same} diff {len(diff)}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

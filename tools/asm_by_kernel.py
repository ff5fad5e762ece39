#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) kernel by kernel, whatever order the kernels were emitted in:

    tools/asm_by_kernel.py before.s after.s

A change that only reorders template instantiations moves whole kernels inside the file and renumbers the compiler's local
labels (.LBB<function>_<block>), which a plain diff reports as thousands of lines.  This prints the kernel symbols of both
files, whether they are the same set, and every kernel whose text differs once the function number is taken out of its
labels; the trailing metadata (one record per kernel) is compared as a set of lines, the compilation unit's id
(__hip_cuid_<hash of the source>) taken out.  Exit status 1 on any difference."""
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")
BLOCK = re.compile(r"\bBB\d+_")  # ("in Loop: Header=BB26_33" comments)
UNIT = re.compile(r"__hip_cuid_[0-9a-f]+")  # the compilation unit's id: a hash of the source text


def sections(path):
    out, name, cur = {}, "<head>", []
    for line in open(path):
        text = re.match(r"\t\.section\t\.text\.(\S+?),", line)
        if text or (name not in ("<head>", "<tail>") and re.match(r"\t\.(section|rodata|amdgpu_metadata)", line)):
            out.setdefault(name, []).extend(cur)
            name, cur = (text.group(1) if text else "<tail>"), []
        cur.append(UNIT.sub("__hip_cuid_n", BLOCK.sub("BBn_", LABEL.sub(r".\1n", line))))
    out.setdefault(name, []).extend(cur)
    return out


def symbols(path):
    return sorted(m.group(1) for m in (re.match(r"\t\.amdhsa_kernel (\S+)", line) for line in open(path)) if m)


def main(before, after):
    a, b = sections(before), sections(after)  # (kernels that are no templates share the leading .text: "<head>")
    ka, kb = symbols(before), symbols(after)
    print(f"{len(ka)} kernels before, {len(kb)} after; same symbols: {ka == kb}; same order in the file: {list(a) == list(b)}")
    for k in kb:
        print("   ", k)
    differing = [k for k in sorted(set(a) | set(b)) if k != "<tail>" and a.get(k) != b.get(k)]
    for k in differing:
        print("DIFFERS:", k)
    tail = sorted(a.get("<tail>", [])) == sorted(b.get("<tail>", []))
    print(f"{len(differing)} sections differ; metadata the same set of lines: {tail}")
    return 1 if differing or not tail or ka != kb else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

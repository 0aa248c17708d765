#!/usr/bin/env python
"""Did a change move the generated code of kernels it was not meant to touch?

    python tools/isa_diff.py OLD.s NEW.s        (e.g. csrc/build/gemm256.s of the parent commit against this tree's)

Compares the two assembly files kernel by kernel: the instruction stream from the kernel's label to its `.Lfunc_end` with comments
dropped and local labels (`.LBB12_3`, `.Ltmp7`) renamed by order of appearance, and the kernel descriptor's resource lines
(registers, scratch, LDS).  Kernels are matched by mangled name; an EMPTY trailing template pack (`...JEEEv`, how the kernel
templates of csrc/gemm.hip / gemm256.hip take their activation tag) is spelled as its absence, since it demangles to the same
name.  Prints IDENTICAL / DIFFERENT / GONE per old kernel and the resources of every new one; exit status 1 if any old kernel
differs or is gone.  Host only -- needs no GPU."""
import re
import sys

RES = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def canon(name):
    return name.replace("JEEEv", "EEv")


def kernels(path):
    """{canonical kernel name: (normalised instruction text, {resource: value})}"""
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        meta[m.group(1)] = {k: (re.search(rf"\.amdhsa_{k}\s+(\S+)", m.group(2)) or [None, "?"])[1] for k in RES}
    out = {}
    for name in meta:
        m = re.search(rf"^{re.escape(name)}:.*?\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        if not m:
            continue
        body, labels = [], {}
        for line in m.group(1).splitlines():
            line = re.sub(r";.*", "", line).rstrip()
            if not line:
                continue
            line = re.sub(r"\.L(?:BB|tmp)[0-9_]+", lambda t: labels.setdefault(t.group(0), f".L{len(labels)}"), line)
            body.append(line.replace(name, "<self>"))
        out[canon(name)] = ("\n".join(body), meta[name])
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(old):
        if name not in new:
            state = "GONE"
        else:
            state = "IDENTICAL" if old[name] == new[name] else "DIFFERENT"
        bad += state != "IDENTICAL"
        extra = "" if state != "DIFFERENT" else f"  {old[name][1]} -> {new[name][1]}, {old[name][0].count(chr(10)) + 1} -> {new[name][0].count(chr(10)) + 1} lines"
        print(f"{state:9s} {name}{extra}")
    for name in sorted(set(new) - set(old)):
        print(f"NEW       {name}  {new[name][1]}")
    print(f"{len(old) - bad} of {len(old)} old kernels identical, {len(set(new) - set(old))} new")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""profiles/tools/isa_cmp.py LIB_A LIB_B PATTERN [PATTERN ...]: compares the gfx950 instruction streams of the kernels whose demangled name
contains one of the PATTERNs, between two builds of libgeosrad.so.  Kernels are matched by their demangled name with the template
arguments a default parameter adds (", false>") and the parameter list removed.  The literal of the s_add_u32 / s_addc_u32 pair that
follows s_getpc_b64 (the pc-relative address of a __constant__ object: it moves with the position of the kernel in the code object) is
masked; everything else, branch targets included, is compared as it is.  Prints one line per kernel: instructions in A, in B, `same` or
the first differing line."""
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["cp", lib, d + "/lib.so"])
        subprocess.check_call([LLVM + "llvm-objdump", "--offloading", d + "/lib.so"], stdout=subprocess.DEVNULL, cwd=d)
        import glob
        for co in sorted(glob.glob(d + "/lib.so.*gfx950*")):
            txt = subprocess.check_output([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "-C", co], text=True)
            name = None
            for line in txt.splitlines():
                m = re.match(r"^<(.*)>:$", line)
                if m:
                    name = m.group(1)
                    out[name] = []
                elif name and line.strip():
                    ins = re.sub(r"\s*//.*$", "", line.strip())
                    if re.match(r"s_addc?_u32 s\d+, s\d+, 0x[0-9a-f]+$", ins) and any("s_getpc_b64" in x for x in out[name][-2:]):
                        ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
                    out[name].append(ins)
    return out


def norm(name):
    return name.split("(")[0].replace(", false>", ">").replace(",false>", ">")


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bn = {norm(k): v for k, v in b.items()}
    for k in sorted(a):
        if not any(p in k for p in sys.argv[3:]):
            continue
        other = bn.get(norm(k))
        if other is None:
            print(f"{k}: {len(a[k])} instructions, not in B")
            continue
        diff = next((i for i, (x, y) in enumerate(zip(a[k], other)) if x != y), None)
        if diff is None and len(a[k]) == len(other):
            print(f"{k}: {len(a[k])} / {len(other)} same")
        else:
            i = diff if diff is not None else min(len(a[k]), len(other))
            print(f"{k}: {len(a[k])} / {len(other)} DIFFERENT at {i}: {a[k][i:i + 1]} | {other[i:i + 1]}")


if __name__ == "__main__":
    main()

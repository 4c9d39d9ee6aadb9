#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libpgr_hip.so instruction by instruction (DESIGN.md sections 9 and 14: "the
existing instances are unchanged").

    python scripts/compare_instances.py OLD/libpgr_hip.so NEW/libpgr_hip.so

The device code object is taken out of each library (objcopy of .hip_fatbin, clang-offload-bundler -unbundle), disassembled
with llvm-objdump -d, and cut into functions.  Kernels are matched by their demangled name; `pgr_fan_kernel` instances by
their first four template arguments <LDS_TAB, ZM, SAVE, PERSIST>, so that a template parameter added behind them with a default
does not unmatch them (instances of the new build whose later arguments are not all false / 0 are new, and are listed as
such).  The padding behind a kernel is left out.  Per pair: identical, or the instructions that differ -- opcode and operands, addresses and encodings left out --
counted by opcode.  Literals of s_add_u32 / s_addc_u32 after an s_getpc_b64 are PC-relative offsets of constants, which move
with a kernel's position in the object."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def code_object(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    co = os.path.join(tmp, "gfx950.co")
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "-unbundle", "-type=o", "-input=" + fat, "-output=" + co,
                    "-targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    return co


def functions(lib):
    """{demangled name: [instruction text, ...]}"""
    with tempfile.TemporaryDirectory() as tmp:
        txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", "--no-leading-addr",
                              code_object(lib, tmp)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    for body in out.values():           # (the padding behind a kernel, up to the next one or the end of the section)
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return out


def key(name):
    m = re.match(r".*(pgr_fan_kernel)<([^>]*)>\(", name)
    if not m:
        return name, True
    args = [a.strip() for a in m.group(2).split(",")]
    old = all(a in ("false", "0") for a in args[4:])
    return m.group(1) + "<" + ", ".join(args[:4]) + ">", old       # (without the signature: the argument struct was renamed)


def main(old_lib, new_lib):
    old = {key(n)[0]: body for n, body in functions(old_lib).items()}
    new, added = {}, []
    for n, body in functions(new_lib).items():
        k, is_old = key(n)
        if is_old:
            new[k] = body
        else:
            added.append(n)
    same, differ = 0, 0
    for k in sorted(old):
        if k not in new:
            print("MISSING in the new build:", k)
            continue
        a, b = old[k], new[k]
        if a == b:
            same += 1
            continue
        differ += 1
        if len(a) != len(b):
            print(f"DIFFERENT LENGTH {len(a)} -> {len(b)}: {k}")
            continue
        ops = collections.Counter(x.split()[0] if x.split()[0] == y.split()[0] else x.split()[0] + "->" + y.split()[0]
                                  for x, y in zip(a, b) if x != y)
        print(f"{sum(ops.values())} of {len(a)} instructions differ ({dict(ops)}): {k}")
    print(f"{same} kernels identical, {differ} differ, {len(added)} only in the new build, "
          f"{len([k for k in new if k not in old])} unmatched old-style kernels in the new build")


if __name__ == "__main__":
    main(*sys.argv[1:3])

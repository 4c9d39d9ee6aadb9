#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libpgr_hip.so instruction by instruction (DESIGN.md sections 9, 14 and 15: "the
existing instances are unchanged").

    python scripts/compare_instances.py OLD/libpgr_hip.so NEW/libpgr_hip.so

The device code object is taken out of each library (objcopy of .hip_fatbin, clang-offload-bundler -unbundle), disassembled
with llvm-objdump -d, and cut into functions.  Kernels are matched by their demangled name; `pgr_fan_kernel` instances by
their whole template argument list <LDS_TAB, ZM, SAVE, PERSIST, LOG>.  Only when the old build predates a template parameter
added behind the others with a default (LOG) are its instances matched to those of the new build whose later arguments are
all false / 0; the new build's other instances are then new, and listed as such.  The padding behind a kernel is left out.  Per pair: identical, or the instructions that differ -- opcode and operands, addresses and encodings left out --
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
    """-> (key, template arguments or None): `pgr_fan_kernel` instances are keyed by their whole argument list"""
    m = re.match(r".*(pgr_fan_kernel)<([^>]*)>\(", name)
    if not m:
        return name, None
    args = [a.strip() for a in m.group(2).split(",")]
    return m.group(1) + "<" + ", ".join(args) + ">", args          # (without the signature: the argument struct was renamed)


def keyed(lib):
    out, n_args = {}, set()
    for n, body in functions(lib).items():
        k, args = key(n)
        out[k] = body
        if args is not None:
            n_args.add(len(args))
    return out, n_args


def main(old_lib, new_lib):
    (old, old_n), (new, new_n) = keyed(old_lib), keyed(new_lib)
    if old_n and new_n and max(old_n) < max(new_n):
        # the old build predates a template parameter (LOG): its instances are those of the new build whose later arguments
        # are all false / 0; the new build's other instances are new
        pad = lambda k: k[:-1] + ", false" * (max(new_n) - max(old_n)) + ">" if k.startswith("pgr_fan_kernel<") else k  # noqa: E731
        old = {pad(k): body for k, body in old.items()}
    count = lambda d: sum(k.startswith("pgr_fan_kernel<") for k in d)  # noqa: E731
    print(f"pgr_fan_kernel instances: {count(old)} in the old build, {count(new)} in the new build")
    same, literals, differ = 0, 0, 0
    for k in sorted(old):
        if k not in new:
            print("MISSING in the new build:", k)
            continue
        a, b = old[k], new[k]
        if a == b:
            same += 1
            continue
        if len(a) != len(b):
            differ += 1
            print(f"DIFFERENT LENGTH {len(a)} -> {len(b)}: {k}")
            continue
        ops = collections.Counter(x.split()[0] if x.split()[0] == y.split()[0] else x.split()[0] + "->" + y.split()[0]
                                  for x, y in zip(a, b) if x != y)
        only_literals = set(ops) <= {"s_add_u32", "s_addc_u32"}
        literals += only_literals
        differ += not only_literals
        print(f"{sum(ops.values())} of {len(a)} instructions differ ({dict(ops)}): {k}")
    added = sorted(k for k in new if k not in old)
    for k in added:
        print("ONLY in the new build:", k)
    print(f"{same} kernels identical, {literals} differ in s_add_u32 / s_addc_u32 literals only, {differ} differ otherwise, "
          f"{len([k for k in old if k not in new])} missing in the new build, {len(added)} only in the new build")


if __name__ == "__main__":
    main(*sys.argv[1:3])

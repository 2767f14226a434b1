"""Compares the gfx950 machine code of two builds of libbkdigest.so kernel by kernel.

Usage: python3 tools/kernel_disasm_diff.py OLD.so NEW.so [--out REPORT]

Extracts each library's gfx950 code object (clang-offload-bundler), disassembles it (llvm-objdump -d)
and compares the instruction text of every kernel symbol the two have in common; addresses and
encodings' positions are dropped, so only a changed instruction, operand or order shows. Prints one
line per kernel of OLD (identical / DIFFERENT / missing in NEW), the kernels only NEW has, and exits 1
if any common kernel differs. The evidence that a change left existing entry points' kernels alone
(profiles/requests_kernel_disasm.txt).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--" + os.environ.get("BKD_OFFLOAD_ARCH", "gfx950")


def kernels(so_path):
    """{symbol: [instruction text, ...]} of the library's device code."""
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "device.co")
        fatbin = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so_path, fatbin],
                       check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                        f"--input={fatbin}", f"--output={co}"], check=True)
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                              check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        line = re.sub(r"//.*$", "", line).strip()  # the trailing address / encoding comment
        if cur is not None and line:
            cur.append(line)
    return out


def demangle(names):
    import shutil
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if not filt:
        return {n: n for n in names}
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines())) if r.returncode == 0 else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--out")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    names = demangle(sorted(set(old) | set(new)))
    lines, differ = [], 0
    for k in sorted(old):
        if k not in new:
            lines.append(f"missing in NEW  {names[k]}")
            differ += 1
        elif old[k] == new[k]:
            lines.append(f"identical  {len(old[k]):6d} instructions  {names[k]}")
        else:
            lines.append(f"DIFFERENT  {len(old[k]):6d} -> {len(new[k]):6d} instructions  {names[k]}")
            differ += 1
    for k in sorted(set(new) - set(old)):
        lines.append(f"new        {len(new[k]):6d} instructions  {names[k]}")
    lines.append(f"{len(old)} kernels in OLD, {len(new)} in NEW, {differ} of OLD's changed or missing")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

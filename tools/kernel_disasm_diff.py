"""Compares the gfx950 machine code of two builds of libbkdigest.so kernel by kernel.

Usage: python3 tools/kernel_disasm_diff.py OLD.so NEW.so [--out REPORT] [--map PATTERN=REPL ...] [--diff REGEX]

Extracts each library's gfx950 code object (clang-offload-bundler), disassembles it (llvm-objdump -d)
and compares the instruction text of every kernel symbol the two have in common; addresses and
encodings' positions are dropped, so only a changed instruction, operand or order shows. Prints one
line per kernel of OLD (identical / DIFFERENT / missing in NEW), the kernels only NEW has, and exits 1
if any common kernel differs. The evidence that a change left existing entry points' kernels alone
(profiles/requests_kernel_disasm.txt).

--map PATTERN=REPL pairs a kernel of OLD whose symbol is not in NEW with the kernel of NEW whose
demangled name (without "void " and the parameter list) is re.sub(PATTERN, REPL, OLD's name): a kernel
that was renamed or became a template, e.g.
  --map 'crc_package_fused_kernel<(.*)>$=crc_package_fused_kernel<\1, bkd::OneLedger>'
--diff REGEX appends the unified diff of every differing pair whose name matches
(profiles/fold_ids_kernel_disasm.txt).
"""
import argparse
import difflib
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


def short(demangled):
    """A demangled kernel name without the return type and the parameter list."""
    depth = 0
    for i, c in enumerate(demangled):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            demangled = demangled[:i]
            break
    return demangled[5:] if demangled.startswith("void ") else demangled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--out")
    ap.add_argument("--map", action="append", default=[], metavar="PATTERN=REPL")
    ap.add_argument("--diff", metavar="REGEX")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    names = demangle(sorted(set(old) | set(new)))
    by_short = {short(names[k]): k for k in new}
    maps = [m.split("=", 1) for m in a.map]
    lines, diffs, differ, paired = [], [], 0, set()
    for k in sorted(old):
        k2, what = k, names[k]
        if k not in new:
            for pat, repl in maps:
                cand, hits = re.subn(pat, repl, short(names[k]))
                if hits and by_short.get(cand) not in (None, k):
                    k2, what = by_short[cand], f"{short(names[k])}  ->  {cand}"
                    paired.add(k2)
                    break
        if k2 not in new:
            lines.append(f"missing in NEW  {names[k]}")
            differ += 1
        elif old[k] == new[k2]:
            lines.append(f"identical  {len(old[k]):6d} instructions  {what}")
        else:
            lines.append(f"DIFFERENT  {len(old[k]):6d} -> {len(new[k2]):6d} instructions  {what}")
            differ += 1
            if a.diff and re.search(a.diff, what):
                diffs += [f"--- {what}"] + list(difflib.unified_diff(old[k], new[k2], "OLD", "NEW", lineterm="", n=0))
    for k in sorted(set(new) - set(old) - paired):
        lines.append(f"new        {len(new[k]):6d} instructions  {names[k]}")
    lines.append(f"{len(old)} kernels in OLD, {len(new)} in NEW, {differ} of OLD's changed or missing")
    lines += diffs
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

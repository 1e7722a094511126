#!/usr/bin/env python3
"""Compare the generated gfx950 code of one translation unit between two trees, kernel by kernel.

    python tools/kernel_code_diff.py PARENT_TREE NEW_TREE [--unit adsb_hip.hip] [--keep DIR] [--show]

Each tree's gr_adsb_amd/csrc/<unit> is compiled device-only with the library's flags (gr_adsb_amd/build.py FLAGS of the
NEW tree), unbundled and disassembled.  A function's text is its instruction lines with the addresses, the encodings and the
branch-target annotations taken off; two functions are equal when these texts are.  This is a comparison of text: it knows
no instruction.  Prints one line per differing kernel (with --show, its unified diff) and a summary; exit status 1 if any
function differs or is missing on one side.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def flags_of(tree):
    sys.path.insert(0, tree)
    from gr_adsb_amd import build as b
    return [f for f in b.FLAGS if f != "-shared"], b.hipcc()


def compile_unit(tree, unit, flags, hipcc, out_dir, tag):
    src = os.path.join(tree, "gr_adsb_amd", "csrc", unit)
    return subprocess.Popen([hipcc] + flags + ["--cuda-device-only", "-c", src, "-o", os.path.join(out_dir, tag + ".bundle")])


def disassemble(out_dir, tag):
    bundle = os.path.join(out_dir, tag + ".bundle")
    elf = os.path.join(out_dir, tag + ".co")
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950", "--unbundle",
                    "--input=" + bundle, "--output=" + elf], check=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", elf], check=True,
                          stdout=subprocess.PIPE, text=True).stdout
    with open(os.path.join(out_dir, tag + ".s"), "w") as f:
        f.write(text)
    return functions(text)


def functions(text):
    """llvm-objdump -d -> {symbol: [instruction text, ...]}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        line = line.split("//")[0]                     # the address (and, where shown, the encoding) behind the instruction
        line = re.sub(r"\s*<[^>]*>\s*$", "", line)     # a branch's target annotation
        line = " ".join(line.split())
        if line:
            cur.append(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--unit", default="adsb_hip.hip")
    ap.add_argument("--keep", help="keep the code objects and disassemblies in this directory")
    ap.add_argument("--show", action="store_true", help="print each differing function's unified diff")
    a = ap.parse_args()
    flags, hipcc = flags_of(os.path.abspath(a.new))
    with tempfile.TemporaryDirectory(prefix="kernel_code_diff_") as tmp:
        out_dir = a.keep or tmp
        os.makedirs(out_dir, exist_ok=True)
        jobs = [compile_unit(os.path.abspath(t), a.unit, flags, hipcc, out_dir, tag) for t, tag in ((a.parent, "parent"), (a.new, "new"))]
        if any([j.wait() for j in jobs]):
            return 2
        old, new = disassemble(out_dir, "parent"), disassemble(out_dir, "new")
    print("%s, flags %s" % (a.unit, " ".join(flags)))
    print("functions: parent %d, new %d" % (len(old), len(new)))
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("ONLY IN %s: %s" % ("new" if name in new else "parent", name))
            bad += 1
        elif old[name] != new[name]:
            d = list(difflib.unified_diff(old[name], new[name], "parent", "new", lineterm="", n=2))
            changed = sum(1 for l in d if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            print("DIFFERS: %s (%d instructions -> %d, %d changed lines)" % (name, len(old[name]), len(new[name]), changed))
            if a.show:
                print("\n".join("    " + l for l in d))
            bad += 1
    names = sorted(set(old) | set(new))
    print("equal: %d of %d" % (len(names) - bad, len(names)))
    for name in names:
        print("  %s %s" % ("=" if old.get(name) == new.get(name) else "!", name))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

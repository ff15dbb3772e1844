#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds of one .hip file, kernel by kernel, and list the resources of the kernels
only one of them has.  No GPU needed.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip --cuda-device-only -S csrc/bcn_kernels.hip -o <tree>/bcn_kernels.s
    tools/isa_compare.py PARENT.s NEW.s [--new-only REGEX] > report.txt

Kernels are matched by mangled name.  Of each kernel's text (its label to .Lfunc_end) comment lines, blank lines and the
.p2align / .size / .type / .section / .text / .globl / .protected directives are dropped and the local .LBB labels renumbered in
order of appearance; everything else, the .amdhsa_ descriptor lines included, is compared line by line.  Resources are the compiler's own report behind each kernel
(NumVgprs, ScratchSize, Occupancy [waves/SIMD], LDSByteSize)."""
import argparse
import difflib
import re
import subprocess
import sys

DROP = re.compile(r"^\s*(;|$|\.p2align|\.size|\.type|\.section|\.text|\.globl|\.protected|\.weak)")
REPORT = {"vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)",
          "occupancy": r"; Occupancy: (\d+)", "lds": r"; LDSByteSize: (\d+)"}


def kernels_of(path):
    """{mangled name: (normalised lines, resources)} of every .amdhsa_kernel of the file"""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    out = {}
    for name in names:
        start = re.search(r"^" + re.escape(name) + r":", text, re.M).start()
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, start).start()
        tail = text[end:text.index("; Occupancy:", end) + 40]
        labels, lines = {}, []
        for ln in text[start:end].split("\n")[1:]:
            if DROP.match(ln):
                continue
            ln = re.sub(r"\s*;.*$", "", ln).strip()
            ln = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), ln)
            lines.append(ln)
        res = {k: int(re.search(p, tail).group(1)) if re.search(p, tail) else -1 for k, p in REPORT.items()}
        res["vmem"] = sum(1 for ln in lines if re.match(r"(global|flat|buffer|scratch)_(load|store|atomic)", ln))
        out[name] = (lines, res)
    return out


def demangle(names):
    got = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", d)) for n, d in zip(names, got)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--new-only", default=".", help="regex over demangled names: which of the kernels only NEW has are listed")
    ap.add_argument("--beside", nargs=2, metavar=("FROM", "TO"),
                    help="list beside each new kernel the one whose name has ONE template argument FROM replaced by TO")
    a = ap.parse_args()
    old, new = kernels_of(a.parent), kernels_of(a.new)
    pretty = demangle(sorted(set(old) | set(new)))
    differ, gone = [], sorted(set(old) - set(new))
    print(f"== kernels of both files: {len(set(old) & set(new))}; only in the parent: {len(gone)}; only in the new file: {len(set(new) - set(old))}")
    for n in sorted(set(old) & set(new), key=pretty.get):
        if old[n][0] != new[n][0] or old[n][1] != new[n][1]:
            differ.append(n)
    print(f"identical, instruction for instruction, with identical resources: {len(set(old) & set(new)) - len(differ)}; differ: {len(differ)}")
    for n in gone:
        print("only in the parent:", pretty[n])
    for n in differ:
        print(f"\n--- {pretty[n]}   resources parent {old[n][1]} new {new[n][1]}")
        sys.stdout.write("\n".join(difflib.unified_diff(old[n][0], new[n][0], "parent", "new", lineterm="", n=1)) + "\n")
    by_pretty = {pretty[n]: n for n in new}
    print("\n== kernels only in the new file: vgpr / agpr / sgpr / LDS bytes / scratch bytes / waves per SIMD / vector-memory instructions / lines")
    for n in sorted(set(new) - set(old), key=pretty.get):
        if not re.search(a.new_only, pretty[n]):
            continue
        r = new[n][1]
        row = f"{pretty[n]:<78} {r['vgpr']:>3} {r['agpr']:>2} {r['sgpr']:>3} {r['lds']:>6} {r['scratch']:>2} {r['occupancy']:>2} {r['vmem']:>3} {len(new[n][0]):>5}"
        if a.beside:
            parts = re.split(r"([<,>] ?)", pretty[n])
            twins = [by_pretty.get("".join(parts[:i] + [a.beside[1]] + parts[i + 1:])) for i, p in enumerate(parts) if p == a.beside[0]]
            twin = next((t for t in twins if t), None)
            if twin:
                t = new[twin][1]
                row += f"   | plain: {t['vgpr']:>3} {t['agpr']:>2} {t['sgpr']:>3} {t['lds']:>6} {t['scratch']:>2} {t['occupancy']:>2} {t['vmem']:>3} {len(new[twin][0]):>5}"
        print(row)


if __name__ == "__main__":
    main()

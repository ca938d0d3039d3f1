#!/usr/bin/env python3
"""Is the device code of two checkouts the same?  No GPU needed.

    python tools/device_code_diff.py <old checkout> <new checkout> [--units a,b] [--jobs N] [--keep DIR]

For every unit of each checkout's lara_amd/csrc/Makefile the device assembly is emitted with the Makefile's own
command line for that unit (`make -n` tells it; `-c` becomes `--cuda-device-only -S`).  Then, per unit:

  * the sets of kernels (`.amdhsa_kernel` symbols) and of other device functions are compared;
  * for every function in both, the instruction stream, and for every kernel the kernel descriptor (registers, LDS,
    scratch, ...), must be the same text.  Local labels (.LBB<function>_<block>, .Ltmp<n>) are renumbered in order of
    appearance, since a function's index in its unit moves when another one leaves; comments are dropped.

Prints what was removed, added and changed (demangled where a c++filt is found) and exits 1 if anything was added or
changed.  Removals are listed and left to the reader: a refactor states which ones it intends.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def compile_lines(checkout):
    """{unit: argv} from the checkout's own Makefile."""
    csrc = os.path.join(checkout, "lara_amd", "csrc")
    out = subprocess.run(["make", "-n", "-B", "-C", csrc], check=True, capture_output=True, text=True).stdout
    units = {}
    for line in out.splitlines():
        argv = line.split()
        if "-c" not in argv or not any(a.endswith(".hip") for a in argv):
            continue
        src = next(a for a in argv if a.endswith(".hip"))
        units[os.path.splitext(os.path.basename(src))[0]] = (csrc, argv)
    return units


def emit(csrc, argv, dst):
    argv = list(argv)
    i = argv.index("-c")
    argv[i:i + 1] = ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument"]
    argv[argv.index("-o") + 1] = dst
    subprocess.run(argv, check=True, cwd=csrc)
    return dst


def parse(path):
    """{symbol: (is_kernel, [body lines], [descriptor lines])}"""
    functions, bodies, descs = [], {}, {}
    lines = open(path).read().splitlines()
    for line in lines:
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:
            functions.append(m.group(1))
    wanted, cur, desc = set(functions), None, None
    for line in lines:
        s = line.split(";", 1)[0].rstrip() if not line.lstrip().startswith(";;#") else line.rstrip()
        if desc is not None:
            if s.strip() == ".end_amdhsa_kernel":
                desc = None
            elif s.strip():
                descs[desc].append(s.strip())
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", s)
        if m:
            desc = m.group(1)
            descs[desc] = []
            continue
        if cur is None:
            if s.endswith(":") and s[:-1] in wanted:
                cur = s[:-1]
                bodies[cur] = []
            continue
        if re.match(r"\.Lfunc_end\d+:", s.strip()):
            cur = None
        elif s.strip():
            bodies[cur].append(s.strip())
    result = {}
    for name in functions:
        seen = {}
        body = [LOCAL_LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), l) for l in bodies.get(name, [])]
        result[name] = (name in descs, body, descs.get(name, []))
    return result


def demangler():
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    for cand in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        if tool is None and os.path.exists(cand):
            tool = cand
    cache = {}

    def dm(sym):
        if tool is None:
            return sym
        if sym not in cache:
            cache[sym] = subprocess.run([tool, sym], capture_output=True, text=True).stdout.strip() or sym
        return cache[sym]
    return dm


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="keep the .s files in this directory (old_<unit>.s, new_<unit>.s)")
    ap.add_argument("--units", help="comma-separated units to compare (default: all of both Makefiles)")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="devdiff_")
    os.makedirs(work, exist_ok=True)
    dm = demangler()
    try:
        sides = {"old": compile_lines(a.old), "new": compile_lines(a.new)}
        if a.units:
            sides = {side: {u: v for u, v in units.items() if u in a.units.split(",")} for side, units in sides.items()}
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            jobs = {(side, u): pool.submit(emit, csrc, argv, os.path.join(work, "%s_%s.s" % (side, u)))
                    for side, units in sides.items() for u, (csrc, argv) in units.items()}
            asm = {k: parse(f.result()) for k, f in jobs.items()}
        bad = 0
        for u in sorted(set(sides["old"]) | set(sides["new"])):
            if (u in sides["old"]) != (u in sides["new"]):
                print("%-12s unit only in %s" % (u, "old" if u in sides["old"] else "new"))
                bad += 1
                continue
            old, new = asm[("old", u)], asm[("new", u)]
            removed, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
            changed = []
            for name in sorted(set(old) & set(new)):
                what = [w for w, i in (("kind", 0), ("instructions", 1), ("descriptor", 2)) if old[name][i] != new[name][i]]
                if what:
                    changed.append((name, what))
            nk = sum(1 for v in new.values() if v[0])
            print("%-12s %3d kernels, %3d other functions: %d removed, %d added, %d changed"
                  % (u, nk, len(new) - nk, len(removed), len(added), len(changed)))
            for name in removed:
                print("    removed  %s %s" % ("kernel  " if old[name][0] else "function", dm(name)))
            for name in added:
                print("    ADDED    %s %s" % ("kernel  " if new[name][0] else "function", dm(name)))
            for name, what in changed:
                print("    CHANGED  %s (%s)" % (dm(name), ", ".join(what)))
                for i in (1, 2):
                    for d in list(difflib.unified_diff(old[name][i], new[name][i], "old", "new", n=1, lineterm=""))[:40]:
                        print("        " + d)
            bad += len(added) + len(changed)
        print("device code: %s" % ("DIFFERS" if bad else "identical for every function in both builds"))
        return 1 if bad else 0
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())

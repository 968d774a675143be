#!/usr/bin/env python3
"""Do two csrc trees give the same device code?   python tools/kernel_identity.py OLD_CSRC NEW_CSRC kernels.hip kernels_ks.hip ...

Each source is compiled in both trees with build.py's FLAGS + EXTRA and `-S --cuda-device-only`; the listing is cut per function symbol (kernels and
the device functions they call), comments, labels and assembler directives are dropped, and the function number inside branch targets (.LBB<fn>_<n>) is
taken out: it is the function's position in the module, so that adding or removing one function would report every later one.  Prints IDENTICAL or DIFF per symbol with the instruction
counts of both sides, and every difference in the kernels' metadata (registers, spills, scratch, LDS).  Exit status 1 on any DIFF.  Whole instruction
streams are compared, whatever they contain.  --asm-dir DIR keeps the listings (DIR/old, DIR/new); a listing newer than every file of its tree is
reused, so the unchanged side of a comparison is compiled once.  --flags "-DSNERF_ABLATE -DABL=2" appends flags to both sides (a diagnostic
build; give each set of flags an --asm-dir of its own)."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "season_nerf_amd"))
import build  # noqa: E402

META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size"]


def listing(tree, src, out, flags=()):
    newest = max(os.path.getmtime(os.path.join(tree, f)) for f in os.listdir(tree))
    if not (os.path.exists(out) and os.path.getmtime(out) > newest):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([build._hipcc()] + build.FLAGS + build.EXTRA.get(src, []) + list(flags) + ["-S", "--cuda-device-only", os.path.join(tree, src), "-o", out])
    return open(out).read()


def functions(asm):
    """symbol -> its instruction lines"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"\s*\.type\s+([\w$.]+),@function", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif re.match(r"\s*\.size\s", line):
            cur = None
        text = re.sub(r"\s+", " ", re.split(r";|//", line)[0]).strip()
        text = re.sub(r"\.LBB\d+_", ".LBB_", text)      # a branch label carries its function's position in the module: not code, and it moves when a function above goes
        if cur is not None and text and not text.endswith(":") and not text.startswith("."):
            cur.append(text)
    return out


def metadata(asm):
    """kernel symbol -> the values of META, from the amdhsa.kernels list of the listing's metadata block"""
    out, cur = {}, {}
    for m in re.finditer(r"^  (-| ) (\.\w+):\s*(.*)$", asm.split("amdhsa.kernels:", 1)[-1], re.M):
        if m.group(1) == "-":
            cur = {}
        cur[m.group(2)] = m.group(3)
        if m.group(2) == ".symbol":
            out[m.group(3).replace(".kd", "")] = cur
    return {k: [v.get(q) for q in META] for k, v in out.items()}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    return dict(zip(names, subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--asm-dir", default=None)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides, in one string")
    a = ap.parse_args()
    keep = a.asm_dir or tempfile.mkdtemp(prefix="kernel_identity_")
    jobs = [(side, tree, s) for s in a.sources for side, tree in (("old", a.old), ("new", a.new))]
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        asm = dict(zip([(side, s) for side, _, s in jobs], ex.map(lambda j: listing(j[1], j[2], os.path.join(keep, j[0], j[2] + ".s"), a.flags.split()), jobs)))
    n_diff = 0
    for s in a.sources:
        fo, fn, mo, mn = functions(asm["old", s]), functions(asm["new", s]), metadata(asm["old", s]), metadata(asm["new", s])
        names = demangle(sorted(set(fo) | set(fn)))
        print(f"== {s}: {len(names)} symbols, {len(mn)} kernels")
        for sym in sorted(names, key=names.get):
            same = fo.get(sym) == fn.get(sym) and mo.get(sym) == mn.get(sym)
            n_diff += not same
            print(f"{'IDENTICAL' if same else 'DIFF':9s} {len(fo.get(sym, [])):6d} {len(fn.get(sym, [])):6d}  {names[sym]}")
            if mo.get(sym) != mn.get(sym):
                old, new = mo.get(sym) or [None] * len(META), mn.get(sym) or [None] * len(META)
                print("          metadata: " + ", ".join(f"{q} {x} -> {y}" for q, x, y in zip(META, old, new) if x != y))
    print(f"{n_diff} DIFF" if n_diff else "all IDENTICAL, metadata equal")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the device code of the back-end units of two trees, function by function, as text.  No GPU needed.

    tools/kernel_text_diff.py A B [--timers] [--jobs N]

A and B are each a directory of .s files (device assembly) or a source tree, whose csrc/be_*.hip are then compiled to device assembly with the
Makefile's flags (--timers: with -DVIO_PHASE_TIMERS).  Every function ( __global__ kernel or device function that was not inlined) is one
symbol; its text is its instructions with comments stripped and block labels normalised (.LBB<n>_ -> .LBB_: <n> counts the functions of the
unit in front of it).  Per symbol of either side one line:
    same   the text is equal (a symbol that several units of a side hold must be equal in all of them)
    DIFF   it is not
    new    only B has it        gone   only A has it
Exit status 1 when any line is DIFF, new or gone."""
import argparse, glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -Wno-unused-variable --cuda-device-only -S".split()


def assemble(tree, timers, jobs, keep):
    csrc = os.path.join(tree, "vins-rgbd-fast_amd", "csrc")
    out = tempfile.mkdtemp(prefix="kernel_text_")
    keep.append(out)
    srcs = sorted(glob.glob(os.path.join(csrc, "be_*.hip")))
    if not srcs:
        sys.exit("no be_*.hip under " + csrc)

    def one(src):
        dst = os.path.join(out, os.path.basename(src)[:-4] + ".s")
        subprocess.run([HIPCC] + FLAGS + (["-DVIO_PHASE_TIMERS"] if timers else []) + [os.path.basename(src), "-o", dst], cwd=csrc, check=True,
                       stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, srcs))
    return out


def functions(path):
    """{symbol: normalised text} of one .s file"""
    fns, types, cur, body = {}, set(), None, []
    for line in open(path):
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", line)
        if m:
            types.add(m.group(1))
            continue
        m = re.match(r"([\w.$]+):", line)
        if cur is None and m and m.group(1) in types:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            fns[cur] = "\n".join(body)
            cur = None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        if line:
            body.append(line)
    return fns


def side(arg, timers, jobs, keep):
    d = arg if glob.glob(os.path.join(arg, "*.s")) else assemble(arg, timers, jobs, keep)
    sym = {}
    for f in sorted(glob.glob(os.path.join(d, "*.s"))):
        for k, v in functions(f).items():
            sym.setdefault(k, []).append((os.path.basename(f), v))
    return sym


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--timers", action="store_true")
    ap.add_argument("--jobs", type=int, default=4)
    o = ap.parse_args()
    keep = []
    A, B = side(o.a, o.timers, o.jobs, keep), side(o.b, o.timers, o.jobs, keep)
    bad = 0
    for k in sorted(set(A) | set(B)):
        if k not in A:
            verdict = "new "
        elif k not in B:
            verdict = "gone"
        else:
            verdict = "same" if len({v for _, v in A[k] + B[k]}) == 1 else "DIFF"
        bad += verdict != "same"
        where = lambda S: ",".join(f for f, _ in S.get(k, [])) or "-"
        lines = (A.get(k) or B.get(k))[0][1].count("\n") + 1
        print("%s  %-72s %6d lines   %s -> %s" % (verdict, k, lines, where(A), where(B)))
    print("%d symbols, %d not the same" % (len(set(A) | set(B)), bad))
    for d in keep:
        for f in glob.glob(os.path.join(d, "*.s")):
            os.remove(f)
        os.rmdir(d)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

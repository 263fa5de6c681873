#!/usr/bin/env python3
r"""Static instruction mix of a rollout kernel's time loop, from hipcc's assembly listing.

    hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -I include -DAMPC_T=double -DAMPC_T_IS_F64=1 \
          --cuda-device-only -S autompc_amd/csrc/launch_mppi.cpp -o mppi_f64.s
    python tools/rollout_valu.py mppi_f64.s [--kernel SUBSTRING ...] [--blocks] [--no-lines]

The time loop is the loop of the kernel that holds the most MFMAs: the lines from its header label to
the last branch back to that label (the tightest such range: blocks that hipcc places ahead of the
header, like the dense-cost path that a diagonal cost never enters, are left out).  Every instruction in
it is classified by the PREFIX of its opcode only (v_mfma -> MFMA, other v_ -> VALU, s_ -> SALU,
ds_ -> LDS, buffer_/global_/flat_/scratch_ -> VMEM); VALU instructions are listed by opcode.  Nothing is
weighted by how often a block runs: blocks that a wave skips (a predicated side path) count like the
others, which is what the per-wave-step figures in DESIGN.md mean.  Default kernel: the c3 relu
instantiation (StaticShape<17,6,17,2,256,0,0>, 16-row tile).
"""
import argparse
import collections
import re
import subprocess
import sys

C3 = ["mppi_rollout_kernel", "Li2ELi1ELi8E", "StaticShapeILi17ELi6ELi17ELi2ELi256ELi0ELi0E"]


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    return "other"


def kernels(lines):
    """(name, first line, last line) of every function body in the listing."""
    out, name, start = [], None, 0
    for n, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, start = m.group(1), n
        elif name is not None and ln.startswith(".Lfunc_end"):
            out.append((name, start, n))
            name = None
    return out


def instructions(lines, lo, hi):
    """(line number, label of the enclosing block, opcode) of lines [lo, hi)."""
    block = "entry"
    for n in range(lo, hi):
        ln = lines[n]
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            block = m.group(1)
            continue
        if not ln.startswith("\t") or ln.startswith("\t.") or ln.startswith("\t;"):
            continue
        yield n, block, ln.split()[0]


def time_loop(lines, lo, hi):
    """Line range of the loop with the most MFMAs: header label .. last branch back to it."""
    label_at = {}
    for n in range(lo, hi):
        m = re.match(r"^(\.LBB\w+):", lines[n])
        if m:
            label_at[m.group(1)] = n
    best = None
    for lab, at in label_at.items():
        back = [n for n in range(at, hi) if re.match(r"^\ts_c?branch\w*\s+" + re.escape(lab) + r"\s*$", lines[n])]
        if not back:
            continue
        end = back[-1] + 1
        mf = sum(1 for _, _, op in instructions(lines, at, end) if classify(op) == "MFMA")
        if best is None or (mf, at - end) > (best[0], best[1] - best[2]):      # ties: the tightest range
            best = (mf, at, end)
    return best


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("--kernel", nargs="*", default=C3, help="substrings the mangled kernel name must contain")
    ap.add_argument("--blocks", action="store_true", help="also print the counts per basic block")
    ap.add_argument("--no-lines", action="store_true", help="leave out the listing's line numbers (tables kept in profiles/)")
    args = ap.parse_args()
    lines = open(args.listing).read().split("\n")
    found = [k for k in kernels(lines) if all(s in k[0] for s in args.kernel)]
    if not found:
        sys.exit("no kernel matches %s" % args.kernel)
    for name, lo, hi in found:
        loop = time_loop(lines, lo, hi)
        if loop is None:
            sys.exit("%s: no loop found" % name)
        _, at, end = loop
        cls = collections.Counter()
        valu = collections.Counter()
        mfma = collections.Counter()
        per_block = collections.OrderedDict()
        for _, block, op in instructions(lines, at, end):
            c = classify(op)
            cls[c] += 1
            per_block.setdefault(block, collections.Counter())[c] += 1
            if c == "VALU":
                valu[op] += 1
            if c == "MFMA":
                mfma[op] += 1
        foot = {}
        for n in range(hi, min(hi + 40, len(lines))):
            m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy|NumSgprs): (\d+)", lines[n])
            if m:
                foot[m.group(1)] = int(m.group(2))
        print(demangle(name))
        print("  registers: %s" % "  ".join("%s %d" % kv for kv in sorted(foot.items())))
        if not args.no_lines:
            print("  time loop: listing lines %d-%d" % (at + 1, end))
        print("  %s" % "  ".join("%s %d" % (k, cls[k]) for k in ("VALU", "MFMA", "LDS", "VMEM", "SALU", "other")))
        print("  MFMA: %s" % "  ".join("%s %d" % kv for kv in sorted(mfma.items())))
        print("  VALU by opcode:")
        for op, n in sorted(valu.items(), key=lambda kv: (-kv[1], kv[0])):
            print("    %-24s %3d" % (op, n))
        if args.blocks:
            print("  per block:")
            for block, c in per_block.items():
                print("    %-12s %s" % (block, "  ".join("%s %d" % (k, c[k]) for k in ("VALU", "MFMA", "LDS", "VMEM", "SALU") if c[k])))
        print()


if __name__ == "__main__":
    main()

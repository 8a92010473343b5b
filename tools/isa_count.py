#!/usr/bin/env python3
"""Opcode histogram of one kernel per loop nest, from the gfx950 assembly the library's flags give (CPU only):

    tools/isa_count.py geneticscre_amd/csrc/gcre_ieq.hip 'k_null_ie_q<10,2,true,false>' [--blocks] [--asm=FILE] [extra hipcc flags...]

The compiler annotates every basic block with the loop it belongs to (`Loop Header` / `in Loop: Header=... Depth=...`
comments); an instruction is counted for the innermost loop that holds its block, so a loop's own line excludes its
child loops.  The counts are static: every block of a loop, rare paths included.  --blocks adds the instruction count
of every basic block, for adding up one path through a loop by hand; --asm=FILE keeps the kernel's assembly.  The
resource-usage remarks of the kernel (registers, spills, scratch, occupancy) are printed in front.  Any opcode that
occurs is counted; nothing is searched for."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geneticscre_amd import build as b  # noqa: E402


def squeeze(s):
    return re.sub(r"\s+", "", s)


def compile_asm(src, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        cmd = [hipcc, *b.BASE_FLAGS, *extra, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr)
        with open(out) as f:
            return f.read().splitlines(), r.stderr.splitlines()


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    r = subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def unit_of(op):
    if op.startswith("s_"):
        if op.startswith(("s_load", "s_buffer_load")):
            return "SMEM"
        if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
            return "branch"
        if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier")):
            return "wait/nop"
        return "SALU"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    return "VALU"


def main():
    args = sys.argv[1:]
    blocks = "--blocks" in args
    keep = [x[6:] for x in args if x.startswith("--asm=")]
    args = [x for x in args if x != "--blocks" and not x.startswith("--asm=")]
    if len(args) < 2:
        sys.exit(__doc__)
    src, want, extra = args[0], squeeze(args[1]), args[2:]
    asm, remarks = compile_asm(src, extra)

    kernels = [m.group(1) for m in (re.match(r"^([A-Za-z_][\w.$]*):\s*; @", ln) for ln in asm) if m]
    names = demangle(kernels)
    hits = [k for k in kernels if want in squeeze(names[k])]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels match {args[1]!r}:\n" + "\n".join(names[k] for k in (hits or kernels)))
    kern = hits[0]
    print(f"kernel: {names[kern]}")
    print(f"flags:  {' '.join(b.BASE_FLAGS + extra)}")

    on = False
    for ln in remarks:
        m = re.search(r"remark:\s*(.*?)\s*\[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1).startswith("Function Name:"):
            on = m.group(1).split()[-1] == kern
        elif on:
            print("  " + m.group(1))

    begin = next(i for i, ln in enumerate(asm) if ln.startswith(kern + ":"))
    end = next(i for i in range(begin, len(asm)) if asm[i].startswith(".Lfunc_end"))
    if keep:
        with open(keep[0], "w") as f:
            f.write("\n".join(asm[begin:end]) + "\n")
    # loop key: (header label, depth); "" = outside every loop
    hist = collections.OrderedDict()
    hist[("", 0)] = collections.Counter()
    parent = {}
    cur = ("", 0)
    label, per_block, pending_parent = "entry", [], ""
    n_block = 0
    for ln in asm[begin + 1:end]:
        m = re.match(r"^\.(LBB\d+_\d+):", ln) or re.match(r"^; (%bb\.\d+):", ln)
        if m:
            if blocks:
                per_block.append((label, cur, n_block))
            label, n_block = m.group(1), 0
            cur = ("", 0)   # until an annotation says otherwise
        text = ln.split(";", 1)
        if len(text) == 2:
            c = text[1]
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", c)
            if m:
                cur = ("L" + m.group(1), int(m.group(2)))
            m = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", c)
            if m:
                cur = (label, int(m.group(1)))
                hist.setdefault(cur, collections.Counter())
                parent[cur] = pending_parent if int(m.group(1)) > 1 else ""
            m = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", c)
            if m:
                pending_parent = "L" + m.group(1)
        code = text[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        hist.setdefault(cur, collections.Counter())[code.split()[0]] += 1
        n_block += 1
    if blocks:
        per_block.append((label, cur, n_block))

    for (hdr, depth), h in hist.items():
        total = sum(h.values())
        units = collections.Counter()
        for op, n in h.items():
            units[unit_of(op)] += n
        where = "outside every loop" if not hdr else f"loop {hdr} depth {depth}" + (f" in {parent[(hdr, depth)]}" if parent.get((hdr, depth)) else "")
        print(f"\n{'  ' * depth}{where}: {total} instructions  (" + ", ".join(f"{u} {n}" for u, n in sorted(units.items())) + ")")
        for op, n in sorted(h.items(), key=lambda x: (-x[1], x[0])):
            print(f"{'  ' * depth}  {n:5d}  {op}")
    if blocks:
        print("\nbasic blocks (label, innermost loop, instructions):")
        for lab, (hdr, depth), n in per_block:
            print(f"  {lab:12s} {hdr or '-':12s} {n:5d}")


if __name__ == "__main__":
    main()

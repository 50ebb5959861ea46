#!/usr/bin/env python
"""How the rolling Gaussian kernel keeps its row loads in flight, read from the compiler's own gfx950 assembly.  No GPU needed:

    python tools/ring_isa.py 5,1,true,false,4,true,true          # template arguments of the k_binomial_roll2 instantiation
    python tools/ring_isa.py 5,1,true,false,4,true,false opencv_amd/csrc/smooth.hip k_binomial_roll2

For the named instantiation it prints, in program order, every global_load / global_store and every `s_waitcnt vmcnt(N)` with the basic block
it sits in, and whether the assembler marks that block as part of a loop; then the registers and the scratch size.  A ring of KS rows that
stays in flight shows waits of 2 (KS - 1) or more inside the loop (two loads per row with one channel); vmcnt(0) / vmcnt(1) there is a drain.
Counts are static: a loop body is listed once."""
import os
import re
import shutil
import subprocess
import sys

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH = os.path.join(ROOT, "opencv_amd", "csrc", "smooth.hip")


def hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


def compile_asm(src=SMOOTH):
    inc = ["-I" + os.path.dirname(os.path.abspath(src)), "-I" + os.path.dirname(SMOOTH), "-I" + os.path.join(ROOT, "include")]
    return subprocess.run([hipcc()] + FLAGS + inc + ["-S", src, "-o", "-"], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout


def mangled(fn, targs):
    """the part of the Itanium name of fn<targs> that names the instantiation (integer and bool template arguments), whatever namespace it is in"""
    frag = ""
    for a in targs.replace(" ", "").split(","):
        frag += "Lb%dE" % (a == "true") if a in ("true", "false") else "Li%dE" % int(a)
    return "%d%sI%sE" % (len(fn), fn, frag)


def events(asm, inst):
    """[(kind, arg, block, in_loop)] in program order for the one kernel whose symbol contains inst (see mangled()): kind is 'load' / 'store' (arg: the
    mnemonic) or 'wait' (arg: N of vmcnt(N)); plus the symbol itself"""
    lines = asm.split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*?%sE?v\w*:" % re.escape(inst), l)]
    if len(starts) != 1:
        raise SystemExit("%d kernels match %s" % (len(starts), inst))
    sym = lines[starts[0]].split(":")[0]
    out, block, in_loop, fresh = [], "entry", False, False
    for l in lines[starts[0] + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            block, in_loop, fresh = m.group(1), False, True
            t = t.split(":", 1)[1].strip()
        if t.startswith(";"):
            # the assembler's loop notes follow the label: "=>This Inner Loop Header", "in Loop: Header=...", "Parent Loop ..."
            if fresh and ("Loop Header" in t or "in Loop:" in t or "Parent Loop" in t):
                in_loop = True
            continue
        if not t or t.startswith("."):
            continue
        fresh = False
        op = t.split()[0]
        if op.startswith("global_load") or op.startswith("buffer_load"):
            out.append(("load", op, block, in_loop))
        elif op.startswith("global_store") or op.startswith("buffer_store"):
            out.append(("store", op, block, in_loop))
        elif op == "s_waitcnt":
            w = re.search(r"vmcnt\((\d+)\)", t)
            if w:
                out.append(("wait", int(w.group(1)), block, in_loop))
    return sym, out


def resources(asm, sym):
    m = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, re.S)
    body = m.group(1)
    g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))
    return {"vgpr": g("next_free_vgpr"), "scratch": g("private_segment_fixed_size")}


def loop_waits(ev):
    return [a for k, a, _, lp in ev if k == "wait" and lp]


def loads_before_first_wait(ev):
    n = 0
    for k, a, _, _ in ev:
        if k == "wait":
            break
        n += k == "load"
    return n


def main():
    targs = sys.argv[1] if len(sys.argv) > 1 else "5,1,true,false,4,true,true"
    src = sys.argv[2] if len(sys.argv) > 2 else SMOOTH
    fn = sys.argv[3] if len(sys.argv) > 3 else "k_binomial_roll2"
    asm = compile_asm(src)
    sym, ev = events(asm, mangled(fn, targs))
    print("%s<%s>  (%s)" % (fn, targs, sym))
    run = []

    def flush():
        if run:
            print("    %-10s %-8s %d x %s" % (run[0][2], "loop" if run[0][3] else "", len(run), run[0][1]))
            del run[:]
    for e in ev:
        if e[0] == "wait":
            flush()
            print("    %-10s %-8s s_waitcnt vmcnt(%d)" % (e[2], "loop" if e[3] else "", e[1]))
        else:
            if run and (run[0][1], run[0][2]) != (e[1], e[2]):
                flush()
            run.append(e)
    flush()
    r = resources(asm, sym)
    lw = loop_waits(ev)
    print("    vmcnt waits inside loops: %s   (min %s)" % (sorted(set(lw)), min(lw) if lw else None))
    print("    loads issued before the first vmcnt wait: %d" % loads_before_first_wait(ev))
    print("    VGPRs %d  scratch %d bytes" % (r["vgpr"], r["scratch"]))


if __name__ == "__main__":
    main()

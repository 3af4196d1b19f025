#!/usr/bin/env python3
"""Static mix of the vector (v_*) instructions of one kernel of the gfx950 code object, by class (tuning aid; needs no GPU):
    python tools/valu_mix.py [UNIT.hip] [KERNEL] [--zeros] [-D... extra compiler flags]
--zeros: instead of the mix, the zero-materialising moves (v_mov_b32 / v_mov_b64 of the constant 0) per source line, from a build with -gline-tables-only.
UNIT.hip: one of the library's translation units by file name (_lib.SOURCES; default: the base one, hrgym_hip.hip); KERNEL: a function of that unit by its name
without the parameter list, or by its symbol (default: hrg_step_kernel).  The unit is compiled with the flags of _lib.build_library.  A static count: every instruction of the function once,
whether it sits on the always-executed path or in a cold branch; s_nop is counted next to it because the DPP and lane-access hazards pad with it."""
import collections, glob, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from human_robot_gym_amd import _lib

CLASSES = ("f64 arithmetic", "DPP moves", "plain moves", "selects", "compares", "lane reads/writes", "other")


def classify(op):
    """The class of one v_* mnemonic."""
    if op.endswith("_dpp"):
        return "DPP moves" if op.startswith("v_mov_") else "other"
    if re.match(r"v_(readlane|writelane|readfirstlane)_b32", op):
        return "lane reads/writes"
    if op.startswith("v_cmp"):
        return "compares"
    if op.startswith("v_cndmask_"):
        return "selects"
    if re.match(r"v_(mov_b32|mov_b64|accvgpr_read|accvgpr_write|accvgpr_mov)", op):
        return "plain moves"
    if "f64" in op:
        return "f64 arithmetic"
    return "other"


def kernel_body(asm, kernel):
    """The instruction lines of function `kernel`: from its label to the end-of-function label."""
    names = re.findall(r"\.type\s+(\S+),@function", asm)
    plain = {n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.split("(")[0].strip() for n in names}
    hits = [n for n in names if kernel in (n, plain[n])]   # by the symbol or by its demangled name without the parameter list
    if len(hits) != 1:
        raise SystemExit("no single function %r in the unit; it has: %s" % (kernel, " ".join(sorted(set(plain.values())))))
    m = re.search(r"^%s:.*$" % re.escape(hits[0]), asm, re.M)
    end = re.search(r"^\.Lfunc_end\d+:", asm[m.end():], re.M)
    return asm[m.end():m.end() + end.start()] if end else asm[m.end():]


def mix(body):
    """(Counter of the classes, Counter of the mnemonics, number of s_nop) of an assembly text."""
    by_class, by_op, nops = collections.Counter(), collections.Counter(), 0
    for line in body.splitlines():
        m = re.match(r"\s*([vs]_[a-z0-9_]+)", line)
        if not m:
            continue
        op = re.sub(r"_(e32|e64|sdwa)$", "", m.group(1))
        if op == "s_nop":
            nops += 1
        if op.startswith("v_"):
            by_class[classify(op)] += 1
            by_op[op] += 1
    return by_class, by_op, nops


def zero_moves(body, files):
    """Counter {(file name, line): zero-materialising moves (v_mov_b32 / v_mov_b64 of the constant 0 into a vector register)} of an assembly text that carries
    .loc directives (-gline-tables-only); `files`: {number: name} of the .file table."""
    at, out = ("?", 0), collections.Counter()
    for line in body.splitlines():
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            at = (files.get(int(m.group(1)), "?"), int(m.group(2)))
        elif re.match(r"\s*v_mov_b(32|64)(_e32|_e64)?\s+v\S*,\s*0\s*(;.*)?$", line):
            out[at] += 1
    return out


def file_table(asm):
    """{number: base name} of the .file directives."""
    return {int(n): os.path.basename(name) for n, name in re.findall(r'^\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', asm, re.M)}


def main(argv):
    args = list(argv)
    zeros = "--zeros" in args
    if zeros:
        args.remove("--zeros")
        args.append("-gline-tables-only")
    src = _lib.SRC
    if args and args[0].endswith(".hip"):
        src = {os.path.basename(s): s for s in _lib.SOURCES}[os.path.basename(args.pop(0))]
    kernel = args.pop(0) if args and not args[0].startswith("-") else "hrg_step_kernel"
    d = tempfile.mkdtemp()
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-save-temps", "-Wno-unused-value", "-Xarch_device", "-fapprox-func", "-mllvm", "-disable-machine-licm",
                    *args, "-o", "t.o", src], cwd=d, stderr=subprocess.DEVNULL, check=True)
    asm = open(glob.glob(d + "/*gfx950*.s")[0]).read()
    if zeros:
        z = zero_moves(kernel_body(asm, kernel), file_table(asm))
        print("%s of %s: zero-materialising moves (v_mov_b32 / v_mov_b64 v, 0) by source line (static): %d" % (kernel, os.path.basename(src), sum(z.values())))
        for (f, ln), n in sorted(z.items()):
            print("  %-22s %5d  %4d" % (f, ln, n))
        return
    by_class, by_op, nops = mix(kernel_body(asm, kernel))
    print("%s of %s: v_* instructions by class (static)" % (kernel, os.path.basename(src)))
    for c in CLASSES:
        print("  %-18s %6d" % (c, by_class[c]))
    print("  %-18s %6d" % ("total", sum(by_class.values())))
    print("  %-18s %6d" % ("s_nop", nops))
    for op in ("v_mov_b32_dpp", "v_mov_b32", "v_max_f64", "v_cndmask_b32", "v_readlane_b32", "v_writelane_b32"):
        print("  . %-16s %6d" % (op, by_op[op]))


if __name__ == "__main__":
    main(sys.argv[1:])

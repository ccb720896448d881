#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every csrc object between two trees (CPU only).

    tools/asm_compare.py PARENT_TREE BRANCH_TREE [object ...]

Each .hip is compiled with the command line `make -n -B -C csrc` prints for it (per-object
flags included) plus --cuda-device-only -S.  Lines holding the source hash symbol
(__hip_cuid_) are dropped; the rest must be byte-identical.  Per kernel it prints the
register, LDS and scratch metadata and the code size.  Exit status 1 on any difference.
"""
import glob, os, re, shlex, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
CODE_LEN = r"^; codeLenInByte = (\d+)"   # one per function, in the order of the .type lines


def commands(tree):
    csrc = os.path.dirname(glob.glob(os.path.join(tree, "*", "csrc", "Makefile"))[0])
    out = subprocess.run(["make", "-n", "-B", "-C", csrc], check=True, capture_output=True,
                         text=True).stdout
    cmds = {}
    for line in out.splitlines():
        m = re.search(r" -c (\w+)\.hip -o \S+$", line)
        if m:
            args = [a for a in shlex.split(line[:m.start()]) if a not in ("-MMD", "-MP")]
            cmds[m.group(1)] = (csrc, args + ["--cuda-device-only", "-S", m.group(1) + ".hip"])
    return cmds


def assemble(job):
    (csrc, args), out = job
    subprocess.run(args + ["-o", out], cwd=csrc, check=True)
    with open(out) as f:
        return "".join(l for l in f if "__hip_cuid_" not in l)


def kernels(asm):
    size = dict(zip(re.findall(r"^\s*\.type\s+(\w+),@function", asm, re.M),
                    re.findall(CODE_LEN, asm, re.M)))
    for k in re.split(r"^\s*- \.agpr_count:", asm.split("amdhsa.kernels:")[-1], flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", k, re.M).group(1)
        meta = [re.search(r"^\s*\%s:\s*(\d+)" % f, k, re.M).group(1) for f in FIELDS]
        yield name, "vgpr %s sgpr %s lds %s scratch %s code %s" % (*meta, size.get(name, "?"))


def main():
    parent, branch = commands(sys.argv[1]), commands(sys.argv[2])
    names = sys.argv[3:] or sorted(set(parent) | set(branch))
    bad = 0
    workers = min(8, os.cpu_count() or 1)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(workers) as pool:
        jobs = [(tree[n], os.path.join(tmp, "%s_%d.s" % (n, i)))
                for n in names for i, tree in enumerate((parent, branch))]
        asm = list(pool.map(assemble, jobs))
    for i, n in enumerate(names):
        a, b = asm[2 * i], asm[2 * i + 1]
        bad += a != b
        code = sum(int(x) for x in re.findall(CODE_LEN, b, re.M))
        print("%s: %s (code %d bytes)" % (n, "identical" if a == b else "DIFFERENT", code))
        ka = dict(kernels(a))
        for name, meta in kernels(b):
            was = "" if ka.get(name) == meta else "  [parent: %s]" % ka.get(name)
            print("    %s %s%s" % (name, meta, was))
    print("%d of %d objects differ" % (bad, len(names)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

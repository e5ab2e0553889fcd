#!/usr/bin/env python3
"""Are the device code objects of two builds of this library the same?  (No GPU needed.)

For every .hip unit: the gfx950 code object is taken out of the object file each build made, disassembled, and compared kernel by
kernel; the compiler's resource lines (VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy) come from compiling the unit's device side once
more per tree with -Rpass-analysis=kernel-resource-usage and the Makefile's flags.

    make -C <tree A>/csrc variant NAME=a && make -C <tree B>/csrc variant NAME=b
    scripts/codeobj_compare.py <tree A>/csrc/build/var_a <tree B>/csrc/build/var_b [LABEL_A LABEL_B] > profiles/<name>.txt

A kernel of equal length whose differing lines each keep opcode, destination and the multiset of source operands reads COMM and counts
as same: the compiler wrote the sources of an instruction in another order (the report names the opcodes, so that the reader sees they
commute).  Any other difference in the code reads CODE, with the number of differing lines and whether the opcode histograms agree.

Exit status 1 when anything differs beyond COMM."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def disassembly(obj, tmp):
    """kernel name -> its instruction lines (addresses and encodings included)"""
    fat = os.path.join(tmp, "fat.bin"); co = os.path.join(tmp, "dev.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co])
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)
    out, name = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1); out[name] = []
        elif name and line.strip():
            out[name].append(line.strip())
    return out


def parse(line):
    """(opcode, destination, sorted source operands) of a disassembly line"""
    op, _, rest = line.split("//")[0].strip().partition(" ")
    args = [a.strip() for a in rest.split(",")] if rest.strip() else []
    return op, args[:1], sorted(args[1:])


def code_diff(a, b):
    """how two kernels' instruction lines differ: (number of differing lines or None when the lengths differ, the opcodes of the differing
    lines when every one of them is the same instruction with its sources in another order, else None, opcode histograms equal)"""
    hist = sorted(parse(x)[0] for x in a) == sorted(parse(x)[0] for x in b)
    if len(a) != len(b):
        return None, None, hist
    pairs = [(parse(x), parse(y)) for x, y in zip(a, b) if x != y]
    return len(pairs), sorted({x[0] for x, _ in pairs}) if all(x == y for x, y in pairs) else None, hist


def resources(src, include):
    """kernel name -> {field: value}, from the compiler's remarks"""
    cmd = [HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-I" + include, "--cuda-device-only", "-c", src, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1); out[name] = {}
            continue
        m = re.search(r"remark: \s*(.+?): (\d+) \[-Rpass", line)
        if m and name and m.group(1).strip() in FIELDS:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def main():
    if len(sys.argv) not in (3, 5):
        sys.exit(__doc__)
    dirs = [os.path.abspath(d) for d in sys.argv[1:3]]
    labels = sys.argv[3:5] or [os.path.join(*d.split(os.sep)[-2:]) for d in dirs]
    csrc = []
    for d in dirs:                                                              # the sources: the directory above the build that holds the Makefile
        while not os.path.exists(os.path.join(d, "Makefile")):
            d = os.path.dirname(d)
        csrc.append(d)
    units = sorted(f[:-4] for f in os.listdir(csrc[1]) if f.endswith(".hip"))
    jobs = [(u, k) for u in units for k in (0, 1)]
    with ThreadPoolExecutor(max_workers=8) as pool:
        res = dict(zip(jobs, pool.map(lambda j: resources(os.path.join(csrc[j[1]], j[0] + ".hip"), os.path.join(csrc[j[1]], "..", "..", "include")), jobs)))
    print("device code objects, gfx950: A = %s\n                             B = %s" % tuple(labels))
    differ = n_comm = 0
    for u in units:
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            da, db = disassembly(os.path.join(dirs[0], u + ".o"), ta), disassembly(os.path.join(dirs[1], u + ".o"), tb)
        ra, rb = res[(u, 0)], res[(u, 1)]
        print("\n%s.hip: %d kernels in A, %d in B" % (u, len(da), len(db)))
        print("  %-7s %6s %5s %5s %5s %7s %6s %4s  %s" % ("code", "instr", "VGPR", "AGPR", "SGPR", "scratch", "LDS", "occ", "kernel"))
        for name in sorted(set(da) | set(db)):
            same_code = da.get(name) == db.get(name)
            # (a device function that is called, not inlined, is a symbol of the code object without remarks of its own: its code alone is compared)
            same_res = ra.get(name) == rb.get(name) and (len(ra.get(name, {})) == len(FIELDS) or (name not in ra and name not in rb))
            r = rb.get(name) or ra.get(name) or {}
            n_lines, comm, hist = (0, None, True) if same_code else code_diff(da.get(name, []), db.get(name, []))
            verdict = "same" if same_code and same_res else ("RES" if same_code else "COMM" if comm and same_res else "CODE")
            differ += verdict not in ("same", "COMM")
            print("  %-7s %6d %5s %5s %5s %7s %6s %4s  %s" % ((verdict, len(db.get(name, da.get(name, [])))) + tuple(r.get(f, "-") for f in FIELDS[:4]) +
                                                                 (r.get(FIELDS[5], "-"), r.get(FIELDS[4], "-"), name)))
            if verdict == "COMM":
                print("          %d lines with their sources in another order: %s" % (n_lines, " ".join(comm)))
                n_comm += 1
            elif verdict != "same":
                print("          A: %d instr, %s\n          B: %d instr, %s" % (len(da.get(name, [])), ra.get(name), len(db.get(name, [])), rb.get(name)))
                if not same_code:
                    print("          %s lines differ, opcode histograms %s" % ("-" if n_lines is None else n_lines, "equal" if hist else "DIFFER"))
    same_txt = "every kernel's disassembly and resource lines are identical" + (", but for %d with commuted sources (COMM)" % n_comm if n_comm else "")
    print("\nverdict: %s" % (same_txt if not differ else "%d kernels differ" % differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Resource and code-size table of agg_update.hip's kernels, keyed by what a kernel is instead of
by its mangled name, so that two versions of the file can be compared kernel by kernel:

    python tools/agg_dispatch_table.py table [csrc/kernels/agg_update.hip] > a.tsv
    python tools/agg_dispatch_table.py compare parent.tsv result.tsv

A key is (form, row type, NP, elements per lane, OPT, single | multi); NP is 0 for the weighted
combine. The resources are the compiler's kernel-resource-usage remarks (as
tools/kernel_resources.py prints them), the code size is the kernel's symbol size in the gfx950
code object. `compare` exits 1 unless both tables hold the same keys with identical VGPRs, AGPRs,
spill, scratch, occupancy and LDS; differences in SGPRs and code size are listed, not judged.
"""
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/llvm/bin"
COLS = ("form", "rows", "NP", "VEC", "OPT", "launch", "vgpr", "agpr", "spill", "scratch", "occ",
        "lds", "sgpr", "bytes")
STRICT = ("vgpr", "agpr", "spill", "scratch", "occ", "lds")
REMARK = {"VGPRs": "vgpr", "AGPRs": "agpr", "VGPRs Spill": "spill",
          "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ",
          "LDS Size [bytes/block]": "lds", "TotalSGPRs": "sgpr"}
ROWS = {"f": "f32", "14__hip_bfloat16": "bf16"}
# the kernels' names up to the fold into agg_kernel / agg_multi (template arguments: T, NP, VEC,
# OPT; agg_sorted_bf16_* without T, agg_weighted_* without NP)
OLD = re.compile(r"_ZN3cml\d+agg_(sorted_bf16|sorted|weighted|near_mixed|near|mixed)_(kernel|multi)I"
                 r"(f|14__hip_bfloat16)?((?:Li\d+E)+)E")
NEW = re.compile(r"_ZN3cml\d+agg_(kernel|multi)INS_4FormI(f|14__hip_bfloat16)Lb([01])ELb([01])E"
                 r"Lb([01])EEE((?:Li\d+E)+)")


def key_of(mangled):
    """(form, rows, NP, VEC, OPT, launch) of a kernel symbol, or None for any other symbol."""
    m = NEW.match(mangled)
    if m:
        launch, rows, near, mix, weighted, ints = m.groups()
        form = "weighted" if weighted == "1" else \
            {"00": "sorted", "10": "near", "01": "mixed", "11": "near_mixed"}[near + mix]
        np_, vec, opt = (int(x) for x in re.findall(r"Li(\d+)E", ints))
        return form, ROWS[rows], np_, vec, opt, "single" if launch == "kernel" else "multi"
    m = OLD.match(mangled)
    if not m:
        return None
    form, launch, rows, ints = m.groups()
    ints = [int(x) for x in re.findall(r"Li(\d+)E", ints)]
    if form == "sorted_bf16":
        form, rows = "sorted", "14__hip_bfloat16"
    if form == "weighted":
        ints = [0] + ints
    return (form, ROWS[rows], *ints, "single" if launch == "kernel" else "multi")


def parse(remarks, elf):
    """Rows (dicts over COLS) from the compiler's remark text and the unbundled code object."""
    rows, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        k, _, v = m.group(1).strip().partition(":")
        if k == "Function Name":
            key = key_of(v.strip())
            cur = rows.setdefault(key, dict(zip(COLS, key))) if key else None
        elif cur is not None and k.strip() in REMARK:
            cur[REMARK[k.strip()]] = v.strip()
    syms = subprocess.run([f"{LLVM}/llvm-readelf", "-sW", elf], capture_output=True, text=True,
                          check=True).stdout
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and key_of(f[7]) in rows:
            rows[key_of(f[7])]["bytes"] = f[2]
    return [rows[k] for k in sorted(rows)]


def table(src):
    with tempfile.TemporaryDirectory() as d:
        co, elf = os.path.join(d, "a.co"), os.path.join(d, "a.elf")
        t0 = time.time()
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                            "-I", os.path.join(ROOT, "csrc"), "--cuda-device-only", "-c", src, "-o",
                            co, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
        print(f"compiled {src} in {time.time() - t0:.0f} s", file=sys.stderr)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={co}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"], check=True)
        return parse(r.stderr, elf)


def dump(rows, out=sys.stdout):
    print("\t".join(COLS), file=out)
    for r in rows:
        print("\t".join(str(r.get(c, "?")) for c in COLS), file=out)


def load(path):
    with open(path) as fh:
        head = fh.readline().split()
        return {tuple(f[:6]): dict(zip(head, f)) for f in (ln.split() for ln in fh) if f}


def compare(a, b):
    A, B = load(a), load(b)
    print(f"{len(A)} kernels in {a}, {len(B)} in {b}")
    only = sorted(set(A) ^ set(B))
    for k in only:
        print("only in", a if k in A else b, ":", " ".join(k))
    both = sorted(set(A) & set(B))
    bad = [k for k in both if any(A[k][c] != B[k][c] for c in STRICT)]
    for k in bad:
        print("RESOURCES DIFFER", " ".join(k), [(c, A[k][c], B[k][c]) for c in STRICT])
    print(f"{len(both) - len(bad)} of {len(both)} shared keys: identical "
          + ", ".join(STRICT))
    for c in ("sgpr", "bytes"):
        diff = [k for k in both if A[k][c] != B[k][c]]
        print(f"{c}: {len(diff)} kernels differ")
        for k in diff:
            print(f"  {' '.join(k)}: {A[k][c]} -> {B[k][c]}")
    return 1 if only or bad else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["compare"] and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if sys.argv[1:2] == ["table"]:
        dump(table(sys.argv[2] if len(sys.argv) > 2
                   else os.path.join(ROOT, "csrc", "kernels", "agg_update.hip")))
    else:
        sys.exit(__doc__)

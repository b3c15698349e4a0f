#!/usr/bin/env python3
"""Compare two builds of one .hip file kernel by kernel: is the machine code the same?

    hipcc <build.py's HIP_FLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage FILE -o A.s 2> A.remarks
    (the same for the other tree -> B.s, B.remarks)
    python profiles/scripts/compare_isa.py A.s A.remarks B.s B.remarks [--drop-template-arg KERNEL:POSITION ...]

Kernels are matched by demangled name; `--drop-template-arg edge_dots_kernel:1` removes template argument 1 (counted from
0) from the names of build A, for a parameter that build B no longer has.  Per kernel: the instruction stream (labels and
the kernel's own symbol made position-independent, comments and directives dropped), the .amdhsa_* descriptor block, and
VGPRs / SGPRs / LDS / scratch / occupancy from the remarks.  Prints one row per kernel; exit status 1 if any differs."""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt", *names], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    # the name and its template arguments; the parameter list repeats them
    return {m: re.sub(r"^void ", "", d).split(">(")[0] + (">" if ">(" in d else "") for m, d in zip(names, out)}


def kernels_of(asm_path, remarks_path):
    with open(asm_path) as f:
        lines = f.read().splitlines()
    kernels, sym, body = {}, None, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m and sym is None:
            sym, body = m.group(1), []
            kernels[sym] = {"text": body, "desc": []}
            continue
        if sym and re.match(r"^\.Lfunc_end\d+:", l):
            sym = None
            continue
        if sym:
            body.append(l)
    # instruction stream: up to s_endpgm's section; descriptor: .amdhsa_ lines (they sit inside the function's span)
    for s, k in kernels.items():
        text, desc = [], []
        for l in k["text"]:
            c = l.split(";")[0].rstrip()
            if not c.strip():
                continue
            c = c.replace(s, "<kernel>")
            c = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", c)
            t = c.strip()
            if t.startswith(".amdhsa_") and not t.startswith(".amdhsa_kernel"):
                desc.append(t)
            elif t.startswith("."):
                if re.match(r"^\.LBB_\d+:", t):
                    text.append(t)
            else:
                text.append(" ".join(t.split()))
        k["text"], k["desc"] = text, desc
        k["count"] = sum(1 for t in text if not t.endswith(":"))
    with open(remarks_path) as f:
        cur = None
        for l in f:
            m = re.search(r"remark: Function Name: (\S+)", l)
            if m:
                cur = kernels.get(m.group(1))
                continue
            m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", l)
            if m and cur is not None:
                cur.setdefault("res", {})[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def drop_arg(name, kernel, pos):
    m = re.match(rf"^(.*\b{kernel})<(.*)>$", name)
    if not m:
        return name
    args = [a.strip() for a in m.group(2).split(",")]
    del args[pos]
    return f"{m.group(1)}<{', '.join(args)}>"


def main(argv):
    drops = []
    while "--drop-template-arg" in argv:
        i = argv.index("--drop-template-arg")
        k, p = argv[i + 1].split(":")
        drops.append((k, int(p)))
        del argv[i:i + 2]
    a, b = kernels_of(argv[1], argv[2]), kernels_of(argv[3], argv[4])
    da, db = demangle(list(a)), demangle(list(b))
    for k, p in drops:
        da = {m: drop_arg(d, k, p) for m, d in da.items()}
    by_name_a, by_name_b = {d: a[m] for m, d in da.items()}, {d: b[m] for m, d in db.items()}
    bad = 0
    print(f"{'kernel':<78} {'instr A':>8} {'instr B':>8}  {'stream':<7} {'descr':<7} VGPR A/B  SGPR A/B  LDS A/B        scratch A/B  occ A/B")
    for name in sorted(set(by_name_a) | set(by_name_b)):
        ka, kb = by_name_a.get(name), by_name_b.get(name)
        short = name.replace("drtk_amd::(anonymous namespace)::", "")
        if ka is None or kb is None:
            print(f"{short:<78} only in build {'A' if kb is None else 'B'}")
            bad += 1
            continue
        same_text, same_desc = ka["text"] == kb["text"], ka["desc"] == kb["desc"]
        ra, rb = ka.get("res", {}), kb.get("res", {})
        bad += not (same_text and same_desc and ra == rb and ra)
        pair = lambda key: f"{ra.get(key, '?')}/{rb.get(key, '?')}"
        print(f"{short:<78} {ka['count']:>8} {kb['count']:>8}  {'equal' if same_text else 'DIFFERS':<7} {'equal' if same_desc else 'DIFFERS':<7} "
              f"{pair('VGPRs'):<9} {pair('TotalSGPRs'):<9} {pair('LDS Size'):<14} {pair('ScratchSize'):<12} {pair('Occupancy')}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

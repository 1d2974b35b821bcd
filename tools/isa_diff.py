#!/usr/bin/env python3
"""Per-kernel instruction histograms of two builds of the same `.s` (`make asm`), and their kernel resource remarks.

    python tools/isa_diff.py base/sfm_kernels.s csrc/sfm_kernels.s [--resources base/resource_usage.txt csrc/resource_usage.txt]

For every kernel symbol: the mnemonics whose counts differ, split into scalar ones (prefix `s_`) and all others, and the
scalar total of both builds.  A refactor that is meant to leave the code as it was passes when
  * both files hold the same kernel symbols,
  * every kernel has the same multiset of non-scalar mnemonics,
  * no kernel has more scalar instructions than before,
  * (with --resources) VGPRs, AGPRs, scratch, spills, occupancy and LDS size are equal; TotalSGPRs moves are listed.
Exit status 0 if all of that holds, 1 otherwise.  Mnemonics are classified by prefix only.
"""
import argparse
import collections
import re
import sys

KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
END = re.compile(r"^\.Lfunc_end\d+:")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
REMARK = re.compile(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis")
EQUAL_FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
                "LDS Size [bytes/block]")


def histograms(path):
    """{kernel symbol: Counter(mnemonic)} -- the instructions between a kernel's label and its .Lfunc_end"""
    lines = open(path).read().splitlines()
    kernels = {m.group(1) for m in map(KERNEL.match, lines) if m}
    out, cur = {}, None
    for ln in lines:
        m = LABEL.match(ln)
        if m and m.group(1) in kernels:
            cur = out.setdefault(m.group(1), collections.Counter())
        elif END.match(ln):
            cur = None
        elif cur is not None:
            m = INSTR.match(ln.split(";")[0])
            if m:
                cur[m.group(1)] += 1
    return out


def resources(path):
    """{kernel symbol: {field: value}} from the -Rpass-analysis=kernel-resource-usage remarks"""
    out, cur = {}, None
    for ln in open(path):
        m = REMARK.search(ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def is_scalar(mnemonic):
    return mnemonic.startswith("s_")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--resources", nargs=2, metavar=("BASE_TXT", "NEW_TXT"))
    args = ap.parse_args()
    a, b = histograms(args.base), histograms(args.new)
    ok = True
    print(f"kernels: {len(a)} in {args.base}, {len(b)} in {args.new}")
    for name in sorted(set(a) ^ set(b)):
        ok = False
        print(f"  only in {'base' if name in a else 'new'}: {name}")
    same = 0
    for name in sorted(set(a) & set(b)):
        ha, hb = a[name], b[name]
        if ha == hb:
            same += 1
            continue
        sa = sum(n for m, n in ha.items() if is_scalar(m))
        sb = sum(n for m, n in hb.items() if is_scalar(m))
        print(f"{name}\n  scalar total {sa} -> {sb}, other total {sum(ha.values()) - sa} -> {sum(hb.values()) - sb}")
        for title, want in (("scalar", True), ("other", False)):
            for m in sorted(set(ha) | set(hb)):
                if is_scalar(m) == want and ha[m] != hb[m]:
                    print(f"  {title:6s} {m:28s} {ha[m]:5d} -> {hb[m]:5d}")
                    if not want:
                        ok = False
        if sb > sa:
            ok = False
    print(f"identical histograms: {same} of {len(set(a) & set(b))} kernels")
    if args.resources:
        ra, rb = resources(args.resources[0]), resources(args.resources[1])
        if set(ra) != set(rb):
            ok = False
            print("resource remarks: different sets of functions")
        moves = 0
        for name in sorted(set(ra) & set(rb)):
            for f in EQUAL_FIELDS:
                if ra[name].get(f) != rb[name].get(f):
                    ok = False
                    print(f"{name}\n  {f}: {ra[name].get(f)} -> {rb[name].get(f)}   (must be equal)")
            if ra[name].get("TotalSGPRs") != rb[name].get("TotalSGPRs"):
                moves += 1
                print(f"{name}\n  TotalSGPRs: {ra[name].get('TotalSGPRs')} -> {rb[name].get('TotalSGPRs')}")
        print(f"resources: {len(set(ra) & set(rb))} functions compared, {moves} TotalSGPRs moves")
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

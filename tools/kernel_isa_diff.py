#!/usr/bin/env python3
"""Which kernels differ between two builds' device assembly (a refactor's check that the kernels stayed the kernels):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --offload-device-only -S -o a.s orbslamm_amd/csrc/orbslamm_hip.hip
    python tools/kernel_isa_diff.py a.s b.s

Splits both files by kernel symbol (the amdhsa metadata lists them), drops comment and blank lines, compares each
kernel's instruction stream line for line (block labels without the function's ordinal) and its metadata row (registers, LDS, scratch, spills; tools/kernel_resources.py
prints the same figures).  Block labels are compared without the function's ordinal in the file (.LBB68_2 -> .LBB_2): a kernel
added in front of a function renumbers them.  That hides nothing as long as labels are the only place the ordinal appears, which
holds for hipcc's output (symbols, metadata and instructions carry none); branch targets still have to match by their local number.
Prints every kernel that differs with both rows; exit status 1 when any does."""
import re
import sys

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
          "sgpr_spill_count")


def metadata(txt):
    md = txt[txt.index("amdhsa.kernels"):]
    out = {}
    for k in md.split("  - .agpr_count:")[1:]:
        k = "  - .agpr_count:" + k
        name = re.search(r"\.name:\s+(\S+)", k).group(1)
        out[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1)) for f in FIELDS)
    return out


def bodies(txt, names):
    """kernel symbol -> its lines from the label to .Lfunc_end, without comments"""
    lines = txt.split("\n")
    labels = ((l.split(":")[0], i) for i, l in enumerate(lines) if l[:1] not in ("", "\t", " ", ".") and ":" in l)
    start = {s: i for s, i in labels if s in names}
    out = {}
    for name, i in start.items():
        body = []
        for l in lines[i + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].rstrip()
            # block labels carry the function's ordinal in the file (.LBB68_2): a kernel added in front renumbers them
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            if l.strip():
                body.append(l)
        out[name] = body
    return out


def main(a, b):
    ta, tb = open(a).read(), open(b).read()
    ma, mb = metadata(ta), metadata(tb)
    ba, bb = bodies(ta, set(ma)), bodies(tb, set(mb))
    bad = 0
    for name in sorted(set(ma) | set(mb)):
        if name not in ma or name not in mb:
            print("%s: only in %s" % (name, a if name in ma else b))
            bad += 1
            continue
        same_isa, same_md = ba[name] == bb[name], ma[name] == mb[name]
        if same_isa and same_md:
            continue
        bad += 1
        print("%s: %s" % (name, "instructions differ (%d against %d lines)" % (len(ba[name]), len(bb[name])) if not same_isa else "metadata differs"))
        for tag, m in ((a, ma[name]), (b, mb[name])):
            print("    %s: %s" % (tag, " ".join("%s %d" % (f, v) for f, v in zip(FIELDS, m))))
    calls = [t.count("s_swappc") for t in (ta, tb)]
    print("%d kernels in %s, %d in %s, %d differ; s_swappc (calls not inlined): %d, %d" % (len(ma), a, len(mb), b, bad, calls[0], calls[1]))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

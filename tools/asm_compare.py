#!/usr/bin/env python3
"""Compare the device code of two builds of one HIP source, kernel by kernel.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \\
        SRC -o A.s 2> A.remarks          (once per commit)
  tools/asm_compare.py A.s A.remarks B.s B.remarks [--filter bpe_lane_kernel]

For every kernel of both builds: whether the instruction streams are identical (labels, comments and directives
dropped), and VGPRs, SGPRs, SGPR spills, VGPR spills, scratch and LDS from the resource remarks of each.
No GPU is needed.
"""
import argparse
import re
import subprocess


def functions(path):
    """name -> list of instructions (labels renumbered in order of appearance)"""
    out, cur, name = {}, None, None
    for line in open(path, errors="replace"):
        s = line.split(";")[0].rstrip()
        m = re.match(r"^(\w+):", s)
        if m and not m.group(1).startswith(".L"):
            name, cur = m.group(1), []
            out[name] = cur
            continue
        if cur is None or not s.strip():
            continue
        t = s.strip()
        if t.startswith(".") and not t.startswith(".L"):
            if t.startswith(".end_amdhsa_kernel") or t.startswith(".section"):
                cur = None
            continue
        cur.append(t)
    for name, body in out.items():
        labels = {}
        for t in body:
            m = re.match(r"^(\.L\w+):", t)
            if m:
                labels.setdefault(m.group(1), "L%d" % len(labels))
        out[name] = [re.sub(r"\.L\w+", lambda m: labels.get(m.group(0), m.group(0)), t) for t in body]
    return out


FIELDS = [("VGPRs", r"VGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("SGPRs", r"TotalSGPRs: (\d+)"), ("SGPRspill", r"SGPRs Spill: (\d+)"),
          ("VGPRspill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("LDS", r"LDS Size \[bytes/block\]: (\d+)")]


def remarks(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        if name:
            for key, pat in FIELDS:
                m = re.search(pat, line)
                if m:
                    out[name].setdefault(key, int(m.group(1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a_s"), ap.add_argument("a_remarks"), ap.add_argument("b_s"), ap.add_argument("b_remarks")
    ap.add_argument("--filter", default="")
    a = ap.parse_args()
    fa, fb, ra, rb = functions(a.a_s), functions(a.b_s), remarks(a.a_remarks), remarks(a.b_remarks)
    names = sorted(n for n in set(ra) | set(rb) if a.filter in n)
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n") if names else []
    rose = 0
    for n, d in zip(names, demangled):
        d = re.sub(r"\(.*", "", d).replace("void swt::", "")
        if n not in ra or n not in rb:
            print("%-70s only in %s" % (d, "A" if n in ra else "B"))
            continue
        if not fa.get(n) or not fb.get(n):
            raise SystemExit("no instructions parsed for %s in %s" % (d, a.a_s if not fa.get(n) else a.b_s))
        same = fa[n] == fb[n]
        up = [k for k, _ in FIELDS if rb[n].get(k, 0) > ra[n].get(k, 0)]
        rose += bool(up)
        print("%-70s %-9s %5d instr | A %s | B %s%s" % (d, "identical" if same else "DIFFERENT", len(fb.get(n, [])),
              " ".join("%s=%d" % (k, ra[n].get(k, 0)) for k, _ in FIELDS), " ".join("%s=%d" % (k, rb[n].get(k, 0)) for k, _ in FIELDS),
              "  ROSE: " + ",".join(up) if up else ""))
    print("%d kernels, %d with a figure that rose" % (len(names), rose))


if __name__ == "__main__":
    main()

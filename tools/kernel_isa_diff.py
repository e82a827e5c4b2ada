#!/usr/bin/env python3
"""Compare the kernels of two AMDGPU assembly files (hipcc -save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s).

    python tools/kernel_isa_diff.py BEFORE.s AFTER.s [--rename REGEX REPL]

Per kernel symbol: the instruction lines with labels normalised, and the four resource figures of its kernel
descriptor (.amdhsa_next_free_vgpr / _sgpr, .amdhsa_private_segment_fixed_size = scratch bytes,
.amdhsa_group_segment_fixed_size = LDS bytes).  One SAME / DIFF line per kernel, `before -> after` where a figure
changed; exit status 1 when a kernel differs or exists on one side only and is not matched by --allow REGEX.
--rename REGEX REPL (repeatable): a kernel of AFTER whose demangled name, with REGEX replaced by REPL, is a kernel of
BEFORE that AFTER no longer has is compared with that one -- for a change that adds template arguments, e.g.
--rename ', false>$' '>' pairs k<3, true, false> with the earlier k<3, true>.
Reads text only: nothing is compiled or run.
"""
import argparse
import re
import subprocess
import sys

FIELDS = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
          ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size"))
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)*")


def parse(path):
    """-> {kernel symbol: (normalised instruction lines, {field: value})}"""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        body = m.group(2)
        res[m.group(1)] = {k: int(re.search(r"^\s*%s\s+(\d+)" % re.escape(d), body, re.M).group(1)) for k, d in FIELDS}
    kernels = {}
    for name, fields in res.items():
        m = re.search(r"^%s:.*?\n(.*?)^\s*\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M)
        if m is None:
            raise SystemExit(f"{path}: no code for kernel {name}")
        lines, labels = [], {}
        for raw in m.group(1).split("\n"):
            line = raw.split(";")[0].strip()  # comments carry compiler statistics and source positions
            if not line or line.startswith(".") and not line.endswith(":"):
                continue  # directives (.p2align, .loc, ...)
            lines.append(line)
        for line in lines:  # labels are numbered per file: renumber them in order of appearance inside the kernel
            for lab in LABEL.findall(line):
                labels.setdefault(lab, ".L%d" % len(labels))
        kernels[name] = ([LABEL.sub(lambda x: labels[x.group(0)], line) for line in lines], fields)
    return kernels


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        short = [re.sub(r"\(anonymous namespace\)::", "", d).split("(")[0].replace("void ", "") for d in out.split("\n")]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--allow", default=None, help="regex on the demangled name: these kernels may differ (exit status)")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"),
                    help="pair a kernel of AFTER with the kernel of BEFORE that its demangled name becomes under re.sub")
    a = ap.parse_args()
    old, new = parse(a.before), parse(a.after)
    if a.rename:
        pretty = demangle(sorted(set(old) | set(new)))
        by_name = {pretty[n]: n for n in old if n not in new}
        for n in [n for n in new if n not in old]:
            was = pretty[n]
            for rx, repl in a.rename:
                was = re.sub(rx, repl, was)
            if was != pretty[n] and was in by_name:
                new[by_name.pop(was)] = new.pop(n)  # (listed under BEFORE's name)
    names = sorted(set(old) | set(new))
    pretty = demangle(names)
    bad = 0
    for n in sorted(names, key=lambda n: pretty[n]):
        if n not in old or n not in new:
            verdict, f = ("ADDED" if n in new else "REMOVED"), (new.get(n) or old.get(n))[1]
            figures = "  ".join(f"{k} {f[k]}" for k, _ in FIELDS)
            ninstr = ""
        else:
            (li, fi), (lj, fj) = old[n], new[n]
            verdict = "SAME" if li == lj and fi == fj else "DIFF"
            figures = "  ".join(f"{k} {fi[k]}" if fi[k] == fj[k] else f"{k} {fi[k]} -> {fj[k]}" for k, _ in FIELDS)
            ninstr = f"  lines {len(li)}" if len(li) == len(lj) else f"  lines {len(li)} -> {len(lj)}"
        if verdict != "SAME" and not (a.allow and re.search(a.allow, pretty[n])):
            bad += 1
        print(f"{verdict:7s} {pretty[n]}  {figures}{ninstr}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Developer check: are the kernels of two device assembly listings (hipcc --cuda-device-only -S) the same instruction for
instruction?  Per kernel: "identical", or for each of the three segments -- before the first MFMA, first to last MFMA, after
the last MFMA -- whether it is identical, and both lengths.  usage: isa_diff.py <before.s> <after.s> [kernel-substring]"""
import re
import sys


def kernels(path):
    """kernel name -> its instructions (comments, labels and directives dropped)"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        ins = line.split(";")[0].strip()
        if ins and not ins.startswith(".") and not ins.endswith(":"):
            cur.append(" ".join(ins.split()))
    return out


def segments(ins):
    mf = [i for i, s in enumerate(ins) if s.startswith("v_mfma")]
    if not mf:
        return [ins, [], []]
    return [ins[:mf[0]], ins[mf[0]:mf[-1] + 1], ins[mf[-1] + 1:]]


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    want = sys.argv[3] if len(sys.argv) > 3 else ""
    differ = 0
    for name in sorted(set(a) | set(b)):
        if want not in name:
            continue
        if name not in a or name not in b:
            differ += 1
            print(f"{name}: only in {sys.argv[1] if name in a else sys.argv[2]}")
        elif a[name] == b[name]:
            print(f"{name}: identical ({len(a[name])} instructions)")
        else:
            differ += 1
            parts = [f"{label} {'identical' if x == y else 'DIFFERS'} ({len(x)} / {len(y)})"
                     for label, x, y in zip(("before the first MFMA", "first to last MFMA", "after the last MFMA"),
                                            segments(a[name]), segments(b[name]))]
            print(f"{name}: DIFFERS: " + ", ".join(parts))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

"""Developer tool: compare the instruction streams of the kernels in two ISA listings (`hipcc -S --cuda-device-only`), kernel by
kernel, comments, directives and block-label numbers aside — settles without a clock whether a change touched a kernel.
    python tools/isa_compare.py old.s new.s"""
import re, sys


def funcs(path):
    out, cur, name = {}, None, None
    for l in open(path):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name, cur = m.group(1), []
            continue
        if l.startswith(".Lfunc_end") and name:
            out[name] = cur
            name, cur = None, None
            continue
        if cur is not None:
            t = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*$", "", l)).strip()
            if t and not t.startswith("."):
                cur.append(t)
    return out


a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
for k in a:
    if k in b:
        print(k, "IDENTICAL" if a[k] == b[k] else "DIFFERENT", len(a[k]), len(b[k]))
    else:
        print(k, "only in old")
for k in b:
    if k not in a:
        print(k, "only in new", len(b[k]))

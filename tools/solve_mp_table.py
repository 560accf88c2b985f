"""Folds the lines tests/solve_mp_common.py::check_impl prints into profiles/solve_mp/e_ref.txt: per case and quantity the worst
trajectory (by share of its bar) of the emulated wide build and of the wide and dense kernels.

    python -m pytest tests/test_solve_mp.py -s > cpu.log            (CPU tier)
    python -m pytest tests/test_gpu_solve_mp.py -s > gpu.log        (on an MI355X)
    python tools/solve_mp_table.py cpu.log gpu.log > profiles/solve_mp/e_ref.txt
"""
import collections
import re
import sys

PAT = re.compile(r"\.*solve_mp (\S+)\[(\d+)\] (\S+)\s*: E_ref (\S+) / (\S+) floor (\S+) \| (.+?) (\S+) bar (\S+) \((\S+) of it\)")
COLUMNS = {"emu": "emu", "kernel variant 1": "wide", "kernel variant 2": "dense"}


def fold(paths):
    rows, packed = collections.OrderedDict(), {}
    for path in paths:
        for line in open(path):
            m = PAT.match(line)
            if not m:
                continue
            name, t, q, e1, e2, fl, who, e, bar, part = m.groups()
            if who.startswith("kernel variant") and who not in COLUMNS:
                packed.setdefault((name, t, q), set()).add(e)
            if who == "kernel variant 1":
                packed.setdefault((name, t, q), set()).add(e)
            if who not in COLUMNS:
                continue
            r = rows.setdefault((name, q), dict(e1=0.0, e2=0.0, fl=0.0, bar=0.0))
            d = r.setdefault(COLUMNS[who], [0.0, -1.0])
            if float(part) > d[1]:
                d[0], d[1] = float(e), float(part)
                if COLUMNS[who] == "emu" or "emu" not in r:
                    r.update(e1=float(e1), e2=float(e2), fl=float(fl), bar=float(bar))
    return rows, packed


if __name__ == "__main__":
    rows, packed = fold(sys.argv[1:])
    worst = lambda cols: max((r[c][1] for r in rows.values() for c in cols if c in r), default=0.0)
    same = all(len(v) == 1 for v in packed.values())
    print(f"""Errors against the 50-digit results of tests/golden/solve_mp.npz, per case and quantity (the worst trajectory of the
case by share of its bar), folded by tools/solve_mp_table.py from the lines the tests print (tests/solve_mp_common.py::check_impl;
python -m pytest tests/test_solve_mp.py tests/test_gpu_solve_mp.py -s gives every trajectory). E_ref = the worst absolute error of the two
oracle builds (shipped / -ffp-contract=off), floor = 8 ulp of the quantity's largest magnitude on the trajectory per knot travelled per sweep
(inner_iters + 1; 1 in group A), bar = 4 max(E_ref, floor) in every group: no group needed a raised factor. emu = the emulated wide build
(cases of at most 65 steps), wide / dense = tsat_batch_* with set_kernel_variant(1 / 2), set_endgame(0) on an MI355X; behind each error the
share of the bar used. The packed builds (variants 3 ... 7, ragged batch and 17-step cases) printed {'the errors of the wide build, digit for digit' if same else 'errors that DIFFER from the wide build'}.
Largest share of a bar: emulator {worst(['emu']):.2f}, kernel {worst(['wide', 'dense']):.2f}.
""")
    print(f"{'case':22s} {'quantity':8s} {'E_ref':>9s} {'(nofma)':>9s} {'floor':>9s} {'bar':>9s} | {'emu':>9s} {'':>6s} | {'wide':>9s} {'':>6s} | {'dense':>9s}")
    for (name, q), r in rows.items():
        f = lambda k: f"{r[k][0]:9.2e} ({r[k][1]:.2f})" if k in r else f"{'-':>9s}       "
        print(f"{name:22s} {q:8s} {r['e1']:9.2e} {r['e2']:9.2e} {r['fl']:9.2e} {r['bar']:9.2e} | {f('emu')} | {f('wide')} | {f('dense')}")

#!/usr/bin/env python
"""True error of the field-table and horizon stages at the edge cases of tests/stage_edges_common.py: the float64
transcription (E_ref), the oracle, the emulated kernel and (--gpu) the GPU kernel against the 80-digit transcription
tests/refmath_mp.py; and the as-written IGRF algorithm next to the poles. Writes profiles/stages/edge_accuracy.txt (--out).

    python tools/edge_accuracy.py [--gpu] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tsat_loader import load_package
    pkg = load_package()
    import conftest
    import oracle_lib as ol
    import refmath_igrf as ri
    import refmath_mp as rmp
    import stage_edges_common as sc
    from mpmath import mpf

    ol.build(); ol.load()
    emu = conftest.Emu(pkg._abi)
    solver = pkg.trajopt.AugmentedLagrangianSolver(None, None) if args.gpu else None
    L = []
    say = lambda s="": (L.append(s), print(s, flush=True))
    say("# tools/edge_accuracy.py" + (" --gpu" if args.gpu else "") + f": errors against tests/refmath_mp.py ({rmp.DPS} digits)")
    say("#\n# Field tables: worst error over the asserted rows; B relative to max|B| of the 80-digit table, pos in km.")
    say("# E_ref = the float64 transcription tests/refmath_igrf.py; the tests hold emulator and GPU to 4 E_ref.")
    cols = ["E_ref", "oracle", "emulator"] + (["GPU"] if args.gpu else [])
    say(f"# {'case':<10}{'rows':>6} | " + " ".join(f"{'B ' + c:>12}" for c in cols) + " | " + " ".join(f"{'pos ' + c:>12}" for c in cols))
    for name, (kep, t0, tf, N) in sc.field_calls().items():
        ref = sc.field_ref(name)
        tabs = [ol.btable_batch(kep, t0, tf, N), emu.btable(kep, t0, tf, N)]
        if args.gpu:
            tabs.append(pkg.magnetic.magnetic_simulation(solver, kep, t0, tf, N))
        for t in range(ref.T):
            eB = [ref.E_B[t]] + [ref.err_B(t, B[t]) for B, _ in tabs]
            eP = [ref.E_pos[t]] + [ref.err_pos(t, p[t]) for _, p in tabs]
            say(f"  {name + '[' + str(t) + ']':<10}{len(ref.rows[t]):>6} | " + " ".join(f"{e:12.3e}" for e in eB) + " | " + " ".join(f"{e:12.3e}" for e in eP))
    say("#\n# Horizon: tf_index equals the 80-digit index in every call; worst relative error of cond_at (cutoffs <= 1e3).")
    say(f"# {'call':<14}{'80-digit index':<44} " + " ".join(f"{c:>12}" for c in cols[1:]))
    calls = sc.horizon_calls(pkg)
    for name in sc.HORIZON_CALL_NAMES:
        c = calls[name]
        res = [ol.horizon_batch(c.B, c.dt, c.cut), emu.horizon(c.B, c.dt, c.cut)]
        if args.gpu:
            res.append(pkg.horizon.condition_based_time(solver, c.B, c.dt, c.cut))
        errs = []
        for idx, cond in res:
            assert np.array_equal(idx, c.idx), (name, idx, c.idx)
            errs.append(max([abs(cond[j] / c.cond[j] - 1) for j in range(len(c.idx)) if c.check_cond[j]], default=0.0))
        say(f"  {name:<14}{str(c.idx.tolist()):<44} " + " ".join(f"{e:12.3e}" for e in errs))
    say("#\n# The as-written igrf12 next to the poles (CPU, r = 6771 km, date 2019): |B - B_80| in ECEF, nT, worst of four")
    say("# longitudes (0.3, 2.0, -1.1, -2.9 rad); lat = +-(pi/2 - d) in float64. Field magnitude there: 4.8e4 nT.")
    say(f"# {'d (rad)':<12}{'north: transcription':>22}{'oracle':>12}{'south: transcription':>24}{'oracle':>12}")
    ned_to_enu = np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1.0]])

    def ecef(b, lat, lon):
        R = np.array([[-np.sin(lon), -np.sin(lat) * np.cos(lon), np.cos(lat) * np.cos(lon)],
                      [np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat) * np.sin(lon)],
                      [0, np.cos(lat), np.sin(lat)]])
        return R @ ned_to_enu @ b

    for d in (1e-2, 1e-3, 1e-4, 1e-6, 1e-8, 0.0):
        row = []
        for sign in (1, -1):
            worst = [0.0, 0.0]
            for lon in (0.3, 2.0, -1.1, -2.9):
                lat = sign * (np.pi / 2 - d)
                want = [x * 1e9 for x in rmp.field_ecef(2019, 6771e3, mpf(lat), mpf(lon))]
                for k, f in enumerate((ri.igrf12, ol.igrf12)):
                    with np.errstate(all="ignore"):
                        got = ecef(np.asarray(f(2019, 6771e3, lat, lon), dtype=np.float64), lat, lon)
                    e = max(float(abs(mpf(float(g)) - w)) for g, w in zip(got, want)) if np.all(np.isfinite(got)) else np.inf
                    worst[k] = max(worst[k], e)
            row += worst
        say(f"  {d:<12.0e}{row[0]:>22.3e}{row[1]:>12.3e}{row[2]:>24.3e}{row[3]:>12.3e}")
    if solver is not None:
        solver.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()

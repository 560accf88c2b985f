"""Developer tool: the CARE bar of the asymptotic periodic LQR, case by case -> profiles/aplqr/care_e_ref.txt.

For every case of tests/test_aplqr.py — the care6 cases (four weight / inertia sets, the reference's own A, twenty random triples) and
the six slews of the synthesis — the normalised elementwise error against the 50-digit P, max_ij |dP_ij| / sqrt(P_ii P_jj), of
scipy.linalg.solve_continuous_are and of the numpy-double restatement of the kernel's iteration (E_ref is the larger, the bar
4 E_ref), the relative residual the restatement leaves, and the error of the kernel source under the lane emulator; with a log of
`pytest tests/test_gpu_aplqr.py -s` as argument, the errors of the slews on an MI355X beside them. The last line is the figure behind
tracking.APLQR_RES_TOL: 100 x the largest residual of the restatement.

    python tools/aplqr_e_ref.py [gpu.log] > profiles/aplqr/care_e_ref.txt"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
from tsat_loader import load_package

pkg = load_package()
import aplqr_common as ac
import oracle_lib as ol

ol.build()
emu = ac.Emu(pkg._abi)
gpu = {}
if len(sys.argv) > 1:
    for m in re.finditer(r"GPU slew (\d+): normalised error (\S+),", open(sys.argv[1]).read()):
        gpu[int(m.group(1))] = float(m.group(2))

print("The CARE bar of tsat_aplqr_gains (tools/aplqr_e_ref.py): errors against the 50-digit P of the same sign iteration (mpmath, step below")
print("1e-45, residual below 1e-40), max_ij |dP_ij| / sqrt(P_ii P_jj). E_ref = the larger of scipy.linalg.solve_continuous_are and the")
print("numpy-double restatement of the kernel's iteration; bar = 4 E_ref. emu = tsat_aplqr.hpp under the lane emulator, MI355X = the")
print("library (the slews only), each with its share of the bar. residual = what the restatement leaves,")
print("|A'P + P A - P G P + Q|_F / (2 |A|_F |P|_F + |G|_F |P|_F^2 + |Q|_F).")
print()
print(f"{'case':36s} {'scipy':>9s} {'numpy':>9s} {'bar':>9s} {'residual':>9s} | {'emu':>9s} {'':6s} | {'MI355X':>9s}")
worst, share = 0.0, 0.0


def row(name, A, G, Q, P_emu, t=None):
    global worst, share
    Pref, e_ref, res, (e_sc, e_np) = ac.care_bar(A, G, Q)
    e = ac.nerr(P_emu, Pref)
    worst, share = max(worst, res), max(share, e / (4 * e_ref), gpu.get(t, 0.0) / (4 * e_ref))
    g = f"{gpu[t]:9.2e} ({gpu[t] / (4 * e_ref):.2f})" if t in gpu else ""
    print(f"{name:36s} {e_sc:9.2e} {e_np:9.2e} {4 * e_ref:9.2e} {res:9.2e} | {e:9.2e} ({e / (4 * e_ref):.2f}) | {g}")


for name, A, G, Q in ac.named_cases() + ac.random_cases():
    P, info = emu.care6(A, G, Q)
    assert info["status"] == 0, name
    row(name, A, G, Q, P)
c = ac.gains_case(pkg)
Kg, info = emu.gains(ac.GainsCall(pkg._abi, c))
ol.load()
for t in range(len(c["lo"])):
    J = c["Jmat"][t].reshape(3, 3).T
    Gm = ac.gamma_numpy(ol, c["xf"][t], c["Btab"][c["bidx"][t], c["lo"][t]:c["hi"][t]], J, c["rd"][t])
    row(f"slew {t}, rows [{c['lo'][t]}, {c['hi'][t]})", ac.double_integrator(), ac.block_g(Gm), np.diag(c["qd"][t]), info["P"][t], t)
print()
print(f"largest share of a bar: {share:.2f}")
print(f"largest residual of the restatement: {worst:.2e}; 100 x that: {100 * worst:.2e}; tracking.APLQR_RES_TOL = {pkg.tracking.APLQR_RES_TOL:.1e}")

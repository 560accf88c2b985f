#!/usr/bin/env python3
"""Generates tortoisesat.jl_amd/csrc/tsat_riccati_dpp.inc: the four inline-asm blocks of one knot of the row-oriented Riccati
recursion (riccati_row_step, tsat_device.hpp) for NH = 6 (error coordinates) and NH = 7 (full state), and the feedback block of
one knot of the closed-loop forward sweep (forward_sweep) for the same two.

A block is a run of v_fmac_f64_dpp / v_mov_b64_dpp with `row_newbcast:n` — src0 is lane n of the reader's 16-lane row, for free
in the FMA itself (profiles/r04/valu_f64_ubench.txt) — written out by hand because (a) hipcc does not fold a 64-bit
update_dpp into the FMA (it keeps a v_mov_b64_dpp per term: twice the instructions) and (b) the order inside a block is chosen so
that an accumulator is touched again only NH + 1 / NC instructions later (a VALU instruction that reads a register written by one
of the previous four issues in 5 cycles instead of 4). The compiler's hazard recogniser does not look inside inline asm: every
block starts with the wait states a DPP read of a just-written VGPR needs (2; the knot's first block 5: a VALU write of EXEC).

    python tools/gen_riccati_dpp.py > tortoisesat.jl_amd/csrc/tsat_riccati_dpp.inc
"""
DPP = " row_newbcast:%d row_mask:0xf bank_mask:0xf"


def block(name, nh, lines, outs, inouts, ins, prefix="TSAT_RB"):
    """one macro: <prefix><name>_<nh>() -> asm volatile(...)"""
    ops = [o for o, _ in outs] + [o for o, _ in inouts] + [o for o, _ in ins]
    txt = "".join('    "%s\\n"\\\n' % l for l in lines)
    cons = []
    cons.append(", ".join('[%s] "=&v"(%s)' % (o, e) for o, e in outs) if outs else "")
    io = ", ".join('[%s] "+v"(%s)' % (o, e) for o, e in inouts)
    out_s = ", ".join(s for s in (cons[0], io) if s)
    in_s = ", ".join('[%s] "v"(%s)' % (o, e) for o, e in ins)
    return "#define %s%s_%d() asm volatile(\\\n%s    : %s\\\n    : %s)\n" % (prefix, name, nh, txt, out_s, in_s)


def gen(nh):
    nc = nh + 3
    out = []
    # ---- block 1: W[r] = sum_m S~[r][m] F[m][j]  (row nh: l_j + s'F); S read through its upper triangle ----------------
    L = ["s_nop 4"]
    for r in range(nh):
        L.append("v_mov_b64 %%[w%d], 0" % r)
    for m in range(nh):
        for r in range(nh + 1):
            # S~[r][m]: row r of lane m's column — for r > m (r a state row) its mirror image, row m of lane r's column, so that
            # only the upper triangle of S is ever read: the cost-to-go the recursion works with is symmetric to the last bit
            if r < nh and r > m:
                L.append(("v_fmac_f64_dpp %%[w%d], %%[s%d], %%[f%d]" % (r, m, m)) + DPP % r)
            else:
                L.append(("v_fmac_f64_dpp %%[w%d], %%[s%d], %%[f%d]" % (r, r, m)) + DPP % m)
    out.append(block("1", nh, L, [("w%d" % r, "W[%d]" % r) for r in range(nh)], [("w%d" % nh, "W[%d]" % nh)],
                     [("s%d" % r, "st.Sc[%d]" % r) for r in range(nh + 1)] + [("f%d" % m, "f[%d]" % m) for m in range(nh)]))
    # ---- block 2: Q[i] += sum_m F[m][i] W[m] --------------------------------------------------------------------------
    L = []      # (its DPP sources, the record columns f, are inputs of block 1 as well: written long before)
    for m in range(nh):
        for i in range(nc):
            L.append(("v_fmac_f64_dpp %%[q%d], %%[f%d], %%[w%d]" % (i, m, m)) + DPP % i)
    out.append(block("2", nh, L, [], [("q%d" % i, "Q[%d]" % i) for i in range(nc)],
                     [("f%d" % m, "f[%d]" % m) for m in range(nh)] + [("w%d" % m, "W[%d]" % m) for m in range(nh)]))
    # ---- block 3: Quu (upper triangle) and Qu to every lane of the row ------------------------------------------------
    L = ["s_nop 1"]
    names = []
    for a in range(3):
        for b in range(a, 3):
            L.append(("v_mov_b64_dpp %%[h%d%d], %%[q%d]" % (a, b, a)) + DPP % (nh + b))
            names.append(("h%d%d" % (a, b), "h%d%d" % (a, b)))
    for a in range(3):
        L.append(("v_mov_b64_dpp %%[u%d], %%[wl]" % a) + DPP % (nh + a))
        names.append(("u%d" % a, "qu[%d]" % a))
    out.append(block("3", nh, L, names, [], [("q%d" % a, "Q[%d]" % (nh + a)) for a in range(3)] + [("wl", "W[%d]" % nh)]))
    # ---- block 4: S(i, j) = Qxx(i, j) + sum_c (Qux[c][i] - rho K[c][i]) K[c][j]   (T[c] = Qux[c][.] - rho K[c][.] of the lane's own column)
    L = ["s_nop 1"]
    for c in range(3):
        for i in range(nh):
            L.append(("v_fmac_f64_dpp %%[q%d], %%[t%d], %%[k%d]" % (i, c, c)) + DPP % i)
    out.append(block("4", nh, L, [], [("q%d" % i, "Q[%d]" % i) for i in range(nh)],
                     [("t%d" % c, "Tc[%d]" % c) for c in range(3)] + [("k%d" % c, "Kc[%d]" % c) for c in range(3)]))
    return "".join(out)


def gen_fwd_gain(nh):
    """TSAT_FG_<nh>: the feedback of one knot of the closed-loop forward sweep (forward_sweep, tsat_device.hpp),
    u_c += sum_j K[c][j] dx_j + alpha d_c. The knot's K, d record (24 doubles: K 3 x 7 row-major, then d) sits two doubles a lane in
    the first twelve lanes of every row — value i in lane i / 2, low or high double — and every term names the lane that holds its
    multiplicand. Per accumulator the terms run j ascending, alpha d_c last: the order (and so the bits) of the plain loop. The
    three accumulators take turns, so that one is touched again only three instructions later."""
    kd = lambda i: (("%[kl]" if i % 2 == 0 else "%[kh]"), i // 2)
    L = ["s_nop 1"]
    for j in range(nh):
        for c in range(3):
            reg, lane = kd(c * 7 + j)
            L.append(("v_fmac_f64_dpp %%[u%d], %s, %%[x%d]" % (c, reg, j)) + DPP % lane)
    for c in range(3):
        reg, lane = kd(21 + c)
        L.append(("v_fmac_f64_dpp %%[u%d], %s, %%[al]" % (c, reg)) + DPP % lane)
    return block("", nh, L, [], [("u%d" % c, "u[%d]" % c) for c in range(3)],
                 [("kl", "kin.kd[0]"), ("kh", "kin.kd[1]")] + [("x%d" % j, "dx[%d]" % j) for j in range(nh)] + [("al", "alpha")], prefix="TSAT_FG")


if __name__ == "__main__":
    print("// GENERATED by tools/gen_riccati_dpp.py — do not edit. Inline-asm blocks of riccati_row_step (tsat_device.hpp).")
    print("// Operands are the local names of that function: st.Sc, f, W, Q, h00..h22, qu, Kc, Tc.")
    for nh in (6, 7):
        print(gen(nh))
    print("// Feedback of one knot of the closed-loop forward sweep. Operands are the local names of forward_sweep's knot: u, kin.kd, dx, alpha.")
    for nh in (6, 7):
        print(gen_fwd_gain(nh))

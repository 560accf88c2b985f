"""CPU tier: the two laws of the ensemble roll-outs (ensemble_rollout of tortoisesat.jl_amd/csrc/tsat_ensemble.hpp, pd_rollout of
tsat_pd.hpp) fly the SAME loop around their command lines. With K_lqr = 0 the TVLQR law commands ``U + 0 * dX`` and with
kd = kp = 0 and feed-forward the PD law commands ``U + 0 * sc``: both are exactly U for finite operands and non-zero U, so whatever
differs between the two emulated calls comes from the loop around the law — lane mapping, start states, statistic, field rows,
limits, noise, RK4 stages, records."""
import numpy as np
import pytest

import dispersed_common as dc
import gg_common as gc
import mpc_held_common as hc
import pd_common as pc

M = 64                                   # 65 lanes: the second wavefront holds only the noise-free lane
IDS = np.array([7, 2 ** 33 + 1], dtype=np.int64)


@pytest.fixture(scope="module")
def cs(pkg, ol):
    """slews 0 and 1 of pd_common.case (N = 20, horizons 20 and 13) with their plan from the oracle; computed once, left unchanged"""
    b8, Rtab = pc.case(pkg)
    b = b8.slice(0, 2)
    r = ol.solve_batch(b, hc.solve_options(ol))
    x0s = pkg.tracking.ensemble_initial_states(b.x0, M, np.random.default_rng(5))
    return dict(b=b, Rtab=Rtab, X=r["X"], U=r["U"], x0s=x0s, o=pc.options(ol), plant=dc.all_five_plants(pkg, b, M))


def test_zero_gain_laws_fly_the_same_loop(pkg, cs):
    b, o = cs["b"], cs["o"]
    assert b.T == 2 and b.N == 20 and list(b.n_knots) == [20, 13]
    assert int(o.noise_mode) == 1 and (o.sigma_gyro > 0 or o.sigma_att > 0 or o.field_amp > 0), "plant noise has to be on"
    for t, n in enumerate(b.n_knots):
        assert np.all(cs["U"][t, :n - 1] != 0.0), "U + 0 is exact only for non-zero U"
    ones7, ones3 = np.ones((b.T, 7)), np.ones((b.T, 3))
    K0 = np.zeros((b.T, b.N - 1, 6, 3))
    tv = gc.EmuGg(pkg._abi).ensemble(b, cs["X"], cs["U"], ones7, ones7, ones3, cs["x0s"], K0, o, cs["plant"], cs["Rtab"], gc.GM, sat=hc.SAT,
                                     noise_id0=IDS)
    pd = pc.EmuPd(pkg._abi).run(b, o, cs["x0s"], np.zeros(3), np.zeros(3), X=cs["X"], U=cs["U"], plant=cs["plant"], Rtab=cs["Rtab"],
                                gm=gc.GM, sat=hc.SAT, limit_mode=0, x0_nom=None, noise_id0=IDS)
    assert tv["n_clipped"].max() > 0, "the limits have to act"
    assert np.any(tv["X_sim"][:, :, 1] != tv["X_sim"][:, :1, 1]), "the realisations have to differ"
    for k in ("X_sim", "stats", "nominal", "n_clipped"):
        where = ""
        if k == "X_sim" and tv[k].tobytes() != pd[k].tobytes():
            where = f": first at (t, k) = {np.argwhere(np.any(tv[k] != pd[k], axis=(1, 3)))[0].tolist()}"
        assert tv[k].tobytes() == pd[k].tobytes(), f"{k} differs between the two laws{where}"

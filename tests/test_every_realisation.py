"""CPU tier of tests/every_realisation_common.py: the kernel source of every family of ensemble roll-outs under the lane emulator
against its numpy reference on EVERY realisation of calls of two and three wavefronts (M = 70, M = 128), where the tiers of the
families themselves fly M = 63 and 64 and compare 34 sampled pairs. One call per law a family has: TVLQR at latency 1 under +-25;
PD track_ff, limit_mode 1, at latency 0 under +-0.6. The conditions — every realisation off the thresholds of the statistic, the
second wavefront distinguishable from the first in the start, the plant record, the sensor record and the generator id — are
asserted on references alone and printed with their figures before anything is compared."""
import numpy as np
import pytest

import every_realisation_common as er
import mpc_held_common as hc


@pytest.fixture(scope="module")
def plan(pkg, ol):
    """the 3 slews, their plan and gains from the oracle; computed once and left unchanged"""
    return er.plan_case(pkg, ol, lambda b: ol.solve_batch(b, hc.solve_options(ol)))


@pytest.fixture(scope="module")
def cases(pkg, plan):
    return {M: er.at(pkg, plan, M) for M in er.MS}


@pytest.fixture(scope="module")
def emus(pkg):
    """the emulator bindings, made (and built) once per family"""
    made = {}

    def of(name):
        if name not in made:
            made[name] = er.row(name).emu(pkg._abi)
        return made[name]
    return of


@pytest.mark.parametrize("M", er.MS)
@pytest.mark.parametrize("family,law", er.PARITY)
def test_emulated_family_matches_reference_on_every_realisation(pkg, ol, emus, cases, family, law, M):
    """M = 70: a second wavefront of 6 realisations, the model slot and 57 duplicates of it; M = 128: two full wavefronts and the
    model slot alone in a third"""
    c, fam = cases[M], er.row(family)
    kw = er.parity_kw(c, fam, law)
    ref, pairs = er.reference_all(pkg, ol, c, fam, law, kw, label=f"{family} {law} M = {M}")
    er.check_all(ref, er.emulated(emus(family), c, law, kw), pairs)


@pytest.mark.parametrize("family", er.NAMES)
def test_emulated_prefix_is_stable_across_wavefront_counts(pkg, emus, cases, family):
    """with explicit generator ids, realisations 0 .. 69 of the M = 128 call are the M = 70 call and realisations 0 .. 126 the
    M = 127 call (the model slot in lane 63 of the second wavefront, nothing dead), byte for byte in every output; ``nominal`` is
    equal in all three. What the GPU tier asserts of the library, here of the emulated source"""
    fam, c = er.row(family), cases[er.M_MAX]
    keys = ("stats", "X_sim", "n_clipped") + (("X_hat", "filt_final") if fam.levels is not None else ())
    for law in fam.laws:
        run = lambda cM: er.emulated(emus(family), cM, law, er.call_kw(cM, fam, law, "track_ff", 1, latency=1, noise_id0=er.ID0))
        large = run(c)
        for M in (70, 127):
            er.same_prefix(run(er.cut(c, M)), large, M, keys)
        assert np.isfinite(large["X_sim"]).all()

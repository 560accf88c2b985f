"""GPU tier of tests/every_realisation_common.py: the library, through the ``tracking`` wrappers with trajectories and estimates asked
for, on EVERY realisation of calls of two and three wavefronts, for every family of ensemble roll-outs whose own tier flies M = 63
and 64 and compares 34 sampled pairs (gg, pd, sensed, filtered, model_filtered, mag_filtered, mag_bias_filtered,
model_mag_filtered).

  - parity: every (t, m) of M = 70 and M = 128 against the numpy reference by the project's bars (``check_all``), one call per law a
    family has, after the conditions on references alone (every realisation off the thresholds; the second wavefront
    distinguishable from the first in start, plant record, sensor record and generator id);
  - breadth: at M = 70, every combination a family has of law / kind, limit_mode and latency against the emulated kernels of the
    same source, which tests/test_every_realisation.py pins to numpy, on every realisation;
  - prefix stability: with explicit generator ids the M = 128 call holds the M = 70 and the M = 127 call byte for byte.

The case is ``pd_common.case(pkg, T=3)``: N = 20, horizons 20 / 13 / 6. The plan is solved once per module at the 1 x 3 budget; the
gains of the references and of the emulator are the oracle's."""
import numpy as np
import pytest

import ensemble_common as ec
import every_realisation_common as er

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver(pkg):
    to = pkg.trajopt
    s = to.AugmentedLagrangianSolver(None, to.AugmentedLagrangianSolverOptions())
    s.opts.opts_uncon.dJ_counter_limit = 1
    yield s
    s.close()


@pytest.fixture(scope="module")
def plan(pkg, ol, solver):
    """the 3 slews, their plan (solved here, 1 x 3 budget) and the oracle's gains of it; computed once and left unchanged"""
    to = pkg.trajopt

    def solve(b):
        solver.opts.iterations, solver.opts.opts_uncon.iterations = 1, 3
        return to.solve_(to.BatchProblem.from_arrays(b), solver, want_K=False)
    return er.plan_case(pkg, ol, solve)


@pytest.fixture(scope="module")
def cases(pkg, plan):
    return {M: er.at(pkg, plan, M) for M in er.MS}


@pytest.fixture(scope="module")
def emus(pkg):
    made = {}

    def of(name):
        if name not in made:
            made[name] = er.row(name).emu(pkg._abi)
        return made[name]
    return of


@pytest.mark.parametrize("M", er.MS)
@pytest.mark.parametrize("family,law", er.PARITY)
def test_gpu_family_matches_reference_on_every_realisation(pkg, ol, solver, cases, family, law, M):
    """M = 70: a second wavefront of 6 realisations, the model slot and 57 duplicates of it; M = 128: two full wavefronts and the
    model slot alone in a third (Mp = 192)"""
    c, fam = cases[M], er.row(family)
    kw = er.parity_kw(c, fam, law)
    ref, pairs = er.reference_all(pkg, ol, c, fam, law, kw, label=f"{family} {law} M = {M}")
    got = er.library(pkg, solver, c, fam, law, kw)
    er.check_all(ref, got, pairs)
    if law == "tv":
        ec.same_gains(c["K"], got["K"])


@pytest.mark.parametrize("family", er.NAMES)
def test_gpu_family_matches_emulator_in_every_combination(pkg, solver, emus, cases, family):
    """M = 70, every realisation, every combination the family has of {tv, track, track_ff, regulate} x limit_mode {0, 1} x latency
    {0, 1}, under +-0.6: X_sim, X_hat and filt_final to 1e-9 and the statistic, off its thresholds, against the emulated kernels"""
    c, fam = cases[70], er.row(family)
    nk, worst = ec.horizons(c["b"]), 0.0
    for label, law, args in er.combinations(fam):
        kw = er.call_kw(c, fam, law, **args)
        worst = max(worst, er.against_emulator(er.emulated(emus(family), c, law, kw), er.library(pkg, solver, c, fam, law, kw), c["o"],
                                               c["b"].xf, nk, f"{family}: {label}"))
    print(f"library against emulator: {family}: worst of {len(er.combinations(fam))} combinations {worst:.2e}")


@pytest.mark.parametrize("family", er.NAMES)
def test_gpu_prefix_is_stable_across_wavefront_counts(pkg, solver, cases, family):
    """with explicit generator ids, byte for byte in every output of the family: realisations 0 .. 69 of the M = 128 call are the
    M = 70 call, realisations 0 .. 126 are the M = 127 call (the model slot in lane 63 of the second wavefront, nothing dead), and
    ``nominal`` is equal in all three. Both laws, latency 1"""
    fam, c = er.row(family), cases[er.M_MAX]
    keys = ("stats", "X_sim", "n_clipped") + (("X_hat", "filt_final") if fam.levels is not None else ())
    for law in fam.laws:
        run = lambda cM: er.library(pkg, solver, cM, fam, law, er.call_kw(cM, fam, law, "track_ff", 1, latency=1, noise_id0=er.ID0))
        large = run(c)
        assert np.isfinite(large["X_sim"]).all() and large["stats"].shape == (er.T, er.M_MAX)
        for M in (70, 127):
            er.same_prefix(run(er.cut(c, M)), large, M, keys)

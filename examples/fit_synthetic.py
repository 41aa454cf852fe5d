#!/usr/bin/env python3
"""End-to-end fit on synthetic inputs, following the reference's main() (mft6.py:3450-3708) minus plotting:

    text model grid --spec_interpolator--> staged + broadened grid            (mft6.py:3512)
    data spectrum (made like mft6.py:3632-3642) + contrast / photometry inputs
    optimize_fit: nwalk random starts, lock-step chi^2 descent on the GPU       (mft6.py:3657)
    best third of the optimiser results seeds the ensemble                      (mft6.py:3668-3679)
    emcee-protocol sampling, walker state resident on the GPU                   (mft6.py:1490-1529)
    samples.txt

    python examples/fit_synthetic.py --out /tmp/fit --nwalk 48 --nstep 40 --nburn 50 --nsteps 300

With ``--tempered T [--beta-min B]`` the sampler is a ladder of T ensembles (mcmc_spec_amd.tempered):
burn-in, reset, production; the swap fractions and the cold rung's summary are printed.  ``--evidence`` adds the cold
rung's autocorrelation time and ln Z by thermodynamic integration and the stepping stone (section 18), from the rows the
run kept on the GPU with ``--autocorr device``; an evidence run wants a much smaller ``--beta-min`` than the default.
``--adaptive N`` first moves the rungs for N iterations until adjacent pairs swap at equal rates (section 19), prints the
ladder before and after with the swap fractions, freezes it and goes on as above.  ``--modes`` prints the posterior's modes
(mcmc_spec_amd.modes; section 23): per mode its probability and the 16 / 50 / 84 percentiles of every coordinate.
``--reweight`` asks the finished chain a second question without a second run (mcmc_spec_amd.reweight; section 24): the
same data staged under a second parallax prior, the effective sample size of the reweighted chain and both sets of
16 / 50 / 84, and the Pareto shape khat of the weights' tail (mcmc_spec_amd.psis; section 25).  ``--loo`` prints PSIS-LOO and
WAIC of the stored chain over the likelihood's own terms: the totals with their standard errors, how many observations have
khat > 0.7 and the worst pixels.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='fit_synthetic_out')
    ap.add_argument('--nwalk', type=int, default=48, help='optimiser start points (the best third become walkers)')
    ap.add_argument('--nstep', type=int, default=40, help='optimiser steps (param `nstep`)')
    ap.add_argument('--nburn', type=int, default=50)
    ap.add_argument('--nsteps', type=int, default=300)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--autocorr', choices=('host', 'device'), default='host',
                    help="where the protocol's convergence checks compute tau ('device': from the chain kept on the GPU)")
    ap.add_argument('--resident-optimiser', action='store_true',
                    help="the optimiser's chains live on the GPU (optimizer.fit_spec_device): same chains, no host round trip per proposal")
    ap.add_argument('--tempered', type=int, default=0, metavar='T',
                    help='parallel tempering: a ladder of T ensembles, geometric from beta = 1 down to --beta-min (0: off)')
    ap.add_argument('--beta-min', type=float, default=0.02, help='the hottest rung of --tempered')
    ap.add_argument('--adaptive', type=int, default=0, metavar='N',
                    help='with --tempered: N adaptive iterations first (the rungs move towards equal swap rates), then the ladder is frozen')
    ap.add_argument('--predictive', action='store_true',
                    help='after the run: the posterior predictive check of the stored chain (chi^2 terms, worst pixels, largest mean residual)')
    ap.add_argument('--ess', action='store_true',
                    help='rank-normalised R-hat, bulk / tail ESS and the MCSE of the 16 / 50 / 84 percentiles (DESIGN.md section 26)')
    ap.add_argument('--loo', action='store_true',
                    help='after the run: PSIS-LOO and WAIC of the stored chain per pixel and filter (totals, how many khat > 0.7, the worst pixels)')
    ap.add_argument('--modes', action='store_true',
                    help="after the run: the posterior's modes (a two-component mixture over the six coordinates), each mode's "
                         "probability and 16 / 50 / 84, and bic1 - bic2 (positive: two modes)")
    ap.add_argument('--reweight', type=float, default=None, metavar='SIGMAS', nargs='?', const=1.0,
                    help="after the run: the posterior under a second parallax prior whose mean lies SIGMAS (default 1) of its "
                         "width higher, by importance reweighting of the stored chain: the ESS and both sets of 16 / 50 / 84")
    ap.add_argument('--evidence', action='store_true',
                    help="with --tempered: print the cold rung's tau and ln Z +- mc_error (ladder ladder_error)")
    args = ap.parse_args()

    import mcmc_spec_amd.mft6 as gpu
    from mcmc_spec_amd import bands, loader, optimizer, staging, synth
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, run_reference_protocol

    os.makedirs(args.out, exist_ok=True)
    rng = np.random.default_rng(args.seed)
    t0 = time.time()

    # ---- "disk": a small BT-Settl-format text grid, isochrone, filters (all synthetic stand-ins) ----
    grid_dir = synth.write_btsettl_text_grid(os.path.join(args.out, 'BT-Settl_M-0.0a+0.0'),
                                             teffs=tuple(range(3000, 4300, 100)), loggs=(4.5, 5.0, 5.5), lo=5300.0,
                                             hi=9700.0, seed=5)
    matrix = synth.make_isochrone_matrix()
    spmin, spmax, res = 0.56, 0.89, 1700
    specs = loader.spec_interpolator([spmin * 1e4, spmax * 1e4], [3000, 4200], [4, 5.5], [5400, 9600], resolution=res,
                                     grid_dir=grid_dir, cache=os.path.join(args.out, 'grid_cache.npz'))
    print('grid: {} nodes x {} samples staged + broadened in {:.2f} s'.format(len(specs) - 1, len(specs['wl']),
                                                                              time.time() - t0))
    ctm = [[list(np.linspace(6000.0, 9500.0, 60))], [list(0.9 * np.ones(60))], [0], [7750.0]]
    ptm = [[], [], [], []]
    tmi, tma = 6000.0, 9500.0
    gpu.set_band_library(bands.make_bands(synth.synthetic_band_tables(), *synth.synthetic_vega()))
    gpu.set_av_prior(*synth.make_av_table())

    # ---- data: composite at the truth, resampled, 1 % noise (mft6.py:3632-3642), normalised (:3506-3507) ----
    truth = np.array([3850.0, 3325.0, 0.15, 0.52, 0.62, 2.0732e-3])
    wl_um = np.linspace(spmin + 0.002, spmax - 0.002, 2048)
    lg = staging.isochrone_logg(truth[:2], matrix)
    w1, c1, con, _, _ = gpu.make_composite(truth[:2], lg, truth[3:5], truth[5], ['x'], [], [wl_um.min(), wl_um.max()],
                                           specs, ctm, ptm, tmi, tma, None, nspec=2)
    c1 = c1 * 10.0 ** (-0.4 * truth[2] * specs.engine.ctx.ccm89_k(w1, 3.1))
    f = np.interp(wl_um * 1e4, w1, c1)
    d = f + rng.normal(0, 0.01 * f)
    data, err = [wl_um, d / np.median(d)], 0.01 * f / np.median(d)
    fr = [[con[0] + 0.01], [0.05], ['x'], [], [], []]
    plx, plx_err = 2.0732e-3, 0.0277e-3

    # ---- optimiser (mft6.py:3657) ----
    t1 = time.time()
    optimizer.optimize_fit(args.out, data, err, specs, args.nwalk, fr, [plx, plx_err], [0.106, 0.01], res, ctm, ptm, tmi,
                           tma, None, matrix, 288.456, 45.802, nspec=2, nstep=args.nstep, dist_fit=True, rad_prior=False,
                           seed=args.seed, resident=args.resident_optimiser)
    chisqs, pars = np.genfromtxt(os.path.join(args.out, 'optimize_cs.txt')), np.genfromtxt(
        os.path.join(args.out, 'optimize_res.txt'))
    best = np.argsort(chisqs)[: int(len(chisqs) / 3)]  # mft6.py:3670-3674
    p0 = pars[best]
    if len(p0) % 2:
        p0 = p0[:-1]
    print('optimiser: {} starts x {} steps in {:.2f} s; best chi^2 {:.1f} at {}'.format(
        args.nwalk, args.nstep, time.time() - t1, chisqs.min(), np.round(pars[np.argmin(chisqs)], 4)))

    # ---- sampler (mft6.py:1490-1529), walker state on the device ----
    t2 = time.time()
    prior = [*np.zeros(10), plx, plx_err]  # mft6.py:3689
    eng = gpu._staged(specs, fr, 2, data, err, [wl_um.min(), wl_um.max()], ctm, ptm, tmi, tma, matrix, 3000.0, 4200.0, prior,
                      True, True, False, need_prior=True)
    if args.tempered:
        return tempered_run(args, eng, p0, truth, t2)
    sampler = DeviceEnsembleSampler(len(p0), 6, eng, seed=args.seed, chunk=50, autocorr=args.autocorr)
    samples = run_reference_protocol(sampler, p0, args.nburn, args.nsteps, nthin=50, dirname=args.out, fname='synthetic')
    print('sampler: {} walkers, {} + {} iterations in {:.2f} s; acceptance {:.2f}'.format(
        len(p0), args.nburn, sampler.iteration, time.time() - t2, sampler.acceptance_fraction.mean()))
    med = np.median(samples, axis=0)
    print('truth   :', truth)
    print('median  :', np.round(med, 5))
    summ = sampler.get_summary()   # (the stored production chain's, selected on the GPU)
    print('posterior 16 / 50 / 84 ({} samples):'.format(int(summ['count'])))
    for nm, (lo, mid, hi) in zip(['T1', 'T2', 'Av', 'R1', 'R2', 'plx'], summ['quantiles']):
        print('  {:4s} {:.6g} / {:.6g} / {:.6g}'.format(nm, lo, mid, hi))
    # ---- derived posteriors (mft6.py:2486-2593): the Kepler contrast and the planet-radius correction factors ----
    kep_wl = np.linspace(4200.0, 9000.0, 200)   # a stand-in for bps/Kepler_Kepler.K.dat (get_transmission('kepler', res))
    kep_tm = np.exp(-0.5 * ((kep_wl - 6400.0) / 1100.0) ** 2)
    eng.stage_products((kep_wl, kep_tm), matrix=matrix)
    prod = sampler.get_products(['kep_contrast', 'pri_corr', 'sec_corr'])
    for nm, (lo, mid, hi) in zip(['dKep', 'f_pri', 'f_sec'], prod['quantiles']):
        print('  {:5s} {:.6g} / {:.6g} / {:.6g}'.format(nm, lo, mid, hi))
    if args.ess:   # how far can the numbers above be trusted?  (Vehtari et al. 2021: want R-hat < 1.01, bulk and tail ESS > 400)
        rr, mc = sampler.get_rank_rhat()['rhat'], sampler.get_mcse()
        bulk, tail = sampler.get_ess(kind='bulk'), sampler.get_ess(kind='tail')
        print('        R-hat (rank)  ESS bulk  ESS tail   MCSE of 16 / 50 / 84')
        for i, nm in enumerate(['T1', 'T2', 'Av', 'R1', 'R2', 'plx']):
            print('  {:5s} {:12.4f} {:9.1f} {:9.1f}   {:.3g} / {:.3g} / {:.3g}'.format(nm, rr[i], bulk[i], tail[i], *mc['quantiles'][i]))
    if args.modes:   # which mode, with what probability?  (the reference's p_t1 and its siblings, mft6.py:2030-2194, jointly)
        from mcmc_spec_amd import modes
        modes.print_table(sampler.get_modes(), ['T1', 'T2', 'Av', 'R1', 'R2', 'plx'], sampler.get_modes(ncomp=1))
    if args.predictive:   # does the model reproduce the data, and which data carry chi^2?  (mft6.py:2361-2438, on every sample)
        from mcmc_spec_amd import predictive
        predictive.print_report(predictive.check(eng, sampler.get_chain(flat=True)), wl_um)
    if args.loo:   # which data can one sample not stand in for, and a score to compare a second model's chain with on the same data
        from mcmc_spec_amd import psis
        psis.print_report(psis.loo(eng, sampler.get_chain(flat=True), wl=wl_um))
    if args.reweight is not None:   # what would another parallax prior have given?  One chain, two questions: a paired comparison
        from mcmc_spec_amd import summary
        from mcmc_spec_amd.engine import Engine
        eng2 = Engine(0)
        eng2.stage_specs(specs)
        prior2 = [*np.zeros(10), plx + args.reweight * plx_err, plx_err]
        eng2.stage_problem(data, err, fr, [wl_um.min(), wl_um.max()], ctm, ptm, tmi, tma, matrix, nspec=2, bands=gpu._BANDS,
                           av_table=gpu._AV_TABLE, tmin=3000.0, tmax=4200.0, prior=prior2, use_av=True, dist_fit=True, rad_prior=False)
        with sampler.get_reweighted(eng2) as rw_:
            n = int(rw_.stats['count'][0])
            print('reweighted to the parallax prior {:.5g} +- {:.2g} (was {:.5g}): ESS {:.1f} of {} samples, {} bad'.format(
                prior2[-2], plx_err, plx, rw_.stats['ess'][0], n, int(rw_.stats['nbad'][0])))
            with rw_.smooth() as sm:   # can these weights be trusted?  Kish's ESS cannot say; the Pareto shape of their tail can
                print('  Pareto-smoothed: khat {:.3f} ({}) from a tail of {}, ESS {:.1f}'.format(
                    sm.khat[0], 'reliable' if sm.khat[0] <= 0.7 else 'NOT reliable: khat > 0.7', int(sm.ntail[0]), sm.stats['ess'][0]))
            (resampled,) = rw_.resample()
            second = summary.summary_of(resampled, resampled.rows)
            resampled.close()
        print('posterior 16 / 50 / 84 under the first prior | under the second:')
        for nm, a3, b3 in zip(['T1', 'T2', 'Av', 'R1', 'R2', 'plx'], summ['quantiles'], second['quantiles'][0]):
            print('  {:4s} {:.6g} / {:.6g} / {:.6g}  |  {:.6g} / {:.6g} / {:.6g}'.format(nm, *a3, *b3))
    print('wrote', os.path.join(args.out, 'samples.txt'), samples.shape)
    return truth, med, samples


def tempered_run(args, eng, p0, truth, t2):
    """The sampler block with a temperature ladder: every rung starts from the optimiser's walkers; rung 0 is the posterior."""
    from mcmc_spec_amd import summary
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    sampler = DeviceTemperedSampler(len(p0), 6, eng, ntemps=args.tempered, beta_min=args.beta_min, seed=args.seed, chunk=50, rng='device',
                                    autocorr=args.autocorr, cap_hint=max(args.nburn, args.nsteps), adaptive=args.adaptive > 0,
                                    adaptation_lag=max(args.adaptive / 2.0, 1.0), adaptation_time=10.0)
    if args.adaptive > 0:
        print('ladder before        :', np.round(sampler.betas, 4))
        p0 = sampler.run_mcmc(p0, args.adaptive, store=False)
        print('swap fractions while the ladder moved ({} iterations):'.format(args.adaptive), np.round(sampler.swap_fraction, 3))
        print('ladder after, frozen :', np.round(sampler.betas, 4), '({} steps skipped)'.format(sampler.ladder_skipped))
        sampler.reset()
    state = sampler.run_mcmc(p0, args.nburn, adapt=False)
    sampler.reset()
    sampler.run_mcmc(state, args.nsteps, adapt=False)
    print('tempered sampler: {} rungs x {} walkers, betas {}, {} + {} iterations in {:.2f} s'.format(
        sampler.ntemps, len(p0), np.round(sampler.betas, 4), args.nburn, sampler.iteration, time.time() - t2))
    print('acceptance per rung :', np.round(sampler.acceptance_fraction.mean(axis=1), 3))
    print('swap fractions      :', np.round(sampler.swap_fraction, 3))
    cold = np.ascontiguousarray(sampler.get_chain(t=0))
    samples = cold.reshape(-1, 6)
    med = np.median(samples, axis=0)
    print('truth   :', truth)
    print('median  :', np.round(med, 5))
    summ = {k: v[0] for k, v in summary.summarize(cold, eng.ctx, None, (0.16, 0.5, 0.84), None, 0, 1).items()}
    print('posterior 16 / 50 / 84 of the cold rung ({} samples):'.format(int(summ['count'])))
    for nm, (lo, mid, hi) in zip(['T1', 'T2', 'Av', 'R1', 'R2', 'plx'], summ['quantiles']):
        print('  {:4s} {:.6g} / {:.6g} / {:.6g}'.format(nm, lo, mid, hi))
    if args.modes:
        from mcmc_spec_amd import modes
        modes.print_table(sampler.get_modes(t=0), ['T1', 'T2', 'Av', 'R1', 'R2', 'plx'], sampler.get_modes(t=0, ncomp=1))
    if args.evidence:
        print('tau of the cold rung :', np.round(sampler.get_autocorr_time(t=0, quiet=True), 2))
        print('R-hat of the cold rung:', np.round(sampler.get_rhat(t=0), 3), '(split, over the walkers)')
        for method in ('ti', 'ss'):
            ev = sampler.log_evidence(blocks=min(8, sampler.iteration), method=method)
            print('ln Z ({}) = {:.4f} +- {:.4f} (ladder {:.4f})'.format(method, ev.log_z, ev.mc_error, ev.ladder_error))
        print('<ln L> per rung      :', np.round(ev.mean_log_like, 3))
    np.savetxt(os.path.join(args.out, 'samples.txt'), samples)
    print('wrote', os.path.join(args.out, 'samples.txt'), samples.shape)
    return truth, med, samples


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Several synthetic targets fitted together: one staged problem per target (each its own Engine), their walkers
evaluated in ONE launch per half-step (TargetGroup), their ensembles stepped in lock-step (GroupSampler; with --device
the ensembles stay on the GPU, DeviceGroupSampler: no host round trip between half-steps, same chains).

Every target gets its own data spectrum (a binary at its own truth, its own pixel count and noise) on one synthetic grid.
Target k's chain is the chain a separate EnsembleSampler with target k's seed would walk.

    python examples/fit_target_group.py --targets 4 --nwalkers 32 --nsteps 200 [--device [--rng device]] [--moves de]

With --moves de every target's iterations take one of three moves -- the stretch move (weight 0.5), the
differential-evolution move (0.4) and its mode-jumping variant gamma0 = 1 (0.1): emcee's remedy for posteriors with two
peaks, whose relative weight the stretch move alone leaves where the initial ensemble put it (mcmc_spec_amd.moves).

With --protocol DIR the targets are fitted the way the reference's driver fits one (run_group_protocol: burn-in, then
production with every target's own convergence check every --nthin iterations; a converged target stops there) and
each target's dumps and samples.txt go to DIR/target<k>/; with --device the checks run on the GPU (autocorr='device').

With --tempered T every target gets a ladder of T rungs and ALL the ladders share every launch
(tempered.DeviceGroupTemperedSampler with --device -- eight launches per iteration for all targets, the rows kept in one
pair of device series -- or its host definition GroupTemperedSampler): the remedy for a posterior whose two modes (primary and
secondary exchanged) differ in width.  --adaptive N first moves every target's ladder for N iterations until adjacent rungs
swap at equal rates, then freezes it for the production run; --evidence prints each target's ln Z (thermodynamic
integration) with its Monte-Carlo and ladder errors.

    python examples/fit_target_group.py --targets 4 --nwalkers 32 --nsteps 200 --device --rng device --tempered 4 --adaptive 100 --evidence
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def print_summary(summ, targets):
    """The 16 / 50 / 84 percentiles of every target's stored chain (sampler.get_summary: selected on the GPU)."""
    names = ['T1', 'T2', 'Av', 'R1', 'R2', 'plx']
    print('posterior 16 / 50 / 84 per target ({} samples each):'.format(', '.join(str(int(c)) for c in summ['count'])))
    for k in range(targets):
        print('target {}: '.format(k) + '  '.join('{} {:.5g} / {:.5g} / {:.5g}'.format(nm, *summ['quantiles'][k, j])
                                                   for j, nm in enumerate(names)))


def print_products(prod, targets):
    """The Kepler contrast and the planet-radius correction factors of every target (mft6.py:2505, :2544-2545), 16 / 50 / 84:
    sampler.get_products, every stored sample through the products kernel with its own target's tables."""
    for k in range(targets):
        print('target {}: '.format(k) + '  '.join('{} {:.5g} / {:.5g} / {:.5g}'.format(nm, *prod['quantiles'][k, j])
                                                   for j, nm in enumerate(['dKep', 'f_pri', 'f_sec'])))


def run_tempered(args, group, p0s, seeds, moves, truths):
    """Every target's ladder in one run: adapt (if asked), freeze, sample; rung 0 of target k is its posterior."""
    from mcmc_spec_amd.tempered import DeviceGroupTemperedSampler, GroupTemperedSampler
    K, T = args.targets, args.tempered
    kw = dict(ntemps=T, beta_min=args.beta_min, seeds=seeds, moves=moves, adaptive=args.adaptive > 0, adaptation_lag=max(10.0, args.adaptive / 10.0),
              adaptation_time=10.0)
    if args.device:
        sampler = DeviceGroupTemperedSampler(group, [args.nwalkers] * K, 6, rng=args.rng, autocorr='device', **kw)
    else:
        sampler = GroupTemperedSampler([args.nwalkers] * K, 6, group, **kw)
    t0 = time.time()
    state = p0s
    if args.adaptive:
        state = sampler.run_mcmc(state, args.adaptive)
        sampler.reset()
        for k in range(K):
            print('target {}: ladder after {} adaptive iterations: {}'.format(k, args.adaptive, np.array2string(sampler.target(k).betas, precision=4)))
    sampler.run_mcmc(state, args.nsteps, adapt=False)
    dt = time.time() - t0
    n = args.adaptive + args.nsteps
    print('{} targets x {} rungs x {} walkers x {} iterations in {:.2f} s ({:.0f} evaluations/s)'.format(
        K, T, args.nwalkers, n, dt, 2.0 * K * T * args.nwalkers * n / dt))
    for k in range(K):
        v = sampler.target(k)
        flat = v.get_chain(0, discard=args.nsteps // 2, flat=True)
        print('target {}: Teff {:.0f} / {:.0f} (truth {:.0f} / {:.0f}), acceptance per rung {}, swaps per pair {}'.format(
            k, *np.median(flat[:, :2], axis=0), *truths[k][:2], np.array2string(v.acceptance_fraction.mean(axis=1), precision=2),
            np.array2string(v.swap_fraction, precision=2)))
        if args.device:
            q = v.get_summary(0, discard=args.nsteps // 2)['quantiles']
            print('          T1 {:.5g} / {:.5g} / {:.5g}   T2 {:.5g} / {:.5g} / {:.5g}   (16 / 50 / 84, selected on the GPU)'.format(*q[0], *q[1]))
        if args.evidence:
            ev = v.log_evidence(discard=args.nsteps // 2, blocks=min(8, max(1, args.nsteps // 2)))
            print('          ln Z = {:.3f} +- {:.3f} (Monte Carlo) +- {:.3f} (ladder; beta_min = {})'.format(
                ev.log_z, ev.mc_error, ev.ladder_error, args.beta_min))
    return sampler


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--targets', type=int, default=4)
    ap.add_argument('--nwalkers', type=int, default=32)
    ap.add_argument('--nsteps', type=int, default=200)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--device', action='store_true', help='keep the ensembles on the GPU (DeviceGroupSampler)')
    ap.add_argument('--rng', choices=('host', 'device'), default='host',
                    help="with --device: who draws the stretch move's randomness -- the host's generators (default), or the GPU "
                         "itself, one launch per chunk and nothing uploaded (another stream: other chains, same posterior)")
    ap.add_argument('--moves', choices=('stretch', 'de'), default='stretch',
                    help="'de': a mixture of the stretch move with differential-evolution moves (for bimodal posteriors)")
    ap.add_argument('--protocol', default=None, metavar='DIR', help="run the reference's driver per target (run_group_protocol)")
    ap.add_argument('--nburn', type=int, default=100)
    ap.add_argument('--nthin', type=int, default=50)
    ap.add_argument('--tempered', type=int, default=0, metavar='T', help='a ladder of T rungs per target, all ladders in one run')
    ap.add_argument('--beta-min', type=float, default=0.02, help='--tempered: the hottest rung (an evidence run wants it much smaller)')
    ap.add_argument('--adaptive', type=int, default=0, metavar='N', help='--tempered: adapt every ladder for N iterations first, then freeze')
    ap.add_argument('--evidence', action='store_true', help="--tempered: print every target's ln Z")
    ap.add_argument('--predictive', action='store_true',
                    help="after a plain run: every target's posterior predictive check (chi^2 terms, worst pixels, largest mean residual)")
    args = ap.parse_args()
    if (args.adaptive or args.evidence) and not args.tempered:
        ap.error('--adaptive and --evidence need --tempered T')
    if args.tempered and args.protocol:
        ap.error('--tempered runs a fixed number of iterations (no --protocol)')
    if args.rng == 'device' and not args.device:
        ap.error('--rng device needs --device (the device draws for the resident sampler)')

    from scipy.interpolate import interp1d
    from mcmc_spec_amd import bands, synth
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup, run_group_protocol
    from mcmc_spec_amd.moves import DEMove, StretchMove
    from oracle import mft6_oracle as orc

    rng = np.random.default_rng(args.seed)
    teffs, loggs = np.arange(3000, 4300, 100), np.array([4.0, 4.5, 5.0, 5.5])
    wl = np.arange(5000, 24000, 0.2)
    specs = synth.grid_to_specs(teffs, loggs, wl, synth.make_grid(teffs, loggs, wl, nlines=800, seed=5))
    matrix = synth.make_isochrone_matrix()
    ctm, ptm = synth.synthetic_contrast_filters(), synth.synthetic_phot_filters()
    tabs, (vw, vf) = synth.synthetic_band_tables(), synth.synthetic_vega()
    fr = [synth.EXAMPLE_CMAG, synth.EXAMPLE_CERR, ['lp600', 'Kp'], synth.EXAMPLE_PMAG, synth.EXAMPLE_PERR,
          ['sdss,r', 'sdss,i', 'sdss,z', 'j', 'h', 'k']]
    tmi = min(min(w) for w in ctm[0] + ptm[0])
    tma = max(max(w) for w in ctm[0] + ptm[0])
    obl = orc.make_band_library(tabs, vw, vf)
    bl = bands.make_bands(tabs, vw, vf)
    tmin, tmax = 3000.0, 4200.0

    kep_wl = np.linspace(4200.0, 9000.0, 200)   # a stand-in for bps/Kepler_Kepler.K.dat (get_transmission('kepler', res))
    kep_tm = np.exp(-0.5 * ((kep_wl - 6400.0) / 1100.0) ** 2)
    engines, truths = [], []
    wls = []
    for k in range(args.targets):
        truth = synth.TRUTH_THETA.copy()
        truth[:2] = np.clip(truth[:2] + rng.uniform(-150.0, 150.0, size=2), tmin + 50.0, tmax - 50.0)
        wl_um = synth.data_wavelengths_um(int(rng.integers(400, 1200)))
        r = [min(wl_um), max(wl_um)]
        lg = [float(orc.get_logg(t, matrix)) for t in truth[:2]]
        w1, c1, _, _, _, _ = orc.make_composite(truth[:2], lg, truth[3:5], truth[5], fr[2], fr[5], r, specs, ctm, ptm,
                                                tmi, tma, bandlib=obl)
        f = interp1d(w1, orc.extinct(w1, c1, truth[2]))(wl_um * 1e4)
        d = f + rng.normal(0, 0.01 * f)
        eng = Engine(0)
        eng.stage_specs(specs)
        eng.stage_problem([wl_um, d / np.median(d)], 0.01 * f / np.median(d), fr, r, ctm, ptm, tmi, tma, matrix, nspec=2,
                          bands=bl, tmin=tmin, tmax=tmax)
        eng.stage_products((kep_wl, kep_tm), matrix=matrix)
        engines.append(eng)
        truths.append(truth)
        wls.append(wl_um)

    group = TargetGroup(engines)
    print('one launch:', group.launch_info([args.nwalkers] * args.targets)['kernel'])
    p0s = [truths[k] + 1e-3 * np.abs(truths[k]) * rng.normal(size=(args.nwalkers, 6)) for k in range(args.targets)]
    seeds = [args.seed + k for k in range(args.targets)]
    moves = [(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)] if args.moves == 'de' else None
    if args.tempered:
        sampler = run_tempered(args, group, p0s, seeds, moves, truths)
        group.close()
        return sampler
    if args.device:
        sampler = DeviceGroupSampler([args.nwalkers] * args.targets, 6, group, seeds=seeds, rng=args.rng,
                                     autocorr='device' if args.protocol else 'host', moves=moves)
    else:
        sampler = GroupSampler([args.nwalkers] * args.targets, 6, group.logposterior, seeds=seeds, moves=moves)
    t0 = time.time()
    if args.protocol:
        out = run_group_protocol(sampler, p0s, args.nburn, args.nsteps, nthin=args.nthin, dirname=args.protocol,
                                 fnames=['target{}'.format(k) for k in range(args.targets)])
        print('protocol: {} targets, production iterations per target {} in {:.2f} s (files under {})'.format(
            args.targets, [len(x) // args.nwalkers for x in out], time.time() - t0, args.protocol))
        for k in range(args.targets):
            print('target {}: Teff {:.0f} / {:.0f} (truth {:.0f} / {:.0f})'.format(k, *np.median(out[k][:, :2], axis=0), *truths[k][:2]))
        if sampler.samplers[0].iteration >= 4:   # (one computation for all targets; on the GPU with --device)
            rhat = sampler.get_rhat()
            for k in range(args.targets):
                print('target {}: split R-hat max {:.3f} (over the walkers; < 1.05 wanted)'.format(k, np.max(rhat[k])))
        if args.device:
            print_summary(sampler.get_summary(), args.targets)
            print_products(sampler.get_products(['kep_contrast', 'pri_corr', 'sec_corr']), args.targets)
        group.close()
        return sampler
    sampler.run_mcmc(p0s, args.nsteps)
    dt = time.time() - t0
    print('{} targets x {} walkers x {} steps in {:.2f} s ({:.0f} evaluations/s)'.format(
        args.targets, args.nwalkers, args.nsteps, dt, args.targets * args.nwalkers * args.nsteps / dt))
    for k in range(args.targets):
        flat = sampler.get_chain(k, discard=args.nsteps // 2, flat=True)
        print('target {}: Teff {:.0f} / {:.0f} (truth {:.0f} / {:.0f}), acceptance {:.2f}'.format(
            k, *np.median(flat[:, :2], axis=0), *truths[k][:2], sampler.acceptance_fraction[k].mean()))
    if args.nsteps - args.nsteps // 2 >= 4:
        rhat = sampler.get_rhat(discard=args.nsteps // 2)
        for k in range(args.targets):
            print('target {}: split R-hat max {:.3f} (second half, over the walkers)'.format(k, np.max(rhat[k])))
    if args.device:
        print_summary(sampler.get_summary(discard=args.nsteps // 2), args.targets)
        print_products(sampler.get_products(['kep_contrast', 'pri_corr', 'sec_corr'], discard=args.nsteps // 2), args.targets)
    if args.predictive:
        from mcmc_spec_amd import predictive
        for k in range(args.targets):
            res = predictive.check(engines[k], sampler.get_chain(k, discard=args.nsteps // 2, flat=True))
            predictive.print_report(res, wls[k], 'target {}: '.format(k))
    group.close()
    return sampler


if __name__ == '__main__':
    main()

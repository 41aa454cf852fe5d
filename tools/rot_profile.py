#!/usr/bin/env python3
"""Staging cost of the rotational broadening (DESIGN.md "Rotational broadening"): the bench's 26 x 4 x 135,000 grid,
broadened over config 2's and config 4's data windows (R = 1700) and then rotated at v sin i = 10 / 60 / 150 / 500 km/s,
limb 0.6.  Run under ``rocprofv3 --kernel-trace --stats`` for the times of rot_broaden_kernel and broaden_conv_kernel;
this script prints, per case, the shapes and the FLOPs the rotation kernel executes (rows x taps that ran x 2), as one
JSON line each (and writes them to the file named by --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def taps_run(wl, vsini):
    """Taps rot_broaden_kernel loops over for each pixel (2 kmax + 1; kmax = min(binnu, int(dlmax / dwl + 2)))."""
    dwl = wl[1] - wl[0]
    vc = vsini / 299792.458
    binnu = int(np.floor(vc * wl[-1] / dwl)) + 1
    kmax = np.minimum(binnu, (vc * wl / dwl + 2.0).astype(np.int64))
    return binnu, int(np.sum(2 * kmax + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.engine import Engine
    wl = np.arange(3000, 30000, 0.2)
    teffs, loggs = np.arange(3000, 5600, 100), np.array([4.0, 4.5, 5.0, 5.5])
    flux = synth.make_grid(teffs, loggs, wl)
    eng = Engine(0)
    rows = len(teffs) * len(loggs)
    lines = []
    for cfg, npix in (('config2', 4096), ('config4', 16384)):
        w = synth.data_wavelengths_um(npix)
        win = [np.floor(w.min() * 1e4), np.ceil(w.max() * 1e4)]
        idx = np.where((wl >= win[0]) & (wl <= win[1]))[0]
        for vsini in (10.0, 60.0, 150.0, 500.0):
            eng.stage_grid(wl, teffs, loggs, flux)
            eng.broaden_grid_window(win, 1700, vsini=vsini, limb=0.6)   # one broaden_conv_kernel + one rot_broaden_kernel
            binnu, taps = taps_run(wl[idx], vsini)
            rec = dict(case=cfg, vsini=vsini, limb=0.6, rows=rows, n=int(idx.size), binnu=binnu,
                       mean_taps=taps / idx.size, flop=2 * rows * taps)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(''.join(json.dumps(r) + '\n' for r in lines))


if __name__ == '__main__':
    main()

"""The sweep behind the default mu of the T2-spectrum fit (t2map.spectrum.DEFAULT_MU), on the CPU statement, no GPU:

    python tools/nnls_mu_sweep.py

synth.phantom_volume() (14 vials of 8 to 1044 ms, 6 echoes); from every vial the 25 voxels
numpy.random.default_rng(0).choice(voxels of the vial, 25, replace=False) draws, vial after vial from one generator; 40
log-spaced T2 from 10 to 2000 ms.  Prints, per mu, the median relative error of the geometric-mean T2 against the vial's T2
over all vials and over the vials of 40 to 700 ms, the mean number of coefficients above 0 and the mean outer steps.  The
figures in README.md and DESIGN.md section 8v are this tool's output."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MUS = (0, 0.003, 0.01, 0.02, 0.03, 0.05, 0.1, 0.2, 0.3, 1.0)


def main():
    from fetal_t2mapping_amd import _nnls as N
    from fetal_t2mapping_amd import synth

    echoes, mask, label, te, gt = synth.phantom_volume()
    grid = N.log_grid(10, 2000, 40)
    A = N.monoexp_basis(te, grid)
    rng = np.random.default_rng(0)
    rows = []
    for i, v in enumerate(gt):
        idx = np.flatnonzero(label.reshape(-1) == i + 1)
        rows += [(j, v) for j in rng.choice(idx, 25, replace=False)]
    y = echoes.reshape(len(te), -1)
    ln_t2 = N.ln_t2_functional(grid)
    for mu in MUS:
        b = N.Basis(A, mu)
        err, mid, ps, nits = [], [], [], []
        for j, v in rows:
            x, P, nit, _ = N.solve_voxel(y[:, j], b)
            g = np.exp((ln_t2 * x).sum() / x.sum())
            err.append(abs(g - v) / v)
            ps.append(len(P))
            nits.append(nit)
            if 40 <= v <= 700:
                mid.append(abs(g - v) / v)
        print(f"mu {mu}: median relative error of the geometric-mean T2, all vials {np.median(err):.4f}, vials of 40 .. 700 ms "
              f"{np.median(mid):.4f}; mean coefficients above 0 {np.mean(ps):.2f}, mean outer steps {np.mean(nits):.1f}", flush=True)
    # the same voxels with the weight chosen per voxel by the chi^2 rule at its defaults
    b = N.Basis(A, 0.0)
    err, mid, ps, nits, mus, rules = [], [], [], [], [], []
    for j, v in rows:
        x, P, nit, _, mu, _, _, rule = N.solve_voxel_chi2(y[:, j], b)
        g = np.exp((ln_t2 * x).sum() / x.sum())
        err.append(abs(g - v) / v)
        ps.append(len(P))
        nits.append(nit)
        mus.append(mu)
        rules.append(rule)
        if 40 <= v <= 700:
            mid.append(abs(g - v) / v)
    print(f"chi2 rule (factor 1.02): median relative error of the geometric-mean T2, all vials {np.median(err):.4f}, vials of 40 .. 700 ms "
          f"{np.median(mid):.4f}; mean coefficients above 0 {np.mean(ps):.2f}, mean outer steps over all solves {np.mean(nits):.1f}; chosen mu "
          f"median {np.median(mus):.4g}, 5 % .. 95 % {np.quantile(mus, 0.05):.4g} .. {np.quantile(mus, 0.95):.4g}; voxels FOUND / EXACT / LOW / HIGH "
          f"{np.bincount(rules, minlength=4).tolist()}", flush=True)


if __name__ == "__main__":
    main()

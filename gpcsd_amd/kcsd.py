"""Kernel CSD in one dimension (kCSD), the third estimator of the reference's comparisons, on the device.

The reference's scripts construct `KCSD1D` from the external `kcsd` package (simulation_studies/sim_from_gp_1D.py:14,112-127,
simple_template_1D.py:99-105, sim_from_gp_1D_mismatch.py, auditory_lfp/fit_mean_function.py:31,112-115); with
`from gpcsd_amd.kcsd import KCSD1D` in place of that import they run here.  The class has the call surface those scripts use, no more.

This is the project's own statement of the method, in closed form: Gaussian sources of width sigma_b = R / 3 at `n_src_init`
centres evenly spaced on [xmin - ext_x, xmax + ext_x]; potential basis b_j(x) = 1 / (2 sigma) int_{-R}^{R} [sqrt((u - d)^2 + h^2) -
|u - d|] g(u) du, d = x - s_j, by a two-panel Gauss-Legendre rule with `ngl` nodes per panel (accurate to ~1e-13 of the largest entry for
h / R >= 0.05 at the default 48; it degrades below that); K = B_pot^T B_pot / M, K~ = B_src^T B_pot / M, estimate K~ (K + lambda I)^-1 V.
Cross-validation is leave-one-electrode-out, err(R, lambda) = sum_i ||V_i - V^_i^(-i)||_2, from the closed form V_i - V^_i^(-i) =
beta_i / ((K + lambda I)^-1)_ii and one eigen-decomposition per R -- no refit per held-out electrode.

It is NOT kcsd-python's table-interpolated potential basis, and its results are not that package's bit for bit: the package is not
among this project's dependencies and no fixture of its outputs exists, so parity is stated against the dense long-double statement in
tests/kcsd_ref.py.  Other source types, 2D / 3D and L-curve selection are out of scope.  Everything runs on the GPU; without one the
compute calls raise (no CPU fallback).
"""
import numpy as np

from . import _hip

#: this project's default ridge grid of cross_validate (the one two of the reference's scripts pass explicitly)
DEFAULT_LAMBDAS = np.logspace(1, -15, 25)


class KCSD1D:
    def __init__(self, ele_pos, pots, src_type='gauss', sigma=1.0, h=1.0, n_src_init=300, ext_x=0.0, gdx=None, xmin=None, xmax=None,
                 R_init=0.23, lambd=0.0, ngl=48):
        if src_type != 'gauss':
            raise NotImplementedError("KCSD1D: src_type %r (only 'gauss' is implemented)" % (src_type,))
        self.ele_pos = np.ascontiguousarray(ele_pos, dtype=np.float64).reshape(-1)
        n = self.ele_pos.size
        pots = np.asarray(pots, dtype=np.float64)
        if pots.ndim not in (2, 3) or pots.shape[0] != n:
            raise ValueError("KCSD1D: pots must be (n_ele, nt) or (n_ele, nt, ntrials) with n_ele = %d, got %s" % (n, pots.shape))
        self._pots_shape = pots.shape
        self.pots = np.ascontiguousarray(pots.reshape(n, -1))
        if n < 1 or self.pots.shape[1] < 1:
            raise ValueError("KCSD1D: empty potentials")
        if not (np.all(np.isfinite(self.ele_pos)) and np.all(np.isfinite(self.pots))):
            raise ValueError("KCSD1D: non-finite electrode positions or potentials")
        self.src_type = src_type
        self.sigma, self.h = float(sigma), float(h)
        self.n_src_init, self.ext_x, self.ngl = int(n_src_init), float(ext_x), int(ngl)
        self.R_init, self.R, self.lambd = float(R_init), float(R_init), float(lambd)
        if not (self.sigma > 0 and self.h > 0 and self.R > 0 and np.isfinite([self.sigma, self.h, self.R]).all()):
            raise ValueError("KCSD1D: sigma, h and R_init must be positive")
        if not (self.lambd >= 0 and np.isfinite(self.lambd)):
            raise ValueError("KCSD1D: lambd must not be negative")
        if self.n_src_init < 1 or self.ngl < 2 or not (self.ext_x >= 0):
            raise ValueError("KCSD1D: n_src_init >= 1, ngl >= 2, ext_x >= 0")
        self.xmin = float(np.min(self.ele_pos) if xmin is None else xmin)
        self.xmax = float(np.max(self.ele_pos) if xmax is None else xmax)
        if not self.xmax >= self.xmin:
            raise ValueError("KCSD1D: xmax < xmin")
        self.gdx = 0.01 * (self.xmax - self.xmin) if gdx is None else float(np.asarray(gdx, dtype=np.float64).reshape(-1)[0])
        if not self.gdx > 0:
            if self.xmax > self.xmin or gdx is not None:
                raise ValueError("KCSD1D: gdx must be positive")
            self.gdx = 1.0
        #: estimation points xmin, xmin + gdx, ... <= xmax
        self.estm_x = self.xmin + self.gdx * np.arange(int(np.floor((self.xmax - self.xmin) / self.gdx * (1 + 1e-12))) + 1)
        #: source centres
        self.src_x = np.linspace(self.xmin - self.ext_x, self.xmax + self.ext_x, self.n_src_init)
        self._gl = np.polynomial.legendre.leggauss(self.ngl)
        self.cv_error = None
        self.cv_status = None
        self.k_pot = None
        self.k_interp_cross = None
        self._est = None              # ((R, lambd), {"csd": .., "pot": ..})

    # ---- device calls ----
    def _problem(self):
        return (self.ele_pos, self.pots, self.src_x, self.estm_x, self.h, self.sigma, self._gl[0], self._gl[1])

    def cross_validate(self, Rs=None, lambdas=None):
        """Leave-one-electrode-out scan of the basis widths `Rs` (default [R_init]) against the ridges `lambdas` (default
        DEFAULT_LAMBDAS = np.logspace(1, -15, 25), this project's default).  Sets R, lambd, cv_error (nR, nlam) and cv_status (1 marks a
        numerically singular pair, whose error is +inf and which is never selected); returns (R, lambd)."""
        Rs = np.array([self.R_init] if Rs is None else Rs, dtype=np.float64).reshape(-1)
        lambdas = np.array(DEFAULT_LAMBDAS if lambdas is None else lambdas, dtype=np.float64).reshape(-1)
        if Rs.size < 1 or lambdas.size < 1:
            raise ValueError("cross_validate: empty Rs or lambdas")
        if not (np.all(np.isfinite(Rs)) and np.all(Rs > 0)):
            raise ValueError("cross_validate: every R must be positive")
        if not (np.all(np.isfinite(lambdas)) and np.all(lambdas >= 0)):
            raise ValueError("cross_validate: no lambda may be negative")
        err, status, best, out = _hip.default_context().kcsd_cross_validate(*self._problem(), Rs, lambdas)
        self.cv_error, self.cv_status = err, status
        if best is None:
            raise np.linalg.LinAlgError("cross_validate: K + lambda I is numerically singular for every pair (R, lambda)")
        self.R, self.lambd = float(Rs[best[0]]), float(lambdas[best[1]])
        self.k_pot, self.k_interp_cross = out["k_pot"], out["k_cross"]
        self._est = ((self.R, self.lambd), {"csd": out["csd"], "pot": out["pot"]})
        return self.R, self.lambd

    def values(self, estimate='CSD'):
        """'CSD': K~ (K + lambd I)^-1 V at estm_x, (n_est, T) or (n_est, nt, ntrials) as the potentials were given; 'POT':
        K (K + lambd I)^-1 V at the electrodes."""
        if estimate not in ('CSD', 'POT'):
            raise ValueError("values: estimate must be 'CSD' or 'POT'")
        if self._est is None or self._est[0] != (self.R, self.lambd):
            out = _hip.default_context().kcsd_estimate(*self._problem(), self.R, self.lambd, want=("csd", "pot", "k_pot", "k_cross"))
            self.k_pot, self.k_interp_cross = out["k_pot"], out["k_cross"]
            self._est = ((self.R, self.lambd), {"csd": out["csd"], "pot": out["pot"]})
        v = self._est[1]["csd" if estimate == 'CSD' else "pot"]
        return v.reshape((v.shape[0],) + tuple(self._pots_shape[1:]))

"""f64 oracle of the per-axis Monte Carlo barostats (include/remd_hip_barostat.h; csrc/barostat.hip baro_axis_* kernels): OpenMM's
MonteCarloAnisotropicBarostat and MonteCarloMembraneBarostat restated on top of oracle.md_oracle.OracleBarostat, and the OracleEngine
that makes its moves.  TEST INFRASTRUCTURE ONLY, never imported by the product package.

Per attempt and replica, V = Lx Ly Lz:
  allowed axes (ascending)   anisotropic: the scaled ones;  membrane: x, y under XYAnisotropic, z under ZFree
  w = philox(seed, STREAM_BAROSTAT, 0, replica, attempt);  axis = allowed[mulhi32(w[0], n_allowed)];  u = u53(w[2], w[3])
  dV = volumeScale[axis] 2 (u - 1/2),  V' = V + dV,  f = V'/V      (the three volumeScales start at 0.01 V)
  s = (1, 1, 1);  s[axis] = f;  membrane XYIsotropic on x: sx = sy = sqrt(f);  ConstantVolume: sz = 1 / (sx sy), V' = V, dV = 0
  dA = Lx sx Ly sy - Lx Ly
  weight = U' - U + c (1/V' - 1/V) + p dV - gamma dA - N_mol kT ln(V'/V);  reject when weight > 0 and u' > exp(-weight / kT)
  after >= 10 attempts on the axis: < 25 % accepted -> volumeScale[axis] /= 1.1,  > 75 % -> min(x 1.1, 0.3 V), window reset
"""
import numpy as np
from oracle import md_oracle as mo
from oracle_engine import OracleEngine

ANISOTROPIC, MEMBRANE = 1, 2
XY_ISOTROPIC, XY_ANISOTROPIC = 0, 1
Z_FREE, Z_FIXED, CONSTANT_VOLUME = 0, 1, 2


def mulhi32(a, b):
    return (int(a) * int(b)) >> 32


class AxisOracleBarostat(mo.OracleBarostat):
    """``axes``: the scale mask scaleX | scaleY << 1 | scaleZ << 2 (anisotropic) or the xy mode (membrane).  ``surface_tension``: a
    number, or a function of the replica key the move is made for (the engine looks up the replica's state).  ``state[replica]`` holds
    dict(scale[3], window_attempted[3], window_accepted[3], attempted[3], accepted[3]); ``last`` the weight and the uniform of
    the latest attempt."""

    def __init__(self, system, seed, molecules, kind, axes, zmode=Z_FREE, surface_tension=0.0):
        super().__init__(system, seed, molecules)
        self.kind, self.axes, self.zmode = int(kind), int(axes), int(zmode)
        self.surface_tension = surface_tension
        self.last = None

    def allowed_axes(self):
        if self.kind == ANISOTROPIC:
            return [a for a in range(3) if (self.axes >> a) & 1]
        return [0] + ([1] if self.axes == XY_ANISOTROPIC else []) + ([2] if self.zmode == Z_FREE else [])

    def attempt(self, x, box, kT, pressure, replica, attempt, long_range=0.0, **lam):
        box = np.asarray(box, dtype=np.float64)
        V = float(np.prod(box))
        st = self.state.get(replica)
        if st is None:
            st = self.state[replica] = dict(scale=np.full(3, 0.01 * V), window_attempted=np.zeros(3, int), window_accepted=np.zeros(3, int),
                                            attempted=np.zeros(3, int), accepted=np.zeros(3, int))
        gamma = self.surface_tension(replica) if callable(self.surface_tension) else float(self.surface_tension)
        if self.kind == ANISOTROPIC:
            gamma = 0.0
        U0 = self.s.potential(x, box, **lam)
        allowed = self.allowed_axes()
        w = mo.draw(self.seed, mo.STREAM_BAROSTAT, 0, replica, attempt)
        axis = allowed[mulhi32(w[0], len(allowed))]
        dV = st['scale'][axis] * 2.0 * (mo.u53(w[2], w[3]) - 0.5)
        newV = V + dV
        f = newV / V
        s = np.ones(3)
        if self.kind == MEMBRANE and axis < 2 and self.axes == XY_ISOTROPIC:
            s[0] = s[1] = np.sqrt(f)
        else:
            s[axis] = f
        if self.kind == MEMBRANE and self.zmode == CONSTANT_VOLUME:
            s[2] = 1.0 / (s[0] * s[1])
            newV, dV = V, 0.0
        dA = box[0] * s[0] * box[1] * s[1] - box[0] * box[1]
        xn = x.copy()
        for m in self.mols:
            c = x[m].mean(axis=0)
            cw = c - np.floor(c / box) * box
            xn[m] += cw * (s - 1.0) - (c - cw)
        boxn = box * s
        U1 = self.s.potential(xn, boxn, **lam)
        wgt = U1 - U0 + long_range * (1.0 / newV - 1.0 / V) + pressure * dV - gamma * dA - len(self.mols) * kT * np.log(newV / V)
        q = mo.draw(self.seed, mo.STREAM_BAROSTAT, 1, replica, attempt)
        uq = mo.u53(q[2], q[3])
        reject = (not (wgt <= 0.0)) and (not (uq <= np.exp(-wgt / kT)))
        self.last = dict(replica=replica, attempt=attempt, axis=axis, weight=float(wgt), uniform=uq, accepted=not reject)
        if reject:
            xn, boxn = x, box
        else:
            st['window_accepted'][axis] += 1; st['accepted'][axis] += 1
        st['window_attempted'][axis] += 1; st['attempted'][axis] += 1
        if st['window_attempted'][axis] >= 10:
            Vc = float(np.prod(boxn))
            if st['window_accepted'][axis] < 0.25 * st['window_attempted'][axis]:
                st['scale'][axis] /= 1.1; st['window_attempted'][axis] = 0; st['window_accepted'][axis] = 0
            elif st['window_accepted'][axis] > 0.75 * st['window_attempted'][axis]:
                st['scale'][axis] = min(st['scale'][axis] * 1.1, Vc * 0.3); st['window_attempted'][axis] = 0; st['window_accepted'][axis] = 0
        return xn, boxn, (not reject)


class AxisOracleEngine(OracleEngine):
    """OracleEngine with HipEngine.set_barostat_axes / barostat_axis_stats: the base engine creates its barostat only when it has
    none, so the per-axis one is put in its place before a move can be made."""

    _axis = None

    def set_barostat(self, pressure, frequency=25):
        super().set_barostat(pressure, frequency)
        self._axis = None

    def set_barostat_axes(self, pressure, surface_tension, kind, xy_or_scale_mask, zmode=0, frequency=25):
        super().set_barostat(pressure, frequency)
        self._axis = (int(kind), int(xy_or_scale_mask), int(zmode))
        self.tension = np.zeros(len(self.pressure)) if surface_tension is None or kind == ANISOTROPIC else np.array(surface_tension, dtype=np.float64)

    def _tension_of(self, key):
        ids = getattr(self, 'noise_ids', None)
        rg = int(key) if ids is None else self.r_begin + int(np.where(ids == key)[0][0])
        return float(self.tension[self.labels[rg]])

    def _axis_barostat(self):
        if self._axis is not None and self._baro is None:
            self._baro = AxisOracleBarostat(self.sys, self.seed_value, mo.molecules_from_desc(self.sys.d), *self._axis,
                                            surface_tension=self._tension_of)

    def propagate(self, iteration):
        self._axis_barostat()
        return super().propagate(iteration)

    def barostat_attempts(self, n_attempts):
        self._axis_barostat()
        return super().barostat_attempts(n_attempts)

    def barostat_axis_stats(self):
        vs, na, nc = np.zeros((self.R, 3)), np.zeros((self.R, 3), np.int64), np.zeros((self.R, 3), np.int64)
        for r in range(self.R):
            st = self._baro.state.get(self._nk(r)) if self._baro is not None else None
            if st is not None:
                vs[r], na[r], nc[r] = st['scale'], st['attempted'], st['accepted']
        return vs, na, nc

    def compute_energies(self, d_rows=None, want_host=True, want_potential=False):
        rows, U = super().compute_energies(d_rows, want_host, want_potential=True)
        if self._axis is not None and self._axis[0] == MEMBRANE and getattr(self, 'pressure', None) is not None:
            # states.py:1915-1916: - beta_l gamma_l A_xy(r)
            rows = rows - self.beta[None, :] * self.tension[None, :] * (self.box[:, 0] * self.box[:, 1])[:, None]
            self._rows = rows
        return (rows, U) if want_potential else rows


# ---- the ideal-gas checks shared by the CPU and the GPU tests ---------------------------------------------------------------------
N_MOVES, N_BURN_IN = 6000, 1000           # the schedule of tests/test_npt_cpu.py::test_oracle_barostat_ideal_gas_volume


def check_ideal_gas_statistics(values, expect, N, attempted, accepted, axes):
    """the three bounds of the ideal-gas tests: mean within 5 sem + 1 %, sigma / mean within 0.8 ... 1.25 of (N + 1)^-1/2 (a
    Gamma(N + 1) distribution), acceptance 0.2 ... 0.9 on every axis that moves"""
    mean = values.mean()
    sem = values.std() / np.sqrt(values.size / 15.0)
    print('mean %.5f expect %.5f sem %.5f rel %.5f (N+1)^-1/2 %.5f acceptance %s' % (mean, expect, sem, values.std() / mean, (N + 1) ** -0.5,
                                                                                    (accepted[:, axes] / attempted[:, axes]).round(3).tolist()))
    assert abs(mean - expect) < 5 * sem + 0.01 * expect, (mean, expect, sem)
    rel = values.std() / mean
    assert 0.8 / np.sqrt(N + 1) < rel < 1.25 / np.sqrt(N + 1), rel
    rate = accepted[:, axes] / attempted[:, axes]
    assert np.all((rate > 0.2) & (rate < 0.9)), rate

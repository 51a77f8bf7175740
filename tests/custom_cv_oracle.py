"""f64 reference for system.RMSDForce and system.CustomCVForce, by a route that shares nothing with csrc/custom_cv.hip: the optimal
superposition by Kabsch's method through numpy.linalg.svd with the determinant correction (the device diagonalises Horn's quaternion
matrix with Jacobi rotations), the energy expression over dual numbers (tests/custom_dual_oracle.py) whose gradient runs over the
collective variables.

RMSD(x) = sqrt(min_U sum_i |x_i - c - U y_i|^2 / n), y the reference centred on its own centroid, c the centroid of x.  At the optimum
the value is stationary in U and c, so dRMSD/dx_i = (x_i - c - U y_i) / (n RMSD).
"""
import numpy as np

import custom_dual_oracle as dual
import tabulated_oracle

MSD_FLOOR = 1e-20                       # nm^2: below it the RMSD is 0 and carries no force (OpenMM's reference behaviour)


def kabsch(x, reference):
    """(rmsd, U [3][3], gradient [n][3]) of the particles x [n][3] against reference [n][3] (neither needs to be centred)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(reference, dtype=np.float64)
    n = len(x)
    xc, yc = x - x.mean(axis=0), y - y.mean(axis=0)
    u, _, vt = np.linalg.svd(xc.T @ yc)                           # sum_i x_i y_i^T = u s vt; maximise tr(U^T u s vt) over proper U
    d = 1.0 if np.linalg.det(u @ vt) > 0.0 else -1.0
    U = u @ np.diag([1.0, 1.0, d]) @ vt
    e = xc - yc @ U.T
    msd = float((e * e).sum() / n)
    if msd < MSD_FLOOR:
        return 0.0, U, np.zeros_like(e)
    rmsd = np.sqrt(msd)
    return rmsd, U, e / (n * rmsd)


def rmsd(x, reference):
    return kabsch(x, reference)[0]


def variables_of(force):
    """[(name, particles, reference rows)] of a CustomCVForce, or of a bare RMSDForce as the variable v"""
    if not hasattr(force, 'getNumCollectiveVariables'):
        pairs = [('v', force)]
    else:
        pairs = [(force.getCollectiveVariableName(i), force.getCollectiveVariable(i)) for i in range(force.getNumCollectiveVariables())]
    out = []
    for name, v in pairs:
        ref = v.getReferencePositions()
        particles = v.getParticles() or list(range(len(ref)))
        out.append((name, particles, ref[particles]))
    return out


def evaluate(force, positions, global_values=None):
    """(energy, forces [N][3], RMSDs [n_cvs], per-variable force contributions [n_cvs][N][3]) of one CustomCVForce or bare RMSDForce"""
    x = np.asarray(positions, dtype=np.float64)
    variables = variables_of(force)
    energy = force.getEnergyFunction() if hasattr(force, 'getEnergyFunction') else 'v'
    g = {}
    functions = {}
    if hasattr(force, 'getNumGlobalParameters'):
        g = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
        for i in range(force.getNumTabulatedFunctions()):
            f = force.getTabulatedFunction(i)
            if type(f).__name__ == 'Continuous1DFunction':
                values, lo, hi = f.getFunctionParameters()[:3]
                functions[force.getTabulatedFunctionName(i)] = tabulated_oracle.Spline(values, lo, hi, f.getPeriodic())
            else:
                functions[force.getTabulatedFunctionName(i)] = tabulated_oracle.Lookup(f.getFunctionParameters())
    g.update(global_values or {})
    k = len(variables)
    V, grads = [], []
    for _, particles, ref in variables:
        v, _, grad = kabsch(x[particles], ref)
        V.append(v); grads.append(grad)
    values = dict(g)
    for i, (name, _, _) in enumerate(variables):
        values[name] = dual.Dual(V[i], np.eye(k)[i])
    e = dual.Expression(energy)(values, dict(dual.FUNCTIONS, **functions))
    if not isinstance(e, dual.Dual):
        e = dual.Dual(e, np.zeros(k))
    parts = np.zeros((k,) + x.shape)
    for i, (_, particles, _) in enumerate(variables):
        parts[i, particles] = -e.g[i] * grads[i]
    return e.v, parts.sum(axis=0), np.array(V), parts

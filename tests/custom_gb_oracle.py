"""TEST INFRASTRUCTURE (oracle): f64 restatement of an OBC-family CustomGBForce (openmmtools_amd/custom_gb.py) with OpenMM's CustomGBForce
semantics for NoCutoff and CutoffPeriodic: the pair computed value I and the pair energy term see the minimum image of every pair, and
only pairs with r < cutoff (no shift, no switch); the single-particle terms are unchanged.  The alchemical forms scale I by s_j, the
single-particle terms by s_i and the pair term's charges by s_i, s_j (s = lambda_electrostatics on the alchemical particles, 1 elsewhere),
as _alchemically_modify_CustomGBForce writes them (the reference's alchemy.py:2223-2345).  Forces by autograd.

Pinned by tests/test_custom_gb_cpu.py against tests/golden/reference_custom_gb.json: the reference's own strings of
testsystems.CustomGBForceSystem and the rewrite rules, evaluated by an interpreter of the CustomGBForce semantics
(tests/golden/make_golden_custom_gb.py).  It lives in tests/ next to oracle_engine.py; oracle/gbsa.py is the NoCutoff OBC2 one.
"""
import numpy as np
import torch

OBC2 = dict(offset=0.009, alpha=1.0, beta=0.8, gamma=4.85, ke=138.935485, surface=28.3919551, probe=0.14)


def custom_gb_energy_torch(x, charge, radius, scale, alchemical, lam, model=None, box=None, cutoff=None, solute_dielectric=1.0,
                           solvent_dielectric=78.5, surface_area=True, return_parts=False):
    """x: [n, 3] tensor (f64).  box: the three edges of a rectangular box (minimum image) or None.  cutoff: pair cutoff or None."""
    m = dict(OBC2, **(model or {}))
    n = x.shape[0]
    q = torch.as_tensor(np.asarray(charge, dtype=np.float64)); R = torch.as_tensor(np.asarray(radius, dtype=np.float64))
    sc = torch.as_tensor(np.asarray(scale, dtype=np.float64)); a = torch.as_tensor(np.asarray(alchemical, dtype=np.float64))
    s = lam * a + (1.0 - a)
    orr = R - m['offset']
    sr = sc * orr
    eye = torch.eye(n, dtype=torch.bool)
    d = x[:, None, :] - x[None, :, :]
    if box is not None:
        L = torch.as_tensor(np.asarray(box, dtype=np.float64))
        d = d - L * torch.round((d / L).detach())
    r = torch.sqrt((d * d).sum(-1) + eye.double())                     # (diagonal: 1, masked below)
    inside = ~eye if cutoff is None else (~eye) & (r < cutoff)
    or1, sr2 = orr[:, None], sr[None, :]
    U = r + sr2
    D = torch.abs(r - sr2)
    Lm = torch.maximum(or1.expand(n, n), D)
    C = 2.0 * (1.0 / or1 - 1.0 / Lm) * (sr2 - r - or1 >= 0).double()
    H = (r + sr2 - or1 >= 0).double() * 0.5 * (1.0 / Lm - 1.0 / U + 0.25 * (r - sr2 ** 2 / r) * (1.0 / U ** 2 - 1.0 / Lm ** 2)
                                                 + 0.5 * torch.log(Lm / U) / r + C)
    I = torch.where(inside, s[None, :] * H, torch.zeros_like(H)).sum(1)
    psi = I * orr
    B = 1.0 / (1.0 / orr - torch.tanh(m['alpha'] * psi - m['beta'] * psi ** 2 + m['gamma'] * psi ** 3) / R)
    tau = 1.0 / solute_dielectric - 1.0 / solvent_dielectric
    e = (-0.5 * m['ke'] * tau * s * q ** 2 / B).sum()
    if surface_area:
        e = e + (s * m['surface'] * (R + m['probe']) ** 2 * (R / B) ** 6).sum()
    BB = B[:, None] * B[None, :]
    f = torch.sqrt(r ** 2 + BB * torch.exp(-r ** 2 / (4.0 * BB)))
    pair = -m['ke'] * tau * (s * q)[:, None] * (s * q)[None, :] / f
    e = e + 0.5 * torch.where(inside, pair, torch.zeros_like(pair)).sum()
    return (e, I, B) if return_parts else e


def custom_gb_energy_forces(x, gb, lam=1.0, box=None, forces=True):
    """energy (kJ/mol) and forces of system_to_desc's d['gbsa'] (model keys included) at positions x [n, 3]"""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=forces)
    model = {k: float(gb[k]) for k in OBC2}
    cutoff = float(gb['cutoff']) if int(gb.get('method', 0)) == 2 else None
    e = custom_gb_energy_torch(xt, gb['charge'], gb['radius'], gb['scale'], gb['alchemical'], lam, model, box if cutoff else None, cutoff,
                               gb['solute_dielectric'], gb['solvent_dielectric'], bool(gb['surface_area']))
    if not forces:
        return float(e.detach()), None
    (g,) = torch.autograd.grad(e, xt)
    return float(e.detach()), -g.numpy()

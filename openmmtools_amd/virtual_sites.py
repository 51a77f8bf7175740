"""Virtual sites on the host: where a site sits for given parents (numpy f64), for whole arrays of positions.

The engine places the sites on the device (csrc/virtual_sites.hip); this is what test systems and callers use to hand in positions
whose sites already sit where they belong, and what reads a site table back into coordinates."""
import numpy as np


def place(kind, parents, weights):
    """The site of OpenMM's definitions: ``kind`` 'TwoParticleAverageSite' / 0, 'ThreeParticleAverageSite' / 1 (x = sum w_i x_i) or
    'OutOfPlaneSite' / 2 (x = x1 + w12 r12 + w13 r13 + wcross r12 x r13); parents [..., n_parents, 3], plain differences."""
    p = np.asarray(parents, dtype=np.float64)
    w = [float(v) for v in weights]
    if kind in ('TwoParticleAverageSite', 0):
        return w[0] * p[..., 0, :] + w[1] * p[..., 1, :]
    if kind in ('ThreeParticleAverageSite', 1):
        return w[0] * p[..., 0, :] + w[1] * p[..., 1, :] + w[2] * p[..., 2, :]
    if kind in ('OutOfPlaneSite', 2):
        r12, r13 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :]
        return p[..., 0, :] + w[0] * r12 + w[1] * r13 + w[2] * np.cross(r12, r13)
    raise NotImplementedError('virtual site kind %r' % (kind,))


def place_all(system, positions):
    """A copy of positions [..., N, 3] with every virtual site of ``system`` at its place."""
    x = np.array(positions, dtype=np.float64)
    for s, site in sorted(getattr(system, 'virtual_sites', {}).items()):
        idx = [site.getParticle(k) for k in range(site.getNumParticles())]
        x[..., s, :] = place(site.kind, x[..., idx, :], site._weights)
    return x

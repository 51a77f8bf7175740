// One term of a CMAPTorsionForce (cmap.hip; include/remd_hip_custom.h, REMD_CUSTOM_CMAP): the two dihedrals of eight particles with
// their gradients, and the map's bicubic patch at them.
//
// The dihedral is that of cst_particles_op (custom_machine.h) and of PeriodicTorsionForce, operation for operation, so a CMAP term and
// the compound-bond expression m(dihedral(p1,p2,p3,p4), dihedral(p5,p6,p7,p8)) agree to rounding: with b1 = p1 - p0, b2 = p2 - p1,
// b3 = p3 - p2, m = b1 x b2, n = b2 x b3, the angle is atan2(|b2| b1.n, m.n) in (-pi, pi], and its gradients are -|b2| m / |m|^2 on p0,
// |b2| n / |n|^2 on p3 and the two combinations that make the four sum to zero.  Degenerate geometry follows that convention too: |m|^2
// and |n|^2 are taken as at least 1e-24 nm^4, so three collinear particles give m = 0 (or n = 0) exactly or nearly and a finite angle
// (atan2 of zeros: 0, or +-pi by the signs of the zeros); the gradient on the end particle of the collinear triple, -|b2| m / max(|m|^2,
// 1e-24), falls to zero with m, the one on the other end particle stays |b2| n / |n|^2, and the middle two follow by the same
// combinations.  Nothing is a NaN as long as the middle bond b2 has a length.
//
// Plain C++ without a device call, so the same text compiles for the host (tests/test_cmap_cpu.py runs the tests' 70-term case
// through it without a GPU).
#pragma once
#include "table2d_patch.h"

struct cm3 { double x, y, z; };

CST_FN cm3 cm3_make(double x, double y, double z) { cm3 r; r.x = x; r.y = y; r.z = z; return r; }
CST_FN double cm3_dot(cm3 a, cm3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
CST_FN cm3 cm3_crs(cm3 a, cm3 b) { return cm3_make(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
CST_FN cm3 cm3_scl(cm3 a, double s) { return cm3_make(a.x * s, a.y * s, a.z * s); }
CST_FN cm3 cm3_add(cm3 a, cm3 b) { return cm3_make(a.x + b.x, a.y + b.y, a.z + b.z); }
CST_FN double cm_image(double d, double L) { return L > 0.0 ? d - L * rint(d / L) : d; }
// q - p of two f32 positions, formed in f64; a minimum image where the box lengths are positive (0: the force is not periodic)
CST_FN cm3 cm3_diff(const float* q, const float* p, double Lx, double Ly, double Lz)
{
    return cm3_make(cm_image((double)q[0] - (double)p[0], Lx), cm_image((double)q[1] - (double)p[1], Ly), cm_image((double)q[2] - (double)p[2], Lz));
}

// the dihedral of the bonds b1, b2, b3 and its gradient with respect to the four particles
CST_FN double cmap_dihedral(cm3 b1, cm3 b2, cm3 b3, cm3& g0, cm3& g1, cm3& g2, cm3& g3)
{
    const cm3 m = cm3_crs(b1, b2), nn = cm3_crs(b2, b3);
    const double mm = cm3_dot(m, m), nn2 = cm3_dot(nn, nn);
    const double m2 = mm > 1e-24 ? mm : 1e-24, n2 = nn2 > 1e-24 ? nn2 : 1e-24;
    const double lb2 = sqrt(cm3_dot(b2, b2));
    const double v = atan2(lb2 * cm3_dot(b1, nn), cm3_dot(m, nn));
    g0 = cm3_scl(m, -lb2 / m2); g3 = cm3_scl(nn, lb2 / n2);
    const double s12 = cm3_dot(b1, b2) / (lb2 * lb2), s32 = cm3_dot(b3, b2) / (lb2 * lb2);
    g1 = cm3_add(cm3_scl(g0, -(1.0 + s12)), cm3_scl(g3, s32));
    g2 = cm3_add(cm3_scl(g3, -(1.0 + s32)), cm3_scl(g0, s12));
    return v;
}

// One term: p[8][4] the particles' f32 positions (x, y, z, unused), B the map's block (table2d_patch.h).  Returns the energy;
// F[0 ... 3] = -dE/dp of the first dihedral's particles, F[4 ... 7] of the second's (a particle both name gets both).
CST_FN double cmap_term(const double* __restrict__ B, const float (&p)[8][4], double Lx, double Ly, double Lz, cm3 (&F)[8])
{
    double ang[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const int q = 4 * d;
        ang[d] = cmap_dihedral(cm3_diff(p[q + 1], p[q], Lx, Ly, Lz), cm3_diff(p[q + 2], p[q + 1], Lx, Ly, Lz), cm3_diff(p[q + 3], p[q + 2], Lx, Ly, Lz),
                               F[q], F[q + 1], F[q + 2], F[q + 3]);
    }
    double v, k[2];
    cst_table2d(B, ang[0], ang[1], v, k[0], k[1]);
#pragma unroll
    for (int a = 0; a < 8; ++a) F[a] = cm3_scl(F[a], -k[a >> 2]);
    return v;
}

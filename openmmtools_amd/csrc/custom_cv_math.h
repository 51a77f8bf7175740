// The optimal superposition behind RMSDForce (custom_cv.hip): from the 3 x 3 correlation matrix S_ab = sum_i x_ia ref_ib of the centred
// particles x and the centred reference, the proper rotation U that minimises sum_i |x_i - U ref_i|^2.  Horn's method (J. Opt. Soc.
// Am. A 4, 629, 1987): U is the rotation of the unit quaternion that is the eigenvector of the largest eigenvalue of a symmetric
// 4 x 4 matrix built from S.  A quaternion always gives det U = +1, so a mirrored set gets the best PROPER rotation with no
// determinant correction.  The eigenpair comes from cyclic Jacobi rotations in f64: slower than Newton on the characteristic
// polynomial, but it needs no well-separated largest root -- a planar or collinear reference, or particles that all coincide, make
// the two largest eigenvalues equal, and then any vector of their eigenspace gives the same U ref_i.
//
// Plain C++ without a device call or a table indexed at run time, so the same text compiles for the host: every loop over matrix
// indices has constant bounds and is unrolled, which keeps the two 4 x 4 matrices in registers (an index known only at run time
// would send them to scratch memory).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define CV_FN __host__ __device__ __forceinline__
#else
#define CV_FN inline
#endif

constexpr int CV_MAX_SWEEPS = 30;          // 5 at most seen (tests/test_custom_cv_cpu.py compiles this file for the host); the cap only bounds a matrix of NaNs
constexpr double CV_OFF_THRESHOLD = 1e-32; // off-diagonal squares below this share of the squared Frobenius norm: converged

// one Jacobi rotation in the plane (P, Q) of the symmetric A, accumulated in the columns of V
template <int P, int Q>
CV_FN void cv_jacobi_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    // (a huge theta: t = 1 / (2 theta) without forming theta^2)
    const double t = fabs(theta) > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    A[P][P] -= t * apq; A[Q][Q] += t * apq;
    A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = A[k][P], akq = A[k][Q];
            A[k][P] = A[P][k] = akp - s * (akq + tau * akp);
            A[k][Q] = A[Q][k] = akq + s * (akp - tau * akq);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = vkp - s * (vkq + tau * vkp);
        V[k][Q] = vkq + s * (vkp - tau * vkq);
    }
}

// S[a][b] = sum_i x_ia ref_ib (both centred) -> U[a][b], row-major, with x_i ~ U ref_i; returns the sweeps taken
CV_FN int cv_superpose(const double (&S)[3][3], double (&U)[3][3])
{
    // Horn's matrix for the rotation that takes the reference onto the particles: his M = sum ref x^T is S transposed
    const double Sxx = S[0][0], Sxy = S[1][0], Sxz = S[2][0], Syx = S[0][1], Syy = S[1][1], Syz = S[2][1], Szx = S[0][2], Szy = S[1][2], Szz = S[2][2];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    int sweeps = 0;
    for (; sweeps < CV_MAX_SWEEPS; ++sweeps) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
        if (!(off > CV_OFF_THRESHOLD * (diag + 2.0 * off))) break;
        cv_jacobi_rotate<0, 1>(A, V); cv_jacobi_rotate<0, 2>(A, V); cv_jacobi_rotate<0, 3>(A, V);
        cv_jacobi_rotate<1, 2>(A, V); cv_jacobi_rotate<1, 3>(A, V); cv_jacobi_rotate<2, 3>(A, V);
    }
    // the column of the largest eigenvalue (the first of equal ones), picked by value
    double lam = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const bool up = A[j][j] > lam;
        lam = up ? A[j][j] : lam;
        q0 = up ? V[0][j] : q0; q1 = up ? V[1][j] : q1; q2 = up ? V[2][j] : q2; q3 = up ? V[3][j] : q3;
    }
    const double nq = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3;
    const double in = nq > 0.0 ? 1.0 / sqrt(nq) : 0.0;       // (nq is 1 within rounding; NaN input stays NaN)
    q0 *= in; q1 *= in; q2 *= in; q3 *= in;
    U[0][0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; U[0][1] = 2.0 * (q1 * q2 - q0 * q3); U[0][2] = 2.0 * (q1 * q3 + q0 * q2);
    U[1][0] = 2.0 * (q1 * q2 + q0 * q3); U[1][1] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3; U[1][2] = 2.0 * (q2 * q3 - q0 * q1);
    U[2][0] = 2.0 * (q1 * q3 - q0 * q2); U[2][1] = 2.0 * (q2 * q3 + q0 * q1); U[2][2] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
    return sweeps;
}

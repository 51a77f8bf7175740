// Constraint units on the device: the arithmetic that moves one unit -- a rigid water (SETTLE), an X-H star cluster (SHAKE) or up to
// four free atoms -- through the V / R / O substeps of a Langevin splitting, with its <= 4 atoms' x, v and 1/m in registers.  ONE copy
// for the integrator chain (integrate.hip), the resident small-molecule kernel (resident.hip) and the FIRE minimiser (minimize.hip).
// Reference semantics (restated):
//   openmmtools/integrators.py:1404-1423  R: x += (dt/n_R) v ; constrain x ; v += (x - x1)/(dt/n_R) ; constrain v
//   openmmtools/integrators.py:1425-1446  V: v += (dt/n_V) f/m ; constrain v
//   openmmtools/integrators.py:1448-1460  O: v = a v + b sigma xi ; constrain v,  a = exp(-gamma h), b = sqrt(1-a^2),
//                                            h = dt/max(1,n_O) (:1142-1146), sigma = sqrt(kT/m) (:1314)
#pragma once
#include "remd_internal.h"
#include "rng.h"

#define UNIT_FREE   0
#define UNIT_SETTLE 1
#define UNIT_SHAKE  2
#define MAX_TOK 24
#define FIXED_TO_F32 (1.0f / 4294967296.0f)      // a 2^32 fixed-point force or momentum word as fp32 (1 / REMD_FORCE_SCALE)

// What every step program holds, whoever runs it (resident_prog: a whole propagation; chain_prog, one launch of the integrator chain,
// has the same fields among its own: the functions below take either).
struct step_prog {
    int n;                 // tokens
    char tok[MAX_TOK];     // 'V','R','O' (the chain has more: integrate.hip)
    int o_index[MAX_TOK];  // for 'O': index of this O inside the step program
    float hV, hR;          // dt/n_V, dt/n_R
    float a, b;            // OU coefficients
    int nO;
};

// The shared fields from a parsed splitting (at most MAX_TOK tokens; none: the caller adds its tokens itself).
template <typename Prog> inline void remd_step_prog_fill(Prog& p, const std::vector<char>& tokens, double dt, double gamma, int nV, int nR, int nO)
{
    p.n = (int)tokens.size();
    int oidx = 0;
    for (int t = 0; t < p.n; ++t) { p.tok[t] = tokens[t]; p.o_index[t] = tokens[t] == 'O' ? oidx++ : 0; }
    p.hV = (float)(dt / (nV > 0 ? nV : 1)); p.hR = (float)(dt / (nR > 0 ? nR : 1));
    const double hO = dt / (nO > 0 ? nO : 1);                   // integrators.py:1142
    p.a = (float)exp(-gamma * hO);                              // :1143
    p.b = (float)sqrt(1.0 - exp(-2.0 * gamma * hO));            // :1146
    p.nO = nO > 0 ? nO : 1;
}

// token t of the program, from registers: a dynamic index into the kernel-argument array is a scalar memory load per token on the
// chain's critical path (the chain is a handful of wavefronts waiting for one thing after another: profiles/r05_15_chain_segments.txt);
// the six words are loaded once with the other arguments
template <typename Prog> __device__ __forceinline__ char prog_tok(const Prog& prog, int t)
{
    static_assert(MAX_TOK == 24, "six 32-bit words of tokens");
    const unsigned int* w = reinterpret_cast<const unsigned int*>(prog.tok);
    const unsigned int w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5];
    const int q = t >> 2;
    const unsigned int x = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : q == 3 ? w3 : q == 4 ? w4 : w5;
    return (char)((x >> ((t & 3) * 8)) & 0xffu);
}

// state of one constraint unit between the segments of a chain (registers)
struct unit_regs { float3 x[4], v[4]; float im[4]; float heat, shadow;
    int shake_it;                            // most Newton updates a position solve of this unit needed in this launch (X-H clusters)
    float cmx, cmy, cmz; int have_cm;        // centre-of-mass velocity from an 'M' token of this launch, for the 'C' that follows it
#ifdef CHAIN_STAMPS
    unsigned long long* stamps; unsigned long long t_last;     // tools/chain_segments.py: per-token wall-clock of workgroup (0, 0)
#endif
};

struct settle_const { float mO, mH, ra, rb, rc, dOH, dHH; };

__device__ __forceinline__ float3 f3(float x, float y, float z) { return make_float3(x, y, z); }
__device__ __forceinline__ float3 operator+(float3 a, float3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ float3 operator-(float3 a, float3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 operator*(float3 a, float s) { return f3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float3 cross3(float3 a, float3 b) {
    return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// One wavefront per SIMD at best (a few hundred waves per launch): the chain kernel is bound by the LATENCY of its
// dependent arithmetic, so the 1-ulp hardware reciprocal / square root / reciprocal square root replace the IEEE
// expansions (~10 dependent instructions each) of '/', sqrtf and rsqrtf; fp32 SETTLE is ~1e-7 relative either way.
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }

// Analytic SETTLE (Miyamoto & Kollman 1992) in coordinates relative to the old O position:
// p0[] old (constrained) positions relative to A0 (p0[0] = 0), p1[] unconstrained new
// positions relative to A0.  Returns constrained new positions (relative to A0) in p1.
__device__ __forceinline__ void settle_positions(const settle_const& sc, const float3* p0, float3* p1)
{
    const float3 b0 = p0[1], c0 = p0[2];
    const float M = sc.mO + 2.f * sc.mH;
    const float3 d0 = (p1[0] * sc.mO + p1[1] * sc.mH + p1[2] * sc.mH) * frcp(M);
    const float3 a1 = p1[0] - d0, b1 = p1[1] - d0, c1 = p1[2] - d0;
    float3 Z = cross3(b0, c0);
    float3 X = cross3(a1, Z);
    float3 Y = cross3(Z, X);
    X = X * frsq(dot3(X, X)); Y = Y * frsq(dot3(Y, Y)); Z = Z * frsq(dot3(Z, Z));
    const float xb0 = dot3(X, b0), yb0 = dot3(Y, b0);
    const float xc0 = dot3(X, c0), yc0 = dot3(Y, c0);
    const float za1 = dot3(Z, a1);
    const float xb1 = dot3(X, b1), yb1 = dot3(Y, b1), zb1 = dot3(Z, b1);
    const float xc1 = dot3(X, c1), yc1 = dot3(Y, c1), zc1 = dot3(Z, c1);
    const float sinphi = za1 * frcp(sc.ra);
    const float cosphi = fsqrt(fmaxf(0.f, 1.f - sinphi * sinphi));
    const float sinpsi = (zb1 - zc1) * frcp(2.f * sc.rc * cosphi);
    const float cospsi = fsqrt(fmaxf(0.f, 1.f - sinpsi * sinpsi));
    const float ya2 = sc.ra * cosphi;
    const float xb2 = -sc.rc * cospsi;
    const float yb2 = -sc.rb * cosphi - sc.rc * sinpsi * sinphi;
    const float yc2 = -sc.rb * cosphi + sc.rc * sinpsi * sinphi;
    const float alpha = xb2 * (xb0 - xc0) + yb0 * yb2 + yc0 * yc2;
    const float beta  = xb2 * (yc0 - yb0) + xb0 * yb2 + xc0 * yc2;
    const float gamma = xb0 * yb1 - xb1 * yb0 + xc0 * yc1 - xc1 * yc0;
    const float al2be2 = alpha * alpha + beta * beta;
    const float sintheta = (alpha * gamma - beta * fsqrt(fmaxf(0.f, al2be2 - gamma * gamma))) * frcp(al2be2);
    const float costheta = fsqrt(fmaxf(0.f, 1.f - sintheta * sintheta));
    const float xa3 = -ya2 * sintheta, ya3 = ya2 * costheta, za3 = za1;
    const float xb3 = xb2 * costheta - yb2 * sintheta, yb3 = xb2 * sintheta + yb2 * costheta, zb3 = zb1;
    const float xc3 = -xb2 * costheta - yc2 * sintheta, yc3 = -xb2 * sintheta + yc2 * costheta, zc3 = zc1;
    p1[0] = X * xa3 + Y * ya3 + Z * za3 + d0;
    p1[1] = X * xb3 + Y * yb3 + Z * zb3 + d0;
    p1[2] = X * xc3 + Y * yc3 + Z * zc3 + d0;
}

// Analytic velocity constraint for a rigid triangle: remove the relative velocity along the
// three bonds by solving the 3x3 Lagrange-multiplier system (Cramer's rule).
__device__ __forceinline__ void settle_velocities(float imA, float imB, float imC, const float3* p, float3* v)
{
    float3 eAB = p[1] - p[0], eBC = p[2] - p[1], eCA = p[0] - p[2];
    eAB = eAB * frsq(dot3(eAB, eAB)); eBC = eBC * frsq(dot3(eBC, eBC)); eCA = eCA * frsq(dot3(eCA, eCA));
    const float dAB = dot3(v[1] - v[0], eAB), dBC = dot3(v[2] - v[1], eBC), dCA = dot3(v[0] - v[2], eCA);
    const float cAB_BC = dot3(eAB, eBC), cAB_CA = dot3(eAB, eCA), cBC_CA = dot3(eBC, eCA);
    const float m00 = imA + imB,        m01 = -cAB_BC * imB,  m02 = -cAB_CA * imA;
    const float m10 = -cAB_BC * imB,    m11 = imB + imC,      m12 = -cBC_CA * imC;
    const float m20 = -cAB_CA * imA,    m21 = -cBC_CA * imC,  m22 = imC + imA;
    const float det = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
    const float idet = frcp(det);
    const float tAB = (dAB * (m11 * m22 - m12 * m21) - m01 * (dBC * m22 - m12 * dCA) + m02 * (dBC * m21 - m11 * dCA)) * idet;
    const float tBC = (m00 * (dBC * m22 - m12 * dCA) - dAB * (m10 * m22 - m12 * m20) + m02 * (m10 * dCA - dBC * m20)) * idet;
    const float tCA = (m00 * (m11 * dCA - dBC * m21) - m01 * (m10 * dCA - dBC * m20) + dAB * (m10 * m21 - m11 * m20)) * idet;
    v[0] = v[0] + (eAB * tAB - eCA * tCA) * imA;
    v[1] = v[1] + (eBC * tBC - eAB * tAB) * imB;
    v[2] = v[2] + (eCA * tCA - eBC * tBC) * imC;
}

// K x K linear solve (K <= 3: the constraints of one X-H star cluster), Cramer's rule, everything in registers
template <int K>
__device__ __forceinline__ void solve_small(const float (&A)[3][3], const float (&b)[3], float (&x)[3])
{
    if (K == 1) {
        x[0] = b[0] * frcp(A[0][0]); x[1] = 0.f; x[2] = 0.f;
    } else if (K == 2) {
        const float idet = frcp(A[0][0] * A[1][1] - A[0][1] * A[1][0]);
        x[0] = (b[0] * A[1][1] - A[0][1] * b[1]) * idet;
        x[1] = (A[0][0] * b[1] - b[0] * A[1][0]) * idet;
        x[2] = 0.f;
    } else {
        const float c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][0] * A[2][2] - A[1][2] * A[2][0], c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
        const float idet = frcp(A[0][0] * c00 - A[0][1] * c01 + A[0][2] * c02);
        x[0] = (b[0] * c00 - A[0][1] * (b[1] * A[2][2] - A[1][2] * b[2]) + A[0][2] * (b[1] * A[2][1] - A[1][1] * b[2])) * idet;
        x[1] = (A[0][0] * (b[1] * A[2][2] - A[1][2] * b[2]) - b[0] * c01 + A[0][2] * (A[1][0] * b[2] - b[1] * A[2][0])) * idet;
        x[2] = (A[0][0] * (A[1][1] * b[2] - b[1] * A[2][1]) - A[0][1] * (A[1][0] * b[2] - b[1] * A[2][0]) + b[0] * c02) * idet;
    }
}

// Position constraints of a star cluster (central atom 0 bonded to atoms 1..NAT-1): p0 old constrained positions, p1
// unconstrained new positions (both relative to the old central atom).  The SHAKE displacements act along the OLD bond
// vectors r0_q with one multiplier per bond; instead of Gauss-Seidel sweeps over the bonds (6-10 sweeps, data dependent,
// and the one wavefront holding the solute's clusters used to set the duration of the whole integrator launch) the K x K
// system  |s_q + sum_p B_qp lam_p r0_p|^2 = d_q^2,  B_qp = 1/m_0 + delta_qp / m_q,  is solved by Newton iterations with the
// exact Jacobian (quadratic convergence: a half step moves bond lengths by < 1 %, so two iterations reach fp32 round-off).
// Round 6: the iteration runs until every bond of the cluster is within the integrator's constraint tolerance (integrators.py:1416-1418:
// addConstrainPositions works to getConstraintTolerance(), a RELATIVE distance error) -- | |r|^2 - d^2 | <= 2 tol d^2 -- with tol no
// smaller than what fp32 lengths can hold (the caller passes max(tol, 2e-7)) and at most SHAKE_MAX_IT updates; before it was a fixed
// three updates whatever the tolerance.  Returns the number of updates made, SHAKE_MAX_IT + 1 when the bound was reached unconverged.
// NAT is a compile-time constant so that every array lives in registers (no scratch).
#define SHAKE_MAX_IT 8
template <int NAT>
__device__ __forceinline__ int shake_positions(const float* im, const float* d, float tol, const float3* p0, float3* p1)
{
    constexpr int K = NAT - 1;
    float3 r0[3], sv[3];
    float lam[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        r0[q] = q < K ? p0[q + 1] - p0[0] : f3(0, 0, 0);
        sv[q] = q < K ? p1[q + 1] - p1[0] : f3(0, 0, 0);
    }
    const float tol2 = 2.f * tol;
    int it = 0;
    for (;; ++it) {
        float3 acc = f3(0, 0, 0);                                   // im0 * sum_p lam_p r0_p (the central atom's share)
#pragma unroll
        for (int p = 0; p < K; ++p) acc = acc + r0[p] * (lam[p] * im[0]);
        float J[3][3], g[3], dl[3];
        bool converged = true;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (q < K) {
                const float3 cur = sv[q] + acc + r0[q] * (lam[q] * im[q + 1]);
                const float d2 = d[q] * d[q];
                g[q] = d2 - dot3(cur, cur);
                converged = converged && fabsf(g[q]) <= tol2 * d2;
#pragma unroll
                for (int p = 0; p < 3; ++p) J[q][p] = p < K ? 2.f * dot3(cur, r0[p]) * (im[0] + (p == q ? im[q + 1] : 0.f)) : 0.f;
            } else {
                g[q] = 0.f;
#pragma unroll
                for (int p = 0; p < 3; ++p) J[q][p] = p == q ? 1.f : 0.f;
            }
        }
        if (converged) break;
        if (it == SHAKE_MAX_IT) { it = SHAKE_MAX_IT + 1; break; }
        solve_small<K>(J, g, dl);
#pragma unroll
        for (int q = 0; q < K; ++q) lam[q] += dl[q];
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
        p1[0] = p1[0] - r0[q] * (lam[q] * im[0]);
        p1[q + 1] = p1[q + 1] + r0[q] * (lam[q] * im[q + 1]);
    }
    return it;
}

// Velocity constraints of a star cluster: the multipliers solve a K x K LINEAR system exactly (no iteration):
//   sum_p (1/m_0 r_q.r_p + delta_qp r_q.r_q / m_q) mu_p = r_q . (v_q - v_0)
template <int NAT>
__device__ __forceinline__ void shake_velocities(const float* im, float /*tol*/, const float3* p, float3* v)
{
    constexpr int K = NAT - 1;
    float3 r[3];
    float A[3][3], b[3], mu[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) r[q] = q < K ? p[q + 1] - p[0] : f3(0, 0, 0);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        b[q] = q < K ? dot3(r[q], v[q + 1] - v[0]) : 0.f;
#pragma unroll
        for (int pp = 0; pp < 3; ++pp)
            A[q][pp] = (q < K && pp < K) ? dot3(r[q], r[pp]) * (im[0] + (pp == q ? im[q + 1] : 0.f)) : (pp == q ? 1.f : 0.f);
    }
    solve_small<K>(A, b, mu);
#pragma unroll
    for (int q = 0; q < K; ++q) {
        v[0] = v[0] + r[q] * (mu[q] * im[0]);
        v[q + 1] = v[q + 1] - r[q] * (mu[q] * im[q + 1]);
    }
}

template <int TYPE, int NAT>
__device__ __forceinline__ void constrain_v(const settle_const& sc, const float* im, float tol, float3* v, const float3* x)
{
    if (TYPE == UNIT_SETTLE) {
        float3 p[3] = { f3(0, 0, 0), x[1] - x[0], x[2] - x[0] };
        settle_velocities(im[0], im[1], im[2], p, v);
    } else if (TYPE == UNIT_SHAKE) {
        float3 p[NAT];
#pragma unroll
        for (int k = 0; k < NAT; ++k) p[k] = x[k] - x[0];
        shake_velocities<NAT>(im, tol, p, v);
    }
}

__device__ __forceinline__ float3 gaussian3(uint64_t seed, uint32_t stream, uint32_t atom, uint32_t replica, uint64_t t)
{
    philox4 w = remd_philox(seed, stream, atom, replica, t);
    const float r1 = fsqrt(-2.f * __logf(remd_u23(w.w[0])));
    const float r2 = fsqrt(-2.f * __logf(remd_u23(w.w[2])));
    float s1, c1, s2, c2;
    __sincosf(6.2831853071795865f * remd_u23(w.w[1]), &s1, &c1);
    __sincosf(6.2831853071795865f * remd_u23(w.w[3]), &s2, &c2);
    (void)s2;
    return f3(r1 * c1, r1 * s1, r2 * c2);
}

// ---- a unit's substeps, on its registers -----------------------------------------------------------------------------------------
// the first half of V: v += h F / m from fixed-point forces F[3][Fs]; constrain_v<TYPE, NAT> completes the substep
template <int NAT>
__device__ __forceinline__ void unit_kick_add(float h, const int* idx, const long long* F, int Fs, unit_regs& S)
{
#pragma unroll
    for (int k = 0; k < NAT; ++k) {
        const float s = h * S.im[k] * FIXED_TO_F32;
        S.v[k].x += s * (float)F[idx[k]];
        S.v[k].y += s * (float)F[Fs + idx[k]];
        S.v[k].z += s * (float)F[2 * Fs + idx[k]];
    }
}

// R: x += h v, position constraints, the position correction put back into v (integrators.py:1417) and -- CONSTRAIN_V -- velocity
// constraints.  The Newton updates of an X-H solve go to S.shake_it.
template <int TYPE, int NAT, bool CONSTRAIN_V = true>
__device__ __forceinline__ void unit_drift(float h, const float* dist, const settle_const& sc, float tol, unit_regs& S)
{
    float3 (&x)[4] = S.x; float3 (&v)[4] = S.v;
    float (&im)[4] = S.im;
    if (TYPE == UNIT_FREE) {
#pragma unroll
        for (int k = 0; k < NAT; ++k) x[k] = x[k] + v[k] * h;
    } else {
        // relative coordinates (origin = old position of atom 0) keep fp32 precision
        float3 p0[NAT], p1[NAT], q[NAT];
#pragma unroll
        for (int k = 0; k < NAT; ++k) {
            p0[k] = x[k] - x[0];
            p1[k] = p0[k] + v[k] * h;
            q[k] = p1[k];
        }
        if (TYPE == UNIT_SETTLE) settle_positions(sc, p0, p1);
        else S.shake_it = max(S.shake_it, shake_positions<NAT>(im, dist, tol, p0, p1));
        const float ih = frcp(h);
        const float3 org = x[0];
#pragma unroll
        for (int k = 0; k < NAT; ++k) {
            v[k] = v[k] + (p1[k] - q[k]) * ih;          // integrators.py:1417
            x[k] = org + p1[k];
        }
        if (CONSTRAIN_V) constrain_v<TYPE, NAT>(sc, im, tol, v, x);
    }
}

// O: v = a v + b sqrt(kT / m) xi with xi from the Philox stream of (atom, noise id rg, counter cnt), then velocity constraints
template <int TYPE, int NAT>
__device__ __forceinline__ void unit_ou(float a, float b, float kT, uint64_t cnt, uint64_t seed, uint32_t rg, const int* idx,
                                        const settle_const& sc, float tol, unit_regs& S)
{
    float3 (&v)[4] = S.v;
#pragma unroll
    for (int k = 0; k < NAT; ++k) {
        const float3 xi = gaussian3(seed, REMD_STREAM_OU, (uint32_t)idx[k], rg, cnt);
        const float sig = b * fsqrt(kT * S.im[k]);
        v[k].x = a * v[k].x + sig * xi.x;
        v[k].y = a * v[k].y + sig * xi.y;
        v[k].z = a * v[k].z + sig * xi.z;
    }
    constrain_v<TYPE, NAT>(sc, S.im, tol, v, S.x);
}

// ---- choosing a unit's instance --------------------------------------------------------------------------------------------------
// The unit's <TYPE, NAT> instance: RUN(TYPE, NAT) is expanded for the one the unit is.  NAT is a compile-time constant in everything
// above so that every array lives in registers.  SETTLE has 3 atoms, SHAKE 2 to 4, FREE 1 or exactly 4 (remd_build_constraints).
// (A macro: through a generic callable the chain and FIRE kernels are compiled to other instruction streams.)
#define UNIT_LADDER(type, a4, RUN) do { \
    if ((type) == UNIT_SETTLE) RUN(UNIT_SETTLE, 3); \
    else if ((type) == UNIT_FREE) { if ((a4).y < 0) RUN(UNIT_FREE, 1); else RUN(UNIT_FREE, 4); } \
    else if ((a4).z < 0) RUN(UNIT_SHAKE, 2); \
    else if ((a4).w < 0) RUN(UNIT_SHAKE, 3); \
    else RUN(UNIT_SHAKE, 4); } while (0)

// ---- the handle's unit tables (remd_build_constraints) ---------------------------------------------------------------------------
struct unit_tables {
    int n_units = 0;
    dev_array<int4> d_atoms; dev_array<unsigned char> d_type; dev_array<float> d_dist;
    settle_const sc{};
};

// GBSA implicit solvent (gfx950): OpenMM's GBSAOBCForce -- OBC2 Born radii + ACE surface term -- in the form the reference's alchemical
// factory gives it (alchemy/alchemy.py:2144-2225, _alchemically_modify_GBSAOBCForce: a CustomGBForce whose expression strings are the
// definition followed here; include/remd_hip.h remd_set_gbsa states them).  NoCutoff systems only (the implicit-solvent test systems of
// the reference: tens to a few thousand atoms).  f64 restatement: oracle/gbsa.py, pinned to the reference's strings.
//
// Three launches per force evaluation, each the direct all-pairs sum of nocutoff.hip (workgroup = 64 atoms i of one replica, 16 wavefronts that
// split the partners j staged through LDS, every pair from both sides so that nothing is reduced across atoms):
//   gb_born_kernel    I_i = sum_j s_j H(r_ij; or_i, sr_j)  ->  B_i and dB_i/dI_i
//   gb_pair_kernel    self + surface + pair energies, the pair term's direct force on i, dE/dB_i  ->  c_i = dE/dB_i dB_i/dI_i
//   gb_chain_kernel   the force through the Born radii: sum_j [c_i s_j H'(r; or_i, sr_j) + c_j s_i H'(r; or_j, sr_i)] (x_j - x_i) / r
// s = lambda_electrostatics of the replica's state on the alchemical particles, 1 elsewhere.
//
// The model constants (include/remd_hip_gb.h remd_set_gb_model: offset, the tanh coefficients, k_e, the surface term) are kernel
// arguments; OBC2 without a cutoff unless a model is set.  The three kernels are templated on the cutoff mode: GB_CUT_NONE (every pair)
// or GB_CUT_PERIODIC (OpenMM's CustomGBForce CutoffPeriodic: the minimum image under the replica's own box, a pair computed value and
// a pair energy term see only pairs with r < cutoff, no shift, no switch; the single-particle terms are unchanged).
#include "remd_internal.h"
#include "../../include/remd_hip_gb.h"
#include "listed_terms.h"
#include <cmath>
#include <algorithm>

#define GB_CUT_NONE 0
#define GB_CUT_PERIODIC 2

// the model as the kernels take it; the derivative of the tanh argument alpha psi - beta psi^2 + gamma psi^3 is (d0 - d1 psi + d2 psi^2),
// (d0, d1, d2) = (alpha, 2 beta, 3 gamma) computed in double and rounded to float once (OBC2: 1, 1.6f, 14.55f)
struct gb_consts {
    float offset, alpha, beta, gamma, d0, d1, d2, ke, sa, probe, cut2;
};

struct gbsa_tables {
    int N = 0, n_tile = 0;
    float tau = 0.f; int sasa = 1;
    bool any_alch = false;
    dev_array<float4> d_par;               // [Npad] q, R, scale, alchemical
    dev_array<float2> d_born;              // [R][Npad] B, dB/dI
    dev_array<float> d_c;                  // [R][Npad] dE/dB dB/dI
    dev_array<float> d_lam; std::vector<float> lam_host;      // [R] lambda_electrostatics of each replica's state
    dev_array<float> d_state_lam; std::vector<float> state_lam_host;   // [K] of every state (u_kl columns)
    // a deep copy of the descriptor of remd_set_gbsa: the blocks of a phased propagation (api.hip) are set up from it
    remd_gbsa_desc store{}; std::vector<double> st_charge, st_radius, st_scale; std::vector<int32_t> st_alch;
    dev_array<double> d_epart; dev_array<double> d_col;     // [R][n_tile], [R]
    remd_gb_model_desc model{}; gb_consts k{}; int method = GB_CUT_NONE;     // remd_set_gb_model (OBC2, NoCutoff until then)
};
void remd_table_deleter::operator()(gbsa_tables* t) const { delete t; }


// H(r; or1, sr2) of the computed value I and its derivative in r (alchemy.py:2195-2201; the step functions are constants under the derivative)
__device__ __forceinline__ void gb_H(float r, float or1, float sr2, float& H, float& dH)
{
    H = 0.f; dH = 0.f;
    if (r + sr2 - or1 < 0.f) return;
    const float U = r + sr2, D = fabsf(r - sr2);
    const bool moving = D > or1;
    const float L = moving ? D : or1, dL = moving ? (r > sr2 ? 1.f : -1.f) : 0.f;
    const bool inside = sr2 - r - or1 >= 0.f;
    const float iL = 1.f / L, iU = 1.f / U, ir = 1.f / r;
    const float C = inside ? 2.f * (1.f / or1 - iL) : 0.f, dC = inside ? 2.f * dL * iL * iL : 0.f;
    const float a = iU * iU - iL * iL, w = r - sr2 * sr2 * ir, lg = logf(L * iU);
    H = 0.5f * (iL - iU + 0.25f * w * a + 0.5f * lg * ir + C);
    dH = 0.5f * (-dL * iL * iL + iU * iU + 0.25f * (1.f + sr2 * sr2 * ir * ir) * a + 0.25f * w * (-2.f * iU * iU * iU + 2.f * dL * iL * iL * iL)
                 + 0.5f * ((dL * iL - iU) * ir - lg * ir * ir) + dC);
}

// the vector from i to j and r^2: as it stands (GB_CUT_NONE) or the minimum image under the box L (GB_CUT_PERIODIC)
template <int CUT>
__device__ __forceinline__ void gb_vec(const float4& xi, const float4& xj, const float4& L, float& dx, float& dy, float& dz, float& r2)
{
    dx = xj.x - xi.x; dy = xj.y - xi.y; dz = xj.z - xi.z;
    if (CUT == GB_CUT_PERIODIC) { dx -= L.x * rintf(dx / L.x); dy -= L.y * rintf(dy / L.y); dz -= L.z * rintf(dz / L.z); }
    r2 = dx * dx + dy * dy + dz * dz;
}

template <int CUT>
__device__ __forceinline__ float4 gb_box(const float* __restrict__ box, int r)
{
    return CUT == GB_CUT_PERIODIC ? reinterpret_cast<const float4*>(box)[r] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// tanh(alpha psi - beta psi^2 + gamma psi^3) -> B and dB/dI.  The first term is fma(alpha or_i, I, -beta psi^2): with alpha = 1 that is
// the contraction the compiler made of OBC2's psi - 0.8f psi^2 + 4.85f psi^3 when the constants were literals (same arithmetic)
__device__ __forceinline__ float2 gb_born_radius(float I, float or_i, float R, const gb_consts& k)
{
    const float psi = I * or_i;
    float arg;
    {
#pragma clang fp contract(off)
        arg = fmaf(k.alpha * or_i, I, -(k.beta * psi * psi)) + k.gamma * psi * psi * psi;
    }
    const float th = tanhf(arg);
    const float B = 1.f / (1.f / or_i - th / R);
    return make_float2(B, B * B * (1.f - th * th) * (k.d0 - k.d1 * psi + k.d2 * psi * psi) * or_i / R);
}

// The three kernels: workgroup = (64 atoms i, replica) of GB_WAVES wavefronts; lane = atom i, wavefront w takes the partners
// j = w (mod GB_WAVES) of every block of GB_BLOCK atoms staged in LDS, an atom's partial sums are added in wavefront order (fixed order).
// (One wavefront per tile summing N dependent partner terms -- each with a logarithm and a handful of divisions -- was 10 + 7 + 17 us for
// 22 atoms: profiles/r06_43.)
#define GB_WAVES 16
#define GB_BLOCK (64 * GB_WAVES)
template <int CUT>
__global__ __launch_bounds__(GB_BLOCK)
void gb_born_kernel(int N, int Npad, gb_consts kc, const float4* __restrict__ par, const float* __restrict__ lam, int lam_stride, const float4* __restrict__ pos,
                    const float* __restrict__ box, float2* __restrict__ born)
{
    __shared__ float4 s_x[GB_BLOCK];       // x, y, z, sr_j
    __shared__ float s_s[GB_BLOCK];        // s_j
    __shared__ float s_part[GB_WAVES][64];
    const int r = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * 64 + lane;
    const float4* P = pos + (size_t)r * Npad;
    const float l = lam[(size_t)r * lam_stride];         // (stride 0: every replica at one state's lambda, a u_kl column)
    const bool live = i < N;
    const float4 xi = live ? P[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 pi = live ? par[i] : make_float4(0.f, 1.f, 0.f, 0.f);
    const float4 L = gb_box<CUT>(box, r);
    const float or_i = pi.y - kc.offset;
    float I = 0.f;
    for (int j0 = 0; j0 < N; j0 += GB_BLOCK) {
        __syncthreads();
        if (j0 + (int)threadIdx.x < N) {
            const float4 xj = P[j0 + threadIdx.x], pj = par[j0 + threadIdx.x];
            s_x[threadIdx.x] = make_float4(xj.x, xj.y, xj.z, pj.z * (pj.y - kc.offset));
            s_s[threadIdx.x] = pj.w != 0.f ? l : 1.f;
        }
        __syncthreads();
        if (!live) continue;
        const int jn = min(GB_BLOCK, N - j0);
        for (int k = w; k < jn; k += GB_WAVES) {
            if (j0 + k == i) continue;
            const float4 xj = s_x[k];
            float dx, dy, dz, r2;
            gb_vec<CUT>(xi, xj, L, dx, dy, dz, r2);
            if (CUT == GB_CUT_PERIODIC && !(r2 < kc.cut2)) continue;
            float H, dH;
            gb_H(sqrtf(r2), or_i, xj.w, H, dH);
            I += s_s[k] * H;
        }
    }
    s_part[w][lane] = I;
    __syncthreads();
    if (w == 0 && live) {
        I = 0.f;
        for (int q = 0; q < GB_WAVES; ++q) I += s_part[q][lane];
        born[(size_t)r * Npad + i] = gb_born_radius(I, or_i, pi.y, kc);
    }
}

template <int CUT, bool ENERGY, bool FORCE>
__global__ __launch_bounds__(GB_BLOCK)
void gb_pair_kernel(int N, int Npad, gb_consts kc, float tau, int sasa, const float4* __restrict__ par, const float* __restrict__ lam, int lam_stride, const float4* __restrict__ pos,
                    const float* __restrict__ box, const float2* __restrict__ born, float* __restrict__ cfac, long long* __restrict__ force, double* __restrict__ epart, int n_tile)
{
    __shared__ float4 s_x[GB_BLOCK];       // x, y, z, B_j
    __shared__ float s_q[GB_BLOCK];        // s_j q_j
    __shared__ float4 s_part[GB_WAVES][64];
    __shared__ double s_e[GB_WAVES];
    const int r = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * 64 + lane;
    const float4* P = pos + (size_t)r * Npad;
    const float2* BR = born + (size_t)r * Npad;
    const float l = lam[(size_t)r * lam_stride];         // (stride 0: every replica at one state's lambda, a u_kl column)
    const bool live = i < N;
    const float4 xi = live ? P[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 pi = live ? par[i] : make_float4(0.f, 1.f, 0.f, 0.f);
    const float2 bi = live ? BR[i] : make_float2(1.f, 0.f);
    const float4 L = gb_box<CUT>(box, r);
    const float si = pi.w != 0.f ? l : 1.f, Qi = si * pi.x;
    float fx = 0.f, fy = 0.f, fz = 0.f, dEdB = 0.f;
    double e = 0.0;
    if (live && w == 0) {
        const float self = 0.5f * kc.ke * tau * si * pi.x * pi.x / bi.x;
        dEdB += self / bi.x;
        if (ENERGY) e -= (double)self;
        if (sasa) {
            const float rb = pi.y / bi.x, rb2 = rb * rb, rb6 = rb2 * rb2 * rb2, pre = si * kc.sa * (pi.y + kc.probe) * (pi.y + kc.probe);
            dEdB -= 6.f * pre * rb6 / bi.x;
            if (ENERGY) e += (double)(pre * rb6);
        }
    }
    for (int j0 = 0; j0 < N; j0 += GB_BLOCK) {
        __syncthreads();
        if (j0 + (int)threadIdx.x < N) {
            const float4 xj = P[j0 + threadIdx.x], pj = par[j0 + threadIdx.x];
            s_x[threadIdx.x] = make_float4(xj.x, xj.y, xj.z, BR[j0 + threadIdx.x].x);
            s_q[threadIdx.x] = (pj.w != 0.f ? l : 1.f) * pj.x;
        }
        __syncthreads();
        if (!live) continue;
        const int jn = min(GB_BLOCK, N - j0);
        for (int k = w; k < jn; k += GB_WAVES) {
            if (j0 + k == i) continue;
            const float4 xj = s_x[k];
            float dx, dy, dz, r2;
            gb_vec<CUT>(xi, xj, L, dx, dy, dz, r2);
            if (CUT == GB_CUT_PERIODIC && !(r2 < kc.cut2)) continue;
            const float D = bi.x * xj.w, ex = __expf(-r2 / (4.f * D)), f2 = r2 + D * ex, inv_f = rsqrtf(f2);
            const float QQ = kc.ke * tau * Qi * s_q[k];
            const float dEdf = QQ / f2;
            dEdB += dEdf * ex * (1.f + r2 / (4.f * D)) * 0.5f * inv_f * xj.w;
            if (FORCE) { const float gr = dEdf * (1.f - 0.25f * ex) * inv_f; fx += gr * dx; fy += gr * dy; fz += gr * dz; }
            if (ENERGY) e -= 0.5 * (double)(QQ * inv_f);
        }
    }
    if (FORCE) {
        s_part[w][lane] = make_float4(fx, fy, fz, dEdB);
        __syncthreads();
        if (w == 0 && live) {
            fx = 0.f; fy = 0.f; fz = 0.f; dEdB = 0.f;
            for (int q = 0; q < GB_WAVES; ++q) { const float4 t = s_part[q][lane]; fx += t.x; fy += t.y; fz += t.z; dEdB += t.w; }
            cfac[(size_t)r * Npad + i] = dEdB * bi.y;
            add_force(force + (size_t)r * 3 * Npad, Npad, i, fx, fy, fz);
        }
    }
    if (ENERGY) {
        for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
        if (lane == 0) s_e[w] = e;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int q = 0; q < GB_WAVES; ++q) tot += s_e[q];
            epart[(size_t)r * n_tile + blockIdx.x] = tot;
        }
    }
}

template <int CUT>
__global__ __launch_bounds__(GB_BLOCK)
void gb_chain_kernel(int N, int Npad, gb_consts kc, const float4* __restrict__ par, const float* __restrict__ lam, int lam_stride, const float4* __restrict__ pos,
                     const float* __restrict__ box, const float* __restrict__ cfac, long long* __restrict__ force)
{
    __shared__ float4 s_x[GB_BLOCK];       // x, y, z, or_j
    __shared__ float4 s_p[GB_BLOCK];       // sr_j, s_j, c_j, -
    __shared__ float4 s_part[GB_WAVES][64];
    const int r = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * 64 + lane;
    const float4* P = pos + (size_t)r * Npad;
    const float* Cf = cfac + (size_t)r * Npad;
    const float l = lam[(size_t)r * lam_stride];         // (stride 0: every replica at one state's lambda, a u_kl column)
    const bool live = i < N;
    const float4 xi = live ? P[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 pi = live ? par[i] : make_float4(0.f, 1.f, 0.f, 0.f);
    const float4 L = gb_box<CUT>(box, r);
    const float or_i = pi.y - kc.offset, sr_i = pi.z * or_i, si = pi.w != 0.f ? l : 1.f, ci = live ? Cf[i] : 0.f;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    for (int j0 = 0; j0 < N; j0 += GB_BLOCK) {
        __syncthreads();
        if (j0 + (int)threadIdx.x < N) {
            const float4 xj = P[j0 + threadIdx.x], pj = par[j0 + threadIdx.x];
            const float orj = pj.y - kc.offset;
            s_x[threadIdx.x] = make_float4(xj.x, xj.y, xj.z, orj);
            s_p[threadIdx.x] = make_float4(pj.z * orj, pj.w != 0.f ? l : 1.f, Cf[j0 + threadIdx.x], 0.f);
        }
        __syncthreads();
        if (!live) continue;
        const int jn = min(GB_BLOCK, N - j0);
        for (int k = w; k < jn; k += GB_WAVES) {
            if (j0 + k == i) continue;
            const float4 xj = s_x[k], pj = s_p[k];
            float dx, dy, dz, r2;
            gb_vec<CUT>(xi, xj, L, dx, dy, dz, r2);
            if (CUT == GB_CUT_PERIODIC && !(r2 < kc.cut2)) continue;     // (out of range: neither I_i nor I_j holds the pair)
            const float rr = sqrtf(r2);
            float H, dH1, dH2;
            gb_H(rr, or_i, pj.x, H, dH1);              // B_i depends on j
            gb_H(rr, xj.w, sr_i, H, dH2);              // B_j depends on i
            const float gr = (ci * pj.y * dH1 + pj.z * si * dH2) / rr;
            fx += gr * dx; fy += gr * dy; fz += gr * dz;
        }
    }
    s_part[w][lane] = make_float4(fx, fy, fz, 0.f);
    __syncthreads();
    if (w == 0 && live) {
        fx = 0.f; fy = 0.f; fz = 0.f;
        for (int q = 0; q < GB_WAVES; ++q) { const float4 t = s_part[q][lane]; fx += t.x; fy += t.y; fz += t.z; }
        add_force(force + (size_t)r * 3 * Npad, Npad, i, fx, fy, fz);
    }
}

__global__ __launch_bounds__(64)
void gb_reduce_kernel(int n, const double* __restrict__ part, double* __restrict__ out, int stride, int offset, int add)
{
    const int r = blockIdx.x;
    double e = 0.0;
    for (int t = threadIdx.x; t < n; t += 64) e += part[(size_t)r * n + t];
    for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
    if (threadIdx.x == 0) { double* o = out + (size_t)r * stride + offset; *o = add ? *o + e : e; }
}

// Systems of up to 64 atoms (the implicit-solvent test systems the reference's sampler tests run on: AlanineDipeptideImplicit, 22 atoms):
// the three kernels above are one wavefront per replica summing N dependent partner terms each -- 10 + 7 + 17 us for 22 atoms
// (profiles/r06_43).  Here ONE launch, a workgroup of 16 wavefronts per replica: lane = atom i, wavefront w takes the partners
// j = w, w + 16, w + 32, w + 48, the 16 partial sums of an atom go through LDS and are added in wavefront order (a fixed order: the
// result does not depend on scheduling); Born radii, dE/dB and c_i stay in LDS between the three passes.
template <bool ENERGY, bool FORCE>
__global__ __launch_bounds__(1024)
void gb_small_kernel(int N, int Npad, gb_consts kc, float tau, int sasa, const float4* __restrict__ par, const float* __restrict__ lam, int lam_stride, const float4* __restrict__ pos,
                     long long* __restrict__ force, double* __restrict__ out, int out_stride, int out_offset, int add)
{
    __shared__ float4 s_x[64];             // x, y, z, or_j
    __shared__ float4 s_p[64];             // q_j, R_j, sr_j, s_j
    __shared__ float2 s_born[64];          // B, dB/dI
    __shared__ float s_c[64];              // dE/dB dB/dI
    __shared__ float4 s_part[16][64];
    __shared__ double s_e[16];
    const int r = blockIdx.x, i = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float4* P = pos + (size_t)r * Npad;
    const float l = lam[(size_t)r * lam_stride];         // (stride 0: every replica at one state's lambda, a u_kl column)
    if (w == 0) {
        const float4 x = i < N ? P[i] : make_float4(0.f, 0.f, 0.f, 0.f), p = i < N ? par[i] : make_float4(0.f, 1.f, 0.f, 0.f);
        const float orj = p.y - kc.offset;
        s_x[i] = make_float4(x.x, x.y, x.z, orj);
        s_p[i] = make_float4(p.x, p.y, p.z * orj, p.w != 0.f ? l : 1.f);
    }
    __syncthreads();
    const bool live = i < N;
    const float4 xi = s_x[i], pi = s_p[i];
    const float or_i = xi.w, sr_i = pi.z, si = pi.w;
    // pass 1: I_i -> B_i, dB_i/dI_i
    {
        float I = 0.f;
        if (live)
            for (int j = w; j < N; j += 16) {
                if (j == i) continue;
                const float4 xj = s_x[j], pj = s_p[j];
                const float dx = xj.x - xi.x, dy = xj.y - xi.y, dz = xj.z - xi.z;
                float H, dH;
                gb_H(sqrtf(dx * dx + dy * dy + dz * dz), or_i, pj.z, H, dH);
                I += pj.w * H;
            }
        s_part[w][i].x = I;
    }
    __syncthreads();
    if (w == 0 && live) {
        float I = 0.f;
        for (int q = 0; q < 16; ++q) I += s_part[q][i].x;
        s_born[i] = gb_born_radius(I, or_i, pi.y, kc);
    }
    __syncthreads();
    // pass 2: self + surface + pair energies, the pair term's direct force on i, dE/dB_i
    float fx = 0.f, fy = 0.f, fz = 0.f;
    {
        const float2 bi = live ? s_born[i] : make_float2(1.f, 0.f);
        const float Qi = si * pi.x;
        float dEdB = 0.f;
        double e = 0.0;
        if (live && w == 0) {
            const float self = 0.5f * kc.ke * tau * si * pi.x * pi.x / bi.x;
            dEdB += self / bi.x;
            if (ENERGY) e -= (double)self;
            if (sasa) {
                const float rb = pi.y / bi.x, rb2 = rb * rb, rb6 = rb2 * rb2 * rb2, pre = si * kc.sa * (pi.y + kc.probe) * (pi.y + kc.probe);
                dEdB -= 6.f * pre * rb6 / bi.x;
                if (ENERGY) e += (double)(pre * rb6);
            }
        }
        if (live)
            for (int j = w; j < N; j += 16) {
                if (j == i) continue;
                const float4 xj = s_x[j], pj = s_p[j];
                const float Bj = s_born[j].x;
                const float dx = xj.x - xi.x, dy = xj.y - xi.y, dz = xj.z - xi.z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                const float D = bi.x * Bj, ex = __expf(-r2 / (4.f * D)), f2 = r2 + D * ex, inv_f = rsqrtf(f2);
                const float QQ = kc.ke * tau * Qi * (pj.w * pj.x);
                const float dEdf = QQ / f2;
                dEdB += dEdf * ex * (1.f + r2 / (4.f * D)) * 0.5f * inv_f * Bj;
                if (FORCE) { const float gr = dEdf * (1.f - 0.25f * ex) * inv_f; fx += gr * dx; fy += gr * dy; fz += gr * dz; }
                if (ENERGY) e -= 0.5 * (double)(QQ * inv_f);
            }
        s_part[w][i] = make_float4(fx, fy, fz, dEdB);
        if (ENERGY) {
            for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
            if (i == 0) s_e[w] = e;
        }
        __syncthreads();
        if (w == 0) {
            fx = 0.f; fy = 0.f; fz = 0.f; dEdB = 0.f;
            for (int q = 0; q < 16; ++q) { const float4 t = s_part[q][i]; fx += t.x; fy += t.y; fz += t.z; dEdB += t.w; }
            s_c[i] = dEdB * bi.y;
            if (ENERGY && i == 0) {
                double tot = 0.0;
                for (int q = 0; q < 16; ++q) tot += s_e[q];
                double* o = out + (size_t)r * out_stride + out_offset;
                *o = add ? *o + tot : tot;
            }
        }
        __syncthreads();
    }
    if (!FORCE) return;
    // pass 3: the force through the Born radii
    {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (live) {
            const float ci = s_c[i];
            for (int j = w; j < N; j += 16) {
                if (j == i) continue;
                const float4 xj = s_x[j], pj = s_p[j];
                const float dx = xj.x - xi.x, dy = xj.y - xi.y, dz = xj.z - xi.z;
                const float rr = sqrtf(dx * dx + dy * dy + dz * dz);
                float H, dH1, dH2;
                gb_H(rr, or_i, pj.z, H, dH1);              // B_i depends on j
                gb_H(rr, xj.w, sr_i, H, dH2);              // B_j depends on i
                const float gr = (ci * pj.w * dH1 + s_c[j] * si * dH2) / rr;
                gx += gr * dx; gy += gr * dy; gz += gr * dz;
            }
        }
        s_part[w][i] = make_float4(gx, gy, gz, 0.f);
        __syncthreads();
        if (w == 0 && live) {
            for (int q = 0; q < 16; ++q) { const float4 t = s_part[q][i]; fx += t.x; fy += t.y; fz += t.z; }
            add_force(force + (size_t)r * 3 * Npad, Npad, i, fx, fy, fz);
        }
    }
}

// OBC2 without a cutoff: the model remd_set_gbsa starts from (the constants of the factory's strings, alchemy.py:2192-2210)
static remd_gb_model_desc gb_default_model()
{
    remd_gb_model_desc m{};
    m.offset = 0.009; m.alpha = 1.0; m.beta = 0.8; m.gamma = 4.85; m.ke = 138.935485; m.surface = 28.3919551; m.probe = 0.14;
    m.method = REMD_GB_NO_CUTOFF; m.cutoff = 0.0;
    return m;
}

static void gb_take_model(gbsa_tables& t, const remd_gb_model_desc& m)
{
    t.model = m;
    t.method = m.method == REMD_GB_CUTOFF_PERIODIC ? GB_CUT_PERIODIC : GB_CUT_NONE;
    t.k.offset = (float)m.offset; t.k.alpha = (float)m.alpha; t.k.beta = (float)m.beta; t.k.gamma = (float)m.gamma;
    t.k.d0 = (float)m.alpha; t.k.d1 = (float)(2.0 * m.beta); t.k.d2 = (float)(3.0 * m.gamma);
    t.k.ke = (float)m.ke; t.k.sa = (float)m.surface; t.k.probe = (float)m.probe;
    t.k.cut2 = t.method == GB_CUT_PERIODIC ? (float)(m.cutoff * m.cutoff) : 0.f;
}

int remd_set_gbsa(remd_handle h, const remd_gbsa_desc* d)
{
    if (!h) return remd_fail(h, -1, "remd_set_gbsa: NULL handle");
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    h->gb.reset(); h->gbsa = 0;
    h->config_version++;
    h->forces_valid = false;
    if (!d) return 0;
    // a periodic system takes GB only with a CutoffPeriodic model (remd_set_gb_model, checked at every evaluation)
    if (!h->has_system || !(h->nocutoff || h->nb_method != REMD_NB_NONE))
        return remd_fail(h, -3, "remd_set_gbsa: GBSA needs a system with a NoCutoff NonbondedForce (call remd_set_system first)");
    if (d->n_atoms != h->N || !d->charge || !d->radius || !d->scale || !(d->solute_dielectric > 0) || !(d->solvent_dielectric > 0)) return remd_fail(h, -1, "remd_set_gbsa: bad arguments");
    remd_table<gbsa_tables> tab(new gbsa_tables());
    gbsa_tables& t = *tab;
    t.N = h->N; t.n_tile = (h->N + 63) / 64;
    t.tau = (float)(1.0 / d->solute_dielectric - 1.0 / d->solvent_dielectric);
    t.sasa = d->surface_area ? 1 : 0;
    gb_take_model(t, gb_default_model());
    std::vector<float4> par(h->Npad, make_float4(0.f, 1.f, 0.f, 0.f));
    for (int i = 0; i < h->N; ++i) {
        if (!(d->radius[i] > 0.009)) return remd_fail(h, -1, "remd_set_gbsa: radii must exceed the offset 0.009 nm");
        const bool a = d->alchemical && d->alchemical[i];
        t.any_alch |= a;
        par[i] = make_float4((float)d->charge[i], (float)d->radius[i], (float)d->scale[i], a ? 1.f : 0.f);
    }
    REMD_TRY(t.d_par.upload(h, par));
    h->gb = std::move(tab);
    h->gbsa = 1;
    if (!h->parent) {
        t.store = *d;
        t.st_charge.assign(d->charge, d->charge + h->N); t.st_radius.assign(d->radius, d->radius + h->N); t.st_scale.assign(d->scale, d->scale + h->N);
        t.store.charge = t.st_charge.data(); t.store.radius = t.st_radius.data(); t.store.scale = t.st_scale.data();
        if (d->alchemical) { t.st_alch.assign(d->alchemical, d->alchemical + h->N); t.store.alchemical = t.st_alch.data(); } else { t.st_alch.clear(); t.store.alchemical = nullptr; }
    }
    return 0;
}

int remd_set_gb_model(remd_handle h, const remd_gb_model_desc* m)
{
    if (!h) return remd_fail(h, -1, "remd_set_gb_model: NULL handle");
    gbsa_tables* tp = h->gb.get();
    if (!tp || !h->gbsa) return remd_fail(h, -2, "remd_set_gb_model: no GBSA on this handle (call remd_set_gbsa first)");
    const remd_gb_model_desc mm = m ? *m : gb_default_model();
    if (!(mm.offset >= 0.0) || !std::isfinite(mm.alpha) || !std::isfinite(mm.beta) || !std::isfinite(mm.gamma) || !(mm.ke > 0.0) ||
        !std::isfinite(mm.surface) || !std::isfinite(mm.probe))
        return remd_fail(h, -1, "remd_set_gb_model: bad model constants");
    if (mm.method != REMD_GB_NO_CUTOFF && mm.method != REMD_GB_CUTOFF_PERIODIC)
        return remd_fail(h, -1, "remd_set_gb_model: method must be REMD_GB_NO_CUTOFF or REMD_GB_CUTOFF_PERIODIC");
    if (mm.method == REMD_GB_CUTOFF_PERIODIC && (h->nocutoff || h->nb_method == REMD_NB_NONE || !(mm.cutoff > 0.0)))
        return remd_fail(h, -1, "remd_set_gb_model: a CutoffPeriodic model needs a periodic system and a cutoff > 0");
    if (mm.method == REMD_GB_NO_CUTOFF && !h->nocutoff)
        return remd_fail(h, -1, "remd_set_gb_model: a NoCutoff model needs a NoCutoff system");
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    for (int i = 0; i < tp->N; ++i)
        if (!(tp->st_radius.empty() || tp->st_radius[i] > mm.offset)) return remd_fail(h, -1, "remd_set_gb_model: radii must exceed the offset");
    gb_take_model(*tp, mm);
    h->config_version++;
    h->forces_valid = false;
    return 0;
}

// the implicit solvent of `parent` on one of its blocks (api.hip phase_children)
int remd_gbsa_clone(remd_ctx* parent, remd_ctx* child)
{
    const gbsa_tables* t = parent->gb.get();
    if (!t || !parent->gbsa) return 0;
    int rc = remd_set_gbsa(child, &t->store);
    if (!rc) rc = remd_set_gb_model(child, &t->model);
    if (rc) return remd_fail(parent, rc, std::string("phases: ") + child->err);
    return 0;
}

static int gb_buffers(remd_ctx* h, gbsa_tables& t)
{
    if (t.d_col.size() == (size_t)h->R) return 0;
    REMD_TRY(t.d_born.alloc(h, (size_t)h->R * h->Npad));
    REMD_TRY(t.d_c.alloc(h, (size_t)h->R * h->Npad));
    REMD_TRY(t.d_lam.alloc(h, h->R));
    REMD_TRY(t.d_epart.alloc(h, (size_t)h->R * t.n_tile));
    REMD_TRY(t.d_col.alloc(h, h->R));
    t.lam_host.clear();
    return 0;
}

static int gb_set_lambdas(remd_ctx* h, gbsa_tables& t, const std::vector<float>& lam)
{
    if (lam == t.lam_host) return 0;
    REMD_CHECK(h, hipMemcpyAsync(t.d_lam, lam.data(), sizeof(float) * lam.size(), hipMemcpyHostToDevice, h->stream));
    REMD_CHECK(h, hipStreamSynchronize(h->stream));
    t.lam_host = lam;
    return 0;
}

// lambda_electrostatics of state k for the alchemical particles: region 1 of the general regions (the factory's GBSA knows one region), else the state's own
static float gb_state_lambda(remd_ctx* h, int k)
{
    double le = 1.0;
    if (h->n_regions > 0) { if (remd_regions_state_le(h, k, 0, &le)) le = 1.0; }
    else if (!h->lam_e.empty() && k >= 0 && k < (int)h->lam_e.size()) le = h->lam_e[k];
    return (float)le;
}

// the one-launch kernel for up to 64 atoms without a cutoff (REMD_GB_SMALL=0: the three launches, for the A/B and the tests of the large path)
static bool gb_small(const remd_ctx* h, const gbsa_tables& t)
{
    return t.method == GB_CUT_NONE && t.N <= 64 && h->sw.gb_small;
}

// the three launches of one evaluation: I -> B, energies + dE/dB, the chain rule through B (no chain without forces)
template <int CUT>
static void gb_launch(remd_ctx* h, const gbsa_tables& t, const float* lam, int lam_stride, bool energy, bool force, long long* d_force)
{
    const dim3 grid(t.n_tile, h->R);
    hipLaunchKernelGGL(gb_born_kernel<CUT>, grid, dim3(GB_BLOCK), 0, h->stream, t.N, h->Npad, t.k, t.d_par, lam, lam_stride, h->d_pos, h->d_box, t.d_born);
    if (energy && force)
        hipLaunchKernelGGL((gb_pair_kernel<CUT, true, true>), grid, dim3(GB_BLOCK), 0, h->stream, t.N, h->Npad, t.k, t.tau, t.sasa, t.d_par, lam, lam_stride, h->d_pos, h->d_box,
                           t.d_born, t.d_c, d_force, t.d_epart, t.n_tile);
    else if (force)
        hipLaunchKernelGGL((gb_pair_kernel<CUT, false, true>), grid, dim3(GB_BLOCK), 0, h->stream, t.N, h->Npad, t.k, t.tau, t.sasa, t.d_par, lam, lam_stride, h->d_pos, h->d_box,
                           t.d_born, t.d_c, d_force, (double*)nullptr, t.n_tile);
    else
        hipLaunchKernelGGL((gb_pair_kernel<CUT, true, false>), grid, dim3(GB_BLOCK), 0, h->stream, t.N, h->Npad, t.k, t.tau, t.sasa, t.d_par, lam, lam_stride, h->d_pos, h->d_box,
                           t.d_born, t.d_c, (long long*)nullptr, t.d_epart, t.n_tile);
    if (force)
        hipLaunchKernelGGL(gb_chain_kernel<CUT>, grid, dim3(GB_BLOCK), 0, h->stream, t.N, h->Npad, t.k, t.d_par, lam, lam_stride, h->d_pos, h->d_box, t.d_c, d_force);
}

static int gb_check_method(remd_ctx* h, const gbsa_tables& t)
{
    if (t.method == GB_CUT_NONE && !h->nocutoff)
        return remd_fail(h, -3, "GBSA on a periodic system needs a CutoffPeriodic model (remd_set_gb_model)");
    return 0;
}

// ep_slot: the energy slot of a NoCutoff system (written); a periodic system's GB energy is ADDED to the slot before the last, the one of
// the custom forces of general alchemical regions -- written earlier on this stream, zero without them -- so that no slot of the
// cutoff pair kernels is touched
int remd_gbsa_forces(remd_ctx* h, bool with_energy, int ep_slot)
{
    gbsa_tables* tp = h->gb.get();
    if (!tp) return remd_fail(h, -2, "GBSA: no tables on this handle");
    gbsa_tables& t = *tp;
    int rc = gb_check_method(h, t);
    if (rc) return rc;
    if ((rc = gb_buffers(h, t))) return rc;
    std::vector<float> lam(h->R, 1.f);
    if (t.any_alch) for (int r = 0; r < h->R; ++r) lam[r] = gb_state_lambda(h, h->labels.empty() ? 0 : (int)h->labels[h->r_begin + r]);
    if ((rc = gb_set_lambdas(h, t, lam))) return rc;
    remd_prof_scope ps(h, "gbsa");
    if (gb_small(h, t)) {
        if (with_energy) hipLaunchKernelGGL((gb_small_kernel<true, true>), dim3(h->R), dim3(1024), 0, h->stream, t.N, h->Npad, t.k, t.tau, t.sasa, t.d_par, t.d_lam, 1, h->d_pos, h->d_force, h->d_epart, h->n_epart, ep_slot, 0);
        else hipLaunchKernelGGL((gb_small_kernel<false, true>), dim3(h->R), dim3(1024), 0, h->stream, t.N, h->Npad, t.k, t.tau, t.sasa, t.d_par, t.d_lam, 1, h->d_pos, h->d_force, (double*)nullptr, 0, 0, 0);
        REMD_CHECK(h, hipGetLastError());
        return 0;
    }
    if (t.method == GB_CUT_PERIODIC) gb_launch<GB_CUT_PERIODIC>(h, t, t.d_lam, 1, with_energy, true, h->d_force);
    else gb_launch<GB_CUT_NONE>(h, t, t.d_lam, 1, with_energy, true, h->d_force);
    if (with_energy) {
        const bool periodic = t.method == GB_CUT_PERIODIC;
        hipLaunchKernelGGL(gb_reduce_kernel, dim3(h->R), dim3(64), 0, h->stream, t.n_tile, t.d_epart, h->d_epart, h->n_epart, periodic ? h->n_epart - 2 : ep_slot, periodic ? 1 : 0);
    }
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

// u_kl: the GB energy of every replica at every state's lambda, ADDED to d_alch[r][k] (alchemical particles only: else it is the same in every column)
int remd_gbsa_ukl(remd_ctx* h, double* d_alch)
{
    gbsa_tables* tp = h->gb.get();
    if (!tp || !tp->any_alch) return 0;
    gbsa_tables& t = *tp;
    int rc = gb_check_method(h, t);
    if (rc) return rc;
    if ((rc = gb_buffers(h, t))) return rc;
    // the states' lambdas on the device (uploaded when they change: one synchronisation then, none per column)
    {
        std::vector<float> sl(h->K);
        for (int k = 0; k < h->K; ++k) sl[k] = gb_state_lambda(h, k);
        if (sl != t.state_lam_host) {
            if ((int)t.state_lam_host.size() != h->K) REMD_TRY(t.d_state_lam.alloc(h, h->K));
            REMD_CHECK(h, hipMemcpyAsync(t.d_state_lam, sl.data(), sizeof(float) * h->K, hipMemcpyHostToDevice, h->stream));
            REMD_CHECK(h, hipStreamSynchronize(h->stream));
            t.state_lam_host = sl;
        }
    }
    for (int k = 0; k < h->K; ++k) {
        if (gb_small(h, t)) {
            hipLaunchKernelGGL((gb_small_kernel<true, false>), dim3(h->R), dim3(1024), 0, h->stream, t.N, h->Npad, t.k, t.tau, t.sasa, t.d_par, t.d_state_lam + k, 0, h->d_pos, (long long*)nullptr, d_alch, h->K, k, 1);
            continue;
        }
        if (t.method == GB_CUT_PERIODIC) gb_launch<GB_CUT_PERIODIC>(h, t, t.d_state_lam + k, 0, true, false, nullptr);
        else gb_launch<GB_CUT_NONE>(h, t, t.d_state_lam + k, 0, true, false, nullptr);
        hipLaunchKernelGGL(gb_reduce_kernel, dim3(h->R), dim3(64), 0, h->stream, t.n_tile, t.d_epart, d_alch, h->K, k, 1);
    }
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

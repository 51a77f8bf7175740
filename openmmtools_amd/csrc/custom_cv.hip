// Collective-variable forces (include/remd_hip_custom.h, REMD_CUSTOM_CV): OpenMM's CustomCVForce over RMSDForce variables -- an energy
// expression of one to three RMSDs, each the root-mean-square deviation of a set of particles from reference coordinates after the
// optimal superposition.  Three launches per force evaluation, behind one another on the stream of the listed terms, issued only for a
// handle that holds such a force (the pattern of custom_centroid.hip):
//
//  1. superposition, grid (variables of all such forces, R), one workgroup of 256 threads each.  Every thread sums its strided share
//     of the variable's particles in f64, from the f32 positions taken relative to the variable's FIRST particle (a set whose centroid
//     lies 40 nm out loses nothing to the offset): the centroid and the 3 x 3 correlation with the reference, twelve sums.  The
//     reference arrives centred on its own centroid (the host does that in f64), so the correlation with x_i - x_first is the one
//     with x_i - c.  Sums: a xor-shuffle tree per wavefront, the four wavefronts added in order (centroid_sum.h's scheme).  Then the
//     rotation U (custom_cv_math.h: Horn's 4 x 4 matrix, cyclic Jacobi, the proper rotation of the largest eigenpair): a few hundred
//     f64 operations on wave-uniform data.  Every lane runs them on the same twelve sums and so holds the same U -- one lane's worth
//     of time, and no broadcast through LDS or barrier behind it.  A second pass over the particles sums |x_i - c - U ref_i|^2
//     directly; the RMSD is the square root of that over n.  (G_x + G_ref - 2 lambda would cancel at small RMSD; the direct sum is
//     stationary in U, so U's rounding enters squared.)  -> W[r][variable] = (V, flag, c[3], U[9], dE/dV).  A mean square
//     deviation below 1e-20 nm^2 gives V = 0 and flag = 1, "no force": OpenMM's reference behaviour, and no 0 / 0 in the spread.
//  2. expression: one wavefront per force (its wavefront of the padded term space, the last part; lane 0 is the force's one term, the
//     other lanes repeat it and add nothing), cst_eval<false> with the variables x0 ... x2 = V under the replica's own globals.  The
//     energy goes to the wavefront's slot of Ewave, so custom_reduce_kernel, the per-force energies and the force-group masks pick
//     it up in descriptor order; dE/dV_k goes to W.
//  3. spread, grid (variables, R): every thread gives its strided share of the particles -(dE/dV) (x_i - c - U ref_i) / (n V)
//     through add_force, rounded to f32 only there; nothing where the flag is set.
//
// Nothing here adds floating-point numbers atomically: W and the forces (fixed-point accumulators) depend on the input alone.  The
// u_kl share is the expression under every state's globals, behind a superposition launch of its own on the main stream.
// No minimum images anywhere (OpenMM's rule for RMSDForce): the host refuses a variable that spans molecules a barostat wraps apart.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"
#include "custom_cv_superpose.h"

namespace {

constexpr int CV_W = 16;            // doubles per (replica, variable) of W: V, flag, c[3], U[9], dE/dV, one spare

// a replica's positions as the superposition reads them (custom_cv_superpose.h)
struct cv_pos4 {
    const float4* __restrict__ P;
    __device__ __forceinline__ void operator()(int a, float& x, float& y, float& z) const { const float4 q = P[a]; x = q.x; y = q.y; z = q.z; }
};

// grid (n_cv, R), CV_BLOCK threads: the two passes of custom_cv_superpose.h
__global__ __launch_bounds__(CV_BLOCK)
void custom_cv_superpose_kernel(int n_cv, const int* __restrict__ cv_off, const int* __restrict__ cv_atoms, const double* __restrict__ cv_ref,
                                int Npad, const float4* __restrict__ pos, double* __restrict__ W /*[R][n_cv][CV_W]*/)
{
    __shared__ double s[12][4];
    const int cv = blockIdx.x, r = blockIdx.y;
    const int b = cv_off[cv], n = cv_off[cv + 1] - b;
    const cv_pos4 X{pos + (size_t)r * Npad};
    cv_fit fit;
    cv_superpose_block(X, cv_atoms, cv_ref, b, n, s, fit);
    if (threadIdx.x == 0) {
        const double msd = fit.msd;
        const bool flat = !(msd >= CV_MSD_FLOOR);                 // (a NaN sets the flag too: no force from it)
        double* o = W + ((size_t)r * n_cv + cv) * CV_W;
        o[0] = flat ? (msd != msd ? msd : 0.0) : sqrt(msd);
        o[1] = flat ? 1.0 : 0.0;
        o[2] = (double)fit.ax + fit.cx; o[3] = (double)fit.ay + fit.cy; o[4] = (double)fit.az + fit.cz;
#pragma unroll
        for (int a = 0; a < 3; ++a) { o[5 + 3 * a] = fit.U[a][0]; o[6 + 3 * a] = fit.U[a][1]; o[7 + 3 * a] = fit.U[a][2]; }
    }
}

// the lane's variables: the RMSDs of the force's collective variables
__device__ __forceinline__ void cv_load(const cst_force& f, const double* __restrict__ Wr, double& x0, double& x1, double& x2)
{
    const double* o = Wr + (size_t)f.cv0 * CV_W;
    x0 = o[0];
    x1 = f.n_cvs > 1 ? o[CV_W] : 0.0;
    x2 = f.n_cvs > 2 ? o[2 * CV_W] : 0.0;
}

// grid (wavefronts of the collective-variable forces, R), 64 threads; w0: the first of them in the padded term space of `waves` wavefronts
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_cv_expression_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                                 const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                                 const double* __restrict__ glob /*[K][ng]*/, int ng, const int64_t* __restrict__ labels, int r_begin,
                                 int n_cv, double* __restrict__ W, double* __restrict__ Ewave /*[R][waves]*/)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int t = w * 64 + lane - f.slot0;
    const double* g = glob + (size_t)labels[r_begin + r] * ng;
    double* Wr = W + (size_t)r * n_cv * CV_W;
    double x0, x1, x2;
    cv_load(f, Wr, x0, x1, x2);
    const cx e = cst_eval<false>(f, prog, consts, par, t, g, x0, x1, x2, 0.0, 0.0, 0.0, S, lane);
    const bool active = t < f.n_terms;
    if (active) {
        double* o = Wr + (size_t)f.cv0 * CV_W;
        o[14] = e.a;
        if (f.n_cvs > 1) o[CV_W + 14] = e.b;
        if (f.n_cvs > 2) o[2 * CV_W + 14] = e.c;
    }
    if (ENERGY) {
        const double ew = cst_wave_sum(active ? e.v : 0.0);
        if (lane == 0) Ewave[(size_t)r * waves + w] = ew;
    }
}

// grid (n_cv, R), CV_BLOCK threads
__global__ __launch_bounds__(CV_BLOCK)
void custom_cv_spread_kernel(int n_cv, const int* __restrict__ cv_off, const int* __restrict__ cv_atoms, const double* __restrict__ cv_ref,
                             const double* __restrict__ W, int Npad, const float4* __restrict__ pos, long long* __restrict__ force)
{
    const int cv = blockIdx.x, r = blockIdx.y;
    const double* o = W + ((size_t)r * n_cv + cv) * CV_W;
    if (o[1] != 0.0) return;                                      // flagged: no force (wave-uniform)
    const int b = cv_off[cv], n = cv_off[cv + 1] - b;
    const double k = -o[14] / ((double)n * o[0]);
    const double c0 = o[2], c1 = o[3], c2 = o[4];
    const double U00 = o[5], U01 = o[6], U02 = o[7], U10 = o[8], U11 = o[9], U12 = o[10], U20 = o[11], U21 = o[12], U22 = o[13];
    const float4* P = pos + (size_t)r * Npad;
    long long* Fr = force + (size_t)r * 3 * Npad;
    for (int i = threadIdx.x; i < n; i += CV_BLOCK) {
        const int a = cv_atoms[b + i];
        const float4 q = P[a];
        const double* y = cv_ref + 3 * (size_t)(b + i);
        const double y0 = y[0], y1 = y[1], y2 = y[2];
        const double ex = (double)q.x - c0 - (U00 * y0 + U01 * y1 + U02 * y2);
        const double ey = (double)q.y - c1 - (U10 * y0 + U11 * y1 + U12 * y2);
        const double ez = (double)q.z - c2 - (U20 * y0 + U21 * y1 + U22 * y2);
        add_force(Fr, Npad, a, (float)(k * ex), (float)(k * ey), (float)(k * ez));
    }
}

// u_kl partials, grid (wavefronts of the collective-variable forces, R): D[r][l][w] = e(g_l) - e(g_own) of the force's one term
// (custom_ukl_kernel over the RMSDs)
__global__ __launch_bounds__(64)
void custom_cv_ukl_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const double* __restrict__ par,
                          const int2* __restrict__ prog, const double* __restrict__ consts, const double* __restrict__ glob, int ng, int K,
                          const int64_t* __restrict__ labels, int r_begin, int n_cv, const double* __restrict__ W, double* __restrict__ D)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int t = w * 64 + lane - f.slot0;
    const double* g_own = glob + (size_t)labels[r_begin + r] * ng;
    double x0, x1, x2;
    cv_load(f, W + (size_t)r * n_cv * CV_W, x0, x1, x2);
    const bool active = t < f.n_terms;
    double e_own = 0.0;
    for (int l = -1; l < K; ++l) {
        const double* g = l < 0 ? g_own : glob + (size_t)l * ng;
        bool same = l >= 0;
        for (int i = 0; i < ng && same; ++i) same = g[i] == g_own[i];
        double d = 0.0;
        if (!same) {
            const double e = cst_eval<false>(f, prog, consts, par, t, g, x0, x1, x2, 0.0, 0.0, 0.0, S, lane).v;
            if (l < 0) e_own = e; else d = active ? e - e_own : 0.0;
        }
        if (l >= 0) {
            d = cst_wave_sum(d);
            if (lane == 0) D[((size_t)r * K + l) * waves + w] = d;
        }
    }
}

void launch_superpose(remd_ctx* h, cst_tables& t, hipStream_t st)
{
    remd_prof_scope ps(h, "custom_cv_superpose", st);
    hipLaunchKernelGGL(custom_cv_superpose_kernel, dim3(t.n_cv, h->R), dim3(CV_BLOCK), 0, st, t.n_cv, t.d_cv_off, t.d_cv_atoms, t.d_cv_ref,
                       h->Npad, h->d_pos, t.d_W);
}

}  // namespace

size_t remd_custom_cv_w() { return CV_W; }

// (the caller, remd_custom_forces, has sized d_W: ensure_buffers of custom_terms.hip)
void remd_custom_cv_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_CV);
    launch_superpose(h, t, st);
    {
        remd_prof_scope ps(h, "custom_cv_expression", st);
        if (with_energy)
            hipLaunchKernelGGL(custom_cv_expression_kernel<true>, dim3(t.end(CST_CV) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force,
                               t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, t.n_cv, t.d_W, t.d_Ewave);
        else
            hipLaunchKernelGGL(custom_cv_expression_kernel<false>, dim3(t.end(CST_CV) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force,
                               t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, t.n_cv, t.d_W, t.d_Ewave);
    }
    remd_prof_scope ps(h, "custom_cv_spread", st);
    hipLaunchKernelGGL(custom_cv_spread_kernel, dim3(t.n_cv, h->R), dim3(CV_BLOCK), 0, st, t.n_cv, t.d_cv_off, t.d_cv_atoms, t.d_cv_ref, t.d_W,
                       h->Npad, h->d_pos, h->d_force);
}

void remd_custom_cv_ukl(remd_ctx* h, cst_tables& t)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_CV);
    launch_superpose(h, t, h->stream);
    hipLaunchKernelGGL(custom_cv_ukl_kernel, dim3(t.end(CST_CV) - w0, h->R), dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force, t.d_par, t.d_prog,
                       t.d_consts, t.d_glob, t.ng, h->K, h->d_labels, h->r_begin, t.n_cv, t.d_W, t.d_D);
}

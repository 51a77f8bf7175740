// Nonbonded custom forces (include/remd_hip_custom.h, REMD_CUSTOM_NONBONDED): OpenMM's CustomNonbondedForce, an energy expression of
// the distance r of two particles, of their per-particle parameters (p1, p2) and of global parameters, summed over every pair inside
// a cutoff that no exclusion names -- the WCA fluids and the custom Lennard-Jones mixture have no other pair interaction.
//
// One wavefront per tile of 64 x 64 atoms of one replica, upper-triangular tiles only (jb >= ib, row by row), so every pair is
// evaluated once.  The tiles of a force ARE its wavefronts in the padded term space (npad = 64 n_tiles; they lie behind the
// compound-bond forces' and in front of the centroid forces'), so the per-wavefront energy and u_kl partials land in the arrays
// custom_reduce_kernel / custom_ukl_reduce_kernel add in their fixed order.  The cost is quadratic in N: every tile is visited, there
// is no cell list and no bounding-box cull.
//
// Two stages per tile.  Candidates: lane = atom i of the row block, the 64 atoms j of the column block staged in LDS; the difference
// in f64 from the f32 positions, minimum image under the replica's own box (CutoffPeriodic); a pair survives when d.d < cutoff^2
// (always without a cutoff), i < j on a diagonal tile, both atoms are real, and j is not excluded (the lane's exclusion row is folded
// into a 64-bit mask of the column block once per tile).  Survivors are appended to an LDS queue at ballot + mbcnt positions: the
// pair -> lane assignment is a function of the inputs alone.  Evaluation: whenever the queue holds 64 pairs, and once for the rest,
// cst_eval<false> runs one pair per lane with x0 = r and the pair's parameters staged as [2 n_params][64] in LDS (particle 1's first);
// E and dE/dr are multiplied by OpenMM's switch S(r) = 1 - 10 t^3 + 15 t^4 - 6 t^5, t = (r - rs) / (rc - rs), plus E S'(r) on the
// derivative; -+(dE/dr) d / r goes to both atoms through the fixed-point accumulators (order-independent: bit-reproducible), r = 0
// gives no force.  The wavefront's energy is a xor-shuffle sum per batch, added in batch order.  No floating-point atomics.
//
// The long-range correction is the host's (custom_expr.long_range_coefficients: one coefficient per state and force,
// remd_set_custom_lrc); the device adds coeff[state of r] / V_r to the replica's energy behind custom_reduce_kernel, V_r from the
// replica's own box (a barostat's trial volume sees it), and beta_l (c_l - c_own) / V_r to the u_kl rows.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"

namespace {

// the k-th upper-triangular tile of nb blocks, row by row: (ib, jb >= ib)
__device__ __forceinline__ void cnb_tile(int k, int nb, int& ib, int& jb)
{
    ib = 0;
    while (k >= nb - ib) { k -= nb - ib; ++ib; }
    jb = ib + k;
}

struct cnb_tile_ctx {
    int ib, jb, lane;
    bool pbc;
    double Lx, Ly, Lz;
};

// the candidate stage of tile (ib, jb): batch(entry, on) is called with 64 queued pairs (row lane << 6 | column lane), wave-uniformly
template <class Batch>
__device__ __forceinline__ void cnb_pairs(const cst_force& f, const cnb_tile_ctx& c, const float4* __restrict__ P,
                                          const int* __restrict__ excl_off, const int* __restrict__ excl_atoms, float4* xi, float4* xj,
                                          int* queue, Batch&& batch)
{
    const int N = f.n_terms, lane = c.lane, i = c.ib * 64 + lane, j0 = c.jb * 64;
    xi[lane] = P[i];                                         // (both blocks end inside Npad = 64 ceil(N / 64); padding atoms never pair)
    xj[lane] = P[j0 + lane];
    unsigned long long ex = 0ull;
    if (i < N)
        for (int k = excl_off[f.excl0 + i]; k < excl_off[f.excl0 + i + 1]; ++k) {
            const int d = excl_atoms[k] - j0;
            if (d >= 0 && d < 64) ex |= 1ull << d;
        }
    __syncthreads();
    const float4 pi = xi[lane];
    const double rc2 = f.cutoff * f.cutoff;
    int qn = 0;
    for (int jj = 0; jj <= 64; ++jj) {                       // (jj = 64: no candidate, the rest of the queue -- one call site of batch)
        if (jj < 64) {
            const int j = j0 + jj;
            bool keep = i < N && j < N && (c.ib != c.jb || i < j) && !((ex >> jj) & 1ull);
            if (keep && f.nb_method != 0) {
                const double3 d = d3img(d3sub(xj[jj], pi), c.pbc, c.Lx, c.Ly, c.Lz);
                keep = d3dot(d, d) < rc2;
            }
            const unsigned long long m = __ballot(keep);
            if (keep) queue[qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = (lane << 6) | jj;
            qn += __popcll(m);
        }
        if (qn >= 64 || (jj == 64 && qn > 0)) {              // (qn < 128: at most 64 join 63)
            const int n = qn < 64 ? qn : 64, rest = qn - n;
            __syncthreads();
            batch(lane < n ? queue[lane] : 0, lane < n);
            const int moved = lane < rest ? queue[64 + lane] : 0;
            __syncthreads();
            if (lane < rest) queue[lane] = moved;
            qn = rest;
        }
    }
}

// a queued pair: its atoms, distance, unit vector j - i (zero at r = 0) and the switch S, S'; its parameters -> PAR[.][lane]
struct cnb_pair { int ai, aj; double r, ux, uy, uz, sw, dsw; };

__device__ __forceinline__ cnb_pair cnb_stage(const cst_force& f, const cnb_tile_ctx& c, int entry, const float4* xi, const float4* xj,
                                              const double* __restrict__ par, int stride, double (*PAR)[64])
{
    const int li = entry >> 6, jj = entry & 63;
    cnb_pair p;
    p.ai = c.ib * 64 + li; p.aj = c.jb * 64 + jj;
    const double3 d = d3img(d3sub(xj[jj], xi[li]), c.pbc, c.Lx, c.Ly, c.Lz);
    p.r = sqrt(d3dot(d, d));
    const double ir = p.r > 0.0 ? 1.0 / p.r : 0.0;
    p.ux = d.x * ir; p.uy = d.y * ir; p.uz = d.z * ir;
    p.sw = 1.0; p.dsw = 0.0;
    if (f.switch_dist >= 0.0 && p.r > f.switch_dist) {
        const double w = 1.0 / (f.cutoff - f.switch_dist), t = (p.r - f.switch_dist) * w;
        p.sw = 1.0 + t * t * t * (-10.0 + t * (15.0 - 6.0 * t));
        p.dsw = t * t * (-30.0 + t * (60.0 - 30.0 * t)) * w;
    }
    for (int k = 0; k < f.n_params; ++k) {
        PAR[k][c.lane] = par[f.par0 + (size_t)k * stride + p.ai];
        PAR[f.n_params + k][c.lane] = par[f.par0 + (size_t)k * stride + p.aj];
    }
    return p;
}

// grid (tiles of the nonbonded forces, R), 64 threads; w0: the first of them in the padded term space of `waves` wavefronts
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_nonbonded_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                             const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                             const double* __restrict__ glob /*[K][ng]*/, int ng, const int* __restrict__ excl_off,
                             const int* __restrict__ excl_atoms, const int64_t* __restrict__ labels, int r_begin, int Npad,
                             const float4* __restrict__ pos, const float* __restrict__ box, long long* __restrict__ force,
                             double* __restrict__ Ewave /*[R][waves]*/)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ float4 xi[64], xj[64];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;            // (the machine reads parameter k of the lane's pair at PAR[k][lane])
    cnb_tile_ctx c;
    cnb_tile(w - f.slot0 / 64, (f.n_terms + 63) / 64, c.ib, c.jb);
    c.lane = lane; c.pbc = f.periodic != 0;
    c.Lx = box[4 * r]; c.Ly = box[4 * r + 1]; c.Lz = box[4 * r + 2];
    const double* g = glob + (size_t)labels[r_begin + r] * ng;
    long long* Fr = force + (size_t)r * 3 * Npad;
    double E = 0.0;
    cnb_pairs(f, c, pos + (size_t)r * Npad, excl_off, excl_atoms, xi, xj, queue, [&](int entry, bool on) {
        const cnb_pair p = cnb_stage(f, c, entry, xi, xj, par, Npad, PAR);
        const cx e = cst_eval<false>(fl, prog, consts, &PAR[0][0], lane, g, p.r, 0.0, 0.0, c.Lx, c.Ly, c.Lz, S, lane);
        if (on) {
            const double k = e.a * p.sw + e.v * p.dsw;       // d(E S)/dr; the force on i is +k (x_j - x_i) / r
            add_force(Fr, Npad, p.ai, (float)(k * p.ux), (float)(k * p.uy), (float)(k * p.uz));
            add_force(Fr, Npad, p.aj, (float)(-k * p.ux), (float)(-k * p.uy), (float)(-k * p.uz));
        }
        if (ENERGY) E += cst_wave_sum(on ? e.v * p.sw : 0.0);
    });
    if (ENERGY && lane == 0) Ewave[(size_t)r * waves + w] = E;
}

// u_kl partials, same grid: D[r][l][w] = sum over the tile's pairs of S(r) (e(g_l) - e(g_own)), the difference formed per pair, the
// batches added in their order by lane 0 alone
__global__ __launch_bounds__(64)
void custom_nonbonded_ukl_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                                 const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                                 const double* __restrict__ glob, int ng, int K, const int* __restrict__ excl_off,
                                 const int* __restrict__ excl_atoms, const int64_t* __restrict__ labels, int r_begin, int Npad,
                                 const float4* __restrict__ pos, const float* __restrict__ box, double* __restrict__ D)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ float4 xi[64], xj[64];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;
    cnb_tile_ctx c;
    cnb_tile(w - f.slot0 / 64, (f.n_terms + 63) / 64, c.ib, c.jb);
    c.lane = lane; c.pbc = f.periodic != 0;
    c.Lx = box[4 * r]; c.Ly = box[4 * r + 1]; c.Lz = box[4 * r + 2];
    const double* g_own = glob + (size_t)labels[r_begin + r] * ng;
    if (lane == 0) for (int l = 0; l < K; ++l) D[((size_t)r * K + l) * waves + w] = 0.0;
    cnb_pairs(f, c, pos + (size_t)r * Npad, excl_off, excl_atoms, xi, xj, queue, [&](int entry, bool on) {
        const cnb_pair p = cnb_stage(f, c, entry, xi, xj, par, Npad, PAR);
        double e_own = 0.0;
        for (int l = -1; l < K; ++l) {
            const double* g = l < 0 ? g_own : glob + (size_t)l * ng;
            bool same = l >= 0;
            for (int i = 0; i < ng && same; ++i) same = g[i] == g_own[i];
            if (same) continue;
            const double e = cst_eval<false>(fl, prog, consts, &PAR[0][0], lane, g, p.r, 0.0, 0.0, c.Lx, c.Ly, c.Lz, S, lane).v;
            if (l < 0) { e_own = e; continue; }
            const double d = cst_wave_sum(on ? (e - e_own) * p.sw : 0.0);
            if (lane == 0) D[((size_t)r * K + l) * waves + w] += d;
        }
    });
}

// grid (R), 64 threads, behind custom_reduce_kernel: E[r][f] and the replica's energy partial gain coeff[state of r][f] / V_r
__global__ __launch_bounds__(64)
void custom_nonbonded_lrc_kernel(int nf, const cst_force* __restrict__ F, const double* __restrict__ lrc /*[K][nf]*/,
                                 const int64_t* __restrict__ labels, int r_begin, const float* __restrict__ box, double* __restrict__ E,
                                 double* __restrict__ epart, int n_epart, int ep_slot)
{
    const int r = blockIdx.x;
    if (threadIdx.x != 0) return;
    const double V = (double)box[4 * r] * (double)box[4 * r + 1] * (double)box[4 * r + 2];
    const double* c = lrc + (size_t)labels[r_begin + r] * nf;
    double total = 0.0;
    for (int i = 0; i < nf; ++i) {
        if (!F[i].lrc) continue;
        const double e = c[i] / V;
        E[(size_t)r * nf + i] += e;
        total += e;
    }
    epart[(size_t)r * n_epart + ep_slot] += total;
}

// grid (K, R), 64 threads, behind custom_ukl_reduce_kernel: rows[r][l] += beta_l sum_f (c_l - c_own) / V_r
__global__ __launch_bounds__(64)
void custom_nonbonded_lrc_ukl_kernel(int nf, int K, const cst_force* __restrict__ F, const double* __restrict__ lrc,
                                     const int64_t* __restrict__ labels, int r_begin, const float* __restrict__ box,
                                     const double* __restrict__ beta, double* __restrict__ rows)
{
    const int l = blockIdx.x, r = blockIdx.y;
    if (threadIdx.x != 0) return;
    const double V = (double)box[4 * r] * (double)box[4 * r + 1] * (double)box[4 * r + 2];
    const double* c_own = lrc + (size_t)labels[r_begin + r] * nf;
    const double* c = lrc + (size_t)l * nf;
    double d = 0.0;
    for (int i = 0; i < nf; ++i) if (F[i].lrc) d += c[i] - c_own[i];
    rows[(size_t)r * K + l] += beta[l] * d / V;
}

}  // namespace

void remd_custom_nonbonded_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_NONBONDED);
    if (with_energy)
        hipLaunchKernelGGL(custom_nonbonded_kernel<true>, dim3(t.end(CST_NONBONDED) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force,
                           t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                           h->d_pos, h->d_box, h->d_force, t.d_Ewave);
    else
        hipLaunchKernelGGL(custom_nonbonded_kernel<false>, dim3(t.end(CST_NONBONDED) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force,
                           t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                           h->d_pos, h->d_box, h->d_force, t.d_Ewave);
}

void remd_custom_nonbonded_lrc(remd_ctx* h, cst_tables& t, int ep_slot, hipStream_t st)
{
    hipLaunchKernelGGL(custom_nonbonded_lrc_kernel, dim3(h->R), dim3(64), 0, st, t.nf, t.d_F, t.d_lrc, h->d_labels, h->r_begin, h->d_box, t.d_E,
                       h->d_epart, h->n_epart, ep_slot);
}

void remd_custom_nonbonded_ukl(remd_ctx* h, cst_tables& t)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_NONBONDED);
    hipLaunchKernelGGL(custom_nonbonded_ukl_kernel, dim3(t.end(CST_NONBONDED) - w0, h->R), dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force,
                       t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->K, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                       h->d_pos, h->d_box, t.d_D);
}

void remd_custom_nonbonded_lrc_ukl(remd_ctx* h, cst_tables& t, double* d_rows)
{
    hipLaunchKernelGGL(custom_nonbonded_lrc_ukl_kernel, dim3(h->K, h->R), dim3(64), 0, h->stream, t.nf, h->K, t.d_F, t.d_lrc, h->d_labels,
                       h->r_begin, h->d_box, h->d_beta, d_rows);
}

// Donor-acceptor custom forces (include/remd_hip_custom.h, REMD_CUSTOM_HBOND): OpenMM's CustomHbondForce, an energy expression of the
// distances, angles and dihedrals among the up to three particles of a donor (d1 d2 d3, particle slots 0 1 2) and the up to three of an
// acceptor (a1 a2 a3, slots 3 4 5), of per-donor, per-acceptor and global parameters, summed over every (donor, acceptor) pair that no
// exclusion names and, with a cutoff, whose d1 - a1 distance is below it -- the base-pairing and cross-stacking terms of coarse-grained
// DNA, the backbone hydrogen bonds of Go-like protein models, the 10-12 term of DREIDING.
//
// The pair search is custom_nonbonded.hip's, the evaluation custom_compound.hip's.  One wavefront per tile of 64 donors x 64 acceptors of
// one replica, ALL ceil(nD / 64) x ceil(nA / 64) tiles, row by row (donors and acceptors are different lists: there is no triangle).  The
// tiles of a force are its wavefronts in the padded term space (npad = 64 n_tiles; the part CST_HBOND lies behind every other kind's, so
// no other force's slot moves), and the per-wavefront energy and u_kl partials land in the arrays custom_reduce_kernel /
// custom_ukl_reduce_kernel add in their fixed order.  The cost is proportional to nD nA per replica: every tile is visited, there is no
// list.
//
// Candidates: lane = donor i of the row block; the d1 of the 64 donors and the a1 of the 64 acceptors of the column block staged in LDS;
// the difference in f64 from the f32 positions, minimum image under the replica's own box (CutoffPeriodic); a pair survives when both
// are real, the acceptor is not in the donor's exclusion row (folded into a 64-bit mask of the column block once per tile) and, with a
// cutoff, d.d < cutoff^2.  Survivors are appended to an LDS queue at ballot + mbcnt positions: the pair -> lane assignment is a function
// of the inputs alone.  Evaluation: whenever the queue holds 64 pairs, and once for the rest, every lane stages its pair's six particle
// positions as f64 (cst_pos X[6]; a slot the donor or acceptor does not have is filled with slot 0's position: the host has made sure
// the program does not name it) and its donor's and acceptor's parameters (PAR[.][lane], the donor's first), and cst_eval<true> runs
// once per particle slot the program names (cst_force::hb_mask) with that slot seeded; each pass's partials go to that particle's
// atom through the fixed-point add_force (order-independent: bit-reproducible).  The energy is the first pass's, summed per batch by
// cst_wave_sum and added in batch order.  The idle lanes of a partial batch run the machine on the batch's first pair and add nothing.
// No floating-point atomics, no scratch.
//
// Static LDS: the 32 KiB stack, 9 KiB positions, 8 KiB parameters, 2 KiB d1 / a1 blocks and the 512 B queue: 51.5 KiB.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"

namespace {

struct chb_tile_ctx {
    int ib, jb, lane;            // donor block, acceptor block
    int ndpad, napad;            // the padded donor and acceptor counts
    bool pbc;
    double Lx, Ly, Lz;
};

__device__ __forceinline__ chb_tile_ctx chb_tile(const cst_force& f, int w, int lane, const float* __restrict__ box, int r)
{
    chb_tile_ctx c;
    c.ndpad = (f.n_terms + 63) / 64 * 64; c.napad = (f.hb_na + 63) / 64 * 64;
    const int t = w - f.slot0 / 64, nbj = c.napad / 64;
    c.ib = t / nbj; c.jb = t - c.ib * nbj;
    c.lane = lane; c.pbc = f.periodic != 0;
    c.Lx = box[4 * r]; c.Ly = box[4 * r + 1]; c.Lz = box[4 * r + 2];
    return c;
}

// the candidate stage of tile (ib, jb): batch(entry, on) is called with up to 64 queued pairs (donor lane << 6 | acceptor lane),
// wave-uniformly; an idle lane gets the batch's first pair
template <class Batch>
__device__ __forceinline__ void chb_pairs(const cst_force& f, const chb_tile_ctx& c, const float4* __restrict__ P, const int* __restrict__ hb_atoms,
                                          const int* __restrict__ excl_off, const int* __restrict__ excl_atoms, float4* xi, float4* xj,
                                          int* queue, Batch&& batch)
{
    const int nD = f.n_terms, nA = f.hb_na, lane = c.lane, i = c.ib * 64 + lane, j0 = c.jb * 64;
    xi[lane] = P[hb_atoms[f.hb_atoms0 + i]];                               // d1 (a padding column repeats the last donor: a real atom)
    xj[lane] = P[hb_atoms[f.hb_atoms0 + 3 * c.ndpad + j0 + lane]];          // a1
    unsigned long long ex = 0ull;
    if (i < nD)
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
            bool keep = i < nD && j0 + jj < nA && !((ex >> jj) & 1ull);
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
            batch(queue[lane < n ? lane : 0], lane < n);
            const int moved = lane < rest ? queue[64 + lane] : 0;
            __syncthreads();
            if (lane < rest) queue[lane] = moved;
            qn = rest;
        }
    }
}

// a queued pair: its donor and acceptor columns; its six particles -> X[.][.][lane], its parameters -> PAR[.][lane]
struct chb_pair { int di, aj; };

__device__ __forceinline__ chb_pair chb_stage(const cst_force& f, const chb_tile_ctx& c, int entry, const float4* __restrict__ P,
                                              const int* __restrict__ hb_atoms, const double* __restrict__ par, cst_pos* X, double (*PAR)[64])
{
    chb_pair p;
    p.di = c.ib * 64 + (entry >> 6); p.aj = c.jb * 64 + (entry & 63);
    const int lane = c.lane;
    const float4 first = P[hb_atoms[f.hb_atoms0 + p.di]];
    for (int q = 0; q < 6; ++q) {
        const int a = q < 3 ? hb_atoms[f.hb_atoms0 + q * c.ndpad + p.di] : hb_atoms[f.hb_atoms0 + 3 * c.ndpad + (q - 3) * c.napad + p.aj];
        float4 x = first;                                    // (a particle the donor or acceptor does not have: slot 0's position, never read by the program)
        if (a >= 0) x = P[a];
        X[q][0][lane] = (double)x.x; X[q][1][lane] = (double)x.y; X[q][2][lane] = (double)x.z;
    }
    for (int k = 0; k < f.hb_npd; ++k) PAR[k][lane] = par[f.par0 + (size_t)k * c.ndpad + p.di];
    const size_t pa0 = (size_t)f.par0 + (size_t)f.hb_npd * c.ndpad;
    for (int k = 0; k < f.hb_npa; ++k) PAR[f.hb_npd + k][lane] = par[pa0 + (size_t)k * c.napad + p.aj];
    return p;
}

// the atom of particle slot q of the pair (>= 0 for every slot of hb_mask: remd_set_custom_terms has checked it)
__device__ __forceinline__ int chb_atom(const cst_force& f, const chb_tile_ctx& c, const chb_pair& p, const int* __restrict__ hb_atoms, int q)
{
    return q < 3 ? hb_atoms[f.hb_atoms0 + q * c.ndpad + p.di] : hb_atoms[f.hb_atoms0 + 3 * c.ndpad + (q - 3) * c.napad + p.aj];
}

// grid (tiles of the donor-acceptor forces, R), 64 threads; w0: the first of them in the padded term space of `waves` wavefronts
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_hbond_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ hb_atoms,
                         const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                         const double* __restrict__ glob /*[K][ng]*/, int ng, const int* __restrict__ excl_off,
                         const int* __restrict__ excl_atoms, const int64_t* __restrict__ labels, int r_begin, int Npad,
                         const float4* __restrict__ pos, const float* __restrict__ box, long long* __restrict__ force,
                         double* __restrict__ Ewave /*[R][waves]*/)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[6];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ float4 xi[64], xj[64];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;            // (the machine reads parameter k of the lane's pair at PAR[k][lane])
    const chb_tile_ctx c = chb_tile(f, w, lane, box, r);
    const double Lx = c.pbc ? c.Lx : 0.0, Ly = c.pbc ? c.Ly : 0.0, Lz = c.pbc ? c.Lz : 0.0;   // (0: cst_image leaves a difference as it is)
    const double* g = glob + (size_t)labels[r_begin + r] * ng;
    const float4* P = pos + (size_t)r * Npad;
    long long* Fr = force + (size_t)r * 3 * Npad;
    double E = 0.0;
    chb_pairs(f, c, P, hb_atoms, excl_off, excl_atoms, xi, xj, queue, [&](int entry, bool on) {
        const chb_pair p = chb_stage(f, c, entry, P, hb_atoms, par, X, PAR);
        double e0 = 0.0;
        bool first = true;
        for (int q = 0; q < 6; ++q) {
            if (!((f.hb_mask >> q) & 1)) continue;
            const cx e = cst_eval<true>(fl, prog, consts, &PAR[0][0], lane, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, q);
            if (first) { e0 = e.v; first = false; }
            if (on) add_force(Fr, Npad, chb_atom(f, c, p, hb_atoms, q), (float)-e.a, (float)-e.b, (float)-e.c);
        }
        if (ENERGY) {
            if (first) e0 = cst_eval<true>(fl, prog, consts, &PAR[0][0], lane, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, -1).v;   // (no particle named: a sum of parameters)
            E += cst_wave_sum(on ? e0 : 0.0);
        }
    });
    if (ENERGY && lane == 0) Ewave[(size_t)r * waves + w] = E;
}

// u_kl partials, same grid: D[r][l][w] = sum over the tile's pairs of e(g_l) - e(g_own), the program unseeded, the difference formed per
// pair, the batches added in their order by lane 0 alone
__global__ __launch_bounds__(64)
void custom_hbond_ukl_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ hb_atoms,
                             const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                             const double* __restrict__ glob, int ng, int K, const int* __restrict__ excl_off,
                             const int* __restrict__ excl_atoms, const int64_t* __restrict__ labels, int r_begin, int Npad,
                             const float4* __restrict__ pos, const float* __restrict__ box, double* __restrict__ D)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[6];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ float4 xi[64], xj[64];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;
    const chb_tile_ctx c = chb_tile(f, w, lane, box, r);
    const double Lx = c.pbc ? c.Lx : 0.0, Ly = c.pbc ? c.Ly : 0.0, Lz = c.pbc ? c.Lz : 0.0;
    const double* g_own = glob + (size_t)labels[r_begin + r] * ng;
    const float4* P = pos + (size_t)r * Npad;
    if (lane == 0) for (int l = 0; l < K; ++l) D[((size_t)r * K + l) * waves + w] = 0.0;
    chb_pairs(f, c, P, hb_atoms, excl_off, excl_atoms, xi, xj, queue, [&](int entry, bool on) {
        chb_stage(f, c, entry, P, hb_atoms, par, X, PAR);
        double e_own = 0.0;
        for (int l = -1; l < K; ++l) {
            const double* g = l < 0 ? g_own : glob + (size_t)l * ng;
            bool same = l >= 0;
            for (int i = 0; i < ng && same; ++i) same = g[i] == g_own[i];
            if (same) continue;
            const double e = cst_eval<true>(fl, prog, consts, &PAR[0][0], lane, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, -1).v;
            if (l < 0) { e_own = e; continue; }
            const double d = cst_wave_sum(on ? e - e_own : 0.0);
            if (lane == 0) D[((size_t)r * K + l) * waves + w] += d;
        }
    });
}

// energy parameter derivatives, same grid and candidate stage: D[r][d][w] = sum over the tile's pairs of dE/dglobal(dcols[d]) under the
// replica's own globals, the machine seeded at the column and at no particle; the batches added in their order by lane 0 alone.
// STATES: under the globals of every state l in turn, D[r][l][d][w]; the candidate queue and each batch's staging run once, the
// states loop inside a batch, so a (state, column)'s batches are added in the order of the own-state kernel
template <bool STATES>
__global__ __launch_bounds__(64)
void custom_hbond_dpar_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ hb_atoms,
                              const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                              const double* __restrict__ glob, int ng, int nd, const int* __restrict__ dcols, const unsigned* __restrict__ dmask,
                              const int* __restrict__ excl_off, const int* __restrict__ excl_atoms, const int64_t* __restrict__ labels,
                              int r_begin, int Npad, const float4* __restrict__ pos, const float* __restrict__ box, double* __restrict__ D, int K)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[6];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ float4 xi[64], xj[64];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const unsigned mask = dmask[wave_force[w]];
    const int nl = STATES ? K : 1;
    if (lane == 0) for (int ld = 0; ld < nl * nd; ++ld) D[((size_t)r * nl * nd + ld) * waves + w] = 0.0;
    if (mask == 0u) return;                                  // (wave-uniform: the force declared no derivative)
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;
    const chb_tile_ctx c = chb_tile(f, w, lane, box, r);
    const double Lx = c.pbc ? c.Lx : 0.0, Ly = c.pbc ? c.Ly : 0.0, Lz = c.pbc ? c.Lz : 0.0;
    const float4* P = pos + (size_t)r * Npad;
    chb_pairs(f, c, P, hb_atoms, excl_off, excl_atoms, xi, xj, queue, [&](int entry, bool on) {
        chb_stage(f, c, entry, P, hb_atoms, par, X, PAR);
        for (int l = 0; l < nl; ++l) {
            const double* g = glob + (size_t)(STATES ? l : labels[r_begin + r]) * ng;
            for (int d = 0; d < nd; ++d) {
                if (!((mask >> d) & 1u)) continue;
                const cx e = cst_eval<true, true>(fl, prog, consts, &PAR[0][0], lane, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, -1, dcols[d]);
                const double v = cst_wave_sum(on ? e.a : 0.0);
                if (lane == 0) D[(((size_t)r * nl + l) * nd + d) * waves + w] += v;
            }
        }
    });
}

}  // namespace

void remd_custom_hbond_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_HBOND);
    if (with_energy)
        hipLaunchKernelGGL(custom_hbond_kernel<true>, dim3(t.end(CST_HBOND) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force, t.d_hb_atoms,
                           t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                           h->d_pos, h->d_box, h->d_force, t.d_Ewave);
    else
        hipLaunchKernelGGL(custom_hbond_kernel<false>, dim3(t.end(CST_HBOND) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force, t.d_hb_atoms,
                           t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                           h->d_pos, h->d_box, h->d_force, t.d_Ewave);
}

void remd_custom_hbond_ukl(remd_ctx* h, cst_tables& t)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_HBOND);
    hipLaunchKernelGGL(custom_hbond_ukl_kernel, dim3(t.end(CST_HBOND) - w0, h->R), dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force, t.d_hb_atoms,
                       t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->K, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                       h->d_pos, h->d_box, t.d_D);
}

void remd_custom_hbond_dpar(remd_ctx* h, cst_tables& t, bool states)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_HBOND);
    const dim3 grid(t.end(CST_HBOND) - w0, h->R);
    if (states)
        hipLaunchKernelGGL(custom_hbond_dpar_kernel<true>, grid, dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force, t.d_hb_atoms,
                           t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, t.d_excl_off, t.d_excl_atoms, h->d_labels,
                           h->r_begin, h->Npad, h->d_pos, h->d_box, t.d_dDK, h->K);
    else
        hipLaunchKernelGGL(custom_hbond_dpar_kernel<false>, grid, dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force, t.d_hb_atoms,
                           t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, t.d_excl_off, t.d_excl_atoms, h->d_labels,
                           h->r_begin, h->Npad, h->d_pos, h->d_box, t.d_dD, 1);
}

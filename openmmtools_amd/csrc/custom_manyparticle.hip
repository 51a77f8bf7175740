// Many-particle custom forces (include/remd_hip_custom.h, REMD_CUSTOM_MANYPARTICLE): OpenMM's CustomManyParticleForce with three
// particles per set, an energy expression of the distances, angles and dihedrals among p1 p2 p3 (particle slots 0 1 2), of per-particle
// parameters (operand 3 q + s: parameter q of the particle in slot s) and of global parameters, summed over sets of three distinct
// particles -- the three-body term of Stillinger-Weber (mW water, silicon), Axilrod-Teller dispersion.
//
// Two launches per evaluation, both rebuilt from the positions every time: there is no list that outlives a call.
//
// 1. Neighbour rows (custom_mp_neighbours_kernel): one wavefront per block of 64 particles of one replica, lane = particle i; it walks
//    the column blocks in ascending order with the 64 j staged in LDS (the candidate stage of custom_nonbonded.hip) and appends to ITS OWN
//    row nbr[r][i][0 .. 128) every j that is real, differs from i (SinglePermutation: j > i), is not in i's exclusion row (the sorted row
//    is walked once, folded into a 64-bit mask per column block) and, with a cutoff, whose f64 minimum-image distance is below it.  The
//    row is filled in ascending j and cnt[r][i] is the count; a lane whose count would pass REMD_CUSTOM_MP_MAX_NEIGHBORS stops storing
//    and keeps counting.  Each lane writes only its own row: no atomics, the list a function of the inputs alone.
//
// 2. Sets (custom_manyparticle_kernel): one wavefront per central particle i and replica -- the force's wavefronts in the padded term
//    space (npad = 64 N; the part CST_MANYPARTICLE lies behind every other kind's, so no other force's slot moves).  The row is copied to
//    LDS; lane t of a batch of 64 decodes the pair (a < b) of row entries, j = row[a] < k = row[b], and tests what the row could not:
//    the j-k exclusion (bisection of j's sorted row), in SinglePermutation the j-k cutoff, and the type filters together with the choice
//    of assignment: the first of (i,j,k) (i,k,j) (j,i,k) (j,k,i) (k,i,j) (k,j,i) -- lexicographic in the atom indices, i < j < k there --
//    that passes all three filters; in UniqueCentralParticle the first of (i,j,k) (i,k,j).  Survivors go to an LDS queue at ballot + mbcnt
//    positions; whenever it holds 64 sets, and once for the rest, every lane stages its set's three positions as f64 (cst_pos X[3]) and
//    parameters (PAR[3 q + s][lane]) and cst_eval<true> runs once per particle slot the program names (cst_force::mp_mask) with that slot
//    seeded; each pass's partials go to that slot's atom through the fixed-point add_force (order-independent: bit-reproducible).  The
//    energy is the first pass's, summed per batch by cst_wave_sum and added in batch order into Ewave[r][w].  A central particle whose
//    type fails the filter of slot 0 in UniqueCentralParticle, or whose cnt < 2, returns at once; one whose cnt exceeds the row writes
//    NaN to its Ewave and evaluates nothing (the device cannot raise: the sampler's NaN check catches it).  A launch without energies
//    (every MD and minimiser step) has no Ewave to write: it drops that particle's sets silently, and the NaN appears at the next
//    evaluation with energies.  Nothing is read or written beyond a row: only row[0 .. min(cnt, 128)) is ever decoded, and every
//    entry is an atom below N by construction.
//
// No floating-point atomics, no scratch.  Static LDS of the set kernels: the 32 KiB stack, 4.5 KiB positions, 8 KiB parameters, 512 B
// row and 512 B queue: 45.5 KiB.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"

namespace {

constexpr int MP_ROW = REMD_CUSTOM_MP_MAX_NEIGHBORS;
// the six assignments of a sorted triple (s0 < s1 < s2) to the slots (p1, p2, p3), lexicographic: per assignment 2 bits per slot
constexpr unsigned long long MP_PERMS = 36ull | 24ull << 6 | 33ull << 12 | 9ull << 18 | 18ull << 24 | 6ull << 30;

__device__ __forceinline__ int mp_pick(int which, int a, int b, int c) { return which == 0 ? a : which == 1 ? b : c; }

// grid (Npad / 64, R), 64 threads: the neighbour rows of force fi
__global__ __launch_bounds__(64)
void custom_mp_neighbours_kernel(int fi, const cst_force* __restrict__ F, const int* __restrict__ excl_off, const int* __restrict__ excl_atoms,
                                 int Npad, const float4* __restrict__ pos, const float* __restrict__ box, int mp_rows,
                                 int* __restrict__ nbr /*[R][mp_rows][MP_ROW]*/, int* __restrict__ cnt /*[R][mp_rows]*/)
{
    __shared__ float4 xj[64];
    const cst_force f = F[fi];
    const int ib = blockIdx.x, r = blockIdx.y, lane = threadIdx.x, N = f.n_terms, i = ib * 64 + lane;
    const float4* P = pos + (size_t)r * Npad;
    const bool pbc = f.periodic != 0;
    const double Lx = box[4 * r], Ly = box[4 * r + 1], Lz = box[4 * r + 2], rc2 = f.cutoff * f.cutoff;
    const float4 pi = P[i];                                  // (i < Npad; a padding atom never pairs)
    int* row = nbr + ((size_t)r * mp_rows + f.mp_row0 + i) * MP_ROW;
    int ek = 0, ee = 0;                                      // the part of the lane's exclusion row not yet passed
    if (i < N) { ek = excl_off[f.excl0 + i]; ee = excl_off[f.excl0 + i + 1]; }
    int n = 0;
    const int nb = (N + 63) / 64;
    for (int jb = f.mp_mode ? 0 : ib; jb < nb; ++jb) {       // (SinglePermutation: j > i, no block below the lane's own)
        const int j0 = jb * 64;
        __syncthreads();
        xj[lane] = P[j0 + lane];
        unsigned long long ex = 0ull;
        while (ek < ee && excl_atoms[ek] < j0 + 64) {        // (sorted: every entry is looked at once over the whole walk)
            const int d = excl_atoms[ek] - j0;
            if (d >= 0) ex |= 1ull << d;
            ++ek;
        }
        __syncthreads();
        for (int jj = 0; jj < 64; ++jj) {
            const int j = j0 + jj;
            bool keep = i < N && j < N && j != i && (f.mp_mode != 0 || j > i) && !((ex >> jj) & 1ull);
            if (keep && f.nb_method != 0) {
                const double3 d = d3img(d3sub(xj[jj], pi), pbc, Lx, Ly, Lz);
                keep = d3dot(d, d) < rc2;
            }
            if (keep) {
                if (n < MP_ROW) row[n] = j;
                ++n;
            }
        }
    }
    cnt[(size_t)r * mp_rows + f.mp_row0 + i] = n;
}

// the sets of central particle i, whose row of n <= MP_ROW entries is in LDS: batch(entry, on) is called with up to 64 queued sets
// (assignment << 14 | a << 7 | b, row entries a < b), wave-uniformly; an idle lane gets the batch's first set
template <class Batch>
__device__ __forceinline__ void mp_sets(const cst_force& f, int i, int n, int lane, bool pbc, double Lx, double Ly, double Lz,
                                        const float4* __restrict__ P, const int* __restrict__ types, const int* __restrict__ excl_off,
                                        const int* __restrict__ excl_atoms, const int* row, int* queue, Batch&& batch)
{
    const int npairs = n * (n - 1) / 2, nbatch = (npairs + 63) / 64, nperm = f.mp_mode ? 2 : 6;
    const double rc2 = f.cutoff * f.cutoff;
    const int ti = types[f.mp_types0 + i];
    int qn = 0;
    for (int bt = 0; bt <= nbatch; ++bt) {                   // (bt = nbatch: no candidate, the rest of the queue -- one call site of batch)
        if (bt < nbatch) {
            const int t = bt * 64 + lane;
            bool keep = t < npairs;
            const int tt = keep ? t : 0;                     // t = b (b - 1) / 2 + a, a < b
            int b = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)tt)) * 0.5f);
            while (b * (b - 1) / 2 > tt) --b;
            while ((b + 1) * b / 2 <= tt) ++b;
            const int a = tt - b * (b - 1) / 2;
            const int j = row[a], k = row[b];                // (a < b < n: inside the row; j < k < N)
            if (keep) {                                      // the j-k exclusion: k in j's sorted row
                int lo = excl_off[f.excl0 + j], hi = excl_off[f.excl0 + j + 1];
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (excl_atoms[mid] < k) lo = mid + 1; else hi = mid; }
                keep = !(lo < excl_off[f.excl0 + j + 1] && excl_atoms[lo] == k);
            }
            if (keep && f.mp_mode == 0 && f.nb_method != 0) {
                const double3 d = d3img(d3sub(P[k], P[j]), pbc, Lx, Ly, Lz);
                keep = d3dot(d, d) < rc2;
            }
            int perm = 0;
            if (keep) {
                const int tj = types[f.mp_types0 + j], tk = types[f.mp_types0 + k];
                bool found = false;
                for (int p = 0; p < nperm; ++p) {
                    const int code = (int)((MP_PERMS >> (6 * p)) & 63ull);
                    const bool ok = ((f.mp_filter[0] >> mp_pick(code & 3, ti, tj, tk)) & 1u) && ((f.mp_filter[1] >> mp_pick((code >> 2) & 3, ti, tj, tk)) & 1u) &&
                                    ((f.mp_filter[2] >> mp_pick((code >> 4) & 3, ti, tj, tk)) & 1u);
                    if (ok && !found) { found = true; perm = p; }
                }
                keep = found;
            }
            const unsigned long long m = __ballot(keep);
            if (keep) queue[qn + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = (perm << 14) | (a << 7) | b;
            qn += __popcll(m);
        }
        if (qn >= 64 || (bt == nbatch && qn > 0)) {          // (qn < 128: at most 64 join 63)
            const int nq = qn < 64 ? qn : 64, rest = qn - nq;
            __syncthreads();
            batch(queue[lane < nq ? lane : 0], lane < nq);
            const int moved = lane < rest ? queue[64 + lane] : 0;
            __syncthreads();
            if (lane < rest) queue[lane] = moved;
            qn = rest;
        }
    }
}

// a queued set: the atoms of its slots p1 p2 p3; its positions -> X[.][.][lane], its parameters -> PAR[3 q + s][lane]
struct mp_set { int p0, p1, p2; };

__device__ __forceinline__ mp_set mp_stage(const cst_force& f, int i, int entry, const int* row, int lane, const float4* __restrict__ P,
                                           const double* __restrict__ par, int Npad, cst_pos* X, double (*PAR)[64])
{
    const int j = row[(entry >> 7) & 127], k = row[entry & 127];
    const int code = (int)((MP_PERMS >> (6 * (entry >> 14))) & 63ull);
    mp_set s;
    s.p0 = mp_pick(code & 3, i, j, k); s.p1 = mp_pick((code >> 2) & 3, i, j, k); s.p2 = mp_pick((code >> 4) & 3, i, j, k);
    for (int q = 0; q < 3; ++q) {
        const int a = mp_pick(q, s.p0, s.p1, s.p2);
        const float4 x = P[a];
        X[q][0][lane] = (double)x.x; X[q][1][lane] = (double)x.y; X[q][2][lane] = (double)x.z;
        for (int k2 = 0; k2 < f.n_params; ++k2) PAR[3 * k2 + q][lane] = par[f.par0 + (size_t)k2 * Npad + a];
    }
    return s;
}

// the row of central particle i -> LDS; returns its count (which may exceed the row)
__device__ __forceinline__ int mp_load_row(const cst_force& f, int i, int r, int lane, int mp_rows, const int* __restrict__ nbr,
                                           const int* __restrict__ cnt, int* row)
{
    const size_t at = (size_t)r * mp_rows + f.mp_row0 + i;
    const int n = cnt[at], m = n < MP_ROW ? n : MP_ROW;
    row[lane] = lane < m ? nbr[at * MP_ROW + lane] : 0;
    row[64 + lane] = 64 + lane < m ? nbr[at * MP_ROW + 64 + lane] : 0;
    __syncthreads();
    return n;
}

// grid (central particles of the many-particle forces, R), 64 threads; w0: the first of them in the padded term space of `waves` wavefronts
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_manyparticle_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ types,
                                const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                                const double* __restrict__ glob /*[K][ng]*/, int ng, const int* __restrict__ excl_off,
                                const int* __restrict__ excl_atoms, const int64_t* __restrict__ labels, int r_begin, int Npad,
                                const float4* __restrict__ pos, const float* __restrict__ box, int mp_rows, const int* __restrict__ nbr,
                                const int* __restrict__ cnt, long long* __restrict__ force, double* __restrict__ Ewave /*[R][waves]*/)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[3];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ int row[MP_ROW];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int i = w - f.slot0 / 64;
    const int n = mp_load_row(f, i, r, lane, mp_rows, nbr, cnt, row);
    const bool central = f.mp_mode == 0 || ((f.mp_filter[0] >> types[f.mp_types0 + i]) & 1u);
    if (n < 2 || !central || n > MP_ROW) {                   // (wave-uniform; a particle that cannot be central returns before its count is looked at)
        if (ENERGY && lane == 0) Ewave[(size_t)r * waves + w] = central && n > MP_ROW ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
        return;
    }
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;            // (the machine reads parameter k of the lane's set at PAR[k][lane])
    const bool pbc = f.periodic != 0;
    const double bx = box[4 * r], by = box[4 * r + 1], bz = box[4 * r + 2];
    const double Lx = pbc ? bx : 0.0, Ly = pbc ? by : 0.0, Lz = pbc ? bz : 0.0;   // (0: cst_image leaves a difference as it is)
    const double* g = glob + (size_t)labels[r_begin + r] * ng;
    const float4* P = pos + (size_t)r * Npad;
    long long* Fr = force + (size_t)r * 3 * Npad;
    double E = 0.0;
    mp_sets(f, i, n, lane, pbc, bx, by, bz, P, types, excl_off, excl_atoms, row, queue, [&](int entry, bool on) {
        const mp_set s = mp_stage(f, i, entry, row, lane, P, par, Npad, X, PAR);
        double e0 = 0.0;
        bool first = true;
        for (int q = 0; q < 3; ++q) {
            if (!((f.mp_mask >> q) & 1)) continue;
            const cx e = cst_eval<true>(fl, prog, consts, &PAR[0][0], lane, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, q);
            if (first) { e0 = e.v; first = false; }
            if (on) add_force(Fr, Npad, mp_pick(q, s.p0, s.p1, s.p2), (float)-e.a, (float)-e.b, (float)-e.c);
        }
        if (ENERGY) {
            if (first) e0 = cst_eval<true>(fl, prog, consts, &PAR[0][0], lane, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, -1).v;   // (no particle named: a sum of parameters)
            E += cst_wave_sum(on ? e0 : 0.0);
        }
    });
    if (ENERGY && lane == 0) Ewave[(size_t)r * waves + w] = E;
}

// u_kl partials, same grid: D[r][l][w] = sum over the central particle's sets of e(g_l) - e(g_own), the program unseeded, the difference
// formed per set, the batches added in their order by lane 0 alone; states whose globals equal the replica's own are skipped
__global__ __launch_bounds__(64)
void custom_manyparticle_ukl_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ types,
                                    const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                                    const double* __restrict__ glob, int ng, int K, const int* __restrict__ excl_off,
                                    const int* __restrict__ excl_atoms, const int64_t* __restrict__ labels, int r_begin, int Npad,
                                    const float4* __restrict__ pos, const float* __restrict__ box, int mp_rows, const int* __restrict__ nbr,
                                    const int* __restrict__ cnt, double* __restrict__ D)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[3];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ int row[MP_ROW];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int i = w - f.slot0 / 64;
    const int n = mp_load_row(f, i, r, lane, mp_rows, nbr, cnt, row);
    const bool central = f.mp_mode == 0 || ((f.mp_filter[0] >> types[f.mp_types0 + i]) & 1u);
    if (lane == 0)
        for (int l = 0; l < K; ++l) D[((size_t)r * K + l) * waves + w] = central && n > MP_ROW ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
    if (n < 2 || n > MP_ROW || !central) return;
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;
    const bool pbc = f.periodic != 0;
    const double bx = box[4 * r], by = box[4 * r + 1], bz = box[4 * r + 2];
    const double Lx = pbc ? bx : 0.0, Ly = pbc ? by : 0.0, Lz = pbc ? bz : 0.0;
    const double* g_own = glob + (size_t)labels[r_begin + r] * ng;
    const float4* P = pos + (size_t)r * Npad;
    mp_sets(f, i, n, lane, pbc, bx, by, bz, P, types, excl_off, excl_atoms, row, queue, [&](int entry, bool on) {
        mp_stage(f, i, entry, row, lane, P, par, Npad, X, PAR);
        double e_own = 0.0;
        for (int l = -1; l < K; ++l) {
            const double* g = l < 0 ? g_own : glob + (size_t)l * ng;
            bool same = l >= 0;
            for (int c = 0; c < ng && same; ++c) same = g[c] == g_own[c];
            if (same) continue;
            const double e = cst_eval<true>(fl, prog, consts, &PAR[0][0], lane, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, -1).v;
            if (l < 0) { e_own = e; continue; }
            const double d = cst_wave_sum(on ? e - e_own : 0.0);
            if (lane == 0) D[((size_t)r * K + l) * waves + w] += d;
        }
    });
}

// energy parameter derivatives, same grid behind the same neighbour rows: D[r][d][w] = sum over the central particle's sets of
// dE/dglobal(dcols[d]) under the replica's own globals; a row over capacity gives NaN in every column the force declared.
// STATES: under the globals of every state l in turn, D[r][l][d][w] (the NaN at every l); the row, the sets and each batch's staging
// run once, the states loop inside a batch, so a (state, column)'s batches are added in the order of the own-state kernel
template <bool STATES>
__global__ __launch_bounds__(64)
void custom_manyparticle_dpar_kernel(int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ types,
                                     const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                                     const double* __restrict__ glob, int ng, int nd, const int* __restrict__ dcols,
                                     const unsigned* __restrict__ dmask, const int* __restrict__ excl_off, const int* __restrict__ excl_atoms,
                                     const int64_t* __restrict__ labels, int r_begin, int Npad, const float4* __restrict__ pos,
                                     const float* __restrict__ box, int mp_rows, const int* __restrict__ nbr, const int* __restrict__ cnt,
                                     double* __restrict__ D, int K)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[3];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ int row[MP_ROW];
    __shared__ int queue[128];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const unsigned mask = dmask[wave_force[w]];
    const int i = w - f.slot0 / 64;
    const int n = mp_load_row(f, i, r, lane, mp_rows, nbr, cnt, row);
    const bool central = f.mp_mode == 0 || ((f.mp_filter[0] >> types[f.mp_types0 + i]) & 1u);
    const int nl = STATES ? K : 1;
    if (lane == 0)
        for (int l = 0; l < nl; ++l)
            for (int d = 0; d < nd; ++d)
                D[(((size_t)r * nl + l) * nd + d) * waves + w] = central && n > MP_ROW && ((mask >> d) & 1u) ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
    if (n < 2 || n > MP_ROW || !central || mask == 0u) return;     // (wave-uniform)
    cst_force fl = f; fl.par0 = 0; fl.npad = 64;
    const bool pbc = f.periodic != 0;
    const double bx = box[4 * r], by = box[4 * r + 1], bz = box[4 * r + 2];
    const double Lx = pbc ? bx : 0.0, Ly = pbc ? by : 0.0, Lz = pbc ? bz : 0.0;
    const float4* P = pos + (size_t)r * Npad;
    mp_sets(f, i, n, lane, pbc, bx, by, bz, P, types, excl_off, excl_atoms, row, queue, [&](int entry, bool on) {
        mp_stage(f, i, entry, row, lane, P, par, Npad, X, PAR);
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

// the neighbour rows of every many-particle force of the handle, on `st`
void mp_neighbours(remd_ctx* h, cst_tables& t, hipStream_t st)
{
    for (int i = 0; i < t.nf; ++i)
        if (t.F[i].kind == REMD_CUSTOM_MANYPARTICLE)
            hipLaunchKernelGGL(custom_mp_neighbours_kernel, dim3(h->Npad / 64, h->R), dim3(64), 0, st, i, t.d_F, t.d_excl_off, t.d_excl_atoms, h->Npad,
                               h->d_pos, h->d_box, t.mp_rows, t.d_mp_nbr, t.d_mp_cnt);
}

}  // namespace

void remd_custom_manyparticle_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_MANYPARTICLE);
    mp_neighbours(h, t, st);
    if (with_energy)
        hipLaunchKernelGGL(custom_manyparticle_kernel<true>, dim3(t.end(CST_MANYPARTICLE) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force,
                           t.d_mp_types, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                           h->d_pos, h->d_box, t.mp_rows, t.d_mp_nbr, t.d_mp_cnt, h->d_force, t.d_Ewave);
    else
        hipLaunchKernelGGL(custom_manyparticle_kernel<false>, dim3(t.end(CST_MANYPARTICLE) - w0, h->R), dim3(64), 0, st, w0, waves, t.d_F, t.d_wave_force,
                           t.d_mp_types, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                           h->d_pos, h->d_box, t.mp_rows, t.d_mp_nbr, t.d_mp_cnt, h->d_force, t.d_Ewave);
}

void remd_custom_manyparticle_ukl(remd_ctx* h, cst_tables& t)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_MANYPARTICLE);
    mp_neighbours(h, t, h->stream);                          // (the rows of the positions this launch sees, whatever an earlier launch left)
    hipLaunchKernelGGL(custom_manyparticle_ukl_kernel, dim3(t.end(CST_MANYPARTICLE) - w0, h->R), dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force,
                       t.d_mp_types, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->K, t.d_excl_off, t.d_excl_atoms, h->d_labels, h->r_begin, h->Npad,
                       h->d_pos, h->d_box, t.mp_rows, t.d_mp_nbr, t.d_mp_cnt, t.d_D);
}

// (the caller has sized the rows: ensure_buffers of custom_terms.hip)
void remd_custom_manyparticle_dpar(remd_ctx* h, cst_tables& t, bool states)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_MANYPARTICLE);
    mp_neighbours(h, t, h->stream);
    const dim3 grid(t.end(CST_MANYPARTICLE) - w0, h->R);
    if (states)
        hipLaunchKernelGGL(custom_manyparticle_dpar_kernel<true>, grid, dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force,
                           t.d_mp_types, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, t.d_excl_off, t.d_excl_atoms,
                           h->d_labels, h->r_begin, h->Npad, h->d_pos, h->d_box, t.mp_rows, t.d_mp_nbr, t.d_mp_cnt, t.d_dDK, h->K);
    else
        hipLaunchKernelGGL(custom_manyparticle_dpar_kernel<false>, grid, dim3(64), 0, h->stream, w0, waves, t.d_F, t.d_wave_force,
                           t.d_mp_types, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, t.d_excl_off, t.d_excl_atoms,
                           h->d_labels, h->r_begin, h->Npad, h->d_pos, h->d_box, t.mp_rows, t.d_mp_nbr, t.d_mp_cnt, t.d_dD, 1);
}

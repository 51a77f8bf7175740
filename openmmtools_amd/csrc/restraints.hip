// Receptor-ligand restraints (include/remd_hip_restraints.h): the radially symmetric restraints of openmmtools/forces.py:234-1108 --
// an energy of the distance between the mass-weighted centroids of two groups of atoms, scaled by the controlling global parameter
// (lambda_restraints) of the replica's state.
//
// One workgroup per replica walks the handle's restraints in order (a system carries one or two).  Per restraint: both centroids in
// f64 (centroid_sum.h, shared with custom_centroid.hip), each thread summing its strided share of a group's atoms, then a xor-shuffle
// tree inside each wavefront and the four wavefronts' sums added in a fixed order -- no atomics touch a centroid, the result does not
// depend on scheduling.  Atom positions enter relative to the group's first atom (minimum image under the replica's own box when the
// force is periodic): a group whose molecules the barostat wrapped one by one keeps its centroid.  Each atom then gets its share
//   F_i = -/+ lambda_own dE/dr (w_i) d / r        (d = centroid 2 - centroid 1, w_i = m_i / M_group)
// through the fixed-point force accumulators; lambda_own E goes to the replica's energy partial (the potential, the barostat and
// the minimiser see it) and the unscaled E to a [R][n] buffer the u_kl rows read.
#include "remd_internal.h"
#include "listed_terms.h"
#include "centroid_sum.h"
#include "../../include/remd_hip_restraints.h"

namespace {

struct rst_param {
    int kind, periodic;
    int b1, n1, b2, n2;          // offsets / counts in the atom and weight tables
    double K, r0;
};

}  // namespace

struct rst_tables {
    int n = 0, K = 0; long long lam_version = -1;     // (lam belongs to the states of that remd_set_states)
    std::vector<rst_param> par; std::vector<int> atoms; std::vector<double> w; std::vector<double> lam;   // host copies (clones)
    dev_array<rst_param> d_par; dev_array<int> d_atoms; dev_array<double> d_w; dev_array<double> d_lam;
    dev_array<double> d_E;             // [R][n]
};
void remd_table_deleter::operator()(rst_tables* t) const { delete t; }

namespace {

template <bool ENERGY>
__global__ __launch_bounds__(256)
void restraint_kernel(int n, const rst_param* __restrict__ par, const int* __restrict__ atoms, const double* __restrict__ w,
                      const double* __restrict__ lam /*[K][n]*/, const int64_t* __restrict__ labels, int r_begin, int Npad,
                      const float4* __restrict__ pos, const float* __restrict__ box, long long* __restrict__ force,
                      double* __restrict__ E_out /*[R][n]*/, double* __restrict__ epart, int n_epart, int ep_slot)
{
    __shared__ double s[3][4];
    const int r = blockIdx.x;
    const float4* P = pos + (size_t)r * Npad;
    long long* F = force + (size_t)r * 3 * Npad;
    const int own = (int)labels[r_begin + r];
    const double Lx = box[4 * r], Ly = box[4 * r + 1], Lz = box[4 * r + 2];
    double e_scaled = 0.0;
    for (int i = 0; i < n; ++i) {
        const rst_param p = par[i];
        const bool pbc = p.periodic != 0;
        const double3 c1 = centroid<256>(P, atoms, w, p.b1, p.n1, pbc, Lx, Ly, Lz, s);
        const double3 c2 = centroid<256>(P, atoms, w, p.b2, p.n2, pbc, Lx, Ly, Lz, s);
        double dx = c2.x - c1.x, dy = c2.y - c1.y, dz = c2.z - c1.z;
        if (pbc) { dx = min_image(dx, Lx); dy = min_image(dy, Ly); dz = min_image(dz, Lz); }
        const double rr = sqrt(dx * dx + dy * dy + dz * dz);
        double E, g;                                   // g = (dE/dr) / r
        if (p.kind == REMD_RESTRAINT_HARMONIC) {
            E = 0.5 * p.K * rr * rr; g = p.K;
        } else {
            const double x = rr - p.r0;
            const double st = x >= 0.0 ? 1.0 : 0.0;    // OpenMM's step(x): 1 at x = 0
            E = st * 0.5 * p.K * x * x;
            g = (x > 0.0 && rr > 0.0) ? p.K * x / rr : 0.0;
        }
        const double l = lam[(size_t)own * n + i];
        const double fx = -l * g * dx, fy = -l * g * dy, fz = -l * g * dz;   // force on centroid 2 (centroid 1: the opposite)
        for (int k = threadIdx.x; k < p.n1; k += 256) {
            const double wk = w[p.b1 + k];
            add_force(F, Npad, atoms[p.b1 + k], (float)(-fx * wk), (float)(-fy * wk), (float)(-fz * wk));
        }
        for (int k = threadIdx.x; k < p.n2; k += 256) {
            const double wk = w[p.b2 + k];
            add_force(F, Npad, atoms[p.b2 + k], (float)(fx * wk), (float)(fy * wk), (float)(fz * wk));
        }
        if (threadIdx.x == 0) E_out[(size_t)r * n + i] = E;
        e_scaled += l * E;
    }
    if (ENERGY && threadIdx.x == 0) epart[(size_t)r * n_epart + ep_slot] = e_scaled;
}

// u_kl column l of replica r: + beta_l (lambda_l - lambda_own) E_r, summed over the restraints
__global__ void restraint_ukl_kernel(int R, int K, int n, const double* __restrict__ lam, const double* __restrict__ E,
                                     const double* __restrict__ beta, const int64_t* __restrict__ labels, int r_begin,
                                     double* __restrict__ rows)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * K) return;
    const int r = t / K, l = t % K;
    const int own = (int)labels[r_begin + r];
    double d = 0.0;
    for (int i = 0; i < n; ++i) d += (lam[(size_t)l * n + i] - lam[(size_t)own * n + i]) * E[(size_t)r * n + i];
    rows[t] += beta[l] * d;
}

int ensure_E(remd_ctx* h, rst_tables& t)
{
    if (t.d_E.size() == (size_t)h->R * t.n) return 0;
    REMD_TRY(t.d_E.alloc(h, (size_t)h->R * t.n));
    REMD_CHECK(h, hipMemset(t.d_E, 0, sizeof(double) * (size_t)h->R * t.n));
    return 0;
}

int set_tables(remd_ctx* h, rst_tables& t)
{
    int rc;
    if ((rc = t.d_par.upload(h, t.par)) || (rc = t.d_atoms.upload(h, t.atoms)) || (rc = t.d_w.upload(h, t.w)) ||
        (rc = t.d_lam.upload(h, t.lam))) return rc;
    t.d_E.reset();
    return 0;
}

}  // namespace

void remd_restraints_release(remd_ctx* h)
{
    if (h->rst) { hipStreamSynchronize(h->stream); h->rst.reset(); }
    h->n_restraints = 0; h->rst_group = 0;
}

int remd_restraints_clone(remd_ctx* parent, remd_ctx* child)
{
    const rst_tables* t = parent->rst.get();
    if (!t || parent->n_restraints == 0) return 0;
    child->rst.reset(new rst_tables());
    rst_tables& c = *child->rst;
    c.n = t->n; c.K = t->K; c.lam_version = t->lam_version == parent->states_version ? child->states_version : -1; c.par = t->par; c.atoms = t->atoms; c.w = t->w; c.lam = t->lam;
    hipSetDevice(child->device);
    const int rc = set_tables(child, c);
    if (rc) return remd_fail(parent, rc, std::string("phases: ") + child->err);
    child->n_restraints = parent->n_restraints; child->rst_group = parent->rst_group;
    child->config_version++;
    return 0;
}

// the restraint launch of a force evaluation (forces.hip: on the stream of the listed terms)
int remd_restraints_forces(remd_ctx* h, bool with_energy, int ep_slot, hipStream_t st)
{
    rst_tables* tp = h->rst.get();
    if (!tp || h->n_restraints == 0) return 0;
    rst_tables& t = *tp;
    if (t.K != h->K || t.lam_version != h->states_version)
        return remd_fail(h, -1, "restraints: the states changed since remd_set_restraint_lambdas (call it after remd_set_states)");
    int rc = ensure_E(h, t); if (rc) return rc;
    remd_prof_scope ps(h, "restraints", st);
    if (with_energy)
        hipLaunchKernelGGL(restraint_kernel<true>, dim3(h->R), dim3(256), 0, st, t.n, t.d_par, t.d_atoms, t.d_w, t.d_lam, h->d_labels,
                           h->r_begin, h->Npad, h->d_pos, h->d_box, h->d_force, t.d_E, h->d_epart, h->n_epart, ep_slot);
    else
        hipLaunchKernelGGL(restraint_kernel<false>, dim3(h->R), dim3(256), 0, st, t.n, t.d_par, t.d_atoms, t.d_w, t.d_lam, h->d_labels,
                           h->r_begin, h->Npad, h->d_pos, h->d_box, h->d_force, t.d_E, h->d_epart, h->n_epart, ep_slot);
    return 0;
}

// the restraints' share of the u_kl rows, added to what the assembly wrote (behind the energy evaluation on the main stream)
int remd_restraints_ukl(remd_ctx* h, double* d_rows)
{
    rst_tables* tp = h->rst.get();
    if (!tp || h->n_restraints == 0) return 0;
    rst_tables& t = *tp;
    if (t.K != h->K || t.lam_version != h->states_version || t.d_E.size() != (size_t)h->R * t.n) return remd_fail(h, -1, "restraints: u_kl without a current energy evaluation");
    const int n = h->R * h->K;
    hipLaunchKernelGGL(restraint_ukl_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->R, h->K, t.n, t.d_lam, t.d_E, h->d_beta,
                       h->d_labels, h->r_begin, d_rows);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

extern "C" {

int remd_set_restraints(remd_handle h, const remd_restraint_desc* desc, int n)
{
    if (!h || n < 0 || (n > 0 && !desc)) return remd_fail(h, -1, "remd_set_restraints: bad arguments");
    if (!h->has_system) return remd_fail(h, -1, "remd_set_restraints: call remd_set_system first");
    hipSetDevice(h->device);
    remd_restraints_release(h);
    h->config_version++;
    if (n == 0) return 0;
    rst_tables t;
    t.n = n;
    for (int i = 0; i < n; ++i) {
        const remd_restraint_desc& d = desc[i];
        if (d.kind != REMD_RESTRAINT_HARMONIC && d.kind != REMD_RESTRAINT_FLAT_BOTTOM) return remd_fail(h, -1, "remd_set_restraints: unknown kind");
        if (!(d.K >= 0.0) || !(d.r0 >= 0.0) || d.n1 <= 0 || d.n2 <= 0 || !d.atoms1 || !d.atoms2)
            return remd_fail(h, -1, "remd_set_restraints: K, r0 >= 0 and two non-empty groups are required");
        if (d.force_group != desc[0].force_group || d.force_group < 0 || d.force_group > 31)
            return remd_fail(h, -1, "remd_set_restraints: every restraint of a handle must sit in one force group (0 ... 31)");
        rst_param p{};
        p.kind = d.kind; p.periodic = d.periodic ? 1 : 0; p.K = d.K; p.r0 = d.r0;
        for (int g = 0; g < 2; ++g) {
            const int m = g ? d.n2 : d.n1;
            const int32_t* a = g ? d.atoms2 : d.atoms1;
            const double* wt = g ? d.weights2 : d.weights1;
            const int b = (int)t.atoms.size();
            double W = 0.0;
            for (int k = 0; k < m; ++k) {
                if (a[k] < 0 || a[k] >= h->N) return remd_fail(h, -1, "remd_set_restraints: atom index out of range");
                double wk;
                if (wt) wk = wt[k];
                else if (h->sysdesc && h->sysdesc->valid) wk = h->sysdesc->d.mass[a[k]];
                else return remd_fail(h, -1, "remd_set_restraints: weights are required");
                if (!(wk >= 0.0)) return remd_fail(h, -1, "remd_set_restraints: negative weight");
                t.atoms.push_back(a[k]); t.w.push_back(wk); W += wk;
            }
            if (!(W > 0.0)) return remd_fail(h, -1, "remd_set_restraints: a group's weights sum to zero");
            for (int k = 0; k < m; ++k) t.w[b + k] /= W;
            if (g) { p.b2 = b; p.n2 = m; } else { p.b1 = b; p.n1 = m; }
        }
        t.par.push_back(p);
    }
    t.K = h->K; t.lam_version = h->states_version;
    t.lam.assign((size_t)std::max(h->K, 0) * n, 1.0);
    int rc = set_tables(h, t);
    if (rc) return rc;
    h->rst.reset(new rst_tables(std::move(t)));
    h->n_restraints = n; h->rst_group = desc[0].force_group;
    return 0;
}

int remd_set_restraint_lambdas(remd_handle h, const double* lambda)
{
    if (!h || !lambda) return remd_fail(h, -1, "remd_set_restraint_lambdas: bad arguments");
    rst_tables* t = h->rst.get();
    if (!t || h->n_restraints == 0) return remd_fail(h, -1, "remd_set_restraint_lambdas: no restraints (remd_set_restraints)");
    if (h->K <= 0) return remd_fail(h, -1, "remd_set_restraint_lambdas: call remd_set_states first");
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    t->K = h->K; t->lam_version = h->states_version;
    t->lam.assign(lambda, lambda + (size_t)h->K * t->n);
    int rc = t->d_lam.upload(h, t->lam);
    if (rc) return rc;
    h->config_version++;
    return 0;
}

int remd_get_restraint_energies(remd_handle h, double* out)
{
    if (!h || !out || h->R <= 0) return remd_fail(h, -1, "remd_get_restraint_energies: bad arguments");
    rst_tables* t = h->rst.get();
    if (!t || h->n_restraints == 0) return remd_fail(h, -1, "remd_get_restraint_energies: no restraints (remd_set_restraints)");
    hipSetDevice(h->device);
    int rc = remd_compute_forces(h, true); if (rc) return rc;
    REMD_CHECK(h, hipMemcpyAsync(out, t->d_E, sizeof(double) * (size_t)h->R * t->n, hipMemcpyDeviceToHost, h->stream));
    REMD_CHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"

// Virtual sites (include/remd_hip_vsites.h): massless particles placed from two or three parents, and the force on them handed to
// the parents.  Two launches around the evaluation and the integrator, only for a handle that holds sites:
//   vsite_place_kernel   one lane per (site, replica): the parents' f32 positions, the site in f64, stored rounded once;
//   vsite_spread_kernel  one lane per (site, replica): the site's fixed-point force words, the chain-rule share of each parent added
//                        through add_force (integer atomics: order-independent, bit-reproducible), then zero in the site's words.
// The integrator never sees a site: remd_build_constraints (integrate.hip) leaves massless particles out of the constraint units, so
// the chain, the velocity assignment and FIRE neither move nor kick them, and their velocity stays the zero it was set to.
#include "remd_internal.h"
#include "listed_terms.h"
#include "../../include/remd_hip_vsites.h"
#include <cmath>

struct vs_tables {
    int n = 0;
    dev_array<int4> d_atoms;           // [n] site, parent 0 .. 2 (an unused third parent repeats the first: never dereferenced out of range)
    dev_array<int> d_kind;             // [n] REMD_VSITE_*
    dev_array<double> d_weight;        // [n][3]
    std::vector<remd_vsite_desc> host; // for the blocks of a phased propagation
};
void remd_table_deleter::operator()(vs_tables* t) const { delete t; }

struct d3 { double x, y, z; };
__device__ __forceinline__ d3 ld3d(const float4* P, int i) { const float4 p = P[i]; return d3{ (double)p.x, (double)p.y, (double)p.z }; }
__device__ __forceinline__ d3 sub(const d3& a, const d3& b) { return d3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ d3 cross(const d3& a, const d3& b) { return d3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }

__global__ __launch_bounds__(256)
void vsite_place_kernel(int n, int R, int Npad, const int4* __restrict__ atoms, const int* __restrict__ kind,
                        const double* __restrict__ weight, float4* __restrict__ pos, float4* __restrict__ vel /*NULL: left alone*/)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n * R) return;
    const int r = (int)(gid / n), s = (int)(gid % n);
    const int4 a = atoms[s];
    const double w0 = weight[3 * s], w1 = weight[3 * s + 1], w2 = weight[3 * s + 2];
    float4* P = pos + (size_t)r * Npad;
    const d3 x1 = ld3d(P, a.y), x2 = ld3d(P, a.z);
    d3 x;
    const int k = kind[s];
    if (k == REMD_VSITE_TWO_AVERAGE) {
        x = d3{ w0 * x1.x + w1 * x2.x, w0 * x1.y + w1 * x2.y, w0 * x1.z + w1 * x2.z };
    } else {
        const d3 x3 = ld3d(P, a.w);
        if (k == REMD_VSITE_THREE_AVERAGE) {
            x = d3{ w0 * x1.x + w1 * x2.x + w2 * x3.x, w0 * x1.y + w1 * x2.y + w2 * x3.y, w0 * x1.z + w1 * x2.z + w2 * x3.z };
        } else {
            const d3 r12 = sub(x2, x1), r13 = sub(x3, x1), c = cross(r12, r13);
            x = d3{ x1.x + w0 * r12.x + w1 * r13.x + w2 * c.x, x1.y + w0 * r12.y + w1 * r13.y + w2 * c.y, x1.z + w0 * r12.z + w1 * r13.z + w2 * c.z };
        }
    }
    P[a.x] = make_float4((float)x.x, (float)x.y, (float)x.z, 0.f);
    if (vel) vel[(size_t)r * Npad + a.x] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256)
void vsite_spread_kernel(int n, int R, int Npad, const int4* __restrict__ atoms, const int* __restrict__ kind,
                         const double* __restrict__ weight, const float4* __restrict__ pos, long long* force)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n * R) return;
    const int r = (int)(gid / n), s = (int)(gid % n);
    const int4 a = atoms[s];
    const double w0 = weight[3 * s], w1 = weight[3 * s + 1], w2 = weight[3 * s + 2];
    long long* F = force + (size_t)r * 3 * Npad;
    // (no other lane of this launch touches a site's words: a parent is never a site)
    const double sc = 1.0 / REMD_FORCE_SCALE;
    const d3 f = d3{ (double)F[a.x] * sc, (double)F[Npad + a.x] * sc, (double)F[2 * Npad + a.x] * sc };
    F[a.x] = 0; F[Npad + a.x] = 0; F[2 * Npad + a.x] = 0;
    const int k = kind[s];
    if (k == REMD_VSITE_TWO_AVERAGE) {
        add_force(F, Npad, a.y, (float)(w0 * f.x), (float)(w0 * f.y), (float)(w0 * f.z));
        add_force(F, Npad, a.z, (float)(w1 * f.x), (float)(w1 * f.y), (float)(w1 * f.z));
    } else if (k == REMD_VSITE_THREE_AVERAGE) {
        add_force(F, Npad, a.y, (float)(w0 * f.x), (float)(w0 * f.y), (float)(w0 * f.z));
        add_force(F, Npad, a.z, (float)(w1 * f.x), (float)(w1 * f.y), (float)(w1 * f.z));
        add_force(F, Npad, a.w, (float)(w2 * f.x), (float)(w2 * f.y), (float)(w2 * f.z));
    } else {
        // x = x1 + w12 r12 + w13 r13 + wc (r12 x r13):  f2 = w12 f + wc (r13 x f),  f3 = w13 f + wc (f x r12),  f1 = f - f2 - f3
        const float4* P = pos + (size_t)r * Npad;
        const d3 x1 = ld3d(P, a.y), r12 = sub(ld3d(P, a.z), x1), r13 = sub(ld3d(P, a.w), x1);
        const d3 c2 = cross(r13, f), c3 = cross(f, r12);
        const d3 f2 = d3{ w0 * f.x + w2 * c2.x, w0 * f.y + w2 * c2.y, w0 * f.z + w2 * c2.z };
        const d3 f3 = d3{ w1 * f.x + w2 * c3.x, w1 * f.y + w2 * c3.y, w1 * f.z + w2 * c3.z };
        add_force(F, Npad, a.y, (float)(f.x - f2.x - f3.x), (float)(f.y - f2.y - f3.y), (float)(f.z - f2.z - f3.z));
        add_force(F, Npad, a.z, (float)f2.x, (float)f2.y, (float)f2.z);
        add_force(F, Npad, a.w, (float)f3.x, (float)f3.y, (float)f3.z);
    }
}

void remd_vsites_release(remd_ctx* h) { h->vs.reset(); h->n_vsites = 0; }

int remd_vsites_place(remd_ctx* h, hipStream_t st, bool zero_velocities)
{
    if (h->n_vsites <= 0 || h->R <= 0 || !h->d_pos) return 0;
    const vs_tables& t = *h->vs;
    remd_prof_scope ps(h, "vsite_place", st);
    const long long lanes = (long long)t.n * h->R;
    hipLaunchKernelGGL(vsite_place_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, t.n, h->R, h->Npad, t.d_atoms, t.d_kind,
                       t.d_weight, h->d_pos, zero_velocities ? h->d_vel.get() : (float4*)nullptr);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

int remd_vsites_spread(remd_ctx* h, hipStream_t st)
{
    if (h->n_vsites <= 0 || h->R <= 0 || !h->d_force) return 0;
    const vs_tables& t = *h->vs;
    remd_prof_scope ps(h, "vsite_spread", st);
    const long long lanes = (long long)t.n * h->R;
    hipLaunchKernelGGL(vsite_spread_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, t.n, h->R, h->Npad, t.d_atoms, t.d_kind,
                       t.d_weight, h->d_pos, h->d_force);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

// what the kernels index unchecked is checked here, against the masses of the descriptor of the last remd_set_system
static int vsites_install(remd_ctx* h, const remd_vsite_desc* sites, int n)
{
    const remd_desc_store* sd = h->parent ? h->parent->sysdesc.get() : h->sysdesc.get();
    if (!sd || !sd->valid || (int)sd->mass.size() != h->N) return remd_fail(h, -1, "remd_set_virtual_sites: call remd_set_system first");
    const std::vector<double>& mass = sd->mass;
    std::vector<char> is_site(h->N, 0);
    for (int s = 0; s < n; ++s) {
        const remd_vsite_desc& v = sites[s];
        if (v.kind < REMD_VSITE_TWO_AVERAGE || v.kind > REMD_VSITE_OUT_OF_PLANE) return remd_fail(h, -3, "remd_set_virtual_sites: unknown kind of site");
        if (v.site < 0 || v.site >= h->N) return remd_fail(h, -3, "remd_set_virtual_sites: site index out of range");
        if (mass[v.site] != 0.0) return remd_fail(h, -3, "remd_set_virtual_sites: a virtual site must have mass 0");
        if (is_site[v.site]) return remd_fail(h, -3, "remd_set_virtual_sites: a site is named twice");
        is_site[v.site] = 1;
        for (int k = 0; k < 3; ++k) if (!std::isfinite(v.weight[k])) return remd_fail(h, -3, "remd_set_virtual_sites: a weight is not finite");
    }
    std::vector<int4> atoms((size_t)n); std::vector<int> kind((size_t)n); std::vector<double> weight(3 * (size_t)n, 0.0);
    for (int s = 0; s < n; ++s) {
        const remd_vsite_desc& v = sites[s];
        const int np = v.kind == REMD_VSITE_TWO_AVERAGE ? 2 : 3;
        for (int k = 0; k < np; ++k) {
            const int p = v.parent[k];
            if (p < 0 || p >= h->N) return remd_fail(h, -3, "remd_set_virtual_sites: parent index out of range");
            if (is_site[p]) return remd_fail(h, -3, "remd_set_virtual_sites: a parent of a virtual site is itself a virtual site");
            if (!(mass[p] > 0.0)) return remd_fail(h, -3, "remd_set_virtual_sites: a parent of a virtual site is massless");
            for (int q = 0; q < k; ++q) if (v.parent[q] == p) return remd_fail(h, -3, "remd_set_virtual_sites: a parent is named twice");
        }
        atoms[s] = make_int4(v.site, v.parent[0], v.parent[1], np == 3 ? v.parent[2] : v.parent[0]);
        kind[s] = v.kind;
        for (int k = 0; k < np; ++k) weight[3 * (size_t)s + k] = v.weight[k];
    }
    std::unique_ptr<vs_tables, remd_table_deleter> t(new vs_tables());
    t->n = n;
    REMD_TRY(t->d_atoms.upload(h, atoms)); REMD_TRY(t->d_kind.upload(h, kind)); REMD_TRY(t->d_weight.upload(h, weight));
    t->host.assign(sites, sites + n);
    REMD_CHECK(h, hipStreamSynchronize(h->stream));      // (a table in use by launches still in flight)
    h->vs = std::move(t);
    h->n_vsites = n;
    return 0;
}

int remd_vsites_clone(remd_ctx* parent, remd_ctx* child)
{
    if (parent->n_vsites <= 0) return 0;
    const int rc = vsites_install(child, parent->vs->host.data(), parent->n_vsites);
    return rc ? remd_fail(parent, rc, std::string("phases: ") + child->err) : 0;
}

extern "C" int remd_set_virtual_sites(remd_handle h, const remd_vsite_desc* sites, int32_t n)
{
    if (!h || !h->has_system) return remd_fail(h, -1, "remd_set_virtual_sites: call remd_set_system first");
    if (n < 0 || (n > 0 && !sites)) return remd_fail(h, -1, "remd_set_virtual_sites: bad arguments");
    hipSetDevice(h->device);
    if (n == 0) { REMD_CHECK(h, hipStreamSynchronize(h->stream)); remd_vsites_release(h); h->config_version++; return 0; }
    REMD_TRY(vsites_install(h, sites, n));
    h->config_version++;
    h->forces_valid = false; h->force_zeroed = false; h->next.reset();
    // replicas that are already there follow the new table (sites placed, their velocities zero)
    REMD_TRY(remd_vsites_place(h, h->stream, true));
    REMD_CHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

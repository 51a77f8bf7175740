// Collective variables of stored frames (include/remd_hip_frame_cvs.h, remd_frame_cvs): the coordinates a free energy surface is taken
// over -- centroid distances, angles and dihedrals, and RMSDs -- at F stored frames, with the conventions of the force kernels
// (multistate/analysis.py: get_collective_variables hands the values to get_pmf).  Two kernels per chunk of frames, each issued only
// where the call has variables of its kind:
//
//  1. the centroid kinds, one wavefront per (frame, variable), four per 256-thread workgroup.  A frame is [n_atoms][3] packed f32:
//     lanes stride over a group's atoms, the centroid is the engine's own (centroid_sum.h: first atom + sum_i w_i img(x_i - x_first),
//     f64, xor-shuffle tree in a fixed order), the groups of the variable one after another.  The geometry -- restraint_kernel's
//     distance, cst_geometry's angle and dihedral (custom_terms.hip) -- is a few dozen f64 operations on wave-uniform data that every
//     lane runs; lane 0 stores.  No LDS, no barrier.
//  2. RMSD, one workgroup of 256 per (frame, variable): the two passes of custom_cv_superpose.h, the code of custom_cv_superpose_kernel.
//
// Nothing adds floating-point numbers atomically, and the order of every sum depends on the variable's own groups alone: a value is
// bit-identical from run to run, for every chunking, and whatever other variables share the call.  A lane beyond a group's end never
// enters the loops: it loads nothing and adds exact zeros to the tree.  Every index a lane follows was checked on the host.
#include "device_object.h"
#include "custom_cv_superpose.h"
#include "../../include/remd_hip_frame_cvs.h"
#include <cmath>

#define FCV_BLOCK            256
#define FCV_WAVES_PER_BLOCK  (FCV_BLOCK / 64)
#define FCV_CHUNK_BYTES      (int64_t(64) << 20)       // positions on the device per launch when the caller leaves the choice to us
#define FCV_MAX_GRID         int64_t(0x7fffffff)

namespace {

struct fcv_tables {                                    // device pointers
    int n_cv;
    const int* kind; const int* periodic; const int* cv_groups; const int* group_off; const int* atoms;
    const double* w; const double* ref;
};

__device__ __forceinline__ double3 fcv_diff(const double3& a, const double3& b, bool pbc, double Lx, double Ly, double Lz)
{
    double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    if (pbc) { dx = min_image(dx, Lx); dy = min_image(dy, Ly); dz = min_image(dz, Lz); }
    return make_double3(dx, dy, dz);
}
__device__ __forceinline__ double fcv_dot(const double3& a, const double3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double3 fcv_cross(const double3& a, const double3& b)
{
    return make_double3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// n_items = n frames x n_list variables of the centroid kinds (list[n_list]: their indices); one wavefront each
__global__ __launch_bounds__(FCV_BLOCK)
void frame_cvs_centroid_kernel(fcv_tables t, const int* __restrict__ list, int n_list, int64_t n_items, int n_atoms,
                               const float* __restrict__ pos /*[n][n_atoms][3]*/, const float* __restrict__ box /*[n][3] or NULL*/,
                               double* __restrict__ out /*[n][n_cv]*/)
{
    const int64_t item = (int64_t)blockIdx.x * FCV_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (item >= n_items) return;                         // (the whole wavefront: nothing below waits for another one)
    const int64_t f = item / n_list;
    const int cv = list[item - f * n_list];
    const int kind = t.kind[cv], g0 = t.cv_groups[cv];
    const float* P = pos + (size_t)f * 3 * (size_t)n_atoms;
    const bool pbc = box != nullptr && t.periodic[cv] != 0;
    double Lx = 0.0, Ly = 0.0, Lz = 0.0;
    if (pbc) { Lx = (double)box[3 * f]; Ly = (double)box[3 * f + 1]; Lz = (double)box[3 * f + 2]; }
    const int n_groups = kind + 2;                       // distance 2, angle 3, dihedral 4
    double3 c0, c1, c2 = make_double3(0.0, 0.0, 0.0), c3 = c2;
    { const int b = t.group_off[g0]; c0 = centroid_wave_xyz(P, t.atoms, t.w, b, t.group_off[g0 + 1] - b, pbc, Lx, Ly, Lz); }
    { const int b = t.group_off[g0 + 1]; c1 = centroid_wave_xyz(P, t.atoms, t.w, b, t.group_off[g0 + 2] - b, pbc, Lx, Ly, Lz); }
    if (n_groups > 2) { const int b = t.group_off[g0 + 2]; c2 = centroid_wave_xyz(P, t.atoms, t.w, b, t.group_off[g0 + 3] - b, pbc, Lx, Ly, Lz); }
    if (n_groups > 3) { const int b = t.group_off[g0 + 3]; c3 = centroid_wave_xyz(P, t.atoms, t.w, b, t.group_off[g0 + 4] - b, pbc, Lx, Ly, Lz); }
    double v;
    if (kind == REMD_FRAME_CV_DISTANCE) {
        const double3 d = fcv_diff(c1, c0, pbc, Lx, Ly, Lz);
        v = sqrt(fcv_dot(d, d));
    } else if (kind == REMD_FRAME_CV_ANGLE) {
        const double3 v0 = fcv_diff(c0, c1, pbc, Lx, Ly, Lz), v1 = fcv_diff(c2, c1, pbc, Lx, Ly, Lz);
        v = acos(fmin(fmax(fcv_dot(v0, v1) / sqrt(fcv_dot(v0, v0) * fcv_dot(v1, v1)), -1.0), 1.0));
    } else {
        const double3 b1 = fcv_diff(c1, c0, pbc, Lx, Ly, Lz), b2 = fcv_diff(c2, c1, pbc, Lx, Ly, Lz), b3 = fcv_diff(c3, c2, pbc, Lx, Ly, Lz);
        const double3 m = fcv_cross(b1, b2), nn = fcv_cross(b2, b3);
        v = atan2(sqrt(fcv_dot(b2, b2)) * fcv_dot(b1, nn), fcv_dot(m, nn));
    }
    if ((threadIdx.x & 63) == 0) out[(size_t)f * t.n_cv + cv] = v;
}

// a frame's positions as the superposition reads them
struct fcv_pos3 {
    const float* __restrict__ P;
    __device__ __forceinline__ void operator()(int a, float& x, float& y, float& z) const
    {
        const float* q = P + 3 * (size_t)a;
        x = q[0]; y = q[1]; z = q[2];
    }
};

// one workgroup per (frame, RMSD variable): block = frame * n_list + index into list
__global__ __launch_bounds__(CV_BLOCK)
void frame_cvs_rmsd_kernel(fcv_tables t, const int* __restrict__ list, int n_list, int n_atoms, const float* __restrict__ pos,
                           double* __restrict__ out /*[n][n_cv]*/)
{
    __shared__ double s[12][4];
    const int64_t f = (int64_t)blockIdx.x / n_list;
    const int cv = list[(int64_t)blockIdx.x - f * n_list];
    const int g = t.cv_groups[cv];
    const int b = t.group_off[g], n = t.group_off[g + 1] - b;
    const fcv_pos3 X{pos + (size_t)f * 3 * (size_t)n_atoms};
    cv_fit fit;
    cv_superpose_block(X, t.atoms, t.ref, b, n, s, fit);
    if (threadIdx.x == 0) {
        const double msd = fit.msd;
        const bool flat = !(msd >= CV_MSD_FLOOR);
        out[(size_t)f * t.n_cv + cv] = flat ? (msd != msd ? msd : 0.0) : sqrt(msd);
    }
}

int refuse(const std::string& msg) { return remd_fail(nullptr, -1, "remd_frame_cvs: " + msg); }

const int GROUPS_OF_KIND[4] = {2, 3, 4, 1};

}  // namespace

extern "C" {

int remd_frame_cvs(int device, int64_t F, int n_atoms, const float* pos, const float* box, const remd_frame_cv_tables* tables,
                   int64_t max_frames_per_launch, double* out, double* kernel_ms)
{
    // ---- everything is checked on the host before the device is touched ----
    if (!tables) return refuse("tables is NULL");
    if (F < 1) return refuse("F must be at least 1");
    if (n_atoms < 1) return refuse("n_atoms must be at least 1");
    if (!pos) return refuse("pos is NULL");
    if (!out) return refuse("out is NULL");
    const remd_frame_cv_tables& T = *tables;
    const int n_cv = T.n_cv;
    if (n_cv < 1) return refuse("no variable (n_cv must be at least 1)");
    if (!T.kind || !T.periodic || !T.cv_groups || !T.group_off || !T.atoms || !T.weights) return refuse("a NULL table");
    if (T.cv_groups[0] != 0 || T.group_off[0] != 0) return refuse("the offsets must start at 0");
    std::vector<int> c_list, r_list;
    bool any_periodic = false;
    for (int v = 0; v < n_cv; ++v) {
        const int k = T.kind[v];
        const std::string who = "variable " + std::to_string(v);
        if (k < 0 || k > 3) return refuse("unknown kind " + std::to_string(k) + " of " + who);
        if (T.cv_groups[v + 1] - T.cv_groups[v] != GROUPS_OF_KIND[k])
            return refuse(who + " of kind " + std::to_string(k) + " must have " + std::to_string(GROUPS_OF_KIND[k]) + " groups");
        for (int g = T.cv_groups[v]; g < T.cv_groups[v + 1]; ++g) {
            const int b = T.group_off[g], e = T.group_off[g + 1];
            if (e <= b) return refuse("an empty group in " + who + " (or offsets that do not ascend)");
            if (k == REMD_FRAME_CV_RMSD && e - b < 3) return refuse("the RMSD " + who + " needs at least 3 particles");
            if (k == REMD_FRAME_CV_RMSD && !T.reference) return refuse("the RMSD " + who + " has no reference");
            long double W = 0.0L;
            for (int i = b; i < e; ++i) {
                if (T.atoms[i] < 0 || T.atoms[i] >= n_atoms)
                    return refuse("atom index " + std::to_string(T.atoms[i]) + " of " + who + " is outside 0 ... n_atoms-1 = " + std::to_string(n_atoms - 1));
                if (k == REMD_FRAME_CV_RMSD) {
                    for (int c = 0; c < 3; ++c)
                        if (!std::isfinite(T.reference[3 * (size_t)i + c])) return refuse("a non-finite reference position in " + who);
                } else {
                    if (!(T.weights[i] >= 0.0) || !std::isfinite(T.weights[i])) return refuse("a negative or non-finite weight in " + who);
                    W += T.weights[i];
                }
            }
            if (k != REMD_FRAME_CV_RMSD && !(fabsl(W - 1.0L) <= 1e-9L)) return refuse("the weights of a group of " + who + " do not sum to 1");
        }
        if (k == REMD_FRAME_CV_RMSD) r_list.push_back(v);
        else { c_list.push_back(v); any_periodic = any_periodic || T.periodic[v] != 0; }
    }
    const bool use_box = box != nullptr && any_periodic;
    if (use_box)
        for (int64_t i = 0; i < 3 * F; ++i)
            if (!std::isfinite(box[i]) || !(box[i] > 0.0f))
                return refuse("frame " + std::to_string(i / 3) + " has a non-finite or non-positive box edge");
    const int n_groups = T.cv_groups[n_cv];
    const size_t n_entries = (size_t)T.group_off[n_groups];
    const int64_t frame_floats = 3 * (int64_t)n_atoms;
    int64_t chunk = max_frames_per_launch > 0 ? max_frames_per_launch : std::max<int64_t>(1, FCV_CHUNK_BYTES / (frame_floats * (int64_t)sizeof(float)));
    chunk = std::min(chunk, F);
    if (!c_list.empty()) chunk = std::min(chunk, FCV_MAX_GRID * FCV_WAVES_PER_BLOCK / (int64_t)c_list.size());   // (the grid of one launch)
    if (!r_list.empty()) chunk = std::min(chunk, FCV_MAX_GRID / (int64_t)r_list.size());
    chunk = std::max<int64_t>(chunk, 1);

    // ---- the device ----
    REMD_TRY(select_device("remd_frame_cvs", device));
    dev_array<int> d_kind, d_periodic, d_cv_groups, d_group_off, d_atoms, d_clist, d_rlist;
    dev_array<double> d_w, d_ref, d_out;
    dev_array<float> d_pos, d_box;
    REMD_TRY(d_kind.upload(nullptr, std::vector<int>(T.kind, T.kind + n_cv)));
    REMD_TRY(d_periodic.upload(nullptr, std::vector<int>(T.periodic, T.periodic + n_cv)));
    REMD_TRY(d_cv_groups.upload(nullptr, std::vector<int>(T.cv_groups, T.cv_groups + n_cv + 1)));
    REMD_TRY(d_group_off.upload(nullptr, std::vector<int>(T.group_off, T.group_off + n_groups + 1)));
    REMD_TRY(d_atoms.upload(nullptr, std::vector<int>(T.atoms, T.atoms + n_entries)));
    REMD_TRY(d_w.upload(nullptr, std::vector<double>(T.weights, T.weights + n_entries)));
    if (!r_list.empty()) {
        std::vector<double> ref(3 * n_entries, 0.0);     // (the rows of the centroid kinds are never read)
        for (int v : r_list) {
            const int g = T.cv_groups[v];
            for (size_t i = 3 * (size_t)T.group_off[g]; i < 3 * (size_t)T.group_off[g + 1]; ++i) ref[i] = T.reference[i];
        }
        REMD_TRY(d_ref.upload(nullptr, ref));
        REMD_TRY(d_rlist.upload(nullptr, r_list));
    }
    if (!c_list.empty()) REMD_TRY(d_clist.upload(nullptr, c_list));
    REMD_TRY(d_pos.alloc(nullptr, (size_t)(chunk * frame_floats)));
    if (use_box) REMD_TRY(d_box.alloc(nullptr, (size_t)(3 * chunk)));
    REMD_TRY(d_out.alloc(nullptr, (size_t)(chunk * n_cv)));
    device_timer tm;                                     // (after the arrays: it waits for its stream before they are freed)
    REMD_TRY(tm.open(device, false));
    fcv_tables t{};
    t.n_cv = n_cv; t.kind = d_kind.get(); t.periodic = d_periodic.get(); t.cv_groups = d_cv_groups.get(); t.group_off = d_group_off.get();
    t.atoms = d_atoms.get(); t.w = d_w.get(); t.ref = r_list.empty() ? nullptr : d_ref.get();
    for (int64_t f0 = 0; f0 < F; f0 += chunk) {
        const int64_t n = std::min(chunk, F - f0);
        DEVICE_CHECK(hipMemcpy(d_pos, pos + f0 * frame_floats, sizeof(float) * (size_t)(n * frame_floats), hipMemcpyHostToDevice));
        if (use_box) DEVICE_CHECK(hipMemcpy(d_box, box + 3 * f0, sizeof(float) * (size_t)(3 * n), hipMemcpyHostToDevice));
        REMD_TRY(tm.begin());
        if (!c_list.empty()) {
            const int64_t items = n * (int64_t)c_list.size();
            const unsigned blocks = (unsigned)((items + FCV_WAVES_PER_BLOCK - 1) / FCV_WAVES_PER_BLOCK);
            hipLaunchKernelGGL(frame_cvs_centroid_kernel, dim3(blocks), dim3(FCV_BLOCK), 0, tm.stream, t, d_clist.get(), (int)c_list.size(), items,
                               n_atoms, d_pos.get(), use_box ? d_box.get() : nullptr, d_out.get());
        }
        if (!r_list.empty())
            hipLaunchKernelGGL(frame_cvs_rmsd_kernel, dim3((unsigned)(n * (int64_t)r_list.size())), dim3(CV_BLOCK), 0, tm.stream, t, d_rlist.get(),
                               (int)r_list.size(), n_atoms, d_pos.get(), d_out.get());
        REMD_TRY(tm.end());
        DEVICE_CHECK(hipMemcpy(out + f0 * n_cv, d_out, sizeof(double) * (size_t)(n * n_cv), hipMemcpyDeviceToHost));
    }
    if (kernel_ms) *kernel_ms = tm.ms;
    return 0;
}

}  // extern "C"

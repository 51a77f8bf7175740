// The analysis pass over stored frames (include/remd_hip_restraints.h, remd_restraint_frames): the unscaled energy and the centroid
// distance of one radially symmetric restraint at F stored frames -- what the analyzer subtracts from u_ln to unbias the restraint
// (multistate/analysis.py, the reference's _compute_restraint_energies: a Python loop over iterations x replicas through a CPU Context).
//
// One wavefront per frame, four frames per 256-thread workgroup.  A frame is [n_atoms][3] packed f32, read once: lanes stride over
// a group's atoms, the centroid is the engine's own (centroid_sum.h: first atom + sum_i w_i img(x_i - x_first), f64, xor-shuffle tree in
// a fixed order, no atomics), the distance is imaged as restraint_kernel images it and the energy forms are restraint_kernel's.  A
// frame's result depends on that frame alone, so it does not depend on how the host cuts F into launches.  No LDS, no barrier.
#include "device_object.h"
#include "centroid_sum.h"
#include "../../include/remd_hip_restraints.h"
#include <cmath>

#define RSTF_BLOCK            256
#define RSTF_FRAMES_PER_BLOCK (RSTF_BLOCK / 64)
#define RSTF_CHUNK_BYTES      (int64_t(64) << 20)      // positions on the device per launch when the caller leaves the choice to us

namespace {

struct rstf_param {
    int kind, periodic, n1, n2;       // group 1: atoms[0 ... n1), group 2: atoms[n1 ... n1 + n2); w alike, each group normalised
    double K, r0;
};

__global__ __launch_bounds__(RSTF_BLOCK)
void restraint_frames_kernel(rstf_param p, const int* __restrict__ atoms, const double* __restrict__ w, int64_t F, int n_atoms,
                             const float* __restrict__ pos /*[F][n_atoms][3]*/, const float* __restrict__ box /*[F][3] or NULL*/,
                             double* __restrict__ E_out /*[F]*/, double* __restrict__ r_out /*[F]*/)
{
    const int64_t f = (int64_t)blockIdx.x * RSTF_FRAMES_PER_BLOCK + (threadIdx.x >> 6);
    if (f >= F) return;                                  // (the whole wavefront: nothing below waits for another one)
    const float* P = pos + (size_t)f * 3 * (size_t)n_atoms;
    const bool pbc = p.periodic != 0;
    double Lx = 0.0, Ly = 0.0, Lz = 0.0;
    if (pbc) { Lx = (double)box[3 * f]; Ly = (double)box[3 * f + 1]; Lz = (double)box[3 * f + 2]; }
    const double3 c1 = centroid_wave_xyz(P, atoms, w, 0, p.n1, pbc, Lx, Ly, Lz);
    const double3 c2 = centroid_wave_xyz(P, atoms, w, p.n1, p.n2, pbc, Lx, Ly, Lz);
    double dx = c2.x - c1.x, dy = c2.y - c1.y, dz = c2.z - c1.z;
    if (pbc) { dx = min_image(dx, Lx); dy = min_image(dy, Ly); dz = min_image(dz, Lz); }
    const double rr = sqrt(dx * dx + dy * dy + dz * dz);
    double E;
    if (p.kind == REMD_RESTRAINT_HARMONIC) {
        E = 0.5 * p.K * rr * rr;
    } else {
        const double x = rr - p.r0;
        const double st = x >= 0.0 ? 1.0 : 0.0;          // OpenMM's step(x): 1 at x = 0
        E = st * 0.5 * p.K * x * x;
    }
    if ((threadIdx.x & 63) == 0) { E_out[f] = E; r_out[f] = rr; }
}

double g_last_kernel_ms = -1.0;                         // the kernels of the last successful call (remd_restraint_frames_last_ms)

int refuse(const std::string& msg) { return remd_fail(nullptr, -1, "remd_restraint_frames: " + msg); }

}  // namespace

extern "C" {

int remd_restraint_frames(int device, const remd_restraint_desc* desc, int64_t F, int n_atoms, const float* pos, const float* box,
                          const double* masses, int64_t max_frames_per_launch, double* energy, double* distance)
{
    // ---- everything is checked on the host before the device is touched ----
    if (!desc) return refuse("desc is NULL");
    if (F < 1) return refuse("F must be at least 1");
    if (n_atoms < 1) return refuse("n_atoms must be at least 1");
    if (!pos) return refuse("pos is NULL");
    const remd_restraint_desc& d = *desc;
    if (d.kind != REMD_RESTRAINT_HARMONIC && d.kind != REMD_RESTRAINT_FLAT_BOTTOM) return refuse("unknown kind " + std::to_string(d.kind));
    if (!(d.K >= 0.0) || !(d.r0 >= 0.0)) return refuse("K and r0 must be >= 0");
    if (d.n1 <= 0 || d.n2 <= 0 || !d.atoms1 || !d.atoms2) return refuse("an empty group (two non-empty groups are required)");
    std::vector<int> atoms;
    std::vector<double> w;
    for (int g = 0; g < 2; ++g) {
        const int m = g ? d.n2 : d.n1;
        const int32_t* a = g ? d.atoms2 : d.atoms1;
        const double* wt = g ? d.weights2 : d.weights1;
        if (!wt && !masses) return refuse("group " + std::to_string(g + 1) + " has no weights and masses is NULL");
        const size_t b = atoms.size();
        long double W = 0.0L;
        for (int k = 0; k < m; ++k) {
            if (a[k] < 0 || a[k] >= n_atoms)
                return refuse("atom index " + std::to_string(a[k]) + " of group " + std::to_string(g + 1) + " is outside 0 ... n_atoms-1 = " + std::to_string(n_atoms - 1));
            const double wk = wt ? wt[k] : masses[a[k]];
            if (!(wk >= 0.0) || !std::isfinite(wk)) return refuse("a negative or non-finite weight in group " + std::to_string(g + 1));
            atoms.push_back(a[k]); w.push_back(wk); W += wk;
        }
        if (!(W > 0.0L)) return refuse("the weights of group " + std::to_string(g + 1) + " sum to zero");
        for (int k = 0; k < m; ++k) w[b + k] = (double)(w[b + k] / W);
    }
    const bool pbc = d.periodic != 0;
    if (pbc) {
        if (!box) return refuse("a periodic restraint needs box");
        for (int64_t i = 0; i < 3 * F; ++i)
            if (!std::isfinite(box[i]) || !(box[i] > 0.0f))
                return refuse("frame " + std::to_string(i / 3) + " has a non-finite or non-positive box edge");
    }
    const int64_t frame_floats = 3 * (int64_t)n_atoms;
    int64_t chunk = max_frames_per_launch > 0 ? max_frames_per_launch : std::max<int64_t>(1, RSTF_CHUNK_BYTES / (frame_floats * (int64_t)sizeof(float)));
    chunk = std::min(chunk, F);
    chunk = std::min<int64_t>(chunk, (int64_t)RSTF_FRAMES_PER_BLOCK * 0x7fffffff);          // (the grid of one launch)

    // ---- the device ----
    REMD_TRY(select_device("remd_restraint_frames", device));
    dev_array<int> d_atoms; dev_array<double> d_w, d_E, d_r; dev_array<float> d_pos, d_box;
    REMD_TRY(d_atoms.upload(nullptr, atoms));
    REMD_TRY(d_w.upload(nullptr, w));
    REMD_TRY(d_pos.alloc(nullptr, (size_t)(chunk * frame_floats)));
    if (pbc) REMD_TRY(d_box.alloc(nullptr, (size_t)(3 * chunk)));
    REMD_TRY(d_E.alloc(nullptr, (size_t)chunk));
    REMD_TRY(d_r.alloc(nullptr, (size_t)chunk));
    device_timer tm;                                     // (after the arrays: it waits for its stream before they are freed)
    REMD_TRY(tm.open(device, false));
    rstf_param p{};
    p.kind = d.kind; p.periodic = pbc ? 1 : 0; p.n1 = d.n1; p.n2 = d.n2; p.K = d.K; p.r0 = d.r0;
    for (int64_t f0 = 0; f0 < F; f0 += chunk) {
        const int64_t n = std::min(chunk, F - f0);
        DEVICE_CHECK(hipMemcpy(d_pos, pos + f0 * frame_floats, sizeof(float) * (size_t)(n * frame_floats), hipMemcpyHostToDevice));
        if (pbc) DEVICE_CHECK(hipMemcpy(d_box, box + 3 * f0, sizeof(float) * (size_t)(3 * n), hipMemcpyHostToDevice));
        const unsigned blocks = (unsigned)((n + RSTF_FRAMES_PER_BLOCK - 1) / RSTF_FRAMES_PER_BLOCK);
        REMD_TRY(tm.begin());
        hipLaunchKernelGGL(restraint_frames_kernel, dim3(blocks), dim3(RSTF_BLOCK), 0, tm.stream, p, d_atoms.get(), d_w.get(), n, n_atoms,
                           d_pos.get(), pbc ? d_box.get() : nullptr, d_E.get(), d_r.get());
        REMD_TRY(tm.end());
        if (energy) DEVICE_CHECK(hipMemcpy(energy + f0, d_E, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        if (distance) DEVICE_CHECK(hipMemcpy(distance + f0, d_r, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    }
    g_last_kernel_ms = tm.ms;
    return 0;
}

int remd_restraint_frames_last_ms(double* ms)
{
    if (!ms) return remd_fail(nullptr, -1, "remd_restraint_frames_last_ms: ms is NULL");
    if (g_last_kernel_ms < 0.0) return remd_fail(nullptr, -1, "remd_restraint_frames_last_ms: no call has completed yet");
    *ms = g_last_kernel_ms;
    return 0;
}

}  // extern "C"

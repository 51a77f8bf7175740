// The weighted centroid of a group of atoms, shared by restraints.hip (256 threads per workgroup) and custom_centroid.hip (64): each
// thread sums its strided share of the group's atoms in f64, then a xor-shuffle tree inside each wavefront, then the wavefronts'
// partials are added in a fixed order -- no atomics touch a centroid, the result depends on the input alone.  Atom positions enter
// relative to the group's first atom (minimum image under the replica's own box when the force is periodic): a group whose molecules
// the barostat wrapped one by one keeps its centroid.
#pragma once
#include "remd_internal.h"

namespace {

__device__ __forceinline__ double wave_sum_d(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup (BLOCK threads = 1 or 4 wavefronts) in a fixed order; every thread gets the result (s: [3][4] doubles of LDS,
// not read by a workgroup of one wavefront)
template <int BLOCK>
__device__ __forceinline__ double3 block_sum3(double3 v, double (*s)[4])
{
    static_assert(BLOCK == 64 || BLOCK == 256, "one or four wavefronts");
    v.x = wave_sum_d(v.x); v.y = wave_sum_d(v.y); v.z = wave_sum_d(v.z);
    if (BLOCK == 64) return v;
    const int wv = threadIdx.x >> 6;
    __syncthreads();                                  // (the previous call's readers are done with s)
    if ((threadIdx.x & 63) == 0) { s[0][wv] = v.x; s[1][wv] = v.y; s[2][wv] = v.z; }
    __syncthreads();
    return make_double3(((s[0][0] + s[0][1]) + s[0][2]) + s[0][3], ((s[1][0] + s[1][1]) + s[1][2]) + s[1][3],
                        ((s[2][0] + s[2][1]) + s[2][2]) + s[2][3]);
}

__device__ __forceinline__ double min_image(double d, double L) { return L > 0.0 ? d - L * rint(d / L) : d; }

// centroid of one group: first atom + sum_i w_i (x_i - x_first), the differences imaged when periodic
template <int BLOCK>
__device__ __forceinline__ double3 centroid(const float4* __restrict__ P, const int* __restrict__ atoms, const double* __restrict__ w,
                                            int b, int n, bool periodic, double Lx, double Ly, double Lz, double (*s)[4])
{
    const float4 a0 = P[atoms[b]];
    double3 acc = make_double3(0.0, 0.0, 0.0);
    for (int k = threadIdx.x; k < n; k += BLOCK) {
        const float4 q = P[atoms[b + k]];
        double dx = (double)q.x - (double)a0.x, dy = (double)q.y - (double)a0.y, dz = (double)q.z - (double)a0.z;
        if (periodic) { dx = min_image(dx, Lx); dy = min_image(dy, Ly); dz = min_image(dz, Lz); }
        const double wk = w[b + k];
        acc.x += wk * dx; acc.y += wk * dy; acc.z += wk * dz;
    }
    acc = block_sum3<BLOCK>(acc, s);
    return make_double3((double)a0.x + acc.x, (double)a0.y + acc.y, (double)a0.z + acc.z);
}

// the same centroid by ONE wavefront of a workgroup of any size, over packed xyz (restraint_frames.hip: one stored frame per wavefront,
// P the frame's [n_atoms][3] floats): lanes stride over the group's atoms, the xor-shuffle tree alone adds them -- no LDS, no barrier
__device__ __forceinline__ double3 centroid_wave_xyz(const float* __restrict__ P, const int* __restrict__ atoms, const double* __restrict__ w,
                                                     int b, int n, bool periodic, double Lx, double Ly, double Lz)
{
    const float* p0 = P + 3 * (size_t)atoms[b];
    const double x0 = (double)p0[0], y0 = (double)p0[1], z0 = (double)p0[2];
    double3 acc = make_double3(0.0, 0.0, 0.0);
    for (int k = threadIdx.x & 63; k < n; k += 64) {
        const float* q = P + 3 * (size_t)atoms[b + k];
        double dx = (double)q[0] - x0, dy = (double)q[1] - y0, dz = (double)q[2] - z0;
        if (periodic) { dx = min_image(dx, Lx); dy = min_image(dy, Ly); dz = min_image(dz, Lz); }
        const double wk = w[b + k];
        acc.x += wk * dx; acc.y += wk * dy; acc.z += wk * dz;
    }
    return make_double3(x0 + wave_sum_d(acc.x), y0 + wave_sum_d(acc.y), z0 + wave_sum_d(acc.z));
}

}  // namespace

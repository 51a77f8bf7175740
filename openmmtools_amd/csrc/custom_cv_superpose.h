// The two passes of an RMSD by one workgroup of 256 threads, shared by custom_cv.hip (the force, positions as float4 per replica) and
// frame_cvs.hip (stored frames, packed xyz): every thread sums its strided share of the particles in f64, from the f32 positions taken
// relative to the FIRST particle -- the centroid and the 3 x 3 correlation with the centred reference, twelve sums (a xor-shuffle
// tree per wavefront, the four wavefronts added in order) -- then the rotation of custom_cv_math.h on wave-uniform data in every
// lane, then the deviation |x_i - c - U ref_i|^2 summed directly.  No atomics: the result depends on the input alone.
#pragma once
#include "centroid_sum.h"
#include "custom_cv_math.h"

namespace {

constexpr int CV_BLOCK = 256;
constexpr double CV_MSD_FLOOR = 1e-20;

// N sums over the workgroup of four wavefronts in a fixed order; every thread gets the results (s: [N][4] doubles of LDS)
template <int N>
__device__ __forceinline__ void cv_block_sum(double (&v)[N], double (*s)[4])
{
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum_d(v[k]);
    const int wv = threadIdx.x >> 6;
    __syncthreads();                                  // (the previous call's readers are done with s)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k][wv] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((s[k][0] + s[k][1]) + s[k][2]) + s[k][3];
}

// what the superposition of one variable leaves in every thread
struct cv_fit {
    double msd;                      // the mean square deviation after the superposition
    float ax, ay, az;                // the first particle
    double cx, cy, cz;               // the centroid relative to it
    double U[3][3];
};

// the particles atoms[b ... b + n) at X(atom) -> x, y, z (f32) against ref[b ... b + n)[3]; s: [12][4] doubles of LDS
template <class POS>
__device__ __forceinline__ void cv_superpose_block(const POS& X, const int* __restrict__ atoms, const double* __restrict__ ref, int b, int n,
                                                   double (*s)[4], cv_fit& o)
{
    float ax, ay, az;
    X(atoms[b], ax, ay, az);
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (int k = threadIdx.x; k < n; k += CV_BLOCK) {
        float qx, qy, qz;
        X(atoms[b + k], qx, qy, qz);
        const double* y = ref + 3 * (size_t)(b + k);
        const double dx = (double)qx - (double)ax, dy = (double)qy - (double)ay, dz = (double)qz - (double)az;
        const double y0 = y[0], y1 = y[1], y2 = y[2];
        acc[0] += dx; acc[1] += dy; acc[2] += dz;
        acc[3] += dx * y0; acc[4] += dx * y1; acc[5] += dx * y2;
        acc[6] += dy * y0; acc[7] += dy * y1; acc[8] += dy * y2;
        acc[9] += dz * y0; acc[10] += dz * y1; acc[11] += dz * y2;
    }
    cv_block_sum<12>(acc, s);
    const double inv_n = 1.0 / (double)n;
    const double cx_ = acc[0] * inv_n, cy_ = acc[1] * inv_n, cz_ = acc[2] * inv_n;     // the centroid relative to the first particle
    const double S[3][3] = {{acc[3], acc[4], acc[5]}, {acc[6], acc[7], acc[8]}, {acc[9], acc[10], acc[11]}};
    cv_superpose(S, o.U);
    double m[1] = {0.0};
    for (int k = threadIdx.x; k < n; k += CV_BLOCK) {
        float qx, qy, qz;
        X(atoms[b + k], qx, qy, qz);
        const double* y = ref + 3 * (size_t)(b + k);
        const double y0 = y[0], y1 = y[1], y2 = y[2];
        const double ex = ((double)qx - (double)ax) - cx_ - (o.U[0][0] * y0 + o.U[0][1] * y1 + o.U[0][2] * y2);
        const double ey = ((double)qy - (double)ay) - cy_ - (o.U[1][0] * y0 + o.U[1][1] * y1 + o.U[1][2] * y2);
        const double ez = ((double)qz - (double)az) - cz_ - (o.U[2][0] * y0 + o.U[2][1] * y1 + o.U[2][2] * y2);
        m[0] += ex * ex + ey * ey + ez * ez;
    }
    cv_block_sum<1>(m, s);
    o.msd = m[0] * inv_n;
    o.ax = ax; o.ay = ay; o.az = az;
    o.cx = cx_; o.cy = cy_; o.cz = cz_;
}

}  // namespace

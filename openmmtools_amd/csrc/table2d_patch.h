// The bicubic Hermite patch of a tabulated function of two arguments (include/remd_hip_custom.h: REMD_CX_TABLE2D), shared by the stack
// machine (custom_machine.h, which documents the discipline of its loads at cst_table1d) and by the CMAP kernel (cmap.hip, cmap_math.h).
//
// Plain C++ without a device call, so the same text compiles for the host (tests/test_cmap_cpu.py holds it to the tests' interpolant
// there, without a GPU).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define CST_FN __host__ __device__ __forceinline__
#else
#include <algorithm>
#define CST_FN inline
using std::min;
using std::max;
#endif

// One argument of REMD_CX_TABLE2D on its axis of n nodes over [lo, hi] with spacing h, by the rules of cst_table1d: the wrap of a
// periodic function, the range test in f64, then the patch index (clamped again) and the offset u = (t - min) / h - i in the patch.
// Returns whether the argument lies inside; `nan` whether it is a NaN (an infinite argument of a periodic function wraps to one).
CST_FN bool cst_table_axis(int n, double lo, double hi, double h, bool periodic, double x, int& i, double& u, bool& nan)
{
    const double L = hi - lo;
    const double w = x - L * floor((x - lo) / L);
    const double t = periodic ? (w < lo ? lo : w > hi ? hi : w) : x;
    const bool inside = t >= lo && t <= hi;
    const double s = inside ? (t - lo) / h : 0.0;
    i = min(max((int)s, 0), n - 2);
    u = s - (double)i;
    nan = t != t;
    return inside;
}

// REMD_CX_TABLE2D (include/remd_hip_custom.h): the bicubic Hermite patch of the block [nx, ny, xmin, xmax, ymin, ymax, periodic, 0],
// node[ny][nx][4] = (f, fx, fy, fxy), with its two partials kx = dF/dx, ky = dF/dy.  The sixteen terms are summed row by row: the two
// corners (j + b, i) and (j + b, i + 1) of a row are 64 contiguous bytes, one access of the memory system's granularity, and only
// their eight numbers are live beside the row's four sums -- sixteen loads in flight at once would not fit beside the stack machine's
// state in the nonbonded tile kernel.  Along x a row gives P = sum_a h0a(u) f_a + hx h1a(u) fx_a and Q, the same of (fy, fxy), with
// their u-derivatives; along y, F = sum_b h0b(w) P_b + hy h1b(w) Q_b.  A lane whose arguments are not both inside loads nothing and
// pushes 0, or NaN where either argument is a NaN (the discipline of cst_table1d, per argument).
CST_FN void cst_table2d(const double* __restrict__ B, double x, double y, double& v, double& kx, double& ky)
{
    const int nx = (int)B[0], ny = (int)B[1];                 // 2 ..., nx ny <= REMD_CUSTOM_MAX_TABLE_CELLS
    const double hx = (B[3] - B[2]) / (double)(nx - 1), hy = (B[5] - B[4]) / (double)(ny - 1);
    const bool periodic = B[6] != 0.0;
    int i, j; double u, w; bool nanx, nany;
    const bool inx = cst_table_axis(nx, B[2], B[3], hx, periodic, x, i, u, nanx);
    const bool iny = cst_table_axis(ny, B[4], B[5], hy, periodic, y, j, w, nany);
    v = nanx || nany ? __builtin_nan("") : 0.0; kx = 0.0; ky = 0.0;
    if (inx && iny) {
        const double u2 = u * u, u3 = u2 * u, w2 = w * w, w3 = w2 * w;
        // h00, h01, hx h10, hx h11 at u and their u-derivatives (the latter still to be divided by hx)
        const double a0 = 2.0 * u3 - 3.0 * u2 + 1.0, a1 = 3.0 * u2 - 2.0 * u3, a2 = hx * (u3 - 2.0 * u2 + u), a3 = hx * (u3 - u2);
        const double d0 = 6.0 * (u2 - u), d2 = hx * (3.0 * u2 - 4.0 * u + 1.0), d3 = hx * (3.0 * u2 - 2.0 * u);      // d1 = -d0
        double F = 0.0, Fu = 0.0, Fw = 0.0;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const double* __restrict__ c = B + 8 + 4 * ((j + b) * nx + i);        // (f, fx, fy, fxy) of corner i, then of corner i + 1
            const double P = a0 * c[0] + a1 * c[4] + a2 * c[1] + a3 * c[5], Q = a0 * c[2] + a1 * c[6] + a2 * c[3] + a3 * c[7];
            const double dP = d0 * (c[0] - c[4]) + d2 * c[1] + d3 * c[5], dQ = d0 * (c[2] - c[6]) + d2 * c[3] + d3 * c[7];
            const double e0 = b ? 3.0 * w2 - 2.0 * w3 : 2.0 * w3 - 3.0 * w2 + 1.0, e1 = hy * (b ? w3 - w2 : w3 - 2.0 * w2 + w);
            const double g0 = b ? -6.0 * (w2 - w) : 6.0 * (w2 - w), g1 = hy * (b ? 3.0 * w2 - 2.0 * w : 3.0 * w2 - 4.0 * w + 1.0);
            F += e0 * P + e1 * Q;
            Fu += e0 * dP + e1 * dQ;
            Fw += g0 * P + g1 * Q;
        }
        v = F; kx = Fu / hx; ky = Fw / hy;
    }
}

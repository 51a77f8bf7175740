// What the device objects that live without a remd_ctx share (mbar.hip, timeseries.hip, energy_store.hip, restraint_frames.hip): the
// fixed-order sums of a 256-thread workgroup, the check of a HIP call, the choice of the device, and the timed stream.
#pragma once
#include "remd_internal.h"

// np.max's NaN: it stays
__device__ __forceinline__ double nanmax(double m, double a) { return (a > m || a != a) ? a : m; }

// Both for a workgroup of 256 threads and in one fixed order: lanes by __shfl_down, then the four waves in wave order; every thread
// gets the result.  sh: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__device__ __forceinline__ double block_nanmax(double v, double* sh)
{
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_down(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return nanmax(nanmax(nanmax(sh[0], sh[1]), sh[2]), sh[3]);
}

#define DEVICE_CHECK(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return remd_hip_fail(nullptr, #expr, _e); } while (0)

// refuses where there is no device (-2) or no such device (-1), else makes `device` the current one
inline int select_device(const char* who, int device)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return remd_fail(nullptr, -2, std::string(who) + ": no HIP device available (" + hipGetErrorString(e) + ")");
    if (device < 0 || device >= n) return remd_fail(nullptr, -1, std::string(who) + ": bad device index");
    DEVICE_CHECK(hipSetDevice(device));
    return 0;
}

// A stream and the two events that time the launches on it.  An object that owns device arrays declares its timer AFTER them: the
// destructor waits for the stream before the arrays are freed.
struct device_timer {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms = 0.0;
    // own_stream = false: the launches go to the null stream (a call that lives for one launch does not pay for a stream)
    int open(int dev, bool own_stream = true)
    {
        device = dev;
        if (own_stream) DEVICE_CHECK(hipStreamCreate(&stream));
        DEVICE_CHECK(hipEventCreate(&ev0));
        DEVICE_CHECK(hipEventCreate(&ev1));
        return 0;
    }
    int begin() { DEVICE_CHECK(hipEventRecord(ev0, stream)); return 0; }
    // waits for the launches since begin() and adds their time to ms
    int end()
    {
        DEVICE_CHECK(hipGetLastError());
        DEVICE_CHECK(hipEventRecord(ev1, stream));
        DEVICE_CHECK(hipStreamSynchronize(stream));
        float t = 0.0f;
        DEVICE_CHECK(hipEventElapsedTime(&t, ev0, ev1));
        ms += t;
        return 0;
    }
    ~device_timer()
    {
        hipSetDevice(device);
        hipStreamSynchronize(stream);
        if (stream) hipStreamDestroy(stream);
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
    }
};

// Single-view pseudo boxes (include/ov3d_liftview.h): every pixel of a frame whose class equals
// a 2D box's label, lifted through depth, pose and alignment.
//   3DOVDet_tools/scannet/lift_boxes.py with VIEW = 'single', utils/projection.py:242-251
// The lifted box depends on (frame, label) only, so the work goes by slots (distinct pairs) and
// a second launch copies every box's slot into its row.  Everything is float64; the file is
// built with -ffp-contract=off (Makefile), so a * b + c is two roundings as in numpy.  Min, max
// and integer counts are order-independent, so the result is deterministic whatever the
// reduction shape.
#include <float.h>
#include <limits.h>

#include "boxreduce.h"
#include "common.h"
#include "../../include/ov3d_liftview.h"

namespace {

constexpr int kViewThreads = 256;
static_assert(kViewThreads == kBoxThreads, "box_reduce_store reduces a workgroup of kBoxThreads");
constexpr int kViewUnroll = 4;          // label loads in flight per thread

__device__ __forceinline__ float depth_metres(const float* d, long long at) { return d[at]; }
// raw millimetres: the float32 quotient, correctly rounded (numpy's raw.astype(float32) / 1000)
__device__ __forceinline__ float depth_metres(const uint16_t* d, long long at) {
    return (float)d[at] / 1000.0f;
}

// One workgroup per slot streams the slot's label map; depth is read and a point computed for
// matching pixels only.  LDS: 7 * kBoxWaves doubles (224 B).
template <typename D>
__global__ void __launch_bounds__(kViewThreads)
liftview_slot_kernel(const D* __restrict__ depth, const int32_t* __restrict__ seg,
                     const int32_t* __restrict__ lut, int lut_n, long long ignore_from, int F,
                     int HW, int W, const double* __restrict__ kinv,
                     const double* __restrict__ pose, const double* __restrict__ align,
                     const int32_t* __restrict__ slot_frame,
                     const int32_t* __restrict__ slot_label, double* __restrict__ slot_lohi,
                     int32_t* __restrict__ slot_count) {
    __shared__ double red[7 * kBoxWaves];
    const int s = blockIdx.x;
    const int f = slot_frame[s], lab = slot_label[s];
    const int npix = (f >= 0 && f < F) ? HW : 0;      // uniform: a foreign frame holds no pixel
    const long long base = (long long)(npix ? f : 0) * HW;
    const double* R = pose + 12ll * (npix ? f : 0);
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    int n = 0;
    for (long long i0 = 0; i0 < npix; i0 += kViewUnroll * kViewThreads) {
        int sv[kViewUnroll];
#pragma unroll
        for (int k = 0; k < kViewUnroll; ++k) {
            const long long i = i0 + k * kViewThreads + threadIdx.x;
            sv[k] = i < npix ? seg[base + i] : 0;
        }
#pragma unroll
        for (int k = 0; k < kViewUnroll; ++k) {
            const long long at = i0 + k * kViewThreads + threadIdx.x;
            if (at >= npix) continue;
            const int i = (int)at;
            const int cls = lut ? ((sv[k] >= 0 && sv[k] < lut_n) ? lut[sv[k]] : -100)
                                : ((long long)sv[k] >= ignore_from ? -100 : sv[k]);
            if (cls != lab) continue;
            const int v = i / W, u = i - v * W;
            const double ud = (double)u, vd = (double)v;
            const double d = (double)depth_metres(depth, base + i);
            double c[3], w[3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                c[a] = ((kinv[3 * a] * ud + kinv[3 * a + 1] * vd) + kinv[3 * a + 2]) * d;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                w[a] = ((c[0] * R[3 * a] + c[1] * R[3 * a + 1]) + c[2] * R[3 * a + 2]) + R[9 + a];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double* m = align + 4 * a;
                const double p = ((m[0] * w[0] + m[1] * w[1]) + m[2] * w[2]) + m[3];
                lo[a] = fmin(lo[a], p);
                hi[a] = fmax(hi[a], p);
            }
            ++n;
        }
    }
    box_reduce_store(lo, hi, n, red, slot_lohi + 6ll * s, slot_count + s);   // n <= H * W < 2^31
}

// every 2D box takes the result of its slot: columns 0-5 of its row, and its count
__global__ void __launch_bounds__(kViewThreads)
liftview_spread_kernel(const int32_t* __restrict__ box_slot, int M, int S,
                       const double* __restrict__ slot_lohi, const int32_t* __restrict__ slot_count,
                       double* __restrict__ lohi, int ld, int32_t* __restrict__ count) {
    const int b = blockIdx.x * kViewThreads + threadIdx.x;
    if (b >= M) return;
    const int s = box_slot[b];
    const bool ok = s >= 0 && s < S;
    double* row = lohi + (long long)ld * b;
#pragma unroll
    for (int a = 0; a < 6; ++a) row[a] = ok ? slot_lohi[6ll * s + a] : 0.0;
    count[b] = ok ? slot_count[s] : 0;
}

}  // namespace

extern "C" int ov3d_liftview_frames(const void* depth, int depth_u16, const int32_t* seg,
                                    const int32_t* lut, int lut_n, long long ignore_from, int F,
                                    int H, int W, const double* kinv, const double* pose,
                                    const double* align, const int32_t* slot_frame,
                                    const int32_t* slot_label, int S, const int32_t* box_slot,
                                    int M, double* slot_lohi, int32_t* slot_count, double* lohi,
                                    int lohi_ld, int32_t* count, void* stream) {
    if (!depth || !seg || !kinv || !pose || !align || !slot_frame || !slot_label || !box_slot ||
        !slot_lohi || !slot_count || !lohi || !count || (depth_u16 != 0 && depth_u16 != 1) ||
        F < 1 || H < 1 || W < 1 || S < 1 || M < 1 || lohi_ld < 6 ||
        (long long)H * W > INT_MAX || (lut ? lut_n < 1 : lut_n != 0))
        return OV3D_EINVAL;
    const int HW = H * W;
    if (depth_u16)
        hipLaunchKernelGGL(liftview_slot_kernel<uint16_t>, dim3(S), dim3(kViewThreads), 0,
                           ov3d_stream(stream), static_cast<const uint16_t*>(depth), seg, lut, lut_n,
                           ignore_from, F, HW, W, kinv, pose, align, slot_frame, slot_label,
                           slot_lohi, slot_count);
    else
        hipLaunchKernelGGL(liftview_slot_kernel<float>, dim3(S), dim3(kViewThreads), 0,
                           ov3d_stream(stream), static_cast<const float*>(depth), seg, lut, lut_n,
                           ignore_from, F, HW, W, kinv, pose, align, slot_frame, slot_label,
                           slot_lohi, slot_count);
    hipLaunchKernelGGL(liftview_spread_kernel, dim3((M + kViewThreads - 1) / kViewThreads),
                       dim3(kViewThreads), 0, ov3d_stream(stream), box_slot, M, S, slot_lohi,
                       slot_count, lohi, lohi_ld, count);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

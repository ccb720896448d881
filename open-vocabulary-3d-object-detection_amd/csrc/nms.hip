// Greedy 3D NMS (float64), batched over scenes, gfx950.
//
// Replaces utils/nms.py:79-162 (nms_3d_faster, nms_3d_faster_samecls) as called
// once per scene on the host by utils/ap_calculator.py:153-190.
// One workgroup per scene:
//   1. rank sort by (score desc, index desc) -- the order of a stable ascending
//      argsort read from the back, i.e. the reference's pick order;
//   2. every thread builds one row of the K x K upper-triangular suppression
//      bitmask in LDS: bit (r,c) = IoU(order[r], order[c]) > thr (same class);
//      the IoU is evaluated exactly as the numpy reference does, picker first:
//      inter / ((area[i] + area[j]) - inter), no contraction;
//   3. one wave walks the rows in order, keeping a row iff its bit is not yet
//      removed and OR-ing its mask into the removed set (64-bit words on lanes).
// The result equals the reference greedy loop because the reference removes
// exactly the boxes whose overlap with an earlier pick exceeds thr.
//
// 512 < K <= 2048 (evaluation at more queries than the K x K mask has LDS for) runs
// nms3d_big_kernel: same rank sort, the rows stored in LDS in pick order, and the greedy
// walk itself tests the rows after each surviving pick (1024 threads, one barrier per pick)
// and ORs the suppressed ones into a removed-bitset; no K x K mask, no workspace.
// ov3d_eval_large_kernels(1) sends every K there (tests: bit-equal with the small kernel).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxK = 512;
constexpr int kWords = kMaxK / 64;
constexpr int kThreads = 512;

__device__ __forceinline__ double np_max(double a, double b) {
    return (isnan(a) || isnan(b)) ? __longlong_as_double(0x7ff8000000000000ll) : (a > b ? a : b);
}
__device__ __forceinline__ double np_min(double a, double b) {
    return (isnan(a) || isnan(b)) ? __longlong_as_double(0x7ff8000000000000ll) : (a < b ? a : b);
}

__global__ __launch_bounds__(kThreads) void nms3d_kernel(const double* __restrict__ boxes,
                                                         const uint8_t* __restrict__ valid, int K,
                                                         int stride, double thr, int old_type,
                                                         int samecls, uint8_t* __restrict__ keep) {
    __shared__ double s_box[kMaxK][8];  // x1,y1,z1,x2,y2,z2,area,cls
    __shared__ double s_score[kMaxK];
    __shared__ unsigned char s_valid[kMaxK];
    __shared__ int s_order[kMaxK];
    __shared__ unsigned long long s_mask[kMaxK][kWords];
    __shared__ int s_nvalid;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const double* bx = boxes + (size_t)b * K * stride;
    if (tid == 0) s_nvalid = 0;
    for (int i = tid; i < K; i += kThreads) {
        const double* p = bx + (size_t)i * stride;
        for (int a = 0; a < 6; ++a) s_box[i][a] = p[a];
        s_box[i][6] = (p[3] - p[0]) * (p[4] - p[1]) * (p[5] - p[2]);
        s_box[i][7] = samecls ? p[7] : 0.0;
        s_score[i] = p[6];
        s_valid[i] = valid ? (valid[(size_t)b * K + i] != 0) : 1;
        keep[(size_t)b * K + i] = 0;
    }
    __syncthreads();
    // 1. rank among valid boxes
    for (int i = tid; i < K; i += kThreads) {
        if (!s_valid[i]) continue;
        const double si = s_score[i];
        int r = 0;
        for (int j = 0; j < K; ++j) {
            if (!s_valid[j]) continue;
            const double sj = s_score[j];
            r += (sj > si) || (sj == si && j > i);
        }
        s_order[r] = i;
        atomicAdd(&s_nvalid, 1);
    }
    __syncthreads();
    const int nv = s_nvalid;
    const int nw = (nv + 63) / 64;
    // 2. suppression rows
    for (int r = tid; r < nv; r += kThreads) {
        const int i = s_order[r];
        const double ax1 = s_box[i][0], ay1 = s_box[i][1], az1 = s_box[i][2];
        const double ax2 = s_box[i][3], ay2 = s_box[i][4], az2 = s_box[i][5];
        const double area_i = s_box[i][6], cls_i = s_box[i][7];
        for (int w = 0; w < nw; ++w) {
            unsigned long long bits = 0ull;
            for (int q = 0; q < 64; ++q) {
                const int c = w * 64 + q;
                if (c <= r || c >= nv) continue;
                const int j = s_order[c];
                const double xx1 = np_max(ax1, s_box[j][0]), yy1 = np_max(ay1, s_box[j][1]),
                             zz1 = np_max(az1, s_box[j][2]);
                const double xx2 = np_min(ax2, s_box[j][3]), yy2 = np_min(ay2, s_box[j][4]),
                             zz2 = np_min(az2, s_box[j][5]);
                const double l = np_max(0.0, xx2 - xx1), wd = np_max(0.0, yy2 - yy1),
                             h = np_max(0.0, zz2 - zz1);
                double o;
                if (old_type) {
                    o = (l * wd * h) / s_box[j][6];
                } else {
                    const double inter = l * wd * h;
                    o = inter / (area_i + s_box[j][6] - inter);
                }
                if (samecls) o = o * (double)(cls_i == s_box[j][7]);
                if (o > thr) bits |= 1ull << q;
            }
            s_mask[r][w] = bits;
        }
    }
    __syncthreads();
    // 3. serial greedy walk by wave 0; lane w < nw holds removed-word w
    if (tid < 64) {
        unsigned long long removed = 0ull;
        for (int r = 0; r < nv; ++r) {
            const unsigned long long word = __shfl(removed, r >> 6);
            if ((word >> (r & 63)) & 1ull) continue;
            if (tid == 0) keep[(size_t)b * K + s_order[r]] = 1;
            if (tid < nw) removed |= s_mask[r][tid];
        }
    }
}

// ---- K <= 2048: rows in LDS in pick order, suppression tested during the walk ----
// LDS: 8 columns x 2048 doubles (128 KiB) + scores 16 KiB + order 4 KiB + flags 2 KiB +
// removed-bitset 256 B = 153,860 B of the CU's 163,840 B: one workgroup per CU.
constexpr int kBigK = 2048;
constexpr int kBigWords = kBigK / 64;
constexpr int kBigThreads = 1024;

__global__ __launch_bounds__(kBigThreads) void nms3d_big_kernel(
    const double* __restrict__ boxes, const uint8_t* __restrict__ valid, int K, int stride,
    double thr, int old_type, int samecls, uint8_t* __restrict__ keep) {
    __shared__ double s_col[8][kBigK];   // x1,y1,z1,x2,y2,z2,area,cls of the r-th pick candidate
    __shared__ double s_score[kBigK];
    __shared__ unsigned short s_order[kBigK];
    __shared__ unsigned char s_flag[kBigK];   // valid while ranking, then "picked"
    __shared__ unsigned long long s_removed[kBigWords];
    __shared__ int s_nvalid;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const double* bx = boxes + (size_t)b * K * stride;
    if (tid == 0) s_nvalid = 0;
    if (tid < kBigWords) s_removed[tid] = 0ull;
    for (int i = tid; i < K; i += kBigThreads) {
        s_score[i] = bx[(size_t)i * stride + 6];
        s_flag[i] = valid ? (valid[(size_t)b * K + i] != 0) : 1;
        s_order[i] = 0;   // NaN scores leave ranks unassigned: those slots stay a valid row
    }
    __syncthreads();
    // 1. rank among valid boxes (score desc, index desc)
    for (int i = tid; i < K; i += kBigThreads) {
        if (!s_flag[i]) continue;
        const double si = s_score[i];
        int r = 0;
        for (int j = 0; j < K; ++j) {
            if (!s_flag[j]) continue;
            const double sj = s_score[j];
            r += (sj > si) || (sj == si && j > i);
        }
        s_order[r] = (unsigned short)i;
        atomicAdd(&s_nvalid, 1);
    }
    __syncthreads();
    const int nv = s_nvalid;
    // 2. rows in pick order
    for (int r = tid; r < nv; r += kBigThreads) {
        const double* p = bx + (size_t)s_order[r] * stride;
        for (int a = 0; a < 6; ++a) s_col[a][r] = p[a];
        s_col[6][r] = (p[3] - p[0]) * (p[4] - p[1]) * (p[5] - p[2]);
        s_col[7][r] = samecls ? p[7] : 0.0;
    }
    for (int i = tid; i < K; i += kBigThreads) s_flag[i] = 0;
    __syncthreads();
    // 3. greedy walk: every thread finds the next surviving row r from the bitset (bits <= r
    //    are final after the barrier of the pick before), then the wave that owns a 64-row
    //    word tests its rows after r against r and ORs the ballot into that word
    int r = 0;
    for (;;) {
        while (r < nv) {
            const unsigned long long alive = ~s_removed[r >> 6] >> (r & 63);
            if (alive) { r += __ffsll((long long)alive) - 1; break; }
            r = (r | 63) + 1;
        }
        if (r >= nv) break;
        if (tid == 0) s_flag[s_order[r]] = 1;
        const double ax1 = s_col[0][r], ay1 = s_col[1][r], az1 = s_col[2][r];
        const double ax2 = s_col[3][r], ay2 = s_col[4][r], az2 = s_col[5][r];
        const double area_i = s_col[6][r], cls_i = s_col[7][r];
        for (int c0 = 0; c0 < nv; c0 += kBigThreads) {
            const int c = c0 + tid;
            if ((c | 63) <= r) continue;   // the whole word is at or before the pick (wave-uniform)
            bool hit = false;
            if (c > r && c < nv) {
                const double xx1 = np_max(ax1, s_col[0][c]), yy1 = np_max(ay1, s_col[1][c]),
                             zz1 = np_max(az1, s_col[2][c]);
                const double xx2 = np_min(ax2, s_col[3][c]), yy2 = np_min(ay2, s_col[4][c]),
                             zz2 = np_min(az2, s_col[5][c]);
                const double l = np_max(0.0, xx2 - xx1), wd = np_max(0.0, yy2 - yy1),
                             h = np_max(0.0, zz2 - zz1);
                double o;
                if (old_type) {
                    o = (l * wd * h) / s_col[6][c];
                } else {
                    const double inter = l * wd * h;
                    o = inter / (area_i + s_col[6][c] - inter);
                }
                if (samecls) o = o * (double)(cls_i == s_col[7][c]);
                hit = o > thr;
            }
            const unsigned long long m = __ballot(hit);
            if ((tid & 63) == 0 && m) s_removed[c >> 6] |= m;
        }
        __syncthreads();
        ++r;
    }
    __syncthreads();
    for (int i = tid; i < K; i += kBigThreads) keep[(size_t)b * K + i] = s_flag[i];
}

__global__ __launch_bounds__(256) void nms_boxes_kernel(const float* __restrict__ corners,
                                                        const float* __restrict__ obj,
                                                        const int64_t* __restrict__ cls, int total,
                                                        double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const float* c = corners + (size_t)t * 24;
    float mn[3] = {c[0], c[1], c[2]}, mx[3] = {c[0], c[1], c[2]};
    for (int v = 1; v < 8; ++v)
        for (int a = 0; a < 3; ++a) {
            const float x = c[v * 3 + a];
            mn[a] = x < mn[a] ? x : mn[a];
            mx[a] = x > mx[a] ? x : mx[a];
        }
    double* o = out + (size_t)t * 8;
    o[0] = mn[0]; o[1] = mn[1]; o[2] = mn[2];
    o[3] = mx[0]; o[4] = mx[1]; o[5] = mx[2];
    o[6] = (double)obj[t];
    o[7] = cls ? (double)cls[t] : 0.0;
}

}  // namespace

// the K <= 2048 NMS and AP-match kernels at every shape (tests; off: dispatch on the shape)
static int g_eval_large = 0;
bool ov3d_eval_large_on() { return g_eval_large != 0; }

extern "C" int ov3d_eval_large_kernels(int on) {
    const int prev = g_eval_large;
    if (on >= 0) g_eval_large = on ? 1 : 0;
    return prev;
}

extern "C" int ov3d_nms3d(const double* boxes, const uint8_t* valid, int B, int K, int stride,
                          double thr, int old_type, int samecls, uint8_t* keep_out, void* stream) {
    if (B < 0 || K < 0 || K > kBigK || stride < 7 || (samecls && stride < 8) || !boxes || !keep_out)
        return OV3D_EINVAL;
    if (B == 0 || K == 0) return OV3D_OK;
    if (K > kMaxK || ov3d_eval_large_on())
        hipLaunchKernelGGL(nms3d_big_kernel, dim3(B), dim3(kBigThreads), 0, ov3d_stream(stream),
                           boxes, valid, K, stride, thr, old_type, samecls, keep_out);
    else
        hipLaunchKernelGGL(nms3d_kernel, dim3(B), dim3(kThreads), 0, ov3d_stream(stream), boxes,
                           valid, K, stride, thr, old_type, samecls, keep_out);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_nms_boxes_from_corners(const float* corners, const float* obj,
                                           const int64_t* cls, int B, int K, double* boxes_out,
                                           void* stream) {
    if (B < 0 || K < 0 || !corners || !obj || !boxes_out) return OV3D_EINVAL;
    const int total = B * K;
    if (total == 0) return OV3D_OK;
    hipLaunchKernelGGL(nms_boxes_kernel, dim3(ov3d_cdiv(total, 256)), dim3(256), 0,
                       ov3d_stream(stream), corners, obj, cls, total, boxes_out);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

// Pseudo boxes from 2D detections (include/ov3d_lift.h): frustum lift, image lift, the tools'
// class-wise NMS, and the match against the proposal pool.
//   3DOVDet_tools/scannet/lift_boxes.py, sunrgbd/lift_boxes.py, utils/projection.py,
//   utils/box_3d_utils.py
// Everything is float64; the file is built with -ffp-contract=off (Makefile), so a * b + c is
// two roundings as in numpy.  Min / max are order-independent, so every result is
// deterministic whatever the reduction shape.
//
// The match in closed form.  The reference walks the boxes kept by the first NMS in pick order
// b_0, b_1, ... and for each one that passes `iou.max() < match` takes j = argmax(iou) and does
//     if score(b) > tmp_score[j]: labels[j], tmp_score[j] = label(b), score(b)
// with tmp_score starting at 0.  The first NMS picks I[-1] of an ascending argsort of the
// scores and only ever deletes from I, so score(b_0) >= score(b_1) >= ...  Let b be the first
// box in pick order with argmax j that passes the threshold.  If score(b) > 0 it writes
// tmp_score[j] = score(b); every later box b' for j has score(b') <= score(b) and the compare
// is strict, so nothing overwrites it.  If score(b) is not > 0 it does not write, tmp_score[j]
// stays 0, and every later b' has score(b') <= score(b) <= 0 and does not write either (a NaN
// score never compares greater).  Hence pool box j is labelled iff the smallest-rank box among
// {kept, not (maxiou < match), score > 0, argmax == j} exists, and takes that box's label and
// score: an atomic minimum over ranks.  tests/test_lift_ref_cpu.py holds this to the loop.
#include <float.h>
#include <limits.h>

#include "boxreduce.h"
#include "common.h"
#include "../../include/ov3d_lift.h"

namespace {

constexpr int kLiftThreads = 256;
constexpr int kNmsThreads = 1024;
constexpr int kWaves = kLiftThreads / 64;
static_assert(kLiftThreads == kBoxThreads, "box_reduce_store reduces a workgroup of kBoxThreads");

__device__ __forceinline__ double map_row(const double* m, double x, double y, double z) {
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

// o = align_inv . p and a = align . o, once per point: ws row = o xyz, a xyz
template <typename T>
__global__ void __launch_bounds__(kLiftThreads)
lift_prep_kernel(const T* __restrict__ pts, int N, const double* __restrict__ align,
                 const double* __restrict__ align_inv, double* __restrict__ ws) {
    const long long i = (long long)blockIdx.x * kLiftThreads + threadIdx.x;
    if (i >= N) return;
    const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
    const double ox = map_row(align_inv, x, y, z), oy = map_row(align_inv + 4, x, y, z),
                 oz = map_row(align_inv + 8, x, y, z);
    double* w = ws + 6 * i;
    w[0] = ox;
    w[1] = oy;
    w[2] = oz;
    w[3] = map_row(align, ox, oy, oz);
    w[4] = map_row(align + 4, ox, oy, oz);
    w[5] = map_row(align + 8, ox, oy, oz);
}

// one workgroup per frustum over all points; only points of the frustum's label are tested
__global__ void __launch_bounds__(kLiftThreads)
lift_frustum_kernel(const double* __restrict__ ws, const int32_t* __restrict__ labels, int N,
                    const double* __restrict__ planes, const int32_t* __restrict__ plabel,
                    double* __restrict__ lohi, int ld, int32_t* __restrict__ count) {
    __shared__ double pl[24];
    __shared__ double red[7 * kBoxWaves];
    const int m = blockIdx.x;
    if (threadIdx.x < 24) pl[threadIdx.x] = planes[(long long)m * 24 + threadIdx.x];
    __syncthreads();
    const int lab = plabel[m];
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    int n = 0;
    for (int i = threadIdx.x; i < N; i += kLiftThreads) {
        if (labels[i] != lab) continue;
        const double* w = ws + 6ll * i;
        double vx = w[0] - pl[18], vy = w[1] - pl[19], vz = w[2] - pl[20];
        double ux = w[0] - pl[21], uy = w[1] - pl[22], uz = w[2] - pl[23];
        const double sv = (vx * vx + vy * vy) + vz * vz;
        const double su = (ux * ux + uy * uy) + uz * uz;
        vx /= sv; vy /= sv; vz /= sv;
        ux /= su; uy /= su; uz /= su;
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            in = in && (((vx * pl[3 * k] + vy * pl[3 * k + 1]) + vz * pl[3 * k + 2]) < 0.0);
            in = in && (((ux * pl[9 + 3 * k] + uy * pl[10 + 3 * k]) + uz * pl[11 + 3 * k]) < 0.0);
        }
        if (!in) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], w[3 + a]);
            hi[a] = fmax(hi[a], w[3 + a]);
        }
        ++n;
    }
    box_reduce_store(lo, hi, n, red, lohi + (long long)ld * m, count + m);
}

template <typename D>
__global__ void __launch_bounds__(kLiftThreads)
lift_image_kernel(const D* __restrict__ depth, const int32_t* __restrict__ seg,
                  const int32_t* __restrict__ lut, int lut_n, int H, int W,
                  const double* __restrict__ boxes, const int32_t* __restrict__ plabel,
                  const double* __restrict__ calib, double* __restrict__ lohi, int ld,
                  int32_t* __restrict__ count) {
    __shared__ double red[7 * kBoxWaves];
    const int b = blockIdx.x;
    const double x = boxes[6ll * b], y = boxes[6ll * b + 1];
    const double xw = x + boxes[6ll * b + 2], yh = y + boxes[6ll * b + 3];
    const int lab = plabel[b];
    // the rectangle's pixel range, clamped to the image (a NaN edge leaves the whole range and
    // fails the exact compares below)
    const int u0 = (int)fmin(fmax(ceil(x), 0.0), (double)W);
    const int u1 = (int)fmax(fmin(floor(xw), (double)(W - 1)), -1.0);
    const int v0 = (int)fmin(fmax(ceil(y), 0.0), (double)H);
    const int v1 = (int)fmax(fmin(floor(yh), (double)(H - 1)), -1.0);
    const long long nw = u1 - u0 + 1, nh = v1 - v0 + 1;
    const long long total = (nw > 0 && nh > 0) ? nw * nh : 0;
    const double fu = calib[0], fv = calib[1], cu = calib[2], cv = calib[3];
    const double* R = calib + 4;
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    int n = 0;
    for (long long idx = threadIdx.x; idx < total; idx += kLiftThreads) {
        const int u = u0 + (int)(idx % nw), v = v0 + (int)(idx / nw);
        const double ud = (double)u, vd = (double)v;
        if (!(ud >= x && ud <= xw && vd >= y && vd <= yh)) continue;
        const long long at = (long long)v * W + u;
        const int s = seg[at];
        const int cls = lut ? ((s >= 0 && s < lut_n) ? lut[s] : -100) : s;
        if (cls != lab) continue;
        const double d = (double)depth[at];
        const double p0 = ((ud - cu) * d) / fu;
        const double p2 = -(((vd - cv) * d) / fv);
        const double p1 = d;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double r = (R[3 * a] * p0 + R[3 * a + 1] * p1) + R[3 * a + 2] * p2;
            lo[a] = fmin(lo[a], r);
            hi[a] = fmax(hi[a], r);
        }
        ++n;
    }
    box_reduce_store(lo, hi, n, red, lohi + (long long)ld * b, count + b);
}

// ---------------------------------------------------------------- NMS (one workgroup)
// LDS: order 32 KiB + suppressed flags 8 KiB + a counter.  Positions come from counting
// (O(K^2) broadcast reads of the keys), then one pass per pick with one barrier each; the test
// of the head's flag is uniform, so suppressed heads cost no barrier.
// A NaN key sorts as -inf, so that the positions are a permutation whatever the input holds.
__device__ __forceinline__ double nms_key(const double* row, int use_size) {
    const double k = use_size ? row[6] * row[8] : row[6];
    return k != k ? -HUGE_VAL : k;
}

__global__ void __launch_bounds__(kNmsThreads)
lift_nms_kernel(const double* __restrict__ boxes, int ld, int K, const int32_t* __restrict__ valid,
                int use_size, double thresh, int32_t* __restrict__ rank,
                uint8_t* __restrict__ keep) {
    __shared__ int order[OV3D_LIFT_NMS_MAX];
    __shared__ uint8_t supp[OV3D_LIFT_NMS_MAX];
    __shared__ int nvalid;
    const int tid = threadIdx.x;
    if (tid == 0) nvalid = 0;
    __syncthreads();
    for (int i = tid; i < K; i += kNmsThreads) {
        rank[i] = -1;
        keep[i] = 0;
        supp[i] = 0;
        if (valid && !valid[i]) continue;
        const double ki = nms_key(boxes + (long long)i * ld, use_size);
        int pos = 0;
        for (int j = 0; j < K; ++j) {
            if (valid && !valid[j]) continue;
            const double kj = nms_key(boxes + (long long)j * ld, use_size);
            pos += (kj > ki || (kj == ki && j > i)) ? 1 : 0;
        }
        order[pos] = i;
        atomicAdd(&nvalid, 1);
    }
    __syncthreads();
    const int n = nvalid;
    int npick = 0;
    for (int r = 0; r < n; ++r) {
        if (supp[r]) continue;
        const int i = order[r];
        if (tid == 0) {
            rank[i] = npick;
            keep[i] = 1;
        }
        ++npick;
        const double* bi = boxes + (long long)i * ld;
        const double x1 = bi[0], y1 = bi[1], z1 = bi[2], x2 = bi[3], y2 = bi[4], z2 = bi[5];
        const double li = bi[7];
        const double vi = ((x2 - x1) * (y2 - y1)) * (z2 - z1) + 1e-8;
        for (int p = r + 1 + tid; p < n; p += kNmsThreads) {
            if (supp[p]) continue;
            const double* bj = boxes + (long long)order[p] * ld;
            const double vj = ((bj[3] - bj[0]) * (bj[4] - bj[1])) * (bj[5] - bj[2]) + 1e-8;
            const double l = fmax(0.0, fmin(x2, bj[3]) - fmax(x1, bj[0]));
            const double w = fmax(0.0, fmin(y2, bj[4]) - fmax(y1, bj[1]));
            const double h = fmax(0.0, fmin(z2, bj[5]) - fmax(z1, bj[2]));
            const double inter = (l * w) * h;
            double o = inter / ((vi + vj) - inter);
            o = o * (li == bj[7] ? 1.0 : 0.0);
            if (o > thresh) supp[p] = 1;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- pool match
__global__ void lift_owner_init_kernel(int32_t* owner, int P) {
    const int j = blockIdx.x * kLiftThreads + threadIdx.x;
    if (j < P) owner[j] = INT_MAX;
}

__global__ void __launch_bounds__(kLiftThreads)
lift_match_kernel(const double* __restrict__ boxes, int ld, const int32_t* __restrict__ rank,
                  const double* __restrict__ pool, int P, double match,
                  int32_t* __restrict__ owner, int32_t* __restrict__ amax,
                  double* __restrict__ maxiou) {
    __shared__ double rv[kWaves];
    __shared__ int ri[kWaves];
    const int b = blockIdx.x;
    const int rk = rank[b];
    if (rk < 0) {
        if (threadIdx.x == 0) {
            amax[b] = -1;
            maxiou[b] = 0.0;
        }
        return;
    }
    const double* q = boxes + (long long)b * ld;
    const double x1 = q[0], y1 = q[1], z1 = q[2], x2 = q[3], y2 = q[4], z2 = q[5];
    const double vq = ((x2 - x1) * (y2 - y1)) * (z2 - z1);
    double best = -DBL_MAX;
    int at = INT_MAX;
    for (int j = threadIdx.x; j < P; j += kLiftThreads) {
        const double* c = pool + 7ll * j;
        const double a1 = c[0] - c[3] / 2, b1 = c[1] - c[4] / 2, c1 = c[2] - c[5] / 2;
        const double a2 = c[3] + a1, b2 = c[4] + b1, c2 = c[5] + c1;
        const double vk = ((a2 - a1) * (b2 - b1)) * (c2 - c1);
        const double ix = fmax(fmin(x2, a2) - fmax(x1, a1), 0.0);
        const double iy = fmax(fmin(y2, b2) - fmax(y1, b1), 0.0);
        const double iz = fmax(fmin(z2, c2) - fmax(z1, c1), 0.0);
        const double inter = (ix * iy) * iz;
        const double iou = inter / (((vq + vk) - inter) + 1e-5);
        if (iou > best) {
            best = iou;
            at = j;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(at, off, 64);
        if (ov > best || (ov == best && oi < at)) {
            best = ov;
            at = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        rv[threadIdx.x >> 6] = best;
        ri[threadIdx.x >> 6] = at;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w)
            if (rv[w] > best || (rv[w] == best && ri[w] < at)) {
                best = rv[w];
                at = ri[w];
            }
        const bool found = at != INT_MAX;
        amax[b] = found ? at : -1;
        maxiou[b] = found ? best : 0.0;
        if (found && !(best < match) && q[6] > 0.0) atomicMin(&owner[at], rk);
    }
}

__global__ void __launch_bounds__(kLiftThreads)
lift_rows_kernel(const double* __restrict__ boxes, int ld, const int32_t* __restrict__ rank, int M,
                 const double* __restrict__ pool, double match, const int32_t* __restrict__ owner,
                 const int32_t* __restrict__ amax, const double* __restrict__ maxiou,
                 int32_t* __restrict__ win, double* __restrict__ rows, double* __restrict__ out) {
    const int b = blockIdx.x * kLiftThreads + threadIdx.x;
    if (b >= M) return;
    const double* q = boxes + (long long)b * ld;
    const int rk = rank[b], j = amax[b];
    const bool w = rk >= 0 && j >= 0 && !(maxiou[b] < match) && q[6] > 0.0 && owner[j] == rk;
    double* r = rows + 10ll * b;
    double* o = out + 10ll * b;
    win[b] = w ? 1 : 0;
    if (!w) {
        for (int a = 0; a < 10; ++a) r[a] = o[a] = 0.0;
        return;
    }
    const double* c = pool + 7ll * j;
    double s[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mn = c[a] - c[3 + a] / 2;
        const double mx = c[3 + a] + mn;
        s[a] = mx - mn;
        r[a] = mn;
        r[3 + a] = mx;
        o[3 + a] = s[a];
        o[a] = mn + s[a] / 2;
    }
    const double vol = (s[0] * s[1]) * s[2];
    const double area = 2 * ((s[0] * s[2] + s[1] * s[0]) + s[2] * s[1]);
    r[6] = q[6];
    r[7] = q[7];
    r[8] = vol;
    r[9] = area;
    o[6] = q[7];
    o[7] = q[6] * vol;
    o[8] = vol;
    o[9] = area;
}

}  // namespace

extern "C" int ov3d_lift_frustum(const void* pts, int pt_f64, int N, const int32_t* labels,
                                 const double* align, const double* align_inv,
                                 const double* planes, const int32_t* plabel, int M, double* ws,
                                 double* lohi, int lohi_ld, int32_t* count, void* stream) {
    if (!pts || !labels || !align || !align_inv || !planes || !plabel || !ws || !lohi || !count ||
        (pt_f64 != 0 && pt_f64 != 1) || N < 1 || M < 1 || lohi_ld < 6)
        return OV3D_EINVAL;
    const dim3 grid((N + kLiftThreads - 1) / kLiftThreads);
    if (pt_f64)
        hipLaunchKernelGGL(lift_prep_kernel<double>, grid, dim3(kLiftThreads), 0, ov3d_stream(stream),
                           static_cast<const double*>(pts), N, align, align_inv, ws);
    else
        hipLaunchKernelGGL(lift_prep_kernel<float>, grid, dim3(kLiftThreads), 0, ov3d_stream(stream),
                           static_cast<const float*>(pts), N, align, align_inv, ws);
    hipLaunchKernelGGL(lift_frustum_kernel, dim3(M), dim3(kLiftThreads), 0, ov3d_stream(stream), ws,
                       labels, N, planes, plabel, lohi, lohi_ld, count);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_lift_image(const void* depth, int depth_f64, const int32_t* seg,
                               const int32_t* lut, int lut_n, int H, int W, const double* boxes,
                               const int32_t* plabel, int k, const double* calib, double* lohi,
                               int lohi_ld, int32_t* count, void* stream) {
    if (!depth || !seg || !boxes || !plabel || !calib || !lohi || !count ||
        (depth_f64 != 0 && depth_f64 != 1) || H < 1 || W < 1 || k < 1 || lohi_ld < 6 ||
        (long long)H * W > INT_MAX || (lut ? lut_n < 1 : lut_n != 0))
        return OV3D_EINVAL;
    if (depth_f64)
        hipLaunchKernelGGL(lift_image_kernel<double>, dim3(k), dim3(kLiftThreads), 0,
                           ov3d_stream(stream), static_cast<const double*>(depth), seg, lut, lut_n, H,
                           W, boxes, plabel, calib, lohi, lohi_ld, count);
    else
        hipLaunchKernelGGL(lift_image_kernel<int32_t>, dim3(k), dim3(kLiftThreads), 0,
                           ov3d_stream(stream), static_cast<const int32_t*>(depth), seg, lut, lut_n,
                           H, W, boxes, plabel, calib, lohi, lohi_ld, count);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_lift_nms(const double* boxes, int ld, int K, const int32_t* valid,
                             int use_size_score, double thresh, int32_t* rank, uint8_t* keep,
                             void* stream) {
    if (!boxes || !rank || !keep || K < 0 || K > OV3D_LIFT_NMS_MAX ||
        (use_size_score != 0 && use_size_score != 1) || ld < 8 + use_size_score || thresh != thresh)
        return OV3D_EINVAL;
    if (K == 0) return OV3D_OK;
    hipLaunchKernelGGL(lift_nms_kernel, dim3(1), dim3(kNmsThreads), 0, ov3d_stream(stream), boxes, ld,
                       K, valid, use_size_score, thresh, rank, keep);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_lift_match(const double* boxes, int ld, const int32_t* rank, int M,
                               const double* pool, int P, double match, int32_t* owner,
                               int32_t* amax, double* maxiou, int32_t* win, double* rows,
                               double* out, void* stream) {
    if (!boxes || !rank || !pool || !owner || !amax || !maxiou || !win || !rows || !out || ld < 8 ||
        M < 1 || P < 1 || match != match)
        return OV3D_EINVAL;
    hipLaunchKernelGGL(lift_owner_init_kernel, dim3((P + kLiftThreads - 1) / kLiftThreads),
                       dim3(kLiftThreads), 0, ov3d_stream(stream), owner, P);
    hipLaunchKernelGGL(lift_match_kernel, dim3(M), dim3(kLiftThreads), 0, ov3d_stream(stream), boxes,
                       ld, rank, pool, P, match, owner, amax, maxiou);
    hipLaunchKernelGGL(lift_rows_kernel, dim3((M + kLiftThreads - 1) / kLiftThreads),
                       dim3(kLiftThreads), 0, ov3d_stream(stream), boxes, ld, rank, M, pool, match,
                       owner, amax, maxiou, win, rows, out);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

// Pseudo boxes scored against ground truth (include/ov3d_boxeval.h): per-class precision and
// recall of a whole split at several IoU thresholds, two launches.
//   3DOVDet_tools/scannet/evaluate_box.py, utils/evaluation/pr_helper.py (PRCalculator),
//   utils/evaluation/eval_det.py (eval_det_cls, get_iou), evaluation/box_util.py (calc_iou)
// Everything is float64; the file is built with -ffp-contract=off (Makefile), so a * b + c is
// two roundings as in numpy.
//
// The closed form.  eval_det_cls walks the detections of a class by descending score; for each
// it takes the best same-class GT box of its scan (jmax, ovmax: strict compare, the first
// maximum wins) and marks a true positive iff ovmax > t and box jmax is not yet taken.  jmax
// and ovmax depend neither on t nor on any other detection.  A GT box j is therefore taken
// exactly once at threshold t iff some detection with jmax == j has ovmax > t (the first such
// detection in the walk takes it, every later one is a false positive), and never otherwise.
// Hence
//     TP(class, t) = #{GT boxes j of the class : max over {p : jmax[p] == j} of ovmax[p] > t}
// whatever the order among equal scores; precision is TP / nd and recall TP / npos.  The flag of
// a single detection does depend on the order: the taker is the first of {p : jmax[p] == j,
// ovmax[p] > t} by (score descending, row ascending), i.e. the one of the smallest rank.
// tests/test_box_eval_cpu.py holds both to the reference's recorded results.
//
// No atomics and no clearing: a scan belongs to one workgroup, ranks are counted (no sort, no
// cap), a GT box collects its claimants by reading what the workgroup wrote before a barrier.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/ov3d_boxeval.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 256;                    // GT boxes staged at once: 7 doubles + class each
constexpr int kMaxT = OV3D_BOXEVAL_MAX_T;
constexpr int kTallyThreads = 1024;
constexpr int kTallyWaves = kTallyThreads / 64;

// rank, jmax, ovmax, best and owner are written and then read by other threads of the same
// workgroup across __syncthreads(): no __restrict__ on them.
__global__ void __launch_bounds__(kThreads)
boxeval_match_kernel(const double* __restrict__ pred, int ldp, const int32_t* __restrict__ pred_cls,
                     const double* __restrict__ score, const int32_t* __restrict__ pred_off, int P,
                     const double* __restrict__ gt, int ldg, const int32_t* __restrict__ gt_cls,
                     const int32_t* __restrict__ gt_off, int G, const double* __restrict__ thr,
                     int T, int32_t* rank, int32_t* jmax, double* ovmax, double* best,
                     int32_t* owner, uint8_t* __restrict__ tp) {
    __shared__ double g_lo[3][kChunk];
    __shared__ double g_hi[3][kChunk];
    __shared__ double g_vol[kChunk];
    __shared__ int g_cls[kChunk];
    __shared__ double thr_s[kMaxT];
    const int s = blockIdx.x, tid = threadIdx.x;
    // the scan's segments, kept inside the arrays whatever the offsets hold
    const int p0 = min(max(pred_off[s], 0), P), p1 = min(max(pred_off[s + 1], p0), P);
    const int g0 = min(max(gt_off[s], 0), G), g1 = min(max(gt_off[s + 1], g0), G);
    if (tid < kMaxT) thr_s[tid] = tid < T ? thr[tid] : HUGE_VAL;

    for (int p = p0 + tid; p < p1; p += kThreads) {
        const double sp = score[p];
        int r = 0;
        for (int q = p0; q < p1; ++q) {
            const double sq = score[q];
            r += (sq > sp || (sq == sp && q < p)) ? 1 : 0;
        }
        rank[p] = r;
        jmax[p] = -1;
        ovmax[p] = -HUGE_VAL;
    }

    for (int c0 = g0; c0 < g1; c0 += kChunk) {
        const int n = min(kChunk, g1 - c0);
        __syncthreads();
        if (tid < n) {
            const double* b = gt + (long long)(c0 + tid) * ldg;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                g_hi[a][tid] = b[a] + b[3 + a] / 2;
                g_lo[a][tid] = b[a] - b[3 + a] / 2;
            }
            g_vol[tid] = (b[3] * b[4]) * b[5];
            g_cls[tid] = gt_cls[c0 + tid];
        }
        __syncthreads();
        for (int p = p0 + tid; p < p1; p += kThreads) {
            const double* b = pred + (long long)p * ldp;
            double hi[3], lo[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                hi[a] = b[a] + b[3 + a] / 2;
                lo[a] = b[a] - b[3 + a] / 2;
            }
            const double vol = (b[3] * b[4]) * b[5];
            const int pc = pred_cls[p];
            double ov = ovmax[p];              // this thread's own running pair
            int jm = jmax[p];
            for (int j = 0; j < n; ++j) {
                if (g_cls[j] != pc) continue;
                const double mx = fmin(hi[0], g_hi[0][j]), xx = fmax(lo[0], g_lo[0][j]);
                const double my = fmin(hi[1], g_hi[1][j]), xy = fmax(lo[1], g_lo[1][j]);
                const double mz = fmin(hi[2], g_hi[2][j]), xz = fmax(lo[2], g_lo[2][j]);
                double iou = 0.0;
                if (mx > xx && my > xy && mz > xz) {
                    const double inter = ((mx - xx) * (my - xy)) * (mz - xz);
                    const double uni = (vol + g_vol[j]) - inter;
                    iou = inter / uni;
                }
                if (iou < 0.0) iou = 0.0;
                if (iou > 1.0) iou = 1.0;
                if (iou > ov) {
                    ov = iou;
                    jm = c0 + j;
                }
            }
            ovmax[p] = ov;
            jmax[p] = jm;
        }
    }
    __syncthreads();

    for (int j = g0 + tid; j < g1; j += kThreads) {
        double b = -HUGE_VAL;
        int own[kMaxT];
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) own[t] = INT_MAX;
        for (int p = p0; p < p1; ++p) {
            if (jmax[p] != j) continue;
            const double ov = ovmax[p];
            const int r = rank[p];
            b = ov > b ? ov : b;
#pragma unroll
            for (int t = 0; t < kMaxT; ++t)    // thr_s[t >= T] = +inf: never exceeded
                own[t] = (ov > thr_s[t] && r < own[t]) ? r : own[t];
        }
        best[j] = b;
#pragma unroll
        for (int t = 0; t < kMaxT; ++t)
            if (t < T) owner[(long long)t * G + j] = own[t];
    }
    __syncthreads();

    for (int p = p0 + tid; p < p1; p += kThreads) {
        const int jm = jmax[p], r = rank[p];
        const double ov = ovmax[p];
        for (int t = 0; t < T; ++t)
            tp[(long long)t * P + p] =
                (jm >= 0 && ov > thr_s[t] && owner[(long long)t * G + jm] == r) ? 1 : 0;
    }
}

// One workgroup per class; counters 0 nd, 1 npos, 2 + t ntp[t].  A class's workgroup reads all
// P + G class ids, so a launch is as long as one workgroup's chain of loads: 1024 threads and
// loops without branches, unrolled, keep several loads of each thread in flight.
__global__ void __launch_bounds__(kTallyThreads)
boxeval_tally_kernel(const int32_t* __restrict__ pred_cls, int P, const int32_t* __restrict__ gt_cls,
                     const double* __restrict__ best, int G, const double* __restrict__ thr, int T,
                     int C, int32_t* __restrict__ nd, int32_t* __restrict__ npos,
                     int32_t* __restrict__ ntp) {
    __shared__ double thr_s[kMaxT];
    __shared__ int red[kTallyWaves][2 + kMaxT];
    const int c = blockIdx.x, tid = threadIdx.x;
    if (tid < kMaxT) thr_s[tid] = tid < T ? thr[tid] : HUGE_VAL;
    __syncthreads();
    int cnt[2 + kMaxT];
#pragma unroll
    for (int k = 0; k < 2 + kMaxT; ++k) cnt[k] = 0;
#pragma unroll 4
    for (int i = tid; i < P; i += kTallyThreads) cnt[0] += pred_cls[i] == c ? 1 : 0;
#pragma unroll 2
    for (int i = tid; i < G; i += kTallyThreads) {
        const bool mine = gt_cls[i] == c;
        const double b = best[i];
        cnt[1] += mine ? 1 : 0;
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) cnt[2 + t] += (mine && b > thr_s[t]) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 2 + kMaxT; ++k) {
        int v = cnt[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 2 + T) {
        int v = 0;
        for (int w = 0; w < kTallyWaves; ++w) v += red[w][tid];
        if (tid == 0)
            nd[c] = v;
        else if (tid == 1)
            npos[c] = v;
        else
            ntp[(long long)(tid - 2) * C + c] = v;
    }
}

bool bad_counts(long long P, long long G, int T) {
    return P < 0 || G < 0 || P > INT_MAX || G > INT_MAX || T < 1 || T > kMaxT;
}

}  // namespace

extern "C" int ov3d_boxeval_match(const double* pred, int ldp, const int32_t* pred_cls,
                                  const double* score, const int32_t* pred_off, long long P,
                                  const double* gt, int ldg, const int32_t* gt_cls,
                                  const int32_t* gt_off, long long G, int S, const double* thr,
                                  int T, int32_t* rank, int32_t* jmax, double* ovmax, double* best,
                                  int32_t* owner, uint8_t* tp, void* stream) {
    if (bad_counts(P, G, T) || S < 1 || ldp < 6 || ldg < 6 || !pred_off || !gt_off || !thr ||
        (P > 0 && (!pred || !pred_cls || !score || !rank || !jmax || !ovmax || !tp)) ||
        (G > 0 && (!gt || !gt_cls || !best || !owner)))
        return OV3D_EINVAL;
    hipLaunchKernelGGL(boxeval_match_kernel, dim3(S), dim3(kThreads), 0, ov3d_stream(stream), pred,
                       ldp, pred_cls, score, pred_off, (int)P, gt, ldg, gt_cls, gt_off, (int)G, thr, T,
                       rank, jmax, ovmax, best, owner, tp);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_boxeval_tally(const int32_t* pred_cls, long long P, const int32_t* gt_cls,
                                  const double* best, long long G, const double* thr, int T, int C,
                                  int32_t* nd, int32_t* npos, int32_t* ntp, void* stream) {
    if (bad_counts(P, G, T) || C < 1 || !thr || !nd || !npos || !ntp || (P > 0 && !pred_cls) ||
        (G > 0 && (!gt_cls || !best)))
        return OV3D_EINVAL;
    hipLaunchKernelGGL(boxeval_tally_kernel, dim3(C), dim3(kTallyThreads), 0, ov3d_stream(stream), pred_cls,
                       (int)P, gt_cls, best, (int)G, thr, T, C, nd, npos, ntp);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

// Detection evaluation on the device.
//
// Replaces the CPU evaluation of utils/ap_calculator.py and utils/eval_det.py:
//   ov3d_box_points_count : remove_empty_box (ap_calculator.py:70-84) — points of the scene
//                           inside each predicted box's convex hull (box_util.py:22-31,
//                           scipy Delaunay.find_simplex), after flip_axis_to_depth; kind 1:
//                           the label vote of pseudo-label generation
//                           (utils/label_formatter.py gen_pseudo) over axis-aligned boxes
//   ov3d_box3d_iou_eval   : box3d_iou (box_util.py:116-141) of every (prediction, GT) pair
//                           of a scene: Sutherland-Hodgman clip of the bird's-eye rectangles
//                           (polygon_clip, box_util.py:34-80) in double, the Python
//                           evaluation order, no contraction; the clipped polygon's area by
//                           the shoelace formula where the reference asks Qhull
//                           (ConvexHull(...).volume, box_util.py:88-97)
//   ov3d_ap_match         : eval_det_cls's TP / FP walk (eval_det.py:104-131) for every
//                           (scene, class): detections by descending confidence, each GT
//                           matched once
//   ov3d_ap_curve         : cumulative precision / recall and voc_ap (eval_det.py:20-52,
//                           133-146) per class from the globally sorted TP flags
#include <float.h>

#include "common.h"

namespace {

// ---------------------------------------------------------------------------
// point-in-hull counts.  The hull facets of the box's 8 corners are the planes through 3
// corners with the other 5 on one side (exactly the convex hull, also for corners that
// float32 rounding left slightly non-coplanar); a point is inside when it is on the inner
// side of every facet (boundary: Qhull's find_simplex tolerance is not reproduced).
constexpr int kBoxesPerWG = 8;
constexpr int kMaxFacets = 56;   // C(8, 3)
constexpr int kCountThreads = 256;

__global__ __launch_bounds__(kCountThreads) void box_points_count_kernel(
    const float* __restrict__ pts, long long pt_sb, long long pt_sn, int N,
    const float* __restrict__ corners, int K, int32_t* __restrict__ counts) {
    const int b = blockIdx.y;
    const int k0 = blockIdx.x * kBoxesPerWG;
    __shared__ double s_pl[kBoxesPerWG][kMaxFacets][4];
    __shared__ int s_nf[kBoxesPerWG];
    __shared__ double s_bb[kBoxesPerWG][6];
    __shared__ int s_cnt[kBoxesPerWG];
    if (threadIdx.x < kBoxesPerWG) {
        const int q = threadIdx.x;
        const int k = k0 + q;
        int nf = 0;
        s_cnt[q] = 0;
        if (k < K) {
            // flip_axis_to_depth (ap_calculator.py:23-27) in float32: (x, z, -y)
            double P[8][3];
            const float* c = corners + ((long long)b * K + k) * 24;
            for (int v = 0; v < 8; ++v) {
                P[v][0] = (double)c[v * 3 + 0];
                P[v][1] = (double)c[v * 3 + 2];
                P[v][2] = (double)(-1.0f * c[v * 3 + 1]);
            }
            double lo[3] = {P[0][0], P[0][1], P[0][2]}, hi[3] = {P[0][0], P[0][1], P[0][2]};
            for (int v = 1; v < 8; ++v)
                for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], P[v][a]); hi[a] = fmax(hi[a], P[v][a]); }
            for (int a = 0; a < 3; ++a) { s_bb[q][a] = lo[a]; s_bb[q][3 + a] = hi[a]; }
            for (int i = 0; i < 8; ++i)
                for (int j = i + 1; j < 8; ++j)
                    for (int l = j + 1; l < 8; ++l) {
                        const double u[3] = {P[j][0] - P[i][0], P[j][1] - P[i][1], P[j][2] - P[i][2]};
                        const double w[3] = {P[l][0] - P[i][0], P[l][1] - P[i][1], P[l][2] - P[i][2]};
                        double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2],
                                       u[0] * w[1] - u[1] * w[0]};
                        if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) continue;
                        bool pos = false, neg = false;
                        for (int m = 0; m < 8; ++m) {
                            if (m == i || m == j || m == l) continue;
                            const double s = n[0] * (P[m][0] - P[i][0]) + n[1] * (P[m][1] - P[i][1]) +
                                             n[2] * (P[m][2] - P[i][2]);
                            pos |= s > 0.0;
                            neg |= s < 0.0;
                        }
                        if (pos && neg) continue;
                        if (pos) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }   // outward normal
                        if (!pos && !neg) continue;                               // all coplanar
                        s_pl[q][nf][0] = n[0];
                        s_pl[q][nf][1] = n[1];
                        s_pl[q][nf][2] = n[2];
                        s_pl[q][nf][3] = n[0] * P[i][0] + n[1] * P[i][1] + n[2] * P[i][2];
                        ++nf;
                    }
        }
        s_nf[q] = nf;
    }
    __syncthreads();
    int cnt[kBoxesPerWG];
#pragma unroll
    for (int q = 0; q < kBoxesPerWG; ++q) cnt[q] = 0;
    const float* P0 = pts + (long long)b * pt_sb;
    for (int i = threadIdx.x; i < N; i += kCountThreads) {
        const float* p = P0 + (long long)i * pt_sn;
        const double x = p[0], y = p[1], z = p[2];
#pragma unroll
        for (int q = 0; q < kBoxesPerWG; ++q) {
            if (s_nf[q] == 0) continue;
            if (x < s_bb[q][0] || y < s_bb[q][1] || z < s_bb[q][2] || x > s_bb[q][3] ||
                y > s_bb[q][4] || z > s_bb[q][5])
                continue;
            bool in = true;
            for (int f = 0; f < s_nf[q] && in; ++f)
                in = s_pl[q][f][0] * x + s_pl[q][f][1] * y + s_pl[q][f][2] * z <= s_pl[q][f][3];
            cnt[q] += in;
        }
    }
#pragma unroll
    for (int q = 0; q < kBoxesPerWG; ++q) {
        int v = cnt[q];
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[q], v);
    }
    __syncthreads();
    if (threadIdx.x < kBoxesPerWG && k0 + (int)threadIdx.x < K)
        counts[(long long)b * K + k0 + threadIdx.x] = s_cnt[threadIdx.x];
}

// ---------------------------------------------------------------------------
// label vote (utils/label_formatter.py:155-158 gen_pseudo, :183-188 crop_pc): per axis-aligned
// box (lo xyz, hi xyz; closed intervals) the histogram of the per-vertex labels inside it and
// scipy.stats.mode's answer, the smallest label among the most frequent.  T is the points' own
// type: numpy compares a float32 point with the float32 bound, a float64 point with the bound
// widened to double.  Same layout as the hull count: 8 boxes per workgroup, every point of the
// scene once per workgroup; hits are sparse, so they go straight into an 8 x 32 LDS histogram.
// Labels are read 4 at a time from the first 4-byte-aligned address of the scene's row.
constexpr int kVoteThreads = 1024;
constexpr int kVoteMaxC = 32;

template <typename T>
__device__ __forceinline__ void vote_point(const T* __restrict__ p, unsigned label, int C,
                                           const T (*s_b)[6], int (*s_hist)[kVoteMaxC]) {
    if (label >= (unsigned)C) return;
    const T x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int q = 0; q < kBoxesPerWG; ++q) {
        // NaN compares false: never inside; lo > hi: nothing inside
        if (x >= s_b[q][0] && y >= s_b[q][1] && z >= s_b[q][2] && x <= s_b[q][3] &&
            y <= s_b[q][4] && z <= s_b[q][5])
            atomicAdd(&s_hist[q][label], 1);
    }
}

template <typename T>
__global__ __launch_bounds__(kVoteThreads) void box_label_vote_kernel(
    const T* __restrict__ pts, long long pt_sb, long long pt_sn, int N,
    const float* __restrict__ boxes, const uint8_t* __restrict__ labels, int C, int K,
    int32_t* __restrict__ counts, int32_t* __restrict__ mode) {
    const int b = blockIdx.y;
    const int k0 = blockIdx.x * kBoxesPerWG;
    __shared__ T s_b[kBoxesPerWG][6];
    __shared__ int s_hist[kBoxesPerWG][kVoteMaxC];
    if (threadIdx.x < kBoxesPerWG * kVoteMaxC) (&s_hist[0][0])[threadIdx.x] = 0;
    if (threadIdx.x < kBoxesPerWG * 6) {
        const int q = threadIdx.x / 6, a = threadIdx.x % 6;
        // a box past K is empty (lo > hi)
        s_b[q][a] = k0 + q < K ? (T)boxes[((long long)b * K + k0 + q) * 6 + a] : (T)(a < 3 ? 1 : 0);
    }
    __syncthreads();
    const T* P0 = pts + (long long)b * pt_sb;
    const uint8_t* L0 = labels + (long long)b * N;
    const int head = min(N, (int)((4 - ((uintptr_t)L0 & 3)) & 3));
    const int groups = (N - head) / 4;
    for (int i = threadIdx.x; i < head; i += kVoteThreads)
        vote_point<T>(P0 + (long long)i * pt_sn, L0[i], C, s_b, s_hist);
    const uint32_t* L4 = reinterpret_cast<const uint32_t*>(L0 + head);
#pragma unroll 2
    for (int g = threadIdx.x; g < groups; g += kVoteThreads) {
        const uint32_t l4 = L4[g];
        const T* p = P0 + (long long)(head + 4 * g) * pt_sn;
#pragma unroll
        for (int j = 0; j < 4; ++j) vote_point<T>(p + j * pt_sn, (l4 >> (8 * j)) & 0xffu, C, s_b, s_hist);
    }
    for (int i = head + 4 * groups + threadIdx.x; i < N; i += kVoteThreads)
        vote_point<T>(P0 + (long long)i * pt_sn, L0[i], C, s_b, s_hist);
    __syncthreads();
    for (int e = threadIdx.x; e < kBoxesPerWG * C; e += kVoteThreads) {
        const int q = e / C, c = e % C;
        if (k0 + q < K) counts[((long long)b * K + k0 + q) * C + c] = s_hist[q][c];
    }
    if (mode && threadIdx.x < kBoxesPerWG && k0 + (int)threadIdx.x < K) {
        int best = -1, most = 0;
        for (int c = 0; c < C; ++c)
            if (s_hist[threadIdx.x][c] > most) { most = s_hist[threadIdx.x][c]; best = c; }
        mode[(long long)b * K + k0 + threadIdx.x] = best;
    }
}

// ---------------------------------------------------------------------------
// box3d_iou: rect = corners 3, 2, 1, 0 in (x, z) (box_util.py:128-129)
struct Pt { double x, y; };

__device__ __forceinline__ bool sh_inside(Pt p, Pt c1, Pt c2) {
    return (c2.x - c1.x) * (p.y - c1.y) > (c2.y - c1.y) * (p.x - c1.x);
}

__device__ __forceinline__ Pt sh_intersect(Pt c1, Pt c2, Pt s, Pt e) {
    const double dc0 = c1.x - c2.x, dc1 = c1.y - c2.y;
    const double dp0 = s.x - e.x, dp1 = s.y - e.y;
    const double n1 = c1.x * c2.y - c1.y * c2.x;
    const double n2 = s.x * e.y - s.y * e.x;
    const double n3 = 1.0 / (dc0 * dp1 - dc1 * dp0);
    return Pt{(n1 * dp0 - n2 * dc0) * n3, (n1 * dp1 - n2 * dc1) * n3};
}

// area of polygon_clip(rect1, rect2) (0 when the clip empties: the reference's None)
__device__ double clip_area(const Pt* r1, const Pt* r2) {
    Pt out[16], in[16];
    int n_out = 4;
    for (int i = 0; i < 4; ++i) out[i] = r1[i];
    Pt c1 = r2[3];
    for (int ci = 0; ci < 4; ++ci) {
        const Pt c2 = r2[ci];
        const int n_in = n_out;
        for (int i = 0; i < n_in; ++i) in[i] = out[i];
        n_out = 0;
        Pt s = in[n_in - 1];
        for (int i = 0; i < n_in; ++i) {
            const Pt e = in[i];
            if (sh_inside(e, c1, c2)) {
                if (!sh_inside(s, c1, c2)) out[n_out++] = sh_intersect(c1, c2, s, e);
                out[n_out++] = e;
            } else if (sh_inside(s, c1, c2)) {
                out[n_out++] = sh_intersect(c1, c2, s, e);
            }
            s = e;
        }
        c1 = c2;
        if (n_out == 0) return 0.0;
    }
    double a = 0.0;
    for (int i = 0; i < n_out; ++i) {
        const Pt p = out[i], q = out[(i + 1) % n_out];
        a += p.x * q.y - q.x * p.y;
    }
    return 0.5 * fabs(a);
}

__device__ __forceinline__ double box_vol(const float* c) {
    double e[3];
    const int pairs[3][2] = {{0, 1}, {1, 2}, {0, 4}};
    for (int q = 0; q < 3; ++q) {
        const double dx = (double)c[pairs[q][0] * 3] - (double)c[pairs[q][1] * 3];
        const double dy = (double)c[pairs[q][0] * 3 + 1] - (double)c[pairs[q][1] * 3 + 1];
        const double dz = (double)c[pairs[q][0] * 3 + 2] - (double)c[pairs[q][1] * 3 + 2];
        e[q] = sqrt(dx * dx + dy * dy + dz * dz);
    }
    return e[0] * e[1] * e[2];
}

__global__ void box3d_iou_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ pvalid,
                                 const float* __restrict__ gt, const uint8_t* __restrict__ gvalid,
                                 int S, int K, int G, double* __restrict__ iou) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)S * K * G) return;
    const int g = (int)(t % G);
    const long long sk = t / G;
    const int s = (int)(sk / K);
    double v = 0.0;
    if (pvalid[sk] && gvalid[(long long)s * G + g]) {
        const float* c1 = pred + sk * 24;
        const float* c2 = gt + ((long long)s * G + g) * 24;
        Pt r1[4], r2[4];
        for (int i = 0; i < 4; ++i) {
            r1[i] = Pt{(double)c1[(3 - i) * 3], (double)c1[(3 - i) * 3 + 2]};
            r2[i] = Pt{(double)c2[(3 - i) * 3], (double)c2[(3 - i) * 3 + 2]};
        }
        const double inter = clip_area(r1, r2);
        const double ymax = fmin((double)c1[1], (double)c2[1]);
        const double ymin = fmax((double)c1[13], (double)c2[13]);
        const double inter_vol = inter * fmax(0.0, ymax - ymin);
        v = inter_vol / (box_vol(c1) + box_vol(c2) - inter_vol);
    }
    iou[t] = v;
}

// ---------------------------------------------------------------------------
// TP / FP of every detection, per (scene, class): detections of the class in that scene in
// descending score (ties: lower box index first), each matched to the first GT of the class
// with the largest IoU; a hit (IoU > thresh) on an unmatched GT is a TP and marks it.
__global__ void ap_match_kernel(const double* __restrict__ iou, const float* __restrict__ scores,
                                const int64_t* __restrict__ gt_cls,
                                const uint8_t* __restrict__ gvalid, int S, int K, int G, int C,
                                double thresh, uint8_t* __restrict__ tp) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)S * C) return;
    const int s = (int)(t / C), c = (int)(t % C);
    const float* sc = scores + (long long)s * K * C + c;
    unsigned long long done[4] = {0, 0, 0, 0};   // K <= 256 processed flags
    unsigned long long det = 0;                  // G <= 64 matched flags
    for (;;) {
        int best = -1;
        float bs = -INFINITY;
        for (int k = 0; k < K; ++k) {
            if ((done[k >> 6] >> (k & 63)) & 1ull) continue;
            const float v = sc[(long long)k * C];
            if (v > bs) { bs = v; best = k; }
        }
        if (best < 0) break;
        done[best >> 6] |= 1ull << (best & 63);
        double ovmax = -INFINITY;
        int jmax = -1;
        for (int g = 0; g < G; ++g) {
            if (!gvalid[(long long)s * G + g] || gt_cls[(long long)s * G + g] != c) continue;
            const double v = iou[((long long)s * K + best) * G + g];
            if (v > ovmax) { ovmax = v; jmax = g; }
        }
        uint8_t hit = 0;
        if (ovmax > thresh && !((det >> jmax) & 1ull)) {
            hit = 1;
            det |= 1ull << jmax;
        }
        tp[((long long)s * K + best) * C + c] = hit;
    }
}

// The same walk for K <= 2048 and G <= 1024, one workgroup per (scene, class), without the
// serial selection scan.  The walk's outcome has a closed form: a detection's GT (first GT of
// the class with the largest IoU, scanned exactly as above) does not depend on the other
// detections, and a GT is marked by the first detection in confidence order that hits it.  So
//   rank_k  = detections of the class before k (higher score; ties: lower box index),
//   j_k     = k's GT if its IoU > thresh, else none,
//   first_j = min rank_k over the detections with j_k = j   (atomicMin in LDS),
//   tp_k    = (j_k is some j and first_j == rank_k).
// A detection is a score > -inf (NaN is none), as the scan above takes them.
constexpr int kMatchMaxK = 2048;
constexpr int kMatchMaxG = 1024;
constexpr int kMatchThreads = 256;

__global__ __launch_bounds__(kMatchThreads) void ap_match_big_kernel(
    const double* __restrict__ iou, const float* __restrict__ scores,
    const int64_t* __restrict__ gt_cls, const uint8_t* __restrict__ gvalid, int K, int G, int C,
    double thresh, uint8_t* __restrict__ tp) {
    __shared__ float s_sc[kMatchMaxK];             // the class's scores, -inf = no detection
    __shared__ unsigned short s_gl[kMatchMaxG];    // the class's GT boxes, ascending
    __shared__ int s_first[kMatchMaxG];            // per listed GT: rank of its first hit
    __shared__ int s_m;
    const int s = blockIdx.x / C, c = blockIdx.x % C;
    const int tid = threadIdx.x;
    const float* sc = scores + (long long)s * K * C + c;
    for (int k = tid; k < K; k += kMatchThreads) {
        const float v = sc[(long long)k * C];
        s_sc[k] = v > -INFINITY ? v : -INFINITY;
    }
    if (tid < 64) {   // wave 0: ordered list of the class's GT boxes
        int m = 0;
        for (int g0 = 0; g0 < G; g0 += 64) {
            const int g = g0 + tid;
            const bool is = g < G && gvalid[(long long)s * G + g] && gt_cls[(long long)s * G + g] == c;
            const unsigned long long bal = __ballot(is);
            if (is) s_gl[m + __popcll(bal & lanemask_lt())] = (unsigned short)g;
            m += __popcll(bal);
        }
        if (tid == 0) s_m = m;
    }
    for (int q = tid; q < G; q += kMatchThreads) s_first[q] = 0x7fffffff;
    __syncthreads();
    const int m = s_m;
    int rank[kMatchMaxK / kMatchThreads], jm[kMatchMaxK / kMatchThreads];
#pragma unroll
    for (int u = 0; u < kMatchMaxK / kMatchThreads; ++u) {
        const int k = u * kMatchThreads + tid;
        rank[u] = -1;
        jm[u] = -1;
        if (k >= K) continue;
        const float si = s_sc[k];
        if (!(si > -INFINITY)) continue;
        int r = 0;
        for (int j = 0; j < K; ++j) {
            const float sj = s_sc[j];
            r += (sj > si) || (sj == si && j < k);
        }
        rank[u] = r;
        const double* row = iou + ((long long)s * K + k) * G;
        double ovmax = -INFINITY;
        int jmax = -1;
        for (int q = 0; q < m; ++q) {
            const double v = row[s_gl[q]];
            if (v > ovmax) { ovmax = v; jmax = q; }
        }
        if (jmax >= 0 && ovmax > thresh) {
            jm[u] = jmax;
            atomicMin(&s_first[jmax], r);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kMatchMaxK / kMatchThreads; ++u) {
        const int k = u * kMatchThreads + tid;
        if (rank[u] < 0) continue;
        tp[((long long)s * K + k) * C + c] = (jm[u] >= 0 && s_first[jm[u]] == rank[u]) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// voc_ap per class (one workgroup each) from TP flags in global descending-score order:
//   prec_d = tp_d / (d + 1), rec_d = tp_d / npos; the area under the precision envelope
//   only changes at TP positions: ap = sum_k (rec_k - rec_{k-1}) * max_{k' >= k} prec_k'.
constexpr int kCurveThreads = 1024;

__global__ __launch_bounds__(kCurveThreads) void ap_curve_kernel(
    const uint8_t* __restrict__ tp_sorted, long long M, const int32_t* __restrict__ nvalid,
    const int32_t* __restrict__ npos, int32_t* __restrict__ tp_pos, long long tp_cap,
    double* __restrict__ ap, double* __restrict__ rec_last) {
    const int c = blockIdx.x;
    const uint8_t* f = tp_sorted + (long long)c * M;
    int32_t* pos = tp_pos + (long long)c * tp_cap;
    const int n = nvalid[c];
    const int np = npos[c];
    __shared__ int s_w[kCurveThreads / 64];
    __shared__ int s_base;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // (1) positions of the TPs, in order
    for (int c0 = 0; c0 < n; c0 += kCurveThreads) {
        const int d = c0 + threadIdx.x;
        const bool hit = d < n && f[d];
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_w[w] = __popcll(m);
        __syncthreads();
        int p = s_base + __popcll(m & lanemask_lt());
        for (int q = 0; q < w; ++q) p += s_w[q];
        if (hit && p < tp_cap) pos[p] = d;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int q = 0; q < kCurveThreads / 64; ++q) tot += s_w[q];
            s_base += tot;
        }
        __syncthreads();
    }
    // (2) suffix max of precision over TP positions + the sum (one thread: T <= #GT)
    if (threadIdx.x == 0) {
        const int T = min(s_base, (int)tp_cap);
        double sum = 0.0, env = 0.0;
        for (int k = T - 1; k >= 0; --k) {
            const double prec = (double)(k + 1) / fmax((double)(pos[k] + 1), DBL_EPSILON);
            env = fmax(env, prec);
            const double r1 = np > 0 ? (double)(k + 1) / (double)np : 0.0;
            const double r0 = np > 0 ? (double)k / (double)np : 0.0;
            sum += (r1 - r0) * env;
        }
        ap[c] = sum;
        rec_last[c] = (n > 0 && np > 0) ? (double)T / (double)np : 0.0;
    }
}

}  // namespace

extern "C" int ov3d_box_points_count(const void* pts, int pt_f64, long long pt_sb, long long pt_sn,
                                     int N, const float* boxes, int kind, const uint8_t* labels,
                                     int C, int B, int K, int32_t* counts, int32_t* mode,
                                     void* stream) {
    if (!pts || !boxes || !counts || pt_sn < 3 || B < 0 || K < 0 || N < 0) return OV3D_EINVAL;
    const dim3 grid((K + kBoxesPerWG - 1) / kBoxesPerWG, B);
    if (kind == 0) {
        if (pt_f64 != 0 || labels || C != 0 || mode) return OV3D_EINVAL;
        if (B == 0 || K == 0) return OV3D_OK;
        hipLaunchKernelGGL(box_points_count_kernel, grid, dim3(kCountThreads), 0,
                           ov3d_stream(stream), static_cast<const float*>(pts), pt_sb, pt_sn, N,
                           boxes, K, counts);
    } else if (kind == 1) {
        if ((pt_f64 != 0 && pt_f64 != 1) || !labels || C < 1 || C > kVoteMaxC || B < 1 ||
            B > 65535 || K < 1 || N < 1)
            return OV3D_EINVAL;
        if (pt_f64)
            hipLaunchKernelGGL(box_label_vote_kernel<double>, grid, dim3(kVoteThreads), 0,
                               ov3d_stream(stream), static_cast<const double*>(pts), pt_sb, pt_sn,
                               N, boxes, labels, C, K, counts, mode);
        else
            hipLaunchKernelGGL(box_label_vote_kernel<float>, grid, dim3(kVoteThreads), 0,
                               ov3d_stream(stream), static_cast<const float*>(pts), pt_sb, pt_sn,
                               N, boxes, labels, C, K, counts, mode);
    } else {
        return OV3D_EINVAL;
    }
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_box3d_iou_eval(const float* pred, const uint8_t* pvalid, const float* gt,
                                   const uint8_t* gvalid, int S, int K, int G, double* iou,
                                   void* stream) {
    if (!pred || !pvalid || !gt || !gvalid || !iou || S < 0 || K < 0 || G < 0) return OV3D_EINVAL;
    const long long n = (long long)S * K * G;
    if (n == 0) return OV3D_OK;
    hipLaunchKernelGGL(box3d_iou_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ov3d_stream(stream), pred, pvalid, gt, gvalid, S, K, G, iou);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_ap_match(const double* iou, const float* scores, const int64_t* gt_cls,
                             const uint8_t* gvalid, int S, int K, int G, int C, double thresh,
                             uint8_t* tp, void* stream) {
    if (!iou || !scores || !gt_cls || !gvalid || !tp || S < 0 || K < 0 || K > kMatchMaxK || G < 0 ||
        G > kMatchMaxG || C <= 0)
        return OV3D_EINVAL;
    const long long n = (long long)S * C;
    if (n == 0 || K == 0) return OV3D_OK;
    if (K > 256 || G > 64 || ov3d_eval_large_on()) {
        if (n > 0x7fffffffll) return OV3D_EINVAL;
        hipLaunchKernelGGL(ap_match_big_kernel, dim3((unsigned)n), dim3(kMatchThreads), 0,
                           ov3d_stream(stream), iou, scores, gt_cls, gvalid, K, G, C, thresh, tp);
    } else {
        hipLaunchKernelGGL(ap_match_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0,
                           ov3d_stream(stream), iou, scores, gt_cls, gvalid, S, K, G, C, thresh, tp);
    }
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_ap_curve(const uint8_t* tp_sorted, long long M, const int32_t* nvalid,
                             const int32_t* npos, int C, int32_t* tp_pos, long long tp_cap,
                             double* ap, double* rec_last, void* stream) {
    if (!tp_sorted || !nvalid || !npos || !tp_pos || !ap || !rec_last || C < 0 || M < 0 ||
        tp_cap <= 0)
        return OV3D_EINVAL;
    if (C == 0) return OV3D_OK;
    hipLaunchKernelGGL(ap_curve_kernel, dim3(C), dim3(kCurveThreads), 0, ov3d_stream(stream),
                       tp_sorted, M, nvalid, npos, tp_pos, tp_cap, ap, rec_last);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

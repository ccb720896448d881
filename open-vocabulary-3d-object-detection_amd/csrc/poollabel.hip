// Proposal-pool labelling and pseudo-label assessment (include/ov3d_poollabel.h).
//   3DOVDet_tools/scannet/assign_box_label_from_gt.py (labeling): per pool box the most
//   frequent per-vertex label among the scan's vertices inside it;
//   3DOVDet_tools/scannet/assess_pseudo_label.py (match): per-pixel agreement of LSeg's labels
//   with the ground-truth frames, here as the whole confusion matrix.
// Both are integer decisions.  The only floating-point operations are the exact widening of a
// float32 vertex to double and compares, so -ffp-contract=off (Makefile) has nothing to change
// here; it is kept so that the whole library is built one way.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/ov3d_poollabel.h"

// boxes of one workgroup, and whether a vertex is first tested against the union of the tile's
// boxes; the defaults are what DESIGN.md "Pool labels and label assessment" measured
#ifndef OV3D_POOLLABEL_TILE
#define OV3D_POOLLABEL_TILE 8
#endif
#ifndef OV3D_POOLLABEL_CULL
#define OV3D_POOLLABEL_CULL 0
#endif

namespace {

constexpr int kVoteThreads = 1024;
constexpr int kTile = OV3D_POOLLABEL_TILE;
constexpr int kMaxC = OV3D_POOLLABEL_MAX_C;
constexpr int kConfThreads = 256;
constexpr int kMaxK = OV3D_POOLLABEL_MAX_K;
constexpr int kMaxCells = (kMaxK + 1) * (kMaxK + 1);

// ---------------------------------------------------------------------------
// vote.  The layout of box_label_vote_kernel (evaldet.hip): a tile of boxes per workgroup, its
// bounds and one histogram per box in LDS, every vertex of the scan read once per workgroup,
// labels four at a time.  Hits are sparse (a pool box holds a small share of its scan), so they
// go into the histogram as LDS atomics.  The bounds stay float64: numpy compares a float32
// vertex with a float64 bound in float64.
template <typename T>
__device__ __forceinline__ void vote_point(const T* __restrict__ p, unsigned label, unsigned lo_label,
                                           unsigned C, const double (*s_b)[6],
                                           const double* s_u, int (*s_hist)[kMaxC]) {
    if (label < lo_label || label >= C) return;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#if OV3D_POOLLABEL_CULL
    if (!(x >= s_u[0] && y >= s_u[1] && z >= s_u[2] && x <= s_u[3] && y <= s_u[4] && z <= s_u[5]))
        return;
#endif
#pragma unroll
    for (int q = 0; q < kTile; ++q) {
        // NaN compares false: never inside; lo > hi: nothing inside
        if (x >= s_b[q][0] && y >= s_b[q][1] && z >= s_b[q][2] && x <= s_b[q][3] &&
            y <= s_b[q][4] && z <= s_b[q][5])
            atomicAdd(&s_hist[q][label], 1);
    }
}

template <typename T>
__global__ __launch_bounds__(kVoteThreads) void poollabel_vote_kernel(
    const T* __restrict__ pts, long long ld, const uint8_t* __restrict__ labels,
    const int32_t* __restrict__ pt_off, int N, const double* __restrict__ boxes,
    const int32_t* __restrict__ box_off, int P, int S, int min_label, int C,
    int32_t* __restrict__ counts, int32_t* __restrict__ mode) {
    __shared__ double s_b[kTile][6];
    __shared__ double s_u[6];
    __shared__ int s_hist[kTile][kMaxC];
    const int tid = threadIdx.x;
    // the workgroup's scan and tile: tiles are numbered scan by scan (the same walk in every
    // thread, over uniform values); the segments are kept inside the arrays whatever the
    // offsets hold
    int s = 0, b0 = 0, b1 = 0;
    int t = blockIdx.x;
    for (; s < S; ++s) {
        b0 = min(max(box_off[s], 0), P);
        b1 = min(max(box_off[s + 1], b0), P);
        const int tiles = (b1 - b0 + kTile - 1) / kTile;
        if (t < tiles) break;
        t -= tiles;
    }
    if (s == S) return;                        // the grid is rounded up by one tile per scan
    const int k0 = b0 + t * kTile;
    const int p0 = min(max(pt_off[s], 0), N);
    const int n = min(max(pt_off[s + 1], p0), N) - p0;

    for (int e = tid; e < kTile * kMaxC; e += kVoteThreads) (&s_hist[0][0])[e] = 0;
    if (tid < kTile * 6) {
        const int q = tid / 6, a = tid % 6;
        // a box past the scan's last is empty (lo > hi)
        s_b[q][a] = k0 + q < b1 ? boxes[(long long)(k0 + q) * 6 + a] : (a < 3 ? 1.0 : 0.0);
    }
    __syncthreads();
#if OV3D_POOLLABEL_CULL
    if (tid < 6) {
        // union of the tile's non-empty boxes; a NaN bound leaves the union alone and its box
        // holds nothing anyway
        double u = tid < 3 ? HUGE_VAL : -HUGE_VAL;
        for (int q = 0; q < kTile; ++q) {
            const bool live = s_b[q][0] <= s_b[q][3] && s_b[q][1] <= s_b[q][4] && s_b[q][2] <= s_b[q][5];
            if (live) u = tid < 3 ? fmin(u, s_b[q][tid]) : fmax(u, s_b[q][tid]);
        }
        s_u[tid] = u;
    }
    __syncthreads();
#endif
    const T* P0 = pts + (long long)p0 * ld;
    const uint8_t* L0 = labels + p0;
    // the row of labels starts at any byte: head and tail from the row's own address
    const int head = min(n, (int)((4 - ((uintptr_t)L0 & 3)) & 3));
    const int groups = (n - head) / 4;
    const unsigned lo_label = (unsigned)min_label, uC = (unsigned)C;
    for (int i = tid; i < head; i += kVoteThreads)
        vote_point<T>(P0 + (long long)i * ld, L0[i], lo_label, uC, s_b, s_u, s_hist);
    const uint32_t* L4 = reinterpret_cast<const uint32_t*>(L0 + head);
#pragma unroll 2
    for (int g = tid; g < groups; g += kVoteThreads) {
        const uint32_t l4 = L4[g];
        const T* p = P0 + (long long)(head + 4 * g) * ld;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            vote_point<T>(p + (long long)j * ld, (l4 >> (8 * j)) & 0xffu, lo_label, uC, s_b, s_u, s_hist);
    }
    for (int i = head + 4 * groups + tid; i < n; i += kVoteThreads)
        vote_point<T>(P0 + (long long)i * ld, L0[i], lo_label, uC, s_b, s_u, s_hist);
    __syncthreads();
    for (int e = tid; e < kTile * C; e += kVoteThreads) {
        const int q = e / C, c = e % C;
        if (k0 + q < b1) counts[(long long)(k0 + q) * C + c] = s_hist[q][c];
    }
    if (tid < kTile && k0 + tid < b1) {
        int best = -1, most = 0;
        for (int c = 0; c < C; ++c)            // strict: the smallest label among the most frequent
            if (s_hist[tid][c] > most) { most = s_hist[tid][c]; best = c; }
        mode[k0 + tid] = best;
    }
}

// ---------------------------------------------------------------------------
// confusion.  grid (x, S): the workgroups of a scan share its pixels 16 bytes per thread and
// step.  Labels are piecewise constant along a row, so a thread carries the current (gt,
// pseudo) byte pair with its run length and touches LDS only when the pair changes: one table
// read and one LDS atomic per run, not per pixel; four pixels that continue the run are one
// compare of two words.
struct ConfRun {
    unsigned pair;                             // gt | pseudo << 8
    int len;                                   // 0: nothing yet (whatever pair holds)
};

__device__ __forceinline__ void conf_flush(const ConfRun& r, const uint8_t* s_map, int* s_hist, int K) {
    if (r.len == 0) return;
    const int g = min((int)s_map[r.pair & 0xffu], K), p = min((int)(r.pair >> 8), K);
    atomicAdd(&s_hist[g * (K + 1) + p], r.len);
}

__device__ __forceinline__ void conf_pixel(ConfRun& r, unsigned pair, const uint8_t* s_map, int* s_hist,
                                           int K) {
    if (pair == r.pair) {
        ++r.len;
    } else {
        conf_flush(r, s_map, s_hist, K);
        r.pair = pair;
        r.len = 1;
    }
}

__device__ __forceinline__ void conf_word(ConfRun& r, uint32_t g4, uint32_t p4, const uint8_t* s_map,
                                          int* s_hist, int K) {
    // four pixels of the running pair: the usual case inside a segment
    if (g4 == (r.pair & 0xffu) * 0x01010101u && p4 == (r.pair >> 8) * 0x01010101u) {
        r.len += 4;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        conf_pixel(r, ((g4 >> (8 * j)) & 0xffu) | (((p4 >> (8 * j)) & 0xffu) << 8), s_map, s_hist, K);
}

__global__ __launch_bounds__(kConfThreads) void poollabel_confusion_kernel(
    const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pseudo,
    const int32_t* __restrict__ frame_off, int F, long long HW, const uint8_t* __restrict__ gt_map,
    int K, unsigned long long* __restrict__ conf) {
    __shared__ int s_hist[kMaxCells];
    __shared__ uint8_t s_map[256];
    const int s = blockIdx.y, tid = threadIdx.x;
    const int cells = (K + 1) * (K + 1);
    const int f0 = min(max(frame_off[s], 0), F), f1 = min(max(frame_off[s + 1], f0), F);
    if (f1 == f0) return;
    for (int e = tid; e < cells; e += kConfThreads) s_hist[e] = 0;
    s_map[tid] = gt_map[tid];                  // kConfThreads == 256
    __syncthreads();

    const long long n = (long long)(f1 - f0) * HW;         // the scan's pixels
    const uint8_t* G0 = gt + (long long)f0 * HW;
    const uint8_t* Q0 = pseudo + (long long)f0 * HW;
    // the scan's rows start at any byte: head and tail from their own addresses; 16-byte reads
    // only where both arrays reach a 16-byte boundary together
    const bool together = (((uintptr_t)G0 ^ (uintptr_t)Q0) & 15) == 0;
    const long long head = together ? min(n, (long long)((16 - ((uintptr_t)G0 & 15)) & 15)) : n;
    const long long vecs = (n - head) / 16;
    const long long first = (long long)blockIdx.x * kConfThreads + tid;
    const long long step = (long long)gridDim.x * kConfThreads;
    ConfRun r{0u, 0};
    for (long long i = first; i < head; i += step)
        conf_pixel(r, G0[i] | ((unsigned)Q0[i] << 8), s_map, s_hist, K);
    const uint4* G16 = reinterpret_cast<const uint4*>(G0 + head);
    const uint4* Q16 = reinterpret_cast<const uint4*>(Q0 + head);
#pragma unroll 2
    for (long long v = first; v < vecs; v += step) {
        const uint4 g = G16[v], p = Q16[v];
        conf_word(r, g.x, p.x, s_map, s_hist, K);
        conf_word(r, g.y, p.y, s_map, s_hist, K);
        conf_word(r, g.z, p.z, s_map, s_hist, K);
        conf_word(r, g.w, p.w, s_map, s_hist, K);
    }
    for (long long i = head + 16 * vecs + first; i < n; i += step)
        conf_pixel(r, G0[i] | ((unsigned)Q0[i] << 8), s_map, s_hist, K);
    conf_flush(r, s_map, s_hist, K);
    __syncthreads();
    for (int e = tid; e < cells; e += kConfThreads) {
        const int v = s_hist[e];
        if (v) atomicAdd(&conf[(long long)s * cells + e], (unsigned long long)v);
    }
}

}  // namespace

extern "C" int ov3d_poollabel_vote(const void* pts, int pt_f64, long long ld, const uint8_t* labels,
                                   const int32_t* pt_off, long long N, const double* boxes,
                                   const int32_t* box_off, long long P, int S, int min_label, int C,
                                   int32_t* counts, int32_t* mode, void* stream) {
    if (N < 0 || P < 0 || N > INT_MAX || P > INT_MAX || S < 1 || ld < 3 || (pt_f64 != 0 && pt_f64 != 1) ||
        C < 1 || C > kMaxC || min_label < 0 || min_label > C || !pt_off || !box_off ||
        (N > 0 && (!pts || !labels)) || (P > 0 && (!boxes || !counts || !mode)))
        return OV3D_EINVAL;
    if (P == 0) return OV3D_OK;
    // one tile more per scan than P / kTile: every scan's last tile may be partial
    const long long grid = (P + kTile - 1) / kTile + S;
    if (grid > INT_MAX) return OV3D_EINVAL;
    if (pt_f64)
        hipLaunchKernelGGL(poollabel_vote_kernel<double>, dim3((unsigned)grid), dim3(kVoteThreads), 0,
                           ov3d_stream(stream), (const double*)pts, ld, labels, pt_off, (int)N, boxes, box_off,
                           (int)P, S, min_label, C, counts, mode);
    else
        hipLaunchKernelGGL(poollabel_vote_kernel<float>, dim3((unsigned)grid), dim3(kVoteThreads), 0,
                           ov3d_stream(stream), (const float*)pts, ld, labels, pt_off, (int)N, boxes, box_off,
                           (int)P, S, min_label, C, counts, mode);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_poollabel_confusion(const uint8_t* gt, const uint8_t* pseudo, const int32_t* frame_off,
                                        long long F, long long HW, int S, const uint8_t* gt_map, int K,
                                        long long* conf, void* stream) {
    if (F < 0 || F > INT_MAX || HW < 1 || HW > INT_MAX || S < 1 || S > 65535 || K < 1 || K > kMaxK ||
        !frame_off || !gt_map || !conf || (F > 0 && (!gt || !pseudo)))
        return OV3D_EINVAL;
    // workgroups per scan: about 16 KiB of each array per workgroup and at most about 4096
    // workgroups in all, and never more than 2^30 pixels per workgroup (int32 partial counts)
    const long long pixels = F * HW;
    long long gx = (pixels / S + 16383) / 16384;
    gx = gx < 1 ? 1 : gx;
    const long long cap = 4096 / S < 1 ? 1 : 4096 / S;
    gx = gx > cap ? cap : gx;
    const long long need = (pixels >> 30) + 1;
    gx = gx < need ? need : gx;
    if (gx > INT_MAX) return OV3D_EINVAL;
    const long long cells = (long long)(K + 1) * (K + 1);
    if (hipMemsetAsync(conf, 0, (size_t)(S * cells) * sizeof(long long), ov3d_stream(stream)) != hipSuccess)
        return OV3D_ELAUNCH;
    if (F == 0) return OV3D_OK;
    hipLaunchKernelGGL(poollabel_confusion_kernel, dim3((unsigned)gx, (unsigned)S), dim3(kConfThreads), 0,
                       ov3d_stream(stream), gt, pseudo, frame_off, (int)F, HW, gt_map, K,
                       reinterpret_cast<unsigned long long*>(conf));
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

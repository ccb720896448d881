// Multiview back-projection (include/ov3d_backproj.h): the frame table, the (F, N+1) index
// tables of image_processor.compute_projection, ProjectionHelper.project as a gather, and the
// fused per-vertex compose.
//   utils/projection.py:191,259  utils/image_util.py:17,65
// float32 throughout (the file is built with -ffp-contract=off, so a * b + c is two roundings
// as in numpy); the order of every sum is the one the header states.  Nothing here uses an
// atomic: the tables are placed by ballot + prefix in point order, the compose keeps the last
// frame per vertex, so every result is the same bits on every run.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/ov3d_backproj.h"

namespace {

constexpr int kRow = OV3D_BACKPROJ_ROW;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kIters = OV3D_BACKPROJ_BLOCK / kThreads;
constexpr int kLdsDepth = 8192;        // floats of one depth map kept in LDS (32 KiB); larger maps
                                       // are read from global memory
constexpr int kComposeVerts = 64;      // vertices per compose workgroup (one lane each, 4 waves
                                       // share the frames)
constexpr int kGatherChannels = 16;    // channels per gather workgroup

static_assert(OV3D_BACKPROJ_BLOCK % kThreads == 0, "block of points = whole passes of the workgroup");

struct BpParams {
    float fx, fy, cx, cy, dmin, dmax, acc;
    float wmax, hmax;                  // the largest float <= W - 1, H - 1
    int W;
};

// ------------------------------------------------------------------ frame table

__global__ void __launch_bounds__(64)
bp_frames_kernel(const float* __restrict__ poses, int F, const float* __restrict__ params,
                 float* __restrict__ table) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    const float* P = poses + 16ll * f;
    float p[16];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        p[i] = P[i];
        finite = finite && isfinite(p[i]);
    }
    const double a00 = p[0], a01 = p[1], a02 = p[2], a03 = p[3], a10 = p[4], a11 = p[5], a12 = p[6],
                 a13 = p[7], a20 = p[8], a21 = p[9], a22 = p[10], a23 = p[11], a30 = p[12],
                 a31 = p[13], a32 = p[14], a33 = p[15];
    const double s0 = a00 * a11 - a10 * a01, s1 = a00 * a12 - a10 * a02, s2 = a00 * a13 - a10 * a03,
                 s3 = a01 * a12 - a11 * a02, s4 = a01 * a13 - a11 * a03, s5 = a02 * a13 - a12 * a03;
    const double c5 = a22 * a33 - a32 * a23, c4 = a21 * a33 - a31 * a23, c3 = a21 * a32 - a31 * a22,
                 c2 = a20 * a33 - a30 * a23, c1 = a20 * a32 - a30 * a22, c0 = a20 * a31 - a30 * a21;
    const double det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
    float b[16];
    b[0] = (float)(((a11 * c5 - a12 * c4) + a13 * c3) / det);
    b[1] = (float)(((-a01 * c5 + a02 * c4) - a03 * c3) / det);
    b[2] = (float)(((a31 * s5 - a32 * s4) + a33 * s3) / det);
    b[3] = (float)(((-a21 * s5 + a22 * s4) - a23 * s3) / det);
    b[4] = (float)(((-a10 * c5 + a12 * c2) - a13 * c1) / det);
    b[5] = (float)(((a00 * c5 - a02 * c2) + a03 * c1) / det);
    b[6] = (float)(((-a30 * s5 + a32 * s2) - a33 * s1) / det);
    b[7] = (float)(((a20 * s5 - a22 * s2) + a23 * s1) / det);
    b[8] = (float)(((a10 * c4 - a11 * c2) + a13 * c0) / det);
    b[9] = (float)(((-a00 * c4 + a01 * c2) - a03 * c0) / det);
    b[10] = (float)(((a30 * s4 - a31 * s2) + a33 * s0) / det);
    b[11] = (float)(((-a20 * s4 + a21 * s2) - a23 * s0) / det);
    b[12] = (float)(((-a10 * c3 + a11 * c1) - a12 * c0) / det);
    b[13] = (float)(((a00 * c3 - a01 * c1) + a02 * c0) / det);
    b[14] = (float)(((-a30 * s3 + a31 * s1) - a32 * s0) / det);
    b[15] = (float)(((a20 * s3 - a21 * s1) + a22 * s0) / det);
#pragma unroll
    for (int i = 0; i < 16; ++i) finite = finite && isfinite(b[i]);

    float c[8][3];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float x = params[8 + 3 * k], y = params[9 + 3 * k], z = params[10 + 3 * k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            c[k][i] = ((p[4 * i] * x + p[4 * i + 1] * y) + p[4 * i + 2] * z) + p[4 * i + 3];
    }
    float* row = table + (long long)kRow * f;
    if (!finite) {
#pragma unroll
        for (int i = 0; i < kRow; ++i) row[i] = 0.0f;
        return;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) row[i] = b[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        row[12 + i] = c[2][i];
        row[15 + i] = c[4][i];
    }
    constexpr int pa[6] = {3, 2, 3, 0, 1, 6}, pb[6] = {1, 5, 6, 7, 4, 4}, po[6] = {0, 1, 2, 3, 0, 5};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float ux = c[pa[k]][0] - c[po[k]][0], uy = c[pa[k]][1] - c[po[k]][1],
                    uz = c[pa[k]][2] - c[po[k]][2];
        const float vx = c[pb[k]][0] - c[po[k]][0], vy = c[pb[k]][1] - c[po[k]][1],
                    vz = c[pb[k]][2] - c[po[k]][2];
        row[18 + 3 * k] = uy * vz - uz * vy;
        row[19 + 3 * k] = uz * vx - ux * vz;
        row[20 + 3 * k] = ux * vy - uy * vx;
    }
    row[36] = 1.0f;
    row[37] = row[38] = row[39] = 0.0f;
}

// ------------------------------------------------------------------ the decision

// r: the frame's table row (LDS or global); depth: the frame's (H,W) map (LDS or global).
// -> kept, and the pixel index when kept
__device__ __forceinline__ bool bp_decide(const float* r, const BpParams& q, const float* depth,
                                          float px, float py, float pz, int& pix) {
    const float vx = px - r[12], vy = py - r[13], vz = pz - r[14];
    const float wx = px - r[15], wy = py - r[16], wz = pz - r[17];
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* n = r + 18 + 3 * k;
        const float dv = (vx * n[0] + vy * n[1]) + vz * n[2];
        const float dw = (wx * n[9] + wy * n[10]) + wz * n[11];
        // rint(t) / 100 < 0 iff rint(t) < 0: a negative integer over 100 is negative and not 0
        in = in && (rintf(100.0f * dv) < 0.0f) && (rintf(100.0f * dw) < 0.0f);
    }
    if (!in) return false;
    const float cmx = ((r[0] * px + r[1] * py) + r[2] * pz) + r[3];
    const float cmy = ((r[4] * px + r[5] * py) + r[6] * pz) + r[7];
    const float cmz = ((r[8] * px + r[9] * py) + r[10] * pz) + r[11];
    const float rx = rintf((cmx * q.fx) / cmz + q.cx);
    const float ry = rintf((cmy * q.fy) / cmz + q.cy);
    if (!(rx >= 0.0f && rx <= q.wmax && ry >= 0.0f && ry <= q.hmax)) return false;
    pix = (int)ry * q.W + (int)rx;
    const float d = depth[pix];
    return d >= q.dmin && d <= q.dmax && fabsf(d - cmz) <= q.acc;
}

__device__ __forceinline__ BpParams bp_params(const float* __restrict__ params, int W, float wmax,
                                              float hmax) {
    BpParams q;
    q.fx = params[0]; q.fy = params[1]; q.cx = params[2]; q.cy = params[3];
    q.dmin = params[4]; q.dmax = params[5]; q.acc = params[6];
    q.wmax = wmax; q.hmax = hmax; q.W = W;
    return q;
}

// ------------------------------------------------------------------ index tables

// One workgroup per (frame, block of OV3D_BACKPROJ_BLOCK points): kIters passes of 256 points.
// kWrite false: the number kept in the block -> counts[frame][block].
// kWrite true: the same decisions again; the block's first slot is 1 + the counts of the blocks
// before it, inside the block a point's slot follows from the ballot of its wave and the counts
// of the waves and passes before it.  Slots past the frame's total are zeroed by the block that
// owns the points of the same numbers, so every slot has exactly one writer.
template <bool kWrite, bool kLds>
__global__ void __launch_bounds__(kThreads)
bp_tables_kernel(const float* __restrict__ pts, int N, const float* __restrict__ depth, int HW,
                 const float* __restrict__ table, const float* __restrict__ params,
                 int W, float wmax, float hmax, int nblk, int32_t* __restrict__ counts,
                 long long* __restrict__ idx3d, long long* __restrict__ idx2d) {
    extern __shared__ float sdepth[];
    __shared__ float srow[kRow];
    __shared__ int swave[kIters][kWaves];
    __shared__ int sred[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x / nblk, b = blockIdx.x % nblk;
    if (tid < kRow) srow[tid] = table[(long long)kRow * f + tid];
    const float* gmap = depth + (long long)f * HW;
    if (kLds)
        for (int i = tid; i < HW; i += kThreads) sdepth[i] = gmap[i];
    int before = 0, total = 0;
    if (kWrite) {
        const int32_t* cf = counts + (long long)f * nblk;
        for (int j = tid; j < nblk; j += kThreads) {
            const int c = cf[j];
            total += c;
            if (j < b) before += c;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            total += __shfl_xor(total, off, 64);
            before += __shfl_xor(before, off, 64);
        }
        if (lane == 0) {
            sred[0][wave] = total;
            sred[1][wave] = before;
        }
    }
    __syncthreads();
    if (kWrite) {
        total = before = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            total += sred[0][w];
            before += sred[1][w];
        }
    }
    const BpParams q = bp_params(params, W, wmax, hmax);
    const bool live = srow[36] != 0.0f;
    const long long base = (long long)b * OV3D_BACKPROJ_BLOCK;
    bool keep[kIters];
    int pix[kIters];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const long long i = base + it * kThreads + tid;
        keep[it] = false;
        pix[it] = 0;
        if (live && i < N)
            keep[it] = bp_decide(srow, q, kLds ? sdepth : gmap, pts[3 * i], pts[3 * i + 1],
                                 pts[3 * i + 2], pix[it]);
        const unsigned long long m = __ballot(keep[it]);
        if (lane == 0) swave[it][wave] = __popcll(m);
    }
    __syncthreads();
    if (!kWrite) {
        if (tid == 0) {
            int n = 0;
#pragma unroll
            for (int it = 0; it < kIters; ++it)
#pragma unroll
                for (int w = 0; w < kWaves; ++w) n += swave[it][w];
            counts[(long long)f * nblk + b] = n;
        }
        return;
    }
    long long* r3 = idx3d + (long long)f * ((long long)N + 1);
    long long* r2 = idx2d + (long long)f * ((long long)N + 1);
    if (b == 0 && tid == 0) r3[0] = r2[0] = total;
    int running = before;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const long long i = base + it * kThreads + tid;
        const unsigned long long m = __ballot(keep[it]);
        int at = running + __popcll(m & lanemask_lt());
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) at += swave[it][w];
            running += swave[it][w];
        }
        if (keep[it]) {
            r3[1 + at] = i;
            r2[1 + at] = pix[it];
        }
        if (i < N && i >= total) r3[1 + i] = r2[1 + i] = 0;
    }
}

// ------------------------------------------------------------------ project (gather)

// one thread per vertex and kGatherChannels channels: is the vertex among idx3d[1..n]
// (ascending: binary search)?  then its column is the pixel's, else zero
template <typename T>
__global__ void __launch_bounds__(kThreads)
bp_gather_kernel(const T* __restrict__ label, int C, long long HW,
                 const long long* __restrict__ idx3d, const long long* __restrict__ idx2d, int N,
                 int nvb, T* __restrict__ out) {
    const int vb = blockIdx.x % nvb, cb = blockIdx.x / nvb;
    const long long v = (long long)vb * kThreads + threadIdx.x;
    if (v >= N) return;
    long long n = idx3d[0];
    n = n < 0 ? 0 : (n > N ? N : n);
    long long lo = 1, hi = n + 1;          // first slot in [1, n] whose value is >= v
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (idx3d[mid] < v) lo = mid + 1; else hi = mid;
    }
    long long pix = -1;
    if (lo <= n && idx3d[lo] == v) pix = idx2d[lo];
    const bool hit = pix >= 0 && pix < HW;
    const int c1 = min(C, (cb + 1) * kGatherChannels);
    for (int c = cb * kGatherChannels; c < c1; ++c)
        out[(long long)c * N + v] = hit ? label[(long long)c * HW + pix] : T(0);
}

// ------------------------------------------------------------------ fused compose

// 64 vertices per workgroup, one per lane; the four waves take a quarter of the frames each and
// walk it from its last frame down, until every lane of the wave has a frame.  The later wave
// wins.  Then all 256 threads copy the winners' channels, the output index running fastest.
template <typename T>
__global__ void __launch_bounds__(kThreads)
bp_compose_kernel(const float* __restrict__ pts, int N, const float* __restrict__ depth, int HW,
                  int F, const float* __restrict__ table, const float* __restrict__ params, int W,
                  float wmax, float hmax, const T* __restrict__ feat, int C, int rows,
                  T* __restrict__ out, int32_t* __restrict__ frame) {
    __shared__ int sbest[kWaves][kComposeVerts];
    __shared__ int spix[kWaves][kComposeVerts];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long v0 = (long long)blockIdx.x * kComposeVerts, v = v0 + lane;
    const BpParams q = bp_params(params, W, wmax, hmax);
    const bool have = v < N;
    const float px = have ? pts[3 * v] : 0.0f, py = have ? pts[3 * v + 1] : 0.0f,
                pz = have ? pts[3 * v + 2] : 0.0f;
    const int per = (F + kWaves - 1) / kWaves;
    const int f0 = wave * per, f1 = min(F, f0 + per);
    int best = have ? -1 : INT_MAX, bpix = 0;      // a lane without a vertex never searches
    for (int f = f1 - 1; f >= f0; --f) {
        const float* r = table + (long long)kRow * f;
        if (best < 0 && r[36] != 0.0f) {
            int pix;
            if (bp_decide(r, q, depth + (long long)f * HW, px, py, pz, pix)) {
                best = f;
                bpix = pix;
            }
        }
        if (__ballot(best < 0) == 0ull) break;
    }
    sbest[wave][lane] = have ? best : -1;
    spix[wave][lane] = bpix;
    __syncthreads();
    if (tid < kComposeVerts) {
        int bf = -1, bp = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
            if (sbest[w][tid] >= 0) {
                bf = sbest[w][tid];
                bp = spix[w][tid];
            }
        sbest[0][tid] = bf;
        spix[0][tid] = bp;
        if (v0 + tid < N) frame[v0 + tid] = bf;
    }
    __syncthreads();
    const int nv = (int)min((long long)kComposeVerts, (long long)N - v0);
    const long long chw = (long long)C * HW;
    if (rows) {
        // out (N, C): nv * C consecutive elements
        T* o = out + v0 * C;
        for (long long e = tid; e < (long long)nv * C; e += kThreads) {
            const int vl = (int)(e / C), c = (int)(e % C);
            const int bf = sbest[0][vl];
            o[e] = bf >= 0 ? feat[bf * chw + (long long)c * HW + spix[0][vl]] : T(0);
        }
    } else {
        // out (C, N): nv consecutive elements per channel
        for (long long e = tid; e < (long long)kComposeVerts * C; e += kThreads) {
            const int c = (int)(e / kComposeVerts), vl = (int)(e % kComposeVerts);
            if (vl >= nv) continue;
            const int bf = sbest[0][vl];
            out[(long long)c * N + v0 + vl] =
                bf >= 0 ? feat[bf * chw + (long long)c * HW + spix[0][vl]] : T(0);
        }
    }
}

// the largest float that is <= n (n >= 0)
float float_at_most(int n) {
    float f = (float)n;
    if ((double)f > (double)n) f = nextafterf(f, 0.0f);
    return f;
}

bool bad_image(int W, int H) { return W < 1 || H < 1 || (long long)H * W > INT_MAX; }

void launch_frames(const float* poses, int F, const float* params, float* table, hipStream_t s) {
    hipLaunchKernelGGL(bp_frames_kernel, dim3((F + 63) / 64), dim3(64), 0, s, poses, F, params, table);
}

}  // namespace

extern "C" int ov3d_backproj_frames(const float* poses, int F, const float* params, float* table,
                                    void* stream) {
    if (!poses || !params || !table || F < 1) return OV3D_EINVAL;
    launch_frames(poses, F, params, table, ov3d_stream(stream));
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_backproj_tables(const float* pts, int N, const float* depth, const float* poses,
                                    int F, const float* params, int W, int H, float* table,
                                    int32_t* counts, int64_t* idx3d, int64_t* idx2d, void* stream) {
    if (!pts || !depth || !poses || !params || !table || !counts || !idx3d || !idx2d || N < 1 ||
        N == INT_MAX || F < 1 || bad_image(W, H))
        return OV3D_EINVAL;
    const long long nblk = ((long long)N + OV3D_BACKPROJ_BLOCK - 1) / OV3D_BACKPROJ_BLOCK;
    if (nblk * F > INT_MAX) return OV3D_EINVAL;
    const int HW = H * W;
    const bool use_lds = HW <= kLdsDepth;
    const size_t lds = use_lds ? sizeof(float) * HW : 0;
    const float wmax = float_at_most(W - 1), hmax = float_at_most(H - 1);
    hipStream_t s = ov3d_stream(stream);
    launch_frames(poses, F, params, table, s);
    const dim3 grid((unsigned)(nblk * F));
    long long* i3 = reinterpret_cast<long long*>(idx3d);
    long long* i2 = reinterpret_cast<long long*>(idx2d);
#define BP_TABLES(WRITE, LDS)                                                                     \
    hipLaunchKernelGGL((bp_tables_kernel<WRITE, LDS>), grid, dim3(kThreads), lds, s, pts, N, depth, \
                       HW, table, params, W, wmax, hmax, (int)nblk, counts, i3, i2)
    if (use_lds) {
        BP_TABLES(false, true);
        BP_TABLES(true, true);
    } else {
        BP_TABLES(false, false);
        BP_TABLES(true, false);
    }
#undef BP_TABLES
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_backproj_gather(const void* label, int bf16, int C, long long HW,
                                    const int64_t* idx3d, const int64_t* idx2d, int N, void* out,
                                    void* stream) {
    if (!label || !idx3d || !idx2d || !out || (bf16 != 0 && bf16 != 1) || C < 1 || HW < 1 ||
        HW > INT_MAX || N < 1 || N == INT_MAX)
        return OV3D_EINVAL;
    const long long nvb = ((long long)N + kThreads - 1) / kThreads;
    const long long ncb = ((long long)C + kGatherChannels - 1) / kGatherChannels;
    if (nvb * ncb > INT_MAX) return OV3D_EINVAL;
    const dim3 grid((unsigned)(nvb * ncb));
    const long long* i3 = reinterpret_cast<const long long*>(idx3d);
    const long long* i2 = reinterpret_cast<const long long*>(idx2d);
    if (bf16)
        hipLaunchKernelGGL(bp_gather_kernel<uint16_t>, grid, dim3(kThreads), 0, ov3d_stream(stream),
                           static_cast<const uint16_t*>(label), C, HW, i3, i2, N, (int)nvb,
                           static_cast<uint16_t*>(out));
    else
        hipLaunchKernelGGL(bp_gather_kernel<uint32_t>, grid, dim3(kThreads), 0, ov3d_stream(stream),
                           static_cast<const uint32_t*>(label), C, HW, i3, i2, N, (int)nvb,
                           static_cast<uint32_t*>(out));
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_backproj_compose(const float* pts, int N, const float* depth, const float* poses,
                                     int F, const float* params, int W, int H, const void* feat,
                                     int bf16, int C, int rows, float* table, void* out,
                                     int32_t* frame, void* stream) {
    if (!pts || !depth || !poses || !params || !feat || !table || !out || !frame || N < 1 ||
        N == INT_MAX || F < 1 || C < 1 || bad_image(W, H) || (bf16 != 0 && bf16 != 1) ||
        (rows != 0 && rows != 1))
        return OV3D_EINVAL;
    const int HW = H * W;
    const float wmax = float_at_most(W - 1), hmax = float_at_most(H - 1);
    hipStream_t s = ov3d_stream(stream);
    const dim3 grid((unsigned)(((long long)N + kComposeVerts - 1) / kComposeVerts));
    launch_frames(poses, F, params, table, s);
    if (bf16)
        hipLaunchKernelGGL(bp_compose_kernel<uint16_t>, grid, dim3(kThreads), 0, s, pts, N, depth, HW,
                           F, table, params, W, wmax, hmax, static_cast<const uint16_t*>(feat), C,
                           rows, static_cast<uint16_t*>(out), frame);
    else
        hipLaunchKernelGGL(bp_compose_kernel<uint32_t>, grid, dim3(kThreads), 0, s, pts, N, depth, HW,
                           F, table, params, W, wmax, hmax, static_cast<const uint32_t*>(feat), C,
                           rows, static_cast<uint32_t*>(out), frame);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

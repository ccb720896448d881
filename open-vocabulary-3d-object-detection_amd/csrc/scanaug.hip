// ScanNet training-data pipeline on the device (second dataset).
//
// Replaces ScannetDetectionDataset.__getitem__ (datasets/scannet.py:256-417) with
// use_image=False, use_height=False: colour normalisation (:287-293), random_sampling
// (:319-321, utils/pc_util.py:24-32), the flips and the small rotation about z (:339-357,
// rotate_aligned_boxes :148-169), the label build and the normalisations (:359-416), and
// the feature_2d row gather (:332-333).
//
// Every random draw comes from the host (scannet.py builds the plan with the reference's
// numpy calls in the reference's order); these kernels apply it.  The reference samples
// first and augments the num_points sampled vertices only, so one launch gathers,
// augments and writes the outputs.  Arithmetic follows numpy operation by operation, in
// the type numpy uses (T = the raw vertices' dtype, float or double):
//   np.dot(points, R^T)        -> dgemm: acc = +0, then fma(a_k, b_k, acc) for k = 0..2, f64
//   f32 array op f64 array     -> computed in f64, stored to the T array (one rounding)
//   f32 array op python scalar -> f32
// so every output is bit-identical to the reference's (tests/test_scannet_aug_*.py); the box
// corners are at angle 0 (cos = 1, sin = 0 exactly) and can differ in the sign of a zero only.
//
// Layout: raw scans resident in HBM, (S, n_stride, 6) vertices of type T (xyz + rgb),
// (S, k_stride, 7) float64 boxes (centre, lengths, nyu40 id); a batch is a list of scan
// indices.
#include <float.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGatherUnroll = 4;   // rows in flight per thread of the row gather

// one element of a BLAS dgemm with K = 3 (np.dot of the reference): the accumulator starts
// at +0 and takes one fma per k (sunaug.hip uses the same chain for the same numpy call)
__device__ __forceinline__ double dgemm3(double a0, double b0, double a1, double b1, double a2,
                                         double b2) {
    return fma(a2, b2, fma(a1, b1, fma(a0, b0, 0.0)));
}

// ---------------------------------------------------------------------------
// (1) sample + augment: out[b, j] = augment(raw[scene_idx[b], choices[b, j]]).
//     params (B, 8) f64: [flip_x, flip_y, cos, sin, 0, 0, 0, 0].  Per-block partial
//     min / max of the written xyz (point_cloud_dims_min / max, scannet.py:360-361).
template <typename T>
__global__ __launch_bounds__(kThreads) void sample_aug_kernel(
    const T* __restrict__ raw, long long n_stride, int S, const int64_t* __restrict__ sidx,
    const int32_t* __restrict__ nverts, const int64_t* __restrict__ choices, int N,
    const double* __restrict__ params, int augment, int use_color, float* __restrict__ out_pc,
    T* __restrict__ out_color, T* __restrict__ part) {
    const int b = blockIdx.y;
    const long long scene = sidx[b];
    const bool scene_ok = scene >= 0 && scene < S;
    const int n = scene_ok ? nverts[scene] : 0;
    const double* P = params + b * 8;
    const int C = use_color ? 6 : 3;
    T lo[3] = {(T)INFINITY, (T)INFINITY, (T)INFINITY}, hi[3] = {-(T)INFINITY, -(T)INFINITY, -(T)INFINITY};
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < N) {
        const long long o = (long long)b * N + j;
        const long long srow = choices[o];
        T v[6] = {(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
        if (srow >= 0 && srow < n) {      // the host draws choices in [0, n): never read past a scan
            const T* src = raw + (scene * n_stride + srow) * 6;
#pragma unroll
            for (int a = 0; a < 6; ++a) v[a] = src[a];
        }
        T x = v[0], y = v[1], z = v[2];
        if (augment) {
            if (P[0] != 0.0) x = -x;                              // -1 * pc[:, 0]
            if (P[1] != 0.0) y = -y;                              // -1 * pc[:, 1]
            // np.dot(pc[:, 0:3], rotz^T) in f64, R = [[c,-s,0],[s,c,0],[0,0,1]], stored as T
            const double c = P[2], s = P[3];
            const double dx = (double)x, dy = (double)y, dz = (double)z;
            x = (T)dgemm3(dx, c, dy, -s, dz, 0.0);
            y = (T)dgemm3(dx, s, dy, c, dz, 0.0);
            z = (T)dgemm3(dx, 0.0, dy, 0.0, dz, 1.0);
        }
        T col[3] = {v[3], v[4], v[5]};
        if (use_color) {
            // (pc[:, 3:] - MEAN_COLOR_RGB) / 256.0: f64, stored into the T array
            col[0] = (T)(((double)v[3] - 109.8) / 256.0);
            col[1] = (T)(((double)v[4] - 97.2) / 256.0);
            col[2] = (T)(((double)v[5] - 83.8) / 256.0);
        }
        float* dst = out_pc + o * C;
        dst[0] = (float)x;
        dst[1] = (float)y;
        dst[2] = (float)z;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (use_color) dst[3 + a] = (float)col[a];
            out_color[o * 3 + a] = col[a];
        }
        lo[0] = x; lo[1] = y; lo[2] = z;
        hi[0] = x; hi[1] = y; hi[2] = z;
    }
    __shared__ T s_red[6][kThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int off = 32; off >= 1; off >>= 1) {
            lo[a] = fmin(lo[a], (T)__shfl_xor(lo[a], off));
            hi[a] = fmax(hi[a], (T)__shfl_xor(hi[a], off));
        }
        if (lane == 0) { s_red[a][w] = lo[a]; s_red[3 + a][w] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        T r = s_red[a][0];
        for (int q = 1; q < kThreads / 64; ++q) r = a < 3 ? fmin(r, s_red[a][q]) : fmax(r, s_red[a][q]);
        part[((long long)b * gridDim.x + blockIdx.x) * 6 + a] = r;
    }
}

// ---------------------------------------------------------------------------
// (2) labels (scannet.py:301-307, 335-416), one workgroup per scene: all threads reduce the
//     dims partials, then one thread per box slot.
template <typename T>
__global__ void scan_labels_kernel(ov3d_scan_labels_args a) {
    const int b = blockIdx.x;
    const int i = threadIdx.x;
    const int G = a.max_num_obj;
    const long long scene = a.scene_idx[b];
    const bool scene_ok = scene >= 0 && scene < a.S;
    const int k = scene_ok ? min(a.nbox[scene], a.k_stride) : 0;
    // point_cloud_dims_min / max from the sampled points' partials (exact in any order)
    const T* dp = (const T*)a.dims_part;
    T dmin[3] = {(T)INFINITY, (T)INFINITY, (T)INFINITY}, dmax[3] = {-(T)INFINITY, -(T)INFINITY, -(T)INFINITY};
    for (int q = i; q < a.n_dims_part; q += blockDim.x) {
        const T* p = dp + ((long long)b * a.n_dims_part + q) * 6;
        for (int c = 0; c < 3; ++c) { dmin[c] = fmin(dmin[c], p[c]); dmax[c] = fmax(dmax[c], p[3 + c]); }
    }
    __shared__ T s_red[6][4];                       // at most 256 threads: 4 waves
    const int nwave = blockDim.x >> 6;
    for (int c = 0; c < 3; ++c) {
        for (int off = 32; off >= 1; off >>= 1) {
            dmin[c] = fmin(dmin[c], (T)__shfl_xor(dmin[c], off));
            dmax[c] = fmax(dmax[c], (T)__shfl_xor(dmax[c], off));
        }
        if ((i & 63) == 0) { s_red[c][i >> 6] = dmin[c]; s_red[3 + c][i >> 6] = dmax[c]; }
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) {
        dmin[c] = s_red[c][0];
        dmax[c] = s_red[3 + c][0];
        for (int q = 1; q < nwave; ++q) { dmin[c] = fmin(dmin[c], s_red[c][q]); dmax[c] = fmax(dmax[c], s_red[3 + c][q]); }
    }
    if (i < 3) {
        a.dims_min[b * 3 + i] = (float)dmin[i];
        a.dims_max[b * 3 + i] = (float)dmax[i];
    }
    if (i >= G) return;
    const long long o = (long long)b * G + i;
    const bool present = i < k;
    // target_bboxes (MAX_NUM_OBJ, 6) float32, zero rows past the scan's boxes (:302, :336)
    float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t sem = 0;
    if (present) {
        const double* bx = a.boxes + (scene * a.k_stride + i) * 7;
        for (int c = 0; c < 6; ++c) t[c] = (float)bx[c];
        const int id = (int)bx[6];
        sem = id >= 0 && id < a.n_id2class ? a.id2class[id] : 0;   // the host validated every id
    }
    float center[3], size[3];
    if (a.augment) {
        const double* P = a.params + b * 8;
        if (P[0] != 0.0) t[0] = -1.f * t[0];
        if (P[1] != 0.0) t[1] = -1.f * t[1];
        // rotate_aligned_boxes (:148-169) on the float32 target, rot_mat float64
        const double c = P[2], s = P[3];
        const double x = (double)t[0], y = (double)t[1], z = (double)t[2];
        center[0] = (float)dgemm3(x, c, y, -s, z, 0.0);
        center[1] = (float)dgemm3(x, s, y, c, z, 0.0);
        center[2] = (float)dgemm3(x, 0.0, y, 0.0, z, 1.0);
        const float dx = t[3] / 2.0f, dy = t[4] / 2.0f;         // lengths / 2.0 stays float32
        const float sx[4] = {-1.f, 1.f, 1.f, -1.f}, sy[4] = {-1.f, -1.f, 1.f, 1.f};
        double mx = -INFINITY, my = -INFINITY;
        for (int q = 0; q < 4; ++q) {
            const double cx = (double)(sx[q] * dx), cy = (double)(sy[q] * dy);
            mx = fmax(mx, dgemm3(cx, c, cy, -s, 0.0, 0.0));
            my = fmax(my, dgemm3(cx, s, cy, c, 0.0, 0.0));
        }
        size[0] = (float)(2.0 * mx);
        size[1] = (float)(2.0 * my);
        size[2] = t[5];
    } else {
        for (int c = 0; c < 3; ++c) { center[c] = t[c]; size[c] = t[3 + c]; }
    }
    // shift_scale_points / scale_points (pc_util.py:61-66, 72) with the sampled points' range
    const T mask = present ? (T)1.0f : (T)0.0f;
    float size_n[3], center_n[3];
    for (int c = 0; c < 3; ++c) {
        const T src_diff = dmax[c] - dmin[c];
        const T v = (((T)center[c] - dmin[c]) * (T)1.0f) / src_diff + (T)0.0f;
        center_n[c] = (float)(v * mask);                         // * target_bboxes_mask[..., None]
        const T inv = (T)1.0 / (dmax[c] - dmin[c]);              // 1.0 / mult_factor
        size_n[c] = (float)((T)size[c] * inv);
    }
    // flip_axis_to_camera_np + get_3d_box_batch_np at angle 0: R = roty(0), cos = 1, sin = 0
    const float cam[3] = {center[0], -1.f * center[2], center[1]};
    const double L = (double)(size[0] / 2), W = (double)(size[1] / 2), H = (double)(size[2] / 2);
    const double px[8] = {L, L, -L, -L, L, L, -L, -L};
    const double py[8] = {H, H, H, H, -H, -H, -H, -H};
    const double pz[8] = {W, -W, -W, W, W, -W, -W, W};
    float* cor = a.corners + o * 24;
    for (int q = 0; q < 8; ++q) {
        const double vx = dgemm3(px[q], 1.0, py[q], 0.0, pz[q], 0.0);
        const double vy = dgemm3(px[q], 0.0, py[q], 1.0, pz[q], 0.0);
        const double vz = dgemm3(px[q], -0.0, py[q], 0.0, pz[q], 1.0);
        cor[q * 3 + 0] = (float)(vx + (double)cam[0]);
        cor[q * 3 + 1] = (float)(vy + (double)cam[1]);
        cor[q * 3 + 2] = (float)(vz + (double)cam[2]);
    }
    for (int c = 0; c < 3; ++c) {
        a.centers[o * 3 + c] = center[c];
        a.centers_normalized[o * 3 + c] = center_n[c];
        a.sizes[o * 3 + c] = size[c];
        a.sizes_normalized[o * 3 + c] = size_n[c];
    }
    a.sem_cls[o] = sem;
    a.present[o] = present ? 1.f : 0.f;
    a.angles[o] = 0.f;
    a.angle_cls[o] = 0;
    a.angle_res[o] = 0.f;
}

// ---------------------------------------------------------------------------
// (3) row gather: out[b, j, :] = feat[scene_idx[b], choices[b, j], :] in units of V
//     (16, 4 or 2 bytes).  1 << lshift threads share a row (consecutive units: coalesced
//     within the row), a workgroup takes kGatherUnroll x (kThreads >> lshift) rows and each
//     thread keeps kGatherUnroll independent loads in flight.  Every byte is touched once, so
//     loads and stores are nontemporal: back to back with other streaming launches that took
//     122 -> 106 us at 8 x 40000 rows of 1 KB (plain stores leave 328 MB of dirty lines for
//     the next launch to wait on).  64-bit offsets throughout: S * rows_per_scene * units
//     passes 2^31 at the real shape.
template <typename V>
__global__ __launch_bounds__(kThreads) void rows_gather_kernel(
    const V* __restrict__ feat, long long rows_per_scene, int units, int S,
    const int64_t* __restrict__ sidx, const int64_t* __restrict__ choices, int N, int lshift,
    V* __restrict__ out) {
    const int b = blockIdx.y;
    const int rows_pass = kThreads >> lshift;
    const int col0 = threadIdx.x & ((1 << lshift) - 1);
    const int sub = threadIdx.x >> lshift;
    const long long scene = sidx[b];
    const bool scene_ok = scene >= 0 && scene < S;
    const V* src[kGatherUnroll];
    V* dst[kGatherUnroll];
#pragma unroll
    for (int u = 0; u < kGatherUnroll; ++u) {
        const long long j = ((long long)blockIdx.x * kGatherUnroll + u) * rows_pass + sub;
        src[u] = nullptr;
        dst[u] = nullptr;
        if (j < N) {
            const long long o = (long long)b * N + j;
            const long long r = choices[o];
            dst[u] = out + o * units;
            if (scene_ok && r >= 0 && r < rows_per_scene) src[u] = feat + (scene * rows_per_scene + r) * units;
        }
    }
    for (int col = col0; col < units; col += 1 << lshift) {
        V v[kGatherUnroll];
#pragma unroll
        for (int u = 0; u < kGatherUnroll; ++u) v[u] = src[u] ? __builtin_nontemporal_load(src[u] + col) : V{};
#pragma unroll
        for (int u = 0; u < kGatherUnroll; ++u)
            if (dst[u]) __builtin_nontemporal_store(v[u], dst[u] + col);
    }
}

template <typename V>
void launch_rows_gather(const void* feat, long long rows_per_scene, long long row_bytes, int S,
                        const int64_t* sidx, const int64_t* choices, int B, int N, void* out,
                        hipStream_t s) {
    const int units = (int)(row_bytes / (long long)sizeof(V));
    int lshift = 0;
    while (lshift < 6 && (1 << lshift) < units) ++lshift;      // threads per row: pow2 <= 64
    const int rows_block = kGatherUnroll * (kThreads >> lshift);
    const dim3 grid(ov3d_cdiv(N, rows_block), B);
    hipLaunchKernelGGL(rows_gather_kernel<V>, grid, dim3(kThreads), 0, s, (const V*)feat,
                       rows_per_scene, units, S, sidx, choices, N, lshift, (V*)out);
}

typedef uint32_t vec16 __attribute__((ext_vector_type(4)));

}  // namespace

extern "C" int ov3d_scan_parts(int n) { return (n + kThreads - 1) / kThreads; }

extern "C" int ov3d_scan_sample_aug(const void* raw, int pc_f64, long long n_stride, int S,
                                    const int64_t* scene_idx, const int32_t* nverts,
                                    const int64_t* choices, int B, int N, const double* params,
                                    int augment, int use_color, float* out_pc, void* out_color,
                                    void* dims_part, void* stream) {
    if (!raw || !scene_idx || !nverts || !choices || !params || !out_pc || !out_color ||
        !dims_part || B <= 0 || N <= 0 || S <= 0 || n_stride <= 0 || B > 65535)
        return OV3D_EINVAL;
    const dim3 grid(ov3d_scan_parts(N), B);
    hipStream_t s = ov3d_stream(stream);
    if (pc_f64)
        hipLaunchKernelGGL(sample_aug_kernel<double>, grid, dim3(kThreads), 0, s, (const double*)raw,
                           n_stride, S, scene_idx, nverts, choices, N, params, augment, use_color,
                           out_pc, (double*)out_color, (double*)dims_part);
    else
        hipLaunchKernelGGL(sample_aug_kernel<float>, grid, dim3(kThreads), 0, s, (const float*)raw,
                           n_stride, S, scene_idx, nverts, choices, N, params, augment, use_color,
                           out_pc, (float*)out_color, (float*)dims_part);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_scan_labels(const ov3d_scan_labels_args* a, void* stream) {
    if (!a || a->B <= 0 || a->S <= 0 || a->max_num_obj <= 0 || a->max_num_obj > 256 ||
        a->k_stride <= 0 || a->n_dims_part <= 0 || a->n_id2class <= 0 || !a->boxes || !a->nbox ||
        !a->scene_idx || !a->params || !a->dims_part || !a->id2class || !a->dims_min ||
        !a->dims_max || !a->corners || !a->centers || !a->centers_normalized || !a->sem_cls ||
        !a->present || !a->sizes || !a->sizes_normalized || !a->angles || !a->angle_cls ||
        !a->angle_res)
        return OV3D_EINVAL;
    const int threads = ((max(a->max_num_obj, 3) + 63) / 64) * 64;
    if (a->pc_f64)
        hipLaunchKernelGGL(scan_labels_kernel<double>, dim3(a->B), dim3(threads), 0,
                           ov3d_stream(stream), *a);
    else
        hipLaunchKernelGGL(scan_labels_kernel<float>, dim3(a->B), dim3(threads), 0,
                           ov3d_stream(stream), *a);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_rows_gather(const void* feat, long long rows_per_scene, long long row_bytes,
                                int S, const int64_t* scene_idx, const int64_t* choices, int B,
                                int N, int vec_bytes, void* out, void* stream) {
    if (!feat || !scene_idx || !choices || !out || B <= 0 || N <= 0 || S <= 0 ||
        rows_per_scene <= 0 || row_bytes <= 0 || (row_bytes & 1) || B > 65535 ||
        row_bytes > (1ll << 30))
        return OV3D_EINVAL;
    const uintptr_t bits = (uintptr_t)feat | (uintptr_t)out | (uintptr_t)row_bytes;
    if (vec_bytes == 0) vec_bytes = (bits & 15) == 0 ? 16 : (bits & 3) == 0 ? 4 : 2;
    if ((vec_bytes != 16 && vec_bytes != 4 && vec_bytes != 2) || (bits & (uintptr_t)(vec_bytes - 1)))
        return OV3D_EINVAL;     // odd base pointer, or misaligned for the path asked for
    hipStream_t s = ov3d_stream(stream);
    if (vec_bytes == 16)
        launch_rows_gather<vec16>(feat, rows_per_scene, row_bytes, S, scene_idx, choices, B, N, out, s);
    else if (vec_bytes == 4)
        launch_rows_gather<uint32_t>(feat, rows_per_scene, row_bytes, S, scene_idx, choices, B, N, out, s);
    else
        launch_rows_gather<uint16_t>(feat, rows_per_scene, row_bytes, S, scene_idx, choices, B, N, out, s);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

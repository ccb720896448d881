/* C ABI of the multiview back-projection kernels (csrc/backproj.hip), part of libov3d_hip.so.
 *
 * Frame features -> per-vertex features (utils/projection.py ProjectionHelper.compute_projection
 * and .project, utils/image_util.py image_processor.compute_projection).  ov3d_amd.projection
 * drives these entries; ov3d_amd._native derives their ctypes signatures from this file, as
 * from every include/ov3d*.h; their guard-band cases are in tests/test_backproj_gpu.py.
 *
 * All arithmetic is float32 without contraction (the world-to-camera inverse alone is formed in
 * float64 and rounded), every sum in the order written here; tests/backproj_ref.py restates it
 * in numpy float32 and agrees bit for bit.  Every entry validates its arguments and returns
 * OV3D_EINVAL before any launch; stream is the HIP stream (NULL: the default stream).  Nothing
 * synchronises.
 *
 * params (32) f32, the helper's constants:
 *   0 fx  1 fy  2 cx  3 cy  4 depth_min  5 depth_max  6 accuracy  7 unused
 *   8..31 corner_points (8,3): the image corners (0,0), (W-1,0), (W-1,H-1), (0,H-1) at depth_min,
 *   then at depth_max, in camera coordinates (formed on the host in double, as the reference
 *   forms them in Python floats, and rounded once).
 * W, H = image_dims[0], image_dims[1] (41, 32); depth maps are (H,W) row-major.
 *
 * Frame table, one row of OV3D_BACKPROJ_ROW f32 per frame, from pose P (4,4) camera-to-world:
 *   0..11  rows 0-2 of the world-to-camera matrix.  With a = (double)P and the 2x2 minors
 *          s0 = a00 a11 - a10 a01, s1 = a00 a12 - a10 a02, s2 = a00 a13 - a10 a03,
 *          s3 = a01 a12 - a11 a02, s4 = a01 a13 - a11 a03, s5 = a02 a13 - a12 a03,
 *          c5 = a22 a33 - a32 a23, c4 = a21 a33 - a31 a23, c3 = a21 a32 - a31 a22,
 *          c2 = a20 a33 - a30 a23, c1 = a20 a32 - a30 a22, c0 = a20 a31 - a30 a21,
 *          det = ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0, the inverse b is
 *          b00 = ((a11 c5 - a12 c4) + a13 c3) / det    b01 = ((-a01 c5 + a02 c4) - a03 c3) / det
 *          b02 = ((a31 s5 - a32 s4) + a33 s3) / det    b03 = ((-a21 s5 + a22 s4) - a23 s3) / det
 *          b10 = ((-a10 c5 + a12 c2) - a13 c1) / det   b11 = ((a00 c5 - a02 c2) + a03 c1) / det
 *          b12 = ((-a30 s5 + a32 s2) - a33 s1) / det   b13 = ((a20 s5 - a22 s2) + a23 s1) / det
 *          b20 = ((a10 c4 - a11 c2) + a13 c0) / det    b21 = ((-a00 c4 + a01 c2) - a03 c0) / det
 *          b22 = ((a30 s4 - a31 s2) + a33 s0) / det    b23 = ((-a20 s4 + a21 s2) - a23 s0) / det
 *          b30 = ((-a10 c3 + a11 c1) - a12 c0) / det   b31 = ((a00 c3 - a01 c1) + a02 c0) / det
 *          b32 = ((-a30 s3 + a31 s1) - a32 s0) / det   b33 = ((a20 s3 - a21 s1) + a22 s0) / det
 *          each rounded to f32 (the reference calls torch.inverse in f32; the difference is
 *          inside the margin the golden data keeps from every threshold).
 *   12..14 frustum corner 2, 15..17 corner 4; corner k = P . (corner_points[k], 1), component
 *          i = ((P[i][0] x + P[i][1] y) + P[i][2] z) + P[i][3].
 *   18..35 the six inward normals (6,3), unnormalised as in the reference:
 *          cross(c[a] - c[o], c[b] - c[o]) for (a, b, o) = (3,1,0) (2,5,1) (3,6,2) (0,7,3)
 *          (1,4,0) (6,4,5), cross(u, v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x).
 *   36     1.0 for a usable frame.
 *   37..39 zero.
 * A frame whose pose or whose rounded inverse (all 16 entries) has a non-finite entry is empty:
 * its row is all zero (flag included) and it maps nothing.  ScanNet ships -inf poses; a singular
 * pose has det = 0.  The reference's torch.inverse raises or yields NaN there: an extension.
 *
 * The decision for (frame, point p), shared by the index tables and the fused compose:
 *   v = p - corner2, w = p - corner4; for normal n_k: dot = (v.x n.x + v.y n.y) + v.z n.z (w
 *   for k >= 3); inside iff rint(100 * dot) / 100 < 0 for all six, rint half to even (so a dot
 *   of exactly -0.005 is outside; the kernel tests rint(100 * dot) < 0, the same predicate).
 *   cam_i = ((b[i][0] p.x + b[i][1] p.y) + b[i][2] p.z) + b[i][3], i = 0..2;
 *   x = (cam.x * fx) / cam.z + cx, y = (cam.y * fy) / cam.z + cy, rx = rint(x), ry = rint(y);
 *   kept iff 0 <= rx < W and 0 <= ry < H; pixel = ry * W + rx; d = depth[pixel];
 *   kept iff depth_min <= d <= depth_max and |d - cam.z| <= accuracy.  Any NaN compares false.
 */
#ifndef OV3D_BACKPROJ_H_
#define OV3D_BACKPROJ_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OV3D_BACKPROJ_ROW 40       /* f32 per frame-table row */
#define OV3D_BACKPROJ_PARAMS 32    /* f32 in params */
#define OV3D_BACKPROJ_BLOCK 1024   /* points per workgroup of the index-table kernels */

/* Frame table alone, one launch of one thread per frame:
 *   poses (F,4,4) f32, params (32) f32 -> table (F, OV3D_BACKPROJ_ROW) f32.  F >= 1. */
int ov3d_backproj_frames(const float* poses, int F, const float* params, float* table,
                         void* stream);

/* Index tables of all frames (image_processor.compute_projection), three launches whatever F
 * and N: the frame table; a count per (frame, block of OV3D_BACKPROJ_BLOCK points); the write,
 * which repeats the decision and places every kept point by ballot and prefix, in point order.
 *   pts (N,3) f32, depth (F,H,W) f32, poses (F,4,4) f32;
 *   table (F, OV3D_BACKPROJ_ROW) f32 and counts (F, ceil(N / OV3D_BACKPROJ_BLOCK)) int32:
 *   workspaces, fully written.
 *   -> idx3d, idx2d (F, N+1) int64: slot 0 the number n of kept points, slots 1..n their indices
 *      ascending (idx3d) and their pixels (idx2d), every further slot 0 (written here, no
 *      memset).  An empty frame's rows are all zero.
 *   N >= 1, F >= 1, W >= 1, H >= 1, H * W < 2^31, N + 1 < 2^31. */
int ov3d_backproj_tables(const float* pts, int N, const float* depth, const float* poses, int F,
                         const float* params, int W, int H, float* table, int32_t* counts,
                         int64_t* idx3d, int64_t* idx2d, void* stream);

/* ProjectionHelper.project on one row of the tables, one launch:
 *   label (C, HW) f32 (bf16 0) or bfloat16 (bf16 1); idx3d, idx2d (N+1) int64 as written by
 *   ov3d_backproj_tables (n = slot 0 clamped to 0..N; slots 1..n of idx3d ascending).
 *   -> out (C, N) of label's type: column idx3d[k] = label[:, idx2d[k]] for k = 1..n, every
 *      other column 0; a pixel outside 0..HW-1 leaves its column 0.
 *   C >= 1, 1 <= HW < 2^31, N >= 1, N + 1 < 2^31. */
int ov3d_backproj_gather(const void* label, int bf16, int C, long long HW, const int64_t* idx3d,
                         const int64_t* idx2d, int N, void* out, void* stream);

/* Fused compose, two launches (the frame table, then one workgroup per 64 vertices): every
 * vertex takes the features of the LAST frame whose decision keeps it, as the loop
 *   out = 0; for i in frames: p = project(feat[i], idx3d[i], idx2d[i]); out[:, kept_i] = p[:, kept_i]
 * does; no tables, no atomics.
 *   pts, depth, poses, params, W, H, table as above; feat (F, C, H, W) f32 or bfloat16;
 *   rows 0: out (C, N); rows 1: out (N, C), of feat's type, 0 for a vertex no frame keeps;
 *   frame (N) int32: the winning frame, -1 for none.
 *   N, F, C, W, H >= 1, H * W < 2^31, N + 1 < 2^31. */
int ov3d_backproj_compose(const float* pts, int N, const float* depth, const float* poses, int F,
                          const float* params, int W, int H, const void* feat, int bf16, int C,
                          int rows, float* table, void* out, int32_t* frame, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OV3D_BACKPROJ_H_ */

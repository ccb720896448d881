/* C ABI of the pseudo-box lifting kernels (csrc/lift.hip), part of libov3d_hip.so.
 *
 * Stage 3 of the open-vocabulary pipeline: 2D detections + per-point (ScanNet) or per-pixel
 * (SUN RGB-D) labels -> 3D pseudo boxes (3DOVDet_tools/{scannet,sunrgbd}/lift_boxes.py with
 * utils/projection.py and utils/box_3d_utils.py).  ov3d_amd.lift_boxes drives these entries;
 * ov3d_amd._native derives their ctypes signatures from this file, as from every
 * include/ov3d*.h; their guard-band cases are in tests/test_lift_gpu.py.
 *
 * All arithmetic is float64 without contraction, in the reference's order wherever an order is
 * specified there.  Every entry validates its arguments and returns OV3D_EINVAL before any
 * launch; stream is the HIP stream (NULL: the default stream).  Nothing synchronises.
 */
#ifndef OV3D_LIFT_H_
#define OV3D_LIFT_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OV3D_LIFT_NMS_MAX 8192   /* rows of one ov3d_lift_nms call (one workgroup) */

/* Frustum lift (ProjectionHelper.compute_frustum_box, view 'multi'), two launches whatever M:
 *   pts (N,3) f32 (pt_f64 0) or f64 (pt_f64 1), axis-aligned, dense; labels (N) int32;
 *   align, align_inv (4,4) f64 row-major; planes (M,24) f64 = six inward normals (6,3), then
 *   frustum corners 2 and 4; plabel (M) int32; ws (N,6) f64 workspace.
 *   Per point once: o = align_inv . p (original frame), a = align . o (re-aligned), each row as
 *   ((m0 x + m1 y) + m2 z) + m3.  Per (frustum, point of its label): v = o - corner2 and
 *   w = o - corner4, each component divided by its squared norm (x^2 + y^2) + z^2; inside iff
 *   ((v.x n.x + v.y n.y) + v.z n.z) < 0 for normals 0-2 and the same with w for normals 3-5.
 *   A NaN compares false: a point on a corner, a zero normal or a non-finite pose is outside.
 *   -> lohi (M, lohi_ld >= 6) f64, columns 0-5 of every row: min xyz then max xyz of a over
 *      the members (zeros when none; further columns are the caller's), count (M) int32
 *      members.  N >= 1, M >= 1. */
int ov3d_lift_frustum(const void* pts, int pt_f64, int N, const int32_t* labels,
                      const double* align, const double* align_inv, const double* planes,
                      const int32_t* plabel, int M, double* ws, double* lohi, int lohi_ld,
                      int32_t* count, void* stream);

/* Image lift (sunrgbd/lift_boxes.py compute_box), one workgroup per 2D box over its rectangle:
 *   depth (H,W) int32 (depth_f64 0) or f64 (1); seg (H,W) int32; lut (lut_n) int32 or NULL:
 *   class of a pixel = lut[seg] for 0 <= seg < lut_n, else -100 (NULL: seg itself);
 *   boxes (k,6) f64 x, y, w, h, score, label; plabel (k) int32 = int(label);
 *   calib (13) f64 = f_u, f_v, c_u, c_v, Rtilt (3,3) row-major.
 *   Pixel (u, v) takes part iff u >= x, u <= x + w, v >= y, v <= y + h (f64) and its class is
 *   plabel; X = ((u - c_u) d) / f_u, Y = ((v - c_v) d) / f_v, point = Rtilt . (X, d, -Y) with
 *   rows (r0 p0 + r1 p1) + r2 p2.  Depth 0 takes part.
 *   -> lohi (k, lohi_ld >= 6) f64 columns 0-5 (zeros when no pixel), count (k) int32.
 *   H, W, k >= 1, H * W < 2^31. */
int ov3d_lift_image(const void* depth, int depth_f64, const int32_t* seg, const int32_t* lut,
                    int lut_n, int H, int W, const double* boxes, const int32_t* plabel, int k,
                    const double* calib, double* lohi, int lohi_ld, int32_t* count, void* stream);

/* Class-wise greedy NMS with box_3d_utils.nms_3d_faster's arithmetic (not ov3d_nms3d's):
 *   boxes (K, ld) f64 rows: 0-5 min xyz, max xyz; 6 score; 7 label; 8 size (read only with
 *   use_size_score: the sort key is score * size).  valid (K) int32 or NULL: rows with 0 are
 *   neither picked nor suppress.  volume = ((x2-x1)(y2-y1))(z2-z1) + 1e-8;
 *   o = inter / ((vol_i + vol_j) - inter) * (label_i == label_j); suppressed iff o > thresh.
 *   Picks go by descending key; equal keys: the higher row first (the reference leaves ties to
 *   argsort; not pinned by the tests).  Keys must not be NaN.
 *   -> rank (K) int32: position in pick order, -1 when not kept; keep (K) u8.
 *   0 <= K <= OV3D_LIFT_NMS_MAX, ld >= 8 (9 with use_size_score). */
int ov3d_lift_nms(const double* boxes, int ld, int K, const int32_t* valid, int use_size_score,
                  double thresh, int32_t* rank, uint8_t* keep, void* stream);

/* Pool match and the labelled pool rows (the loop over box_3d_iou of lift_boxes.py, closed form
 * proved in csrc/lift.hip), three launches:
 *   boxes (M, ld) f64 as ov3d_lift_nms's with rank (M) from it; pool (P,7) f64 centre, size;
 *   owner (P) int32 workspace.  Pool box j spans c - s/2 .. s + (c - s/2) (cs2vv);
 *   iou = inter / (((vq + vk) - inter) + 1e-5).  For every kept box: amax (M) int32 the first
 *   index of the largest iou (-1 for a dropped box) and maxiou (M) f64 (0 for a dropped box);
 *   the box is a candidate unless maxiou < match or its score is not > 0; pool box j takes the
 *   candidate of the smallest rank among those with amax == j.
 *   -> win (M) int32 1 for a box whose pool box took it; rows (M,10) f64: pool min, max, score,
 *      label, volume (sx sy) sz, area 2 ((sx sz + sy sx) + sz sy), ready for ov3d_lift_nms
 *      with use_size_score; out (M,10) f64: centre, size, label, score * volume, volume, area
 *      (vv2cs and the column swap).  Rows of boxes that did not win are zero.
 *   M >= 1, P >= 1, ld >= 8. */
int ov3d_lift_match(const double* boxes, int ld, const int32_t* rank, int M, const double* pool,
                    int P, double match, int32_t* owner, int32_t* amax, double* maxiou,
                    int32_t* win, double* rows, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OV3D_LIFT_H_ */

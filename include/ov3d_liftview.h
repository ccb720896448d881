/* C ABI of the single-view pseudo-box lift (csrc/liftview.hip), part of libov3d_hip.so.
 *
 * The 'single' view of 3DOVDet_tools/scannet/lift_boxes.py (utils/projection.py:242-251): a 2D
 * box of a frame lifts every pixel of the frame whose class equals the box's label, through the
 * depth map, the camera pose and the alignment matrix.  The lifted box depends on (frame, label)
 * only, so the host deduplicates the 2D boxes into slots, one per distinct pair; the cost
 * follows the slots, not the boxes.  ov3d_amd.lift_boxes drives the entry; ov3d_amd._native
 * derives its ctypes signature from this file, as from every include/ov3d*.h; the guard-band
 * cases are in tests/test_lift_single_gpu.py.
 *
 * All arithmetic is float64 without contraction in the order stated below.  The entry validates
 * its arguments and returns OV3D_EINVAL before any launch; stream is the HIP stream (NULL: the
 * default stream).  Nothing synchronises.
 */
#ifndef OV3D_LIFTVIEW_H_
#define OV3D_LIFTVIEW_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Single-view lift, two launches whatever F, S and M:
 *   depth (F,H,W): float32 metres (depth_u16 0) or uint16 raw millimetres (depth_u16 1), read as
 *   (float)raw / 1000.0f, the correctly rounded float32 quotient; seg (F,H,W) int32;
 *   lut (lut_n) int32 or NULL: class of a pixel = lut[seg] for 0 <= seg < lut_n, else -100;
 *   without a lut the class is seg itself, or -100 where seg >= ignore_from (compared as 64-bit
 *   integers, so 2^31 and above switches it off);
 *   kinv (3,3) f64 row-major, the inverse of the intrinsic; pose (F,12) f64: per frame the
 *   rotation R (3,3) row-major, then the translation t (3); align (4,4) f64 row-major;
 *   slot_frame, slot_label (S) int32; box_slot (M) int32: the slot of every 2D box;
 *   slot_lohi (S,6) f64 and slot_count (S) int32: workspace, the result per slot.
 *   Per slot, over every pixel (u, v) of its frame whose class equals slot_label (int32
 *   equality: a label of -100 lifts the ignored pixels), with depth d widened to f64:
 *     r_i = (kinv[i][0] u + kinv[i][1] v) + kinv[i][2],  c_i = r_i d
 *     w_i = ((c_0 R[i][0] + c_1 R[i][1]) + c_2 R[i][2]) + t_i
 *     a_i = ((A[i][0] w_0 + A[i][1] w_1) + A[i][2] w_2) + A[i][3]
 *   Depth 0 takes part (it lands on the camera centre).  Min and max skip a NaN.
 *   A slot whose frame is outside 0 .. F-1 holds no pixel; a box whose slot is outside
 *   0 .. S-1 lifts nothing.
 *   -> lohi (M, lohi_ld >= 6) f64, columns 0-5 of every row: min xyz then max xyz of a over the
 *      pixels of the box's slot (zeros when none; further columns are the caller's), count (M)
 *      int32 pixels.  F, H, W, S, M >= 1, H * W < 2^31. */
int ov3d_liftview_frames(const void* depth, int depth_u16, const int32_t* seg, const int32_t* lut,
                         int lut_n, long long ignore_from, int F, int H, int W,
                         const double* kinv, const double* pose, const double* align,
                         const int32_t* slot_frame, const int32_t* slot_label, int S,
                         const int32_t* box_slot, int M, double* slot_lohi, int32_t* slot_count,
                         double* lohi, int lohi_ld, int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OV3D_LIFTVIEW_H_ */

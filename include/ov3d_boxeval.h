/* C ABI of the pseudo-box evaluation kernels (csrc/boxeval.hip), part of libov3d_hip.so.
 *
 * Scores a split of pseudo boxes against ground-truth boxes by per-class precision and recall
 * at up to OV3D_BOXEVAL_MAX_T IoU thresholds at once (3DOVDet_tools/scannet/evaluate_box.py with
 * utils/evaluation/pr_helper.py PRCalculator, eval_det.py eval_det_cls and get_iou, and
 * evaluation/box_util.py calc_iou).  ov3d_amd.box_eval drives these entries; ov3d_amd._native
 * derives their ctypes signatures from this file, as from every include/ov3d*.h; their
 * guard-band cases are in tests/test_box_eval_gpu.py.
 *
 * All arithmetic is float64 without contraction, in the reference's order.  Every entry
 * validates its arguments and returns OV3D_EINVAL before any launch; stream is the HIP stream
 * (NULL: the default stream).  Nothing synchronises; no atomics; every output element is
 * written by exactly one thread, so no output needs clearing.
 */
#ifndef OV3D_BOXEVAL_H_
#define OV3D_BOXEVAL_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OV3D_BOXEVAL_MAX_T 16   /* thresholds of one call */

/* Match, one workgroup per scan.  The scans are in CSR form: scan s owns the prediction rows
 * pred_off[s] .. pred_off[s+1]-1 and the GT rows gt_off[s] .. gt_off[s+1]-1 (pred_off, gt_off
 * (S+1) int32, ascending, pred_off[0] = gt_off[0] = 0, pred_off[S] = P, gt_off[S] = G).
 *   pred (P, ldp >= 6) f64 and gt (G, ldg >= 6) f64: centre xyz, size xyz in columns 0-5, the
 *   further columns are not read; pred_cls (P), gt_cls (G) int32; score (P) f64; thr (T) f64.
 *   Values must be finite (the host refuses others).
 * Per prediction p of a scan:
 *   rank[p]   the number of predictions of the scan with a larger score, or an equal score and
 *             a lower row (its place in the scan's descending order);
 *   jmax[p], ovmax[p]   a walk over the scan's GT rows of p's class in row order:
 *             hi = c + s/2, lo = c - s/2 per box and axis; m = min(hi_p, hi_g),
 *             x = max(lo_p, lo_g); iou = 0.0 unless m > x on all three axes, else
 *             inter = ((mx-xx)(my-xy))(mz-xz), union = (vol_p + vol_g) - inter with
 *             vol = (sx sy) sz, iou = inter / union, below 0 -> 0, above 1 -> 1; the row is
 *             taken iff iou > ovmax (strict: the first maximum wins; a NaN is never taken).
 *             jmax is the global GT row; -1 with ovmax = -inf when no row was taken.
 * Per GT row j: best[j] the largest ovmax over the predictions with jmax == j (-inf without
 *   one); owner[t*G + j] the smallest rank over those with ovmax > thr[t] (2^31-1 without one).
 * tp[t*P + p] = ovmax[p] > thr[t] && owner[t*G + jmax[p]] == rank[p]: the detection that
 *   eval_det_cls marks as the true positive of its GT box when detections go by descending
 *   score, equal scores by ascending row.
 * P == 0 or G == 0 is valid (their pointers may then be NULL); S >= 1, 1 <= T <= MAX_T. */
int ov3d_boxeval_match(const double* pred, int ldp, const int32_t* pred_cls, const double* score,
                       const int32_t* pred_off, long long P, const double* gt, int ldg,
                       const int32_t* gt_cls, const int32_t* gt_off, long long G, int S,
                       const double* thr, int T, int32_t* rank, int32_t* jmax, double* ovmax,
                       double* best, int32_t* owner, uint8_t* tp, void* stream);

/* Tally, one workgroup per class c of 0 .. C-1 over all predictions and GT rows:
 *   nd[c] predictions of the class, npos[c] GT rows of the class, ntp[t*C + c] GT rows of the
 *   class with best > thr[t] = the true positives of the class at thr[t] (closed form in
 *   csrc/boxeval.hip; equal to the sum of tp over the class's predictions).  Class ids
 *   outside 0 .. C-1 are counted nowhere.
 *   C >= 1, 1 <= T <= MAX_T; P == 0 or G == 0 is valid. */
int ov3d_boxeval_tally(const int32_t* pred_cls, long long P, const int32_t* gt_cls,
                       const double* best, long long G, const double* thr, int T, int C,
                       int32_t* nd, int32_t* npos, int32_t* ntp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OV3D_BOXEVAL_H_ */

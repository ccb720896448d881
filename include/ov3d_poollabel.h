/* C ABI of the proposal-pool labelling and pseudo-label assessment kernels (csrc/poollabel.hip),
 * part of libov3d_hip.so.
 *
 * ov3d_poollabel_vote labels an unlabelled proposal pool by a per-box vote over per-vertex
 * labels (3DOVDet_tools/scannet/assign_box_label_from_gt.py, labeling); ov3d_poollabel_confusion
 * counts the agreement of per-pixel pseudo labels with ground-truth frames
 * (3DOVDet_tools/scannet/assess_pseudo_label.py, match).  ov3d_amd.pool_label and
 * ov3d_amd.label_assess drive them; ov3d_amd._native derives their ctypes signatures from this
 * file, as from every include/ov3d*.h; their guard-band cases are in
 * tests/test_pool_label_gpu.py.
 *
 * Both are integer decisions: no floating-point arithmetic happens on the device, only the
 * exact widening of a float32 vertex to double and compares.  Every entry validates its
 * arguments and returns OV3D_EINVAL before any launch; stream is the HIP stream (NULL: the
 * default stream).  Nothing synchronises; both are legal inside a hipGraph capture.
 */
#ifndef OV3D_POOLLABEL_H_
#define OV3D_POOLLABEL_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OV3D_POOLLABEL_MAX_C 64   /* label bins of the vote */
#define OV3D_POOLLABEL_MAX_K 31   /* classes of the confusion matrix (bin K: ignored) */

/* Vote of a group of scans, one launch.  The scans are in CSR form: scan s owns the vertices
 * pt_off[s] .. pt_off[s+1]-1 and the pool boxes box_off[s] .. box_off[s+1]-1 (pt_off, box_off
 * (S+1) int32, ascending, pt_off[0] = box_off[0] = 0, pt_off[S] = N, box_off[S] = P).
 *   pts     N rows of ld >= 3 elements, float32 (pt_f64 = 0) or float64 (pt_f64 = 1): xyz in
 *           elements 0-2 of a row, the further ones are not read;
 *   labels  (N) uint8, one per vertex;
 *   boxes   (P, 6) f64: closed bounds lo xyz, hi xyz.
 * A vertex is inside a box iff (double)x >= lo && (double)x <= hi on all three axes: a NaN is
 * never inside, lo > hi is empty.  A vertex votes iff min_label <= label < C.
 *   counts  (P, C) int32: counts[b][l] the voting vertices of b's scan inside box b with label l
 *           (the bins below min_label are written as 0);
 *   mode    (P) int32: the smallest label among the most frequent (scipy.stats.mode), -1 when no
 *           vertex voted.
 * Every element of counts and mode is written by exactly one thread: nothing needs clearing.
 * 1 <= C <= OV3D_POOLLABEL_MAX_C, 0 <= min_label <= C, S >= 1; N == 0 or P == 0 is valid (their
 * pointers may then be NULL; P == 0 launches nothing), and so are empty scans and scans without
 * boxes.  Offsets past a scan's base are 64-bit: N * ld * sizeof(element) may exceed 2^31. */
int ov3d_poollabel_vote(const void* pts, int pt_f64, long long ld, const uint8_t* labels,
                        const int32_t* pt_off, long long N, const double* boxes,
                        const int32_t* box_off, long long P, int S, int min_label, int C,
                        int32_t* counts, int32_t* mode, void* stream);

/* Label agreement of a group of scans, one launch behind a clear.  Scan s owns the frames
 * frame_off[s] .. frame_off[s+1]-1 (frame_off (S+1) int32, ascending, frame_off[0] = 0,
 * frame_off[S] = F).
 *   gt, pseudo  (F, HW) uint8, dense; gt_map (256) uint8.
 * Per pixel g = min(gt_map[gt], K) and p = min(pseudo, K): bin K is "ignored".
 *   conf  (S, K+1, K+1) int64: conf[s][g][p] the number of pixels of scan s with that pair.
 * The entry clears conf itself (a memset node on the same stream ahead of the kernel): the
 * caller clears nothing.  Workgroups keep int32 partial histograms in LDS and add their
 * non-zero cells into conf with 64-bit integer atomics, so the result does not depend on the
 * order of arrival.  Rows are read 16 bytes at a time from the first 16-byte-aligned address
 * of the scan's own rows when gt and pseudo share that alignment, byte by byte otherwise.
 * 1 <= K <= OV3D_POOLLABEL_MAX_K, S >= 1, HW >= 1; F == 0 is valid (gt and pseudo may then be
 * NULL) and so are scans without frames. */
int ov3d_poollabel_confusion(const uint8_t* gt, const uint8_t* pseudo, const int32_t* frame_off,
                             long long F, long long HW, int S, const uint8_t* gt_map, int K,
                             long long* conf, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OV3D_POOLLABEL_H_ */

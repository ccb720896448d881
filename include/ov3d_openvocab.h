/* C ABI of the open-vocabulary classification kernel (csrc/openvocab.hip), part of
 * libov3d_hip.so.
 *
 * Feature vectors against the text embeddings of a vocabulary -> one class index per vector:
 * the step the reference leaves open (datasets/scannet.py:272, "TODO: acquire semantic labels
 * using LSeg / OpenSeg + projection") and whose results its tools read from disk.
 * ov3d_amd.open_vocab drives the entry; ov3d_amd._native derives its ctypes signature from this
 * file, as from every include/ov3d*.h; its guard-band cases are in
 * tests/test_open_vocab_gpu.py.
 *
 * The entry validates its arguments and returns OV3D_EINVAL before any launch; stream is the
 * HIP stream (NULL: the default stream).  One launch, nothing synchronises, no atomics; legal
 * inside a hipGraph capture.
 */
#ifndef OV3D_OPENVOCAB_H_
#define OV3D_OPENVOCAB_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OV3D_OPENVOCAB_F32 0
#define OV3D_OPENVOCAB_BF16 1
#define OV3D_OPENVOCAB_F16 2
#define OV3D_OPENVOCAB_MAX_T 256    /* vocabulary entries */
#define OV3D_OPENVOCAB_MAX_C 4096   /* channels */
#define OV3D_OPENVOCAB_ROWS 64      /* feature vectors per workgroup */

/* R feature vectors ("rows") of C channels against text (T, C), all of one element type
 * (dtype: OV3D_OPENVOCAB_F32 / _BF16 / _F16).
 *   planes 0: feat (R, C) contiguous; P is not read.
 *   planes 1: feat (F, C, P) contiguous with R = F * P: row r = f * P + p has channel c at
 *             (f * C + c) * P + p.  This is a stack of channel-first maps (F, C, H, W), P = H * W.
 * Per row, s_t = sum over c of feat[c] * text[t][c]: the products are exact in float32 and
 * the sum is kept in float32 (MFMA 16x16x32 for the 2-byte types, the float32-input 16x16x4
 * form for float32, whose operands are not rounded).  The channels are taken in chunks of 128
 * bytes of a row in ascending order, each output element in an accumulator of its own: what a
 * row gets depends on its own values and the text only, never on the layout, on its place in
 * the launch or on its neighbours.
 *   label (R) int32: the smallest t with the largest s_t (t ascending, replaced on a strict >
 *                    only; a NaN s_t never wins);
 *   score (R) f32:   that s_t;
 *   norm  (R) f32:   sqrt(sum of feat[c]^2), float32 sum, correctly rounded root.
 * A row whose elements are all zero (+0 or -0), and a row whose every s_t is NaN, takes
 * label = unseen and score = +0.
 * 1 <= R < 2^31, 1 <= C <= OV3D_OPENVOCAB_MAX_C, 1 <= T <= OV3D_OPENVOCAB_MAX_T; planes 1:
 * P >= 1 and R a multiple of P.  feat and text are read 16 bytes at a time where their address
 * and C * sizeof(element) are multiples of 16 (rows, text), element by element otherwise. */
int ov3d_openvocab_classify(const void* feat, int dtype, int planes, long long R, int C,
                            long long P, const void* text, int T, int unseen, int32_t* label,
                            float* score, float* norm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OV3D_OPENVOCAB_H_ */

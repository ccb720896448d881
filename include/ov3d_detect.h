/* C ABI of the vocabulary scoring kernel (csrc/vocabscore.hip), part of libov3d_hip.so.
 *
 * Query embeddings against the text embeddings of a vocabulary chosen at inference time ->
 * objectness, log-sum-exp and the K most probable classes of every query: the step from the
 * model's visual_embeds to detections under any list of names.  The reference has no such
 * code (its compute_objectness_and_cls_prob asserts the training class count).
 * ov3d_amd.detect drives the entry; ov3d_amd._native derives its ctypes signature from this
 * file, as from every include/ov3d*.h; its guard-band cases are in tests/test_detect_gpu.py.
 *
 * The entry validates its arguments and returns OV3D_EINVAL before any launch; stream is the
 * HIP stream (NULL: the default stream).  One launch, nothing synchronises, no atomics; legal
 * inside a hipGraph capture.
 */
#ifndef OV3D_DETECT_H_
#define OV3D_DETECT_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OV3D_DETECT_MAX_T 4096   /* text rows */
#define OV3D_DETECT_MAX_C 4096   /* channels */
#define OV3D_DETECT_MAX_K 16     /* classes kept per row */
#define OV3D_DETECT_TILE_T 256   /* text rows per vocabulary tile */

/* R feature vectors ("rows") of C channels, row r at feat + r * ldf (ldf >= C elements),
 * against text (T, C) contiguous, both of one element type (dtype: OV3D_OPENVOCAB_F32 = 0 or
 * OV3D_OPENVOCAB_BF16 = 1).  bg is the "no object" text row, 0 <= bg < T, or -1 for none;
 * 1 <= K <= OV3D_DETECT_MAX_K classes are kept per row; scale is finite.
 *
 * Per row, s_t = scale * sum over c of feat[c] * text[t][c].  Products and sum are float32 on
 * MFMA exactly as ov3d_openvocab_classify forms them (16x16x32 for bfloat16, the float32-input
 * 16x16x4 form for float32, whose operands are not rounded), the channels in ascending chunks
 * of 128 bytes of a row, each output element in an accumulator of its own; then one float32
 * multiply by scale (scale = 1.0f changes nothing).  What a row gets depends on its own values
 * and the text only, never on R, on its place in the launch or on its neighbours.
 *   m   = max_t s_t
 *   e_t = expf(s_t - m)                   (the accurate expf)
 *   F   = sum of e_t over t != bg,  Z = F + e_bg  (Z = F when bg = -1)
 *   obj (R) f32 = F / Z: 1 - p_bg without the cancellation; exactly 1 when bg = -1, 0 when
 *                 T = 1 and bg = 0
 *   lse (R) f32 = m + logf(Z)
 *   top_cls (R, K) int32, top_prob (R, K) f32: the foreground rows t != bg ordered by s_t
 *                 descending, equal scores the smaller t first; top_prob = expf(s_t - m) / Z
 *                 from the final m and Z (never carried through a rescaling).  Slots beyond
 *                 the foreground count hold class -1 and probability 0.
 * A row in which any s_t is not finite takes obj = 0, lse = NaN, every class -1 and every
 * probability 0.  The (R, T) scores never reach memory: the vocabulary goes by in tiles of
 * OV3D_DETECT_TILE_T rows with a running maximum, a rescaled sum and a running top-K, so F and
 * Z carry one expf(m_old - m_new) factor per tile that raises the maximum.
 * 1 <= R < 2^31, 1 <= C <= OV3D_DETECT_MAX_C, 1 <= T <= OV3D_DETECT_MAX_T.  feat and text are
 * read 16 bytes at a time where their address, their row pitch in bytes and C * sizeof(element)
 * are multiples of 16, element by element otherwise. */
int ov3d_vocab_score(const void* feat, int dtype, long long R, int C, long long ldf,
                     const void* text, int T, int bg, float scale, int K,
                     float* obj, float* lse, int32_t* top_cls, float* top_prob, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OV3D_DETECT_H_ */

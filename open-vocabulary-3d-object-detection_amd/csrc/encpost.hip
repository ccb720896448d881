// The encoder layer's row-local chain after its self-attention in ONE launch each way
// (models/transformer.py:262-280 TransformerEncoderLayer.forward_pre: out-projection, residual
// + dropout, norm2, linear1 -> ReLU -> dropout -> linear2), C = 256, F = 128, bf16 training.
//
// Forward (ov3d_enc_post_fwd), per 64-row tile:
//     y1 = bf16(o Wo^T + bo)                         never stored
//     s1 = s + dropout_p1(y1)                        fp32, the rowdrop.h hash at site1
//     x2 = bf16(LN(s1) * g2 + be2)
//     h  = dropout_pf(relu(bf16(x2 W1^T + b1)))      site_ffn
//     y2 = bf16(h W2^T + b2)
// Backward (ov3d_enc_post_bwd), from ds1 (fp32) and dy2 (bf16):
//     d1  = h > 0 ? bf16(bf16(dy2 W2) / (1 - pf)) : 0
//     dx2 = bf16(d1 W1)                              never stored
//     g   = ds1 + rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)),  dxh = dx2 * g2
//     ds  = g;  dy1 = bf16(dropout_p1(g));  do = bf16(dy1 Wo)
//     LayerNorm column partials in resnorm_bwd's layout (ov3d_resnorm_bwd_parts(R, 256) blocks)
//
// These are the four launches of the unfused path each way (tile GEMM / resnorm / tile GEMM
// with the activation epilogue / tile GEMM) with the tile's rows kept in LDS between them, and
// the arithmetic is theirs operation for operation, so the outputs equal theirs bit for bit:
//   * the products are tilegemm.hip's: v_mfma_f32_32x32x16_bf16 with the W fragment first, K
//     walked in order in 64-deep chunks, one accumulation chain per output, the same k order
//     inside a 16-k step (forward: 8 consecutive k a lane; backward: W read transposed, k order
//     8(j>>2) + 4h + (j&3)), bias added in fp32 before the one rounding;
//   * k_quarters = 1 sums every product's K in four quarters, (q0 + q1) + (q2 + q3), which is
//     rowsgemm.hip's order: the unfused path runs on that kernel for short row blocks;
//   * the row passes are resnorm.hip's (32 lanes a row, 8 channels a lane, rowsum.h), and the
//     backward's column partials are summed over the same rows in the same order.
//
// Layout: a workgroup = 64 rows and 8 waves forward, 32 rows and 4 waves backward (row halves x 4
// column quarters; a wave holds a 32 x 64 or 32 x 32 output block: 32 accumulator registers).
// Two workgroups share a CU (74 KB / 55 KB of LDS each): 16384 rows are 256 forward workgroups,
// which fit beside a neighbour kernel that holds a few CUs, and 512 backward ones, which hide
// each other's weight-chunk waits.  LDS: one row image (BM x 256 bf16: o -> y1 -> x2 -> h -> y2
// forward, dy2 -> d1 -> dx2 -> dy1 -> do backward; every store to global memory leaves from it
// as whole row pieces) and one weight chunk (N x 64 k); the next chunk's global loads are in
// flight while the current one is multiplied.
#include "common.h"
#include "mfma.h"
#include "rowdrop.h"
#include "rowsum.h"

#include <type_traits>

namespace {

constexpr int C = 256;            // model width
constexpr int F = 128;            // feed-forward width
// rows per workgroup (BM, a kernel template parameter): 64 forward, 32 backward, as measured
// (DESIGN.md "Encoder post-attention chain"); BM / 32 wave rows x 4 wave columns, 32 lanes a row
// in the row passes
constexpr int FWD_BM = 64, BWD_BM = 32;
constexpr int RMULT = 64;         // row counts served (ov3d_enc_post_supported)
constexpr int BK = 64;            // K chunk
// forward images: 16-byte fragment reads (rows of 528 / 272 bytes); W chunk [n][k], 144-byte rows
constexpr int LDI = C + 8, LDH = F + 8, LDW = BK + 8;
// backward images: two 8-byte fragment reads (rows of 130 / 66 dwords: 32 rows on distinct bank
// pairs); W chunk [k][n], rows of N + 32 (16 dwords mod 64 for the transposed reads)
constexpr int LDIB = C + 4, LDHB = F + 4, LDWB = C + 32, LDWBF = F + 32;
constexpr int WSZ = C * LDW;      // = BK * LDWB; also the backward's RPP x 2 x 256 fp32 column terms
static_assert(BK * LDWB <= WSZ && 16 * 2 * C * 2 <= WSZ && RMULT % FWD_BM == 0 && RMULT % BWD_BM == 0,
              "W chunk region");

// The accumulators of a wave's NTL 32 x 32 blocks over a K-deep product.  QS: K in four
// quarters, each its own chain from zero, summed (q0 + q1) + (q2 + q3).
template <int NTL, int K, bool QS>
struct Chain {
    f32x16 acc[NTL], s01[NTL], s23[NTL];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[nt][v] = 0.f;
    }
    // after the 16-k step sg (0 .. K / 16 - 1)
    __device__ __forceinline__ void close(int sg) {
        if (!QS) return;
        constexpr int SPQ = K / 64;   // steps per quarter
        if ((sg + 1) % SPQ) return;
        const int q = (sg + 1) / SPQ - 1;
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                if (q == 0) {
                    s01[nt][v] = acc[nt][v];
                    acc[nt][v] = 0.f;
                } else if (q == 1) {
                    s01[nt][v] = s01[nt][v] + acc[nt][v];
                    acc[nt][v] = 0.f;
                } else if (q == 2) {
                    s23[nt][v] = acc[nt][v];
                    acc[nt][v] = 0.f;
                } else {
                    acc[nt][v] = s01[nt][v] + (s23[nt][v] + acc[nt][v]);
                }
            }
    }
};

// chunk `chunk` of a forward product (trans_b = 1): ap = the lane's image row at the chunk's k
// + 8h, wp = the lane's first W chunk row + 8h
template <int NTL, int K, bool QS>
__device__ __forceinline__ void mma_fwd(Chain<NTL, K, QS>& ch, const bf16* ap, const bf16* wp, int chunk) {
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(ap + 16 * s);
        bf16x8 wf[NTL];
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) wf[nt] = *reinterpret_cast<const bf16x8*>(wp + 32 * nt * LDW + 16 * s);
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) ch.acc[nt] = mfma(wf[nt], af, ch.acc[nt]);
        ch.close(chunk * (BK / 16) + s);
    }
}

// chunk of a backward product (trans_b = 0): ap = the lane's image row at the chunk's k + 4h,
// wp = the W chunk at the lane's transposed-read origin (row 4(g>>1) + (i>>2), column
// wave origin + 16(g&1) + 4(i&3)); LW the chunk's row stride
template <int NTL, int K, bool QS, int LW>
__device__ __forceinline__ void mma_bwd(Chain<NTL, K, QS>& ch, const bf16* ap, const bf16* wp, int chunk) {
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(ap + 16 * s);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(ap + 16 * s + 8);
        const bf16x8 af = join8(lo, hi);
        bf16x8 wf[NTL];
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
            const bf16x4 wl = tr16(wp + 16 * s * LW + 32 * nt);
            const bf16x4 wh = tr16(wp + (16 * s + 8) * LW + 32 * nt);
            wf[nt] = join8(wl, wh);
        }
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) ch.acc[nt] = mfma(wf[nt], af, ch.acc[nt]);
        ch.close(chunk * (BK / 16) + s);
    }
}

// ---------------------------------------------------------------- forward
struct FwdArgs {
    const float* s; const bf16* o;
    const bf16* Wo; long long ldwo; const bf16* bo;
    uint32_t thresh1; float ks1; const int64_t* seed; uint32_t site1;
    const float* g2; const float* be2; float eps;
    const bf16* W1; long long ldw1; const bf16* b1;
    uint32_t threshf; float ksf; uint32_t sitef;
    const bf16* W2; long long ldw2; const bf16* b2;
    float* s1; float* mean; float* rstd; bf16* x2; bf16* h; bf16* y2;
};

template <bool QS, int BM>
__global__ __launch_bounds__(BM * 8, QS ? BM / 32 : BM / 16) void enc_post_fwd_kernel(FwdArgs a) {
    constexpr int NT = BM * 8;     // threads: BM / 32 x 4 waves
    constexpr int RPP = NT / 32;   // rows of one row-pass round
    __shared__ __attribute__((aligned(16))) bf16 img[BM * LDI];
    __shared__ __attribute__((aligned(16))) bf16 ws[WSZ];
    __shared__ __attribute__((aligned(16))) bf16 bias_s[2 * C + F];   // bo, b2, b1
    __shared__ __attribute__((aligned(16))) float ln_s[2 * C];        // g2, be2
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r32 = lane & 31, h = lane >> 5;
    const int wm = wave >> 2, wn = wave & 3;
    const int m0 = blockIdx.x * BM;
    const int arow = wm * 32 + r32;   // the lane's tile row in the products

    // the bias and LayerNorm rows, staged once: 2 C + F bf16 = 80 16-byte pieces, 2 C fp32 = 128
    {
        const int t = tid < 80 ? tid : 0;
        const bf16* bsrc = t < 32 ? a.bo + 8 * t : t < 64 ? a.b2 + 8 * (t - 32) : a.b1 + 8 * (t - 64);
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(bsrc);
        const int u = tid & 127;
        const float4 lv = *reinterpret_cast<const float4*>((u < 64 ? a.g2 : a.be2 - C) + 4 * u);
        if (tid < 80) *reinterpret_cast<bf16x8*>(bias_s + 8 * tid) = bv;
        if (tid < 128) *reinterpret_cast<float4*>(ln_s + 4 * tid) = lv;
    }
    const bf16* const bo_s = bias_s;
    const bf16* const b2_s = bias_s + C;
    const bf16* const b1_s = bias_s + 2 * C;

    // W chunk: rows n = idx >> 3 of the chunk's 64 k, 16-byte pieces; NP pieces a thread
    constexpr int NPC = C * BK / 8 / NT, NPF = F * BK / 8 / NT;   // pieces of a 256- / 128-row chunk
    bf16x8 rw[NPC];
    auto wload = [&](const bf16* W, long long ldw, int kc, int np) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NPC; ++j)
            if (j < np) {
                const int idx = tid + NT * j;
                rw[j] = *reinterpret_cast<const bf16x8*>(W + (size_t)(idx >> 3) * ldw + kc + 8 * (idx & 7));
            }
    };
    auto wstore = [&](int np) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NPC; ++j)
            if (j < np) {
                const int idx = tid + NT * j;
                *reinterpret_cast<bf16x8*>(&ws[(idx >> 3) * LDW + 8 * (idx & 7)]) = rw[j];
            }
    };

    // the tile's o rows and Wo's first chunk
    {
        bf16x8 ra[BM * C / 8 / NT];
#pragma unroll
        for (int j = 0; j < BM * C / 8 / NT; ++j) {
            const int idx = tid + NT * j;
            ra[j] = *reinterpret_cast<const bf16x8*>(a.o + (size_t)(m0 + (idx >> 5)) * C + 8 * (idx & 31));
        }
        wload(a.Wo, a.ldwo, 0, NPC);
#pragma unroll
        for (int j = 0; j < BM * C / 8 / NT; ++j) {
            const int idx = tid + NT * j;
            *reinterpret_cast<bf16x8*>(&img[(idx >> 5) * LDI + 8 * (idx & 31)]) = ra[j];
        }
        wstore(NPC);
    }
    __syncthreads();

    const uint32_t smix1 = a.thresh1 ? rowdrop::seed_mix(a.seed, a.site1) : 0u;
    const bool dropf = a.threshf != 0;
    const uint32_t smixf = dropf ? rowdrop::seed_mix(a.seed, a.sitef) : 0u;

    // ---- y1 = bf16(o Wo^T + bo)
    {
        Chain<2, C, QS> ch;
        ch.zero();
        const bf16* ap = img + arow * LDI + 8 * h;
        const bf16* wp = ws + (wn * 64 + r32) * LDW + 8 * h;
#pragma unroll
        for (int c = 0; c < C / BK; ++c) {
            if (c + 1 < C / BK) wload(a.Wo, a.ldwo, BK * (c + 1), NPC);
            else wload(a.W1, a.ldw1, 0, NPF);
            mma_fwd(ch, ap + BK * c, wp, c);
            __syncthreads();   // the chunk (and after the last one the o rows) is read
            if (c + 1 < C / BK) {
                wstore(NPC);
                __syncthreads();
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = wn * 64 + 32 * nt + 8 * g + 4 * h;
                const bf16x4 bb = *reinterpret_cast<const bf16x4*>(bo_s + col);
                bf16x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = (bf16)(ch.acc[nt][4 * g + q] + (float)bb[q]);
                *reinterpret_cast<bf16x4*>(&img[arow * LDI + col]) = o;
            }
        wstore(NPF);   // W1's first chunk
    }
    __syncthreads();

    // ---- the resnorm_fwd row pass (csrc/resnorm.hip, 32 lanes a row): rows tid / 32 + RPP it
    wload(a.W1, a.ldw1, BK, NPF);
    {
        const int c = (tid & 31) * 8, lr0 = tid >> 5;
        float sv[4][8];
#pragma unroll
        for (int it = 0; it < 4; ++it) ld8f(a.s + (size_t)(m0 + lr0 + RPP * it) * C + c, sv[it]);
        float ga[8], ba[8];
        ld8f(ln_s + c, ga);
        ld8f(ln_s + C + c, ba);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int lr = lr0 + RPP * it;
            const long long r = m0 + lr;
            const size_t off = (size_t)r * C + c;
            float* s = sv[it];
            const bf16x8 yv = *reinterpret_cast<const bf16x8*>(&img[lr * LDI + c]);
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = (float)yv[j];
            if (a.thresh1) {
                bool keep[8];
                rowdrop::keep8(rowdrop::row_base(smix1, r), c, a.thresh1, keep);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = (float)(bf16)(y[j] * a.ks1);
                    s[j] += keep[j] ? d : 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] += y[j];
            }
            st8f(a.s1 + off, s);
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) t += s[j];
            const float mu = row_sum32_lanes(t) / (float)C;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) q += (s[j] - mu) * (s[j] - mu);
            const float rs = rsqrtf(row_sum32_lanes(q) / (float)C + a.eps);
            if (c == 0) {
                a.mean[r] = mu;
                a.rstd[r] = rs;
            }
            bf16x8 xo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xh = (s[j] - mu) * rs;
                xo[j] = (bf16)(xh * ga[j] + ba[j]);
            }
            *reinterpret_cast<bf16x8*>(a.x2 + off) = xo;
            *reinterpret_cast<bf16x8*>(&img[lr * LDI + c]) = xo;
        }
    }
    __syncthreads();

    // ---- h = dropout_pf(relu(bf16(x2 W1^T + b1)))
    {
        Chain<1, C, QS> ch;
        ch.zero();
        const bf16* ap = img + arow * LDI + 8 * h;
        const bf16* wp = ws + (wn * 32 + r32) * LDW + 8 * h;
#pragma unroll
        for (int c = 0; c < C / BK; ++c) {
            if (c > 0) {   // chunk 1 went out before the row pass
                if (c + 1 < C / BK) wload(a.W1, a.ldw1, BK * (c + 1), NPF);
                else wload(a.W2, a.ldw2, 0, NPC);
            }
            mma_fwd(ch, ap + BK * c, wp, c);
            __syncthreads();   // the chunk (and after the last one the x2 rows) is read
            if (c + 1 < C / BK) {
                wstore(NPF);
                __syncthreads();
            }
        }
        const uint32_t rbase = dropf ? rowdrop::row_base(smixf, m0 + arow) : 0u;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = wn * 32 + 8 * g + 4 * h;
            const bf16x4 bb = *reinterpret_cast<const bf16x4*>(b1_s + col);
            bf16x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = (bf16)(ch.acc[0][4 * g + q] + (float)bb[q]);
            bool keep[4] = {true, true, true, true};
            if (dropf) {   // one hash per channel pair (rowdrop.h keep8's pairs)
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    const uint32_t hs = rowdrop::mix24(rbase + (uint32_t)((col + j) >> 1) * 0x27D4EB2Fu);
                    keep[j] = (hs & 0xffffu) >= a.threshf;
                    keep[j + 1] = (hs >> 16) >= a.threshf;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float rr = fmaxf((float)o[q], 0.f);
                o[q] = keep[q] ? (bf16)(rr * a.ksf) : (bf16)0.f;   // scale 1 at p = 0
            }
            *reinterpret_cast<bf16x4*>(&img[arow * LDH + col]) = o;
        }
        wstore(NPC);   // W2's first chunk
    }
    __syncthreads();
    wload(a.W2, a.ldw2, BK, NPC);
#pragma unroll
    for (int j = 0; j < BM * F / 8 / NT; ++j) {   // the h rows, 16 bytes a lane
        const int idx = tid + NT * j, r = idx >> 4, pc = idx & 15;
        *reinterpret_cast<bf16x8*>(a.h + (size_t)(m0 + r) * F + 8 * pc) =
            *reinterpret_cast<const bf16x8*>(&img[r * LDH + 8 * pc]);
    }

    // ---- y2 = bf16(h W2^T + b2)
    {
        Chain<2, F, QS> ch;
        ch.zero();
        const bf16* ap = img + arow * LDH + 8 * h;
        const bf16* wp = ws + (wn * 64 + r32) * LDW + 8 * h;
#pragma unroll
        for (int c = 0; c < F / BK; ++c) {
            mma_fwd(ch, ap + BK * c, wp, c);
            __syncthreads();   // the chunk (and after the last one the h rows) is read
            if (c + 1 < F / BK) {
                wstore(NPC);
                __syncthreads();
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = wn * 64 + 32 * nt + 8 * g + 4 * h;
                const bf16x4 bb = *reinterpret_cast<const bf16x4*>(b2_s + col);
                bf16x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = (bf16)(ch.acc[nt][4 * g + q] + (float)bb[q]);
                *reinterpret_cast<bf16x4*>(&img[arow * LDI + col]) = o;
            }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BM * C / 8 / NT; ++j) {
        const int idx = tid + NT * j, r = idx >> 5, pc = idx & 31;
        *reinterpret_cast<bf16x8*>(a.y2 + (size_t)(m0 + r) * C + 8 * pc) =
            *reinterpret_cast<const bf16x8*>(&img[r * LDI + 8 * pc]);
    }
}

// ---------------------------------------------------------------- backward
struct BwdArgs {
    const float* ds1; const bf16* dy2;
    const float* s1; const float* mean; const float* rstd;
    const bf16* h; const float* g2;
    const bf16* Wo; long long ldwo;
    const bf16* W1; long long ldw1;
    const bf16* W2; long long ldw2;
    uint32_t thresh1; float ks1; const int64_t* seed; uint32_t site1;
    float ksf;
    float* ds; bf16* dy1; bf16* dout; bf16* d1; float* partials;
};

// IT4: resnorm_bwd's 32-row partial blocks (R >= 4096: a thread sums 4 rows 8 apart, then the
// 8 row phases in order); else its 8-row blocks
template <bool QS, bool IT4, int BM>
__global__ __launch_bounds__(BM * 8, QS ? BM / 32 : BM / 16) void enc_post_bwd_kernel(BwdArgs a) {
    constexpr int NT = BM * 8;     // threads: BM / 32 x 4 waves
    constexpr int RPP = NT / 32;   // rows of one row-pass round
    __shared__ __attribute__((aligned(16))) bf16 img[BM * LDI];   // >= BM * LDIB
    __shared__ __attribute__((aligned(16))) bf16 ws[WSZ];
    __shared__ __attribute__((aligned(16))) float g2_s[C];
    float* const red = reinterpret_cast<float*>(ws);   // [2][RPP][C] column terms (row pass only)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r32 = lane & 31, h = lane >> 5;
    const int wm = wave >> 2, wn = wave & 3;
    const int m0 = blockIdx.x * BM;
    const int arow = wm * 32 + r32;
    const int gq = lane >> 4, i16 = lane & 15;
    // the lane's transposed-read origin inside a W chunk, without the wave's column origin
    const int trow = 4 * (gq >> 1) + (i16 >> 2), tcol = 16 * (gq & 1) + 4 * (i16 & 3);

    {
        const float4 lv = *reinterpret_cast<const float4*>(a.g2 + 4 * (tid & 63));
        if (tid < 64) *reinterpret_cast<float4*>(g2_s + 4 * tid) = lv;
    }

    // W chunk [k][N]: 64 rows of N / 8 16-byte pieces
    bf16x8 rw[BK * C / 8 / NT];
    auto wload = [&](const bf16* W, long long ldw, int kc, auto n_c) __attribute__((always_inline)) {
        constexpr int N = decltype(n_c)::value;
#pragma unroll
        for (int j = 0; j < BK * N / 8 / NT; ++j) {
            const int idx = tid + NT * j, k = idx / (N / 8), pc = idx % (N / 8);
            rw[j] = *reinterpret_cast<const bf16x8*>(W + (size_t)(kc + k) * ldw + 8 * pc);
        }
    };
    auto wstore = [&](auto n_c) __attribute__((always_inline)) {
        constexpr int N = decltype(n_c)::value;
#pragma unroll
        for (int j = 0; j < BK * N / 8 / NT; ++j) {
            const int idx = tid + NT * j, k = idx / (N / 8), pc = idx % (N / 8);
            *reinterpret_cast<bf16x8*>(&ws[k * (N + 32) + 8 * pc]) = rw[j];
        }
    };
    using NF = std::integral_constant<int, F>;
    using NC = std::integral_constant<int, C>;

    // the tile's dy2 rows and W2's first chunk
    {
        bf16x8 ra[BM * C / 8 / NT];
#pragma unroll
        for (int j = 0; j < BM * C / 8 / NT; ++j) {
            const int idx = tid + NT * j;
            ra[j] = *reinterpret_cast<const bf16x8*>(a.dy2 + (size_t)(m0 + (idx >> 5)) * C + 8 * (idx & 31));
        }
        wload(a.W2, a.ldw2, 0, NF{});
#pragma unroll
        for (int j = 0; j < BM * C / 8 / NT; ++j) {   // 520-byte rows: 8-byte aligned only
            const int idx = tid + NT * j;
            bf16* d = &img[(idx >> 5) * LDIB + 8 * (idx & 31)];
            const bf16x8 v = ra[j];
            *reinterpret_cast<bf16x4*>(d) = bf16x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<bf16x4*>(d + 4) = bf16x4{v[4], v[5], v[6], v[7]};
        }
        wstore(NF{});
    }
    __syncthreads();

    // ---- d1 = h > 0 ? bf16(bf16(dy2 W2) / (1 - pf)) : 0
    {
        Chain<1, C, QS> ch;
        ch.zero();
        const bf16* ap = img + arow * LDIB + 4 * h;
        const bf16* wp = ws + trow * LDWBF + wn * 32 + tcol;
        bf16x4 hv[4];
#pragma unroll
        for (int c = 0; c < C / BK; ++c) {
            if (c + 1 < C / BK) {
                wload(a.W2, a.ldw2, BK * (c + 1), NF{});
            } else {
                wload(a.W1, a.ldw1, 0, NC{});
#pragma unroll
                for (int g = 0; g < 4; ++g)   // the activation values of the epilogue
                    hv[g] = *reinterpret_cast<const bf16x4*>(a.h + (size_t)(m0 + arow) * F + wn * 32 + 8 * g + 4 * h);
            }
            mma_bwd<1, C, QS, LDWBF>(ch, ap + BK * c, wp, c);
            __syncthreads();   // the chunk (and after the last one the dy2 rows) is read
            if (c + 1 < C / BK) {
                wstore(NF{});
                __syncthreads();
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = wn * 32 + 8 * g + 4 * h;
            bf16x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bf16 v = (bf16)(ch.acc[0][4 * g + q] + 0.f);
                o[q] = (float)hv[g][q] > 0.f ? (bf16)((float)v * a.ksf) : (bf16)0.f;
            }
            *reinterpret_cast<bf16x4*>(&img[arow * LDHB + col]) = o;
        }
        wstore(NC{});   // W1's first chunk
    }
    __syncthreads();
    wload(a.W1, a.ldw1, BK, NC{});
#pragma unroll
    for (int j = 0; j < BM * F / 8 / NT; ++j) {   // the d1 rows, 16 bytes a lane
        const int idx = tid + NT * j, r = idx >> 4, pc = idx & 15;
        const bf16* sp = &img[r * LDHB + 8 * pc];
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(sp), hi = *reinterpret_cast<const bf16x4*>(sp + 4);
        *reinterpret_cast<bf16x8*>(a.d1 + (size_t)(m0 + r) * F + 8 * pc) =
            join8(lo, hi);
    }

    // ---- dx2 = bf16(d1 W1)
    {
        Chain<2, F, QS> ch;
        ch.zero();
        const bf16* ap = img + arow * LDHB + 4 * h;
        const bf16* wp = ws + trow * LDWB + wn * 64 + tcol;
#pragma unroll
        for (int c = 0; c < F / BK; ++c) {
            if (c + 1 == F / BK) wload(a.Wo, a.ldwo, 0, NC{});
            mma_bwd<2, F, QS, LDWB>(ch, ap + BK * c, wp, c);
            __syncthreads();   // the chunk (and after the last one the d1 rows) is read
            if (c + 1 < F / BK) {
                wstore(NC{});
                __syncthreads();
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = wn * 64 + 32 * nt + 8 * g + 4 * h;
                bf16x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = (bf16)(ch.acc[nt][4 * g + q] + 0.f);
                *reinterpret_cast<bf16x4*>(&img[arow * LDIB + col]) = o;
            }
    }
    __syncthreads();

    // ---- the resnorm_bwd row pass (csrc/resnorm.hip bwd_row, dxa = dx2, no second affine):
    // RPP row phases x 4 rows; IT4: phase = (32-row block, row phase of 8), rows 8 apart
    {
        const int c = (tid & 31) * 8, ph = tid >> 5;
        const uint32_t sm = a.thresh1 ? rowdrop::seed_mix(a.seed, a.site1) : 0u;
        float ga[8];
        ld8f(g2_s + c, ga);
        float acc0[8], acc1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc0[j] = acc1[j] = 0.f;
        // two rows' loads in flight at a time
        float gv[4][8], svv[4][8], mu4[4], rs4[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (!(it & 1)) {
#pragma unroll
                for (int u = it; u < it + 2; ++u) {
                    const int lu = IT4 ? 32 * (ph >> 3) + (ph & 7) + 8 * u : ph + RPP * u;
                    const size_t offu = (size_t)(m0 + lu) * C + c;
                    ld8f(a.ds1 + offu, gv[u]);
                    ld8f(a.s1 + offu, svv[u]);
                    mu4[u] = a.mean[m0 + lu];
                    rs4[u] = a.rstd[m0 + lu];
                }
            }
            const int lr = IT4 ? 32 * (ph >> 3) + (ph & 7) + 8 * it : ph + RPP * it;
            const long long r = m0 + lr;
            const size_t off = (size_t)r * C + c;
            float* g = gv[it];
            const float* sv = svv[it];
            const float mu = mu4[it], rs = rs4[it];
            float da[8];
            {
                const bf16* sp = &img[lr * LDIB + c];
                const bf16x4 lo = *reinterpret_cast<const bf16x4*>(sp), hi = *reinterpret_cast<const bf16x4*>(sp + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    da[j] = (float)lo[j];
                    da[4 + j] = (float)hi[j];
                }
            }
            float xh[8], dxh[8], s1 = 0.f, s2 = 0.f;
            float t0[8], t1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                xh[j] = (sv[j] - mu) * rs;
                dxh[j] = da[j] * ga[j] + 0.f;   // + db * gb of the absent second affine
                s1 += dxh[j];
                s2 += dxh[j] * xh[j];
                t0[j] = da[j] * xh[j];
                t1[j] = da[j];
            }
            s1 = row_sum32_lanes(s1) / (float)C;
            s2 = row_sum32_lanes(s2) / (float)C;
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] += rs * (dxh[j] - s1 - xh[j] * s2);
            st8f(a.ds + off, g);
            float d[8];
            if (a.thresh1) {
                bool keep[8];
                rowdrop::keep8(rowdrop::row_base(sm, r), c, a.thresh1, keep);
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = keep[j] ? g[j] * a.ks1 : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = g[j];
            }
            bf16x8 dv;
#pragma unroll
            for (int j = 0; j < 8; ++j) dv[j] = (bf16)d[j];
            *reinterpret_cast<bf16x8*>(a.dy1 + off) = dv;
            {
                bf16* dp = &img[lr * LDIB + c];
                *reinterpret_cast<bf16x4*>(dp) = bf16x4{dv[0], dv[1], dv[2], dv[3]};
                *reinterpret_cast<bf16x4*>(dp + 4) = bf16x4{dv[4], dv[5], dv[6], dv[7]};
            }
            if (IT4) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    acc0[j] += t0[j];
                    acc1[j] += t1[j];
                }
            } else {
                // this round's RPP rows are whole 8-row blocks of the tile
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    red[ph * C + c + j] = 0.f + t0[j];
                    red[(RPP + ph) * C + c + j] = 0.f + t1[j];
                }
                __syncthreads();
                {
                    const int blk = tid >> 8, col = tid & 255;   // RPP / 8 blocks x 256 columns
                    float u0 = 0.f, u1 = 0.f;
#pragma unroll
                    for (int p = 0; p < 8; ++p) {
                        u0 += red[(8 * blk + p) * C + col];
                        u1 += red[(RPP + 8 * blk + p) * C + col];
                    }
                    float* pp = a.partials + ((size_t)(m0 / 8) + (RPP / 8) * it + blk) * 4 * C;
                    pp[col] = u0;
                    pp[C + col] = u1;
                    pp[2 * C + col] = 0.f;
                    pp[3 * C + col] = 0.f;
                }
                __syncthreads();
            }
        }
        if (IT4) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                red[ph * C + c + j] = acc0[j];
                red[(RPP + ph) * C + c + j] = acc1[j];
            }
            __syncthreads();
            {
                const int blk = tid >> 8, col = tid & 255;   // RPP / 8 blocks x 256 columns
                float u0 = 0.f, u1 = 0.f;
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    u0 += red[(8 * blk + p) * C + col];
                    u1 += red[(RPP + 8 * blk + p) * C + col];
                }
                float* pp = a.partials + ((size_t)(m0 / 32) + blk) * 4 * C;
                pp[col] = u0;
                pp[C + col] = u1;
                pp[2 * C + col] = 0.f;
                pp[3 * C + col] = 0.f;
            }
            __syncthreads();
        }
    }
    wstore(NC{});   // Wo's first chunk (the column terms are read)
    __syncthreads();

    // ---- do = bf16(dy1 Wo)
    {
        Chain<2, C, QS> ch;
        ch.zero();
        const bf16* ap = img + arow * LDIB + 4 * h;
        const bf16* wp = ws + trow * LDWB + wn * 64 + tcol;
#pragma unroll
        for (int c = 0; c < C / BK; ++c) {
            if (c + 1 < C / BK) wload(a.Wo, a.ldwo, BK * (c + 1), NC{});
            mma_bwd<2, C, QS, LDWB>(ch, ap + BK * c, wp, c);
            __syncthreads();   // the chunk (and after the last one the dy1 rows) is read
            if (c + 1 < C / BK) {
                wstore(NC{});
                __syncthreads();
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = wn * 64 + 32 * nt + 8 * g + 4 * h;
                bf16x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = (bf16)(ch.acc[nt][4 * g + q] + 0.f);
                *reinterpret_cast<bf16x4*>(&img[arow * LDIB + col]) = o;
            }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BM * C / 8 / NT; ++j) {
        const int idx = tid + NT * j, r = idx >> 5, pc = idx & 31;
        const bf16* sp = &img[r * LDIB + 8 * pc];
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(sp), hi = *reinterpret_cast<const bf16x4*>(sp + 4);
        *reinterpret_cast<bf16x8*>(a.dout + (size_t)(m0 + r) * C + 8 * pc) =
            join8(lo, hi);
    }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool bad_p(float p) { return !(p >= 0.f && p < 1.f); }
bool bad_w(const void* W, long long ldw, int K) { return !W || !al16(W) || ldw % 8 || ldw < K; }

}  // namespace

extern "C" int ov3d_enc_post_supported(int R, int C_, int F_) {
    return R > 0 && R % RMULT == 0 && C_ == C && F_ == F;
}

extern "C" int ov3d_enc_post_fwd(int R, const float* s, const void* o, const void* Wo, long long ldwo,
                                 const void* bo, float p1, const int64_t* seed, int site1,
                                 const float* g2, const float* be2, float eps, const void* W1,
                                 long long ldw1, const void* b1, float pf, int site_ffn,
                                 const void* W2, long long ldw2, const void* b2, int k_quarters,
                                 float* s1, float* mean, float* rstd, void* x2, void* h, void* y2,
                                 void* stream) {
    if (!ov3d_enc_post_supported(R, C, F) || !s || !o || !bo || !g2 || !be2 || !b1 || !b2 || !s1 ||
        !mean || !rstd || !x2 || !h || !y2)
        return OV3D_EINVAL;
    if (bad_p(p1) || bad_p(pf) || ((p1 > 0.f || pf > 0.f) && !seed)) return OV3D_EINVAL;
    if (bad_w(Wo, ldwo, C) || bad_w(W1, ldw1, C) || bad_w(W2, ldw2, F)) return OV3D_EINVAL;
    if (!al16(s) || !al16(o) || !al16(bo) || !al16(g2) || !al16(be2) || !al16(b1) || !al16(b2) ||
        !al16(s1) || !al16(x2) || !al16(h) || !al16(y2))
        return OV3D_EINVAL;
    FwdArgs a{s, (const bf16*)o, (const bf16*)Wo, ldwo, (const bf16*)bo, rowdrop::thresh(p1),
              1.f / (1.f - p1), seed, (uint32_t)site1, g2, be2, eps, (const bf16*)W1, ldw1,
              (const bf16*)b1, rowdrop::thresh(pf), 1.f / (1.f - pf), (uint32_t)site_ffn,
              (const bf16*)W2, ldw2, (const bf16*)b2, s1, mean, rstd, (bf16*)x2, (bf16*)h, (bf16*)y2};
    hipStream_t st = ov3d_stream(stream);
    constexpr int BM = FWD_BM;
    if (k_quarters) enc_post_fwd_kernel<true, BM><<<R / BM, BM * 8, 0, st>>>(a);
    else enc_post_fwd_kernel<false, BM><<<R / BM, BM * 8, 0, st>>>(a);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

extern "C" int ov3d_enc_post_bwd(int R, const float* ds1, const void* dy2, const float* s1,
                                 const float* mean, const float* rstd, const void* h, const float* g2,
                                 const void* Wo, long long ldwo, const void* W1, long long ldw1,
                                 const void* W2, long long ldw2, float p1, const int64_t* seed,
                                 int site1, float pf, int k_quarters, float* ds, void* dy1,
                                 void* dout, void* d1, float* partials, int nparts, void* stream) {
    if (!ov3d_enc_post_supported(R, C, F) || !ds1 || !dy2 || !s1 || !mean || !rstd || !h || !g2 ||
        !ds || !dy1 || !dout || !d1 || !partials)
        return OV3D_EINVAL;
    if (bad_p(p1) || bad_p(pf) || (p1 > 0.f && !seed)) return OV3D_EINVAL;
    // input-gradient layout: Wo (C, C), W1 (F, C), W2 (C, F) rows
    if (bad_w(Wo, ldwo, C) || bad_w(W1, ldw1, C) || bad_w(W2, ldw2, F)) return OV3D_EINVAL;
    if (!al16(ds1) || !al16(dy2) || !al16(s1) || !al16(h) || !al16(g2) || !al16(ds) || !al16(dy1) ||
        !al16(dout) || !al16(d1) || !al16(partials))
        return OV3D_EINVAL;
    const bool it4 = R >= 4096;   // resnorm_bwd's rows per partial block: 32 from 4096 rows, else 8
    if (nparts != ov3d_resnorm_bwd_parts(R, C) || nparts != R / (it4 ? 32 : 8)) return OV3D_EINVAL;
    BwdArgs a{ds1, (const bf16*)dy2, s1, mean, rstd, (const bf16*)h, g2, (const bf16*)Wo, ldwo,
              (const bf16*)W1, ldw1, (const bf16*)W2, ldw2, rowdrop::thresh(p1), 1.f / (1.f - p1),
              seed, (uint32_t)site1, 1.f / (1.f - pf), ds, (bf16*)dy1, (bf16*)dout, (bf16*)d1,
              partials};
    hipStream_t st = ov3d_stream(stream);
    constexpr int BM = BWD_BM, NT = BM * 8;
    const int grid = R / BM;
    if (k_quarters) {
        if (it4) enc_post_bwd_kernel<true, true, BM><<<grid, NT, 0, st>>>(a);
        else enc_post_bwd_kernel<true, false, BM><<<grid, NT, 0, st>>>(a);
    } else {
        if (it4) enc_post_bwd_kernel<false, true, BM><<<grid, NT, 0, st>>>(a);
        else enc_post_bwd_kernel<false, false, BM><<<grid, NT, 0, st>>>(a);
    }
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

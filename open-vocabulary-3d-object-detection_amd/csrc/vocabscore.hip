// Vocabulary scoring (include/ov3d_detect.h): R query embeddings against the (T, C) text
// embeddings -> objectness, log-sum-exp and the K most probable classes, one launch.
//
// The dot products are those of openvocab.hip (textdot.h): a lane's accumulators hold 4 text rows
// per 16-row text block of ONE feature row.  The vocabulary goes by in tiles of 256 text rows
// (16 blocks).  After a tile's channels the lanes of a row agree on the new maximum, every lane
// rescales its own partial sums and adds its own terms, and offers its scores to its own sorted
// list of K (score, index) pairs in LDS ([slot][thread], conflict free).  A lane meets its text
// rows in ascending order and inserts on a strict > only, so equal scores keep the smaller
// index first.  At the end the partial sums are added in one fixed order and one lane merges
// the row's lists.
//
// Three workgroup shapes, one arithmetic.  The detector's R = B * Q is small against the chip and
// every workgroup streams the whole text, so the shape trades grid size against text traffic
// (DESIGN.md):
//   kOne    1 wave,  16 rows, every block of the tile                 (T <= 32 or K > 8)
//   kSplit  4 waves, 16 rows, wave w takes quarter w of the blocks    (R <= 4096)
//   kRows   4 waves, 64 rows, every wave every block of its 16 rows   (R > 4096)
// A row's partial sums are kept per (lane of the row, quarter of the tile's blocks) in every
// shape, the tile maximum is exact whichever way it is gathered, and the quarters are added
// ((q0 + q1) + q2) + q3 after the lanes, so the three shapes give a row the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "textdot.h"
#include "../../include/ov3d_detect.h"

namespace {

constexpr int kTT = OV3D_DETECT_TILE_T / 16;
constexpr int kOne = 0, kRows = 1, kSplit = 2;
constexpr int kSplitMaxK = 8;    // K above it: kOne (the lists of 256 threads would not fit 64 KB)
constexpr int kExchange = 4 * 64 * 4;   // bytes: tile maxima, sums, background terms, flags of 4 waves x 16 rows

// `rows` LDS rows from src rows row0 .. (pitch ld elements), the first `valid` of them exist;
// channels k0 .. k0 + KC - 1, those >= C zero
template <typename E, int NT>
__device__ __forceinline__ void stage_rows(unsigned char* dst, const E* src, long long row0, long long ld, int rows,
                                           int valid, int C, int k0, bool vec) {
    constexpr int KC = kChunk / (int)sizeof(E);
    constexpr int PER = 16 / (int)sizeof(E);
    if (vec) {
        // 8 loads in flight per thread before the first LDS write: one wave may stage a tile alone
        constexpr int U = 8;
        const int n = rows * 8;
        for (int e0 = threadIdx.x; e0 < n; e0 += NT * U) {
            uint4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + u * NT, row = e >> 3, k = k0 + (e & 7) * PER;
                v[u] = make_uint4(0u, 0u, 0u, 0u);
                if (e < n && row < valid && k < C) v[u] = *reinterpret_cast<const uint4*>(src + (row0 + row) * ld + k);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + u * NT;
                if (e < n) {
                    uint2* d = reinterpret_cast<uint2*>(dst + (e >> 3) * kStride + (e & 7) * 16);
                    d[0] = make_uint2(v[u].x, v[u].y);
                    d[1] = make_uint2(v[u].z, v[u].w);
                }
            }
        }
    } else {
        for (int e = threadIdx.x; e < rows * KC; e += NT) {
            const int row = e / KC, kk = e % KC;
            E v = (E)0.0f;
            if (row < valid && k0 + kk < C) v = src[(row0 + row) * ld + k0 + kk];
            reinterpret_cast<E*>(dst + row * kStride)[kk] = v;
        }
    }
}

// the 16-byte pieces of stage_rows' vector path held in registers between their global load and
// their LDS write, N per thread: the next chunk's loads fly during this chunk's MFMAs
template <int N>
struct Pieces {
    uint4 v[N];
};

template <typename E, int NT, int N>
__device__ __forceinline__ void load_pieces(Pieces<N>& p, const E* src, long long row0, long long ld, int rows,
                                            int valid, int C, int k0) {
    constexpr int PER = 16 / (int)sizeof(E);
    const int n = rows * 8;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int e = threadIdx.x + u * NT, row = e >> 3, k = k0 + (e & 7) * PER;
        p.v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (e < n && row < valid && k < C) p.v[u] = *reinterpret_cast<const uint4*>(src + (row0 + row) * ld + k);
    }
}

template <int NT, int N>
__device__ __forceinline__ void store_pieces(const Pieces<N>& p, unsigned char* dst, int rows) {
    const int n = rows * 8;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int e = threadIdx.x + u * NT;
        if (e < n) {
            uint2* d = reinterpret_cast<uint2*>(dst + (e >> 3) * kStride + (e & 7) * 16);
            d[0] = make_uint2(p.v[u].x, p.v[u].y);
            d[1] = make_uint2(p.v[u].z, p.v[u].w);
        }
    }
}

// float32: a chunk is 2 groups of 16 channels; lane (r, h) holds channels 16 g + 4 h + j of its
// row and the 16x16x4 MFMA number j sums over h.  bfloat16: 2 steps of 32 channels, lane (r, h)
// holds channels 32 s + 8 h + j, the operand layout of the 16x16x32 MFMA.
template <typename E, int TW>
__device__ __forceinline__ void mfma_chunk(f32x4 (&acc)[TW], const unsigned char* frow, const unsigned char* trow,
                                           int h, int ntt) {
    if constexpr (sizeof(E) == 4) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const Frag fb = lds_frag(frow + (16 * g + 4 * h) * 4);
            const float b[4] = {__uint_as_float(fb.lo.x), __uint_as_float(fb.lo.y), __uint_as_float(fb.hi.x),
                                __uint_as_float(fb.hi.y)};
#pragma unroll
            for (int tt = 0; tt < TW; ++tt) {
                if (tt < ntt) {
                    const Frag fa = lds_frag(trow + tt * 16 * kStride + (16 * g + 4 * h) * 4);
                    const float a[4] = {__uint_as_float(fa.lo.x), __uint_as_float(fa.lo.y), __uint_as_float(fa.hi.x),
                                        __uint_as_float(fa.hi.y)};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[tt], 0, 0, 0);
                }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 b = __builtin_bit_cast(bf16x8, lds_frag(frow + (32 * s + 8 * h) * 2));
#pragma unroll
            for (int tt = 0; tt < TW; ++tt) {
                if (tt < ntt) {
                    const bf16x8 a =
                        __builtin_bit_cast(bf16x8, lds_frag(trow + tt * 16 * kStride + (32 * s + 8 * h) * 2));
                    acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[tt], 0, 0, 0);
                }
            }
        }
    }
}

constexpr int threads_of(int mode) { return mode == kOne ? 64 : 256; }
constexpr int rows_of(int mode) { return mode == kRows ? 64 : 16; }

// LDS: [feature rows | text tile | list scores (K, NT) | list indices (K, NT) | exchange]
template <int TT, int MODE>
constexpr int lds_bytes(int K) {
    return (rows_of(MODE) + 16 * TT) * kStride + K * threads_of(MODE) * 8 + kExchange;
}

template <typename E, int TT, int MODE>
__global__ __launch_bounds__(threads_of(MODE)) void vocabscore_kernel(
    const E* __restrict__ feat, const E* __restrict__ text, long long R, int C, long long ldf, int T, int bg,
    float scale, int K, int vec_feat, int vec_text, float* __restrict__ obj, float* __restrict__ lse,
    int32_t* __restrict__ top_cls, float* __restrict__ top_prob) {
    constexpr int NT = threads_of(MODE), ROWS = rows_of(MODE), W = 16 * TT;
    constexpr int KC = kChunk / (int)sizeof(E);
    constexpr int NQ = TT >= 4 ? 4 : TT;                 // quarters of the tile's blocks
    constexpr int QW = TT / NQ;                          // blocks per quarter
    constexpr int TW = MODE == kSplit ? QW : TT;         // blocks this wave accumulates
    constexpr int NQL = MODE == kSplit ? 1 : NQ;         // partial sums this lane keeps
    constexpr int NL = MODE == kSplit ? 16 : 4;          // lists of a row
    constexpr int NTP = (W * 8 + NT - 1) / NT;           // 16-byte pieces of a text chunk per thread
    constexpr int NFP = (ROWS * 8 + NT - 1) / NT;        // and of the feature chunk
    static_assert(MODE != kSplit || TT >= 4, "a quarter is at least one block");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* fs = smem;
    unsigned char* ts = smem + ROWS * kStride;
    float* ls = reinterpret_cast<float*>(ts + W * kStride);
    int* li = reinterpret_cast<int*>(ls + K * NT);
    float* xm = reinterpret_cast<float*>(li + K * NT);   // [wave][row]: tile maxima
    float* xs = xm + 64;                                 // quarter sums
    float* xe = xs + 64;                                 // background terms
    int* xb = reinterpret_cast<int*>(xe + 64);           // non-finite flags
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, h = lane >> 4;
    const long long r0 = (long long)blockIdx.x * ROWS;
    const int valid = (int)((R - r0) < ROWS ? (R - r0) : ROWS);
    const int tt0 = MODE == kSplit ? wave * TW : 0;      // this wave's first block of a tile

    for (int k = 0; k < K; ++k) {
        ls[k * NT + tid] = -INFINITY;
        li[k * NT + tid] = -1;
    }
    float m = -INFINITY, EB = 0.f, thr = -INFINITY;
    float Fq[NQL];
#pragma unroll
    for (int q = 0; q < NQL; ++q) Fq[q] = 0.f;
    int bad = 0;

    const unsigned char* frow = fs + ((MODE == kRows ? wave * 16 : 0) + r) * kStride;
    const unsigned char* trow = ts + (tt0 * 16 + r) * kStride;

    for (int t0 = 0; t0 < T; t0 += W) {
        const int left = T - t0;
        const int ntt = (left >= W ? TT : (left + 15) >> 4) - tt0;   // this wave's blocks below it exist
        f32x4 acc[TW];
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};

        const int trows = (ntt + tt0) * 16;             // text rows of this tile, whole blocks
        bool piped = false;
        if constexpr (NTP <= 8) {
            if (vec_feat && vec_text) {
                // chunk k + 1 travels from memory while the MFMAs of chunk k run
                piped = true;
                Pieces<NFP> pf;
                Pieces<NTP> pt;
                load_pieces<E, NT, NFP>(pf, feat, r0, ldf, ROWS, valid, C, 0);
                load_pieces<E, NT, NTP>(pt, text, t0, C, trows, left, C, 0);
                for (int k0 = 0; k0 < C; k0 += KC) {
                    store_pieces<NT, NFP>(pf, fs, ROWS);
                    store_pieces<NT, NTP>(pt, ts, trows);
                    __syncthreads();
                    if (k0 + KC < C) {
                        load_pieces<E, NT, NFP>(pf, feat, r0, ldf, ROWS, valid, C, k0 + KC);
                        load_pieces<E, NT, NTP>(pt, text, t0, C, trows, left, C, k0 + KC);
                    }
                    mfma_chunk<E, TW>(acc, frow, trow, h, ntt);
                    __syncthreads();
                }
            }
        }
        if (!piped) {
            for (int k0 = 0; k0 < C; k0 += KC) {
                stage_rows<E, NT>(fs, feat, r0, ldf, ROWS, valid, C, k0, vec_feat != 0);
                stage_rows<E, NT>(ts, text, t0, C, trows, left, C, k0, vec_text != 0);
                __syncthreads();
                mfma_chunk<E, TW>(acc, frow, trow, h, ntt);
                __syncthreads();
            }
        }

        // this lane: text rows t0 + 16 (tt0 + tt) + 4 h + j of feature row r, ascending
        float mt = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float s = acc[tt][j] * scale;
                acc[tt][j] = s;
                if (t0 + (tt0 + tt) * 16 + h * 4 + j < T) {
                    bad |= !(fabsf(s) < INFINITY);
                    mt = fmaxf(mt, s);
                }
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        if constexpr (MODE == kSplit) {
            // the four waves of the row; the chunk loop's barriers separate this tile's reads from
            // the next tile's writes
            if (h == 0) xm[wave * 16 + r] = mt;
            __syncthreads();
            mt = fmaxf(fmaxf(xm[r], xm[16 + r]), fmaxf(xm[32 + r], xm[48 + r]));
        }
        const float mn = fmaxf(m, mt);
        const float resc = expf(m - mn);           // the first tile: expf(-inf) = 0 on sums of 0
#pragma unroll
        for (int q = 0; q < NQL; ++q) Fq[q] *= resc;
        EB *= resc;
        m = mn;
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = t0 + (tt0 + tt) * 16 + h * 4 + j;
                if (t < T) {
                    const float s = acc[tt][j];
                    const float e = expf(s - m);
                    if (t == bg) {
                        EB = e;
                    } else {
                        Fq[MODE == kSplit ? 0 : tt / QW] += e;
                        if (s > thr) {             // beats this lane's K-th: insert behind its equals
                            int p = K - 1;
                            while (p > 0 && ls[(p - 1) * NT + tid] < s) {
                                ls[p * NT + tid] = ls[(p - 1) * NT + tid];
                                li[p * NT + tid] = li[(p - 1) * NT + tid];
                                --p;
                            }
                            ls[p * NT + tid] = s;
                            li[p * NT + tid] = t;
                            thr = ls[(K - 1) * NT + tid];
                        }
                    }
                }
            }
        }
    }

    // the four lanes of the row, then the quarters in ascending order
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
        for (int q = 0; q < NQL; ++q) Fq[q] += __shfl_xor(Fq[q], off);
        EB += __shfl_xor(EB, off);
        bad |= __shfl_xor(bad, off);
    }
    float F = Fq[0];
    if constexpr (MODE == kSplit) {
        if (h == 0) {
            xs[wave * 16 + r] = F;
            xe[wave * 16 + r] = EB;
            xb[wave * 16 + r] = bad;
        }
    } else {
#pragma unroll
        for (int q = 1; q < NQL; ++q) F += Fq[q];
    }
    __syncthreads();                               // the lists of the row's other lanes, the quarters
    if constexpr (MODE == kSplit) {
        F = ((xs[r] + xs[16 + r]) + xs[32 + r]) + xs[48 + r];
        EB = ((xe[r] + xe[16 + r]) + xe[32 + r]) + xe[48 + r];
        bad = xb[r] | xb[16 + r] | xb[32 + r] | xb[48 + r];
    }
    const long long row = r0 + (MODE == kRows ? wave * 16 : 0) + r;
    if (h == 0 && (MODE != kSplit || wave == 0) && row < R) {
        const float Z = bg >= 0 ? F + EB : F;
        int32_t* oc = top_cls + row * K;
        float* op = top_prob + row * K;
        if (bad) {
            obj[row] = 0.f;
            lse[row] = __int_as_float(0x7fc00000);
            for (int j = 0; j < K; ++j) {
                oc[j] = -1;
                op[j] = 0.f;
            }
        } else {
            obj[row] = F / Z;
            lse[row] = m + logf(Z);
            // merge the row's lists, heads in registers: the larger score, the smaller index among
            // equals.  List l belongs to thread base + slot(l): lane group l & 3 of wave l >> 2.
            const int base = MODE == kSplit ? r : tid;
            float hs[NL];
            int hi[NL], pos[NL];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const int th = base + (l >> 2) * 64 + (l & 3) * 16;
                hs[l] = ls[th];
                hi[l] = li[th];
                pos[l] = 0;
            }
            for (int j = 0; j < K; ++j) {
                float bs = 0.f;
                int bi = -1, bl = -1;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    if (hi[l] >= 0 && (bi < 0 || hs[l] > bs || (hs[l] == bs && hi[l] < bi))) {
                        bs = hs[l];
                        bi = hi[l];
                        bl = l;
                    }
                }
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    if (l == bl) {
                        const int th = base + (l >> 2) * 64 + (l & 3) * 16;
                        ++pos[l];
                        hi[l] = pos[l] < K ? li[pos[l] * NT + th] : -1;
                        hs[l] = pos[l] < K ? ls[pos[l] * NT + th] : 0.f;
                    }
                }
                oc[j] = bi;
                op[j] = bi < 0 ? 0.f : expf(bs - m) / Z;
            }
        }
    }
}

template <typename E, int TT, int MODE>
void launch_mode(const void* feat, const void* text, long long R, int C, long long ldf, int T, int bg, float scale,
                 int K, int vec_feat, int vec_text, float* obj, float* lse, int32_t* top_cls, float* top_prob,
                 hipStream_t stream) {
    constexpr int ROWS = rows_of(MODE);
    static_assert(lds_bytes<TT, MODE>(MODE == kOne ? OV3D_DETECT_MAX_K : kSplitMaxK) <= 64 * 1024, "LDS");
    const unsigned grid = (unsigned)((R + ROWS - 1) / ROWS);
    const unsigned lds = (unsigned)lds_bytes<TT, MODE>(K);
    hipLaunchKernelGGL((vocabscore_kernel<E, TT, MODE>), dim3(grid), dim3(threads_of(MODE)), lds, stream,
                       static_cast<const E*>(feat), static_cast<const E*>(text), R, C, ldf, T, bg, scale, K, vec_feat,
                       vec_text, obj, lse, top_cls, top_prob);
}

template <typename E, int TT, typename... A>
void launch_t(long long R, int K, A... a) {
    if constexpr (TT >= 4) {
        if (K <= kSplitMaxK) {
            if (R > 4096) launch_mode<E, TT, kRows>(a...);
            else launch_mode<E, TT, kSplit>(a...);
            return;
        }
    }
    launch_mode<E, TT, kOne>(a...);
}

template <typename E, typename... A>
void launch(int T, long long R, int K, A... a) {
    if (T <= 16) launch_t<E, 1>(R, K, a...);
    else if (T <= 32) launch_t<E, 2>(R, K, a...);
    else if (T <= 64) launch_t<E, 4>(R, K, a...);
    else if (T <= 128) launch_t<E, 8>(R, K, a...);
    else launch_t<E, kTT>(R, K, a...);
}

}  // namespace

extern "C" int ov3d_vocab_score(const void* feat, int dtype, long long R, int C, long long ldf, const void* text,
                                int T, int bg, float scale, int K, float* obj, float* lse, int32_t* top_cls,
                                float* top_prob, void* stream) {
    if (!feat || !text || !obj || !lse || !top_cls || !top_prob || (dtype != 0 && dtype != 1) || R < 1 ||
        R > INT_MAX || C < 1 || C > OV3D_DETECT_MAX_C || ldf < C || T < 1 || T > OV3D_DETECT_MAX_T || bg < -1 ||
        bg >= T || K < 1 || K > OV3D_DETECT_MAX_K || !(fabsf(scale) < INFINITY))
        return OV3D_EINVAL;
    const int size = dtype == 0 ? 4 : 2;
    const bool line = ((long long)C * size) % 16 == 0;
    const int vec_feat = line && (ldf * size) % 16 == 0 && reinterpret_cast<uintptr_t>(feat) % 16 == 0;
    const int vec_text = line && reinterpret_cast<uintptr_t>(text) % 16 == 0;
    hipStream_t st = ov3d_stream(stream);
    if (dtype == 0)
        launch<float>(T, R, K, feat, text, R, C, ldf, T, bg, scale, K, vec_feat, vec_text, obj, lse, top_cls, top_prob,
                      st);
    else
        launch<__bf16>(T, R, K, feat, text, R, C, ldf, T, bg, scale, K, vec_feat, vec_text, obj, lse, top_cls,
                       top_prob, st);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

// Open-vocabulary classification (include/ov3d_openvocab.h): R feature vectors against the
// (T, C) text embeddings -> arg max, its dot product and the vector's norm, one launch.
//
// A workgroup of 4 waves owns 64 rows, a wave 16 of them.  The channels go by in chunks of
// 128 bytes of a row (64 2-byte or 32 float32 elements): the workgroup stages the chunk of
// its 64 rows and of all T text rows in LDS (rows and text: 8 lanes per 128-byte line; planes:
// a wave per channel, 64 consecutive pixels), then every wave runs the MFMAs of its 16 rows
// against every tile of 16 text rows.  The text is the A operand and the features the B
// operand, so a lane's accumulators hold 4 text rows of ONE feature row: the arg max is a scan
// of the lane's registers and two xor steps over the four lanes that share the row.  The
// LDS row pitch, the chunk and the fragment read are textdot.h's, shared with vocabscore.hip.
#include <limits.h>

#include <type_traits>

#include "common.h"
#include "textdot.h"
#include "../../include/ov3d_openvocab.h"

namespace {

constexpr int kRows = OV3D_OPENVOCAB_ROWS;
constexpr int kThreads = 256;

// rows layout (features and text): `rows` LDS rows from src rows row0 .., the first `valid` of
// them exist; channels k0 .. k0 + KC - 1, those >= C zero
template <typename E>
__device__ __forceinline__ void stage_rows(unsigned char* dst, const E* src, long long row0, int rows,
                                           int valid, int C, int k0, bool vec) {
    constexpr int KC = kChunk / (int)sizeof(E);
    constexpr int PER = 16 / (int)sizeof(E);
    if (vec) {
        for (int e = threadIdx.x; e < rows * 8; e += kThreads) {
            const int row = e >> 3, pc = e & 7, k = k0 + pc * PER;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < valid && k < C) v = *reinterpret_cast<const uint4*>(src + (row0 + row) * C + k);
            uint2* d = reinterpret_cast<uint2*>(dst + row * kStride + pc * 16);
            d[0] = make_uint2(v.x, v.y);
            d[1] = make_uint2(v.z, v.w);
        }
    } else {
        for (int e = threadIdx.x; e < rows * KC; e += kThreads) {
            const int row = e / KC, kk = e % KC;
            E v = (E)0.0f;
            if (row < valid && k0 + kk < C) v = src[(row0 + row) * C + k0 + kk];
            reinterpret_cast<E*>(dst + row * kStride)[kk] = v;
        }
    }
}

// planes layout: thread (i = tid & 63, kk = tid >> 6, +4 ...) takes row r0 + i, channel k0 + kk
template <typename E>
__device__ __forceinline__ void stage_planes(unsigned char* dst, const E* feat, long long r0, long long R,
                                             int C, long long P, int k0) {
    constexpr int KC = kChunk / (int)sizeof(E);
    const int i = threadIdx.x & 63;
    const long long r = r0 + i;
    const bool valid = r < R;
    const long long f = valid ? r / P : 0, p = valid ? r % P : 0;
    const E* base = feat + f * C * P + p;
    E* d = reinterpret_cast<E*>(dst + i * kStride);
#pragma unroll 4
    for (int kk = threadIdx.x >> 6; kk < KC; kk += kThreads / 64) {
        E v = (E)0.0f;
        if (valid && k0 + kk < C) v = base[(long long)(k0 + kk) * P];
        d[kk] = v;
    }
}

// float32: a chunk is 2 groups of 16 channels; lane (r, h) holds channels 16 g + 4 h + j of its
// row and the 16x16x4 MFMA number j sums over h.  2-byte types: 2 steps of 32 channels, lane
// (r, h) holds channels 32 s + 8 h + j, the operand layout of the 16x16x32 MFMA.
template <typename E, int TT>
__global__ __launch_bounds__(kThreads) void openvocab_kernel(const E* __restrict__ feat, const E* __restrict__ text,
                                                             long long R, int C, int T, long long P, int planes,
                                                             int vec_feat, int vec_text, int unseen,
                                                             int32_t* __restrict__ label, float* __restrict__ score,
                                                             float* __restrict__ norm) {
    constexpr int KC = kChunk / (int)sizeof(E);
    __shared__ __attribute__((aligned(16))) unsigned char smem[(kRows + TT * 16) * kStride];
    unsigned char* fs = smem;
    unsigned char* ts = smem + kRows * kStride;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, h = lane >> 4;
    const long long r0 = (long long)blockIdx.x * kRows;
    const int valid = (int)((R - r0) < kRows ? (R - r0) : kRows);

    f32x4 acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float n2 = 0.f;
    int nz = 0;

    const unsigned char* frow = fs + (wave * 16 + r) * kStride;
    const unsigned char* trow = ts + r * kStride;

    for (int k0 = 0; k0 < C; k0 += KC) {
        if (planes) stage_planes<E>(fs, feat, r0, R, C, P, k0);
        else stage_rows<E>(fs, feat, r0, kRows, valid, C, k0, vec_feat != 0);
        stage_rows<E>(ts, text, 0, TT * 16, T, C, k0, vec_text != 0);
        __syncthreads();
        if constexpr (sizeof(E) == 4) {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const Frag fb = lds_frag(frow + (16 * g + 4 * h) * 4);
                const float b[4] = {__uint_as_float(fb.lo.x), __uint_as_float(fb.lo.y), __uint_as_float(fb.hi.x),
                                    __uint_as_float(fb.hi.y)};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    n2 = fmaf(b[j], b[j], n2);
                    nz |= (b[j] != 0.f);
                }
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    const Frag fa = lds_frag(trow + tt * 16 * kStride + (16 * g + 4 * h) * 4);
                    const float a[4] = {__uint_as_float(fa.lo.x), __uint_as_float(fa.lo.y), __uint_as_float(fa.hi.x),
                                        __uint_as_float(fa.hi.y)};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[tt], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const Frag fb = lds_frag(frow + (32 * s + 8 * h) * 2);
                using V = typename std::conditional<std::is_same<E, __bf16>::value, bf16x8, f16x8>::type;
                const V b = __builtin_bit_cast(V, fb);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = (float)b[j];
                    n2 = fmaf(x, x, n2);
                    nz |= (x != 0.f);
                }
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    const V a = __builtin_bit_cast(V, lds_frag(trow + tt * 16 * kStride + (32 * s + 8 * h) * 2));
                    if constexpr (std::is_same<E, __bf16>::value)
                        acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[tt], 0, 0, 0);
                    else
                        acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[tt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // this lane: text rows 16 tt + 4 h + j of feature row r, ascending
    float bv = 0.f;
    int bi = -1;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = tt * 16 + h * 4 + j;
            const float s = acc[tt][j];
            if (t < T && ((bi < 0 && s == s) || s > bv)) {
                bv = s;
                bi = t;
            }
        }
    }
    // the four lanes of a row: the larger value, the smaller index among equals
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
        n2 += __shfl_xor(n2, off);
        nz |= __shfl_xor(nz, off);
    }
    const long long row = r0 + wave * 16 + r;
    if (h == 0 && row < R) {
        const bool none = nz == 0 || bi < 0;
        label[row] = none ? unseen : bi;
        score[row] = none ? 0.f : bv;
        norm[row] = sqrtf(n2);
    }
}

template <typename E, int TT>
void launch_tt(const void* feat, const void* text, long long R, int C, int T, long long P, int planes,
               int vec_feat, int vec_text, int unseen, int32_t* label, float* score, float* norm,
               hipStream_t stream) {
    const unsigned grid = (unsigned)((R + kRows - 1) / kRows);
    hipLaunchKernelGGL((openvocab_kernel<E, TT>), dim3(grid), dim3(kThreads), 0, stream,
                       static_cast<const E*>(feat), static_cast<const E*>(text), R, C, T, P, planes, vec_feat,
                       vec_text, unseen, label, score, norm);
}

template <typename E, typename... A>
void launch(int T, A... a) {
    if (T <= 16) launch_tt<E, 1>(a...);
    else if (T <= 32) launch_tt<E, 2>(a...);
    else if (T <= 64) launch_tt<E, 4>(a...);
    else if (T <= 128) launch_tt<E, 8>(a...);
    else launch_tt<E, 16>(a...);
}

}  // namespace

extern "C" int ov3d_openvocab_classify(const void* feat, int dtype, int planes, long long R, int C,
                                       long long P, const void* text, int T, int unseen, int32_t* label,
                                       float* score, float* norm, void* stream) {
    if (!feat || !text || !label || !score || !norm || dtype < 0 || dtype > 2 || (planes != 0 && planes != 1) ||
        R < 1 || R > INT_MAX || C < 1 || C > OV3D_OPENVOCAB_MAX_C || T < 1 || T > OV3D_OPENVOCAB_MAX_T)
        return OV3D_EINVAL;
    if (planes && (P < 1 || R % P != 0)) return OV3D_EINVAL;
    const int size = dtype == OV3D_OPENVOCAB_F32 ? 4 : 2;
    const bool line = ((long long)C * size) % 16 == 0;
    const int vec_feat = !planes && line && reinterpret_cast<uintptr_t>(feat) % 16 == 0;
    const int vec_text = line && reinterpret_cast<uintptr_t>(text) % 16 == 0;
    hipStream_t st = ov3d_stream(stream);
    if (dtype == OV3D_OPENVOCAB_F32)
        launch<float>(T, feat, text, R, C, T, P, planes, vec_feat, vec_text, unseen, label, score, norm, st);
    else if (dtype == OV3D_OPENVOCAB_BF16)
        launch<__bf16>(T, feat, text, R, C, T, P, planes, vec_feat, vec_text, unseen, label, score, norm, st);
    else
        launch<_Float16>(T, feat, text, R, C, T, P, planes, vec_feat, vec_text, unseen, label, score, norm, st);
    OV3D_LAUNCH_CHECK();
    return OV3D_OK;
}

// The LDS layout of the feature x text dot products on MFMA, shared by openvocab.hip and
// vocabscore.hip.  16 feature rows per MFMA; the channels go by in chunks of 128 bytes of a row
// (64 2-byte or 32 float32 elements) staged in LDS; the text is the A operand and the features
// the B operand, so a lane's accumulators hold 4 text rows per 16-row text block of ONE feature
// row.  LDS rows are 136 bytes apart (128 + 8): fragments are read 8 bytes at a time.
//
// Each kernel keeps its own stage_rows and MFMA loop.  One template for both was measured on the
// MI355X against openvocab.hip's own code (tools/openvocab_time.py, R = 150 000, C = 512): shared
// staging cost float32 T = 200 2 %, the shared MFMA loop with the norm folded in through a
// callable cost bfloat16 T = 19 6 %.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma.h"

constexpr int kChunk = 128;      // bytes of a row per K-chunk
constexpr int kStride = 136;     // LDS row pitch in bytes

struct alignas(8) Frag {         // 16 bytes of an LDS row, 8-byte aligned
    uint2 lo, hi;
};

__device__ __forceinline__ Frag lds_frag(const unsigned char* p) {
    Frag f;
    f.lo = *reinterpret_cast<const uint2*>(p);
    f.hi = *reinterpret_cast<const uint2*>(p + 8);
    return f;
}

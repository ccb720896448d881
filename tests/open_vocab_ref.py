"""float64 restatement of ov3d_openvocab_classify (include/ov3d_openvocab.h) and the seeded
inputs, error bars and exclusion rule of tests/test_open_vocab_cpu.py and _gpu.py.

The bar is derived, not measured: a float32 dot product over C channels rounds every product
and every addition at most once, so |score - s| <= eps * sum_c |f_c text_c| with
eps = (C + 1) * 2^-23 (a whole ulp each, which covers truncating adders).  The products of two
2-byte values are exact in float32, so the same bar holds for bfloat16 and float16; a kernel that
rounded float32 inputs to a 2-byte type would be off by 2^-9 per product and fail it.  Two
classes whose float64 scores are closer than 2 eps max_t sum|f text| may legitimately swap:
those rows are excluded from the label comparison, and EXCLUDED_CAP bounds their share."""
import numpy as np
import torch

EXCLUDED_CAP = 0.02
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def eps(C):
    return (C + 1) * 2.0 ** -23


def rounded(x, dtype):
    """float64 array -> (tensor of dtype, its exact values in float64)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.float32).to(dtype)
    return t, t.to(torch.float64).numpy()


def classify(feat, text, unseen=None):
    """feat (R, C), text (T, C) float64 -> dict: label (R) int32, score (R), n2 (R) the squared
    norm, s (R, T) every dot product, absdot (R, T) = sum_c |f_c text_c|"""
    f, t = np.asarray(feat, dtype=np.float64), np.asarray(text, dtype=np.float64)
    T = t.shape[0]
    unseen = T if unseen is None else unseen
    with np.errstate(all="ignore"):
        s = f @ t.T
        absdot = np.abs(f) @ np.abs(t).T
        n2 = (f * f).sum(1)
    # ascending t, replaced on a strict > only, NaN never wins: the first of the largest non-NaN
    valid = ~np.isnan(s)
    masked = np.where(valid, s, -np.inf)
    first = (valid & (masked == masked.max(1, keepdims=True))).argmax(1)
    wins = valid.any(1) & (f != 0).any(1)
    label = np.where(wins, first, unseen).astype(np.int32)
    score = np.where(wins, s[np.arange(len(f)), first], 0.0)
    return {"label": label, "score": score, "n2": n2, "s": s, "absdot": absdot}


def excluded(ref, C):
    """rows whose float64 top-2 margin is within 2 eps max_t sum|f text|: their label may differ"""
    s = np.where(np.isnan(ref["s"]), -np.inf, ref["s"])
    if s.shape[1] == 1:
        return np.zeros(len(s), bool)
    top = np.sort(s, axis=1)
    with np.errstate(invalid="ignore"):
        margin = top[:, -1] - top[:, -2]
    return ~(margin > 2 * eps(C) * ref["absdot"].max(1))


def to_planes(rows, F, P):
    """(F * P, C) rows -> (F, C, P) planes holding the same vectors"""
    return np.ascontiguousarray(rows.reshape(F, P, rows.shape[1]).transpose(0, 2, 1))


def exact_case(R, C, T, seed=0):
    """integers: features in [-4, 4], text in [-3, 3]; every partial sum < 2^24, so any order
    of accumulation is exact in float32 and ties are plentiful"""
    rng = np.random.default_rng(1000003 * seed + 4099 * R + 17 * C + T)
    return (rng.integers(-4, 5, (R, C)).astype(np.float64), rng.integers(-3, 4, (T, C)).astype(np.float64))


def normalised(text):
    return text / np.sqrt((text * text).sum(1, keepdims=True))


def normal_case(R, C, T, seed=0):
    """unit-normal features against L2-normalised normal text"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((R, C)), normalised(rng.standard_normal((T, C)))


def prototype_case(R, C, T, seed=0):
    """every feature is one text prototype plus 2 / sqrt(C) noise: wide margins"""
    rng = np.random.default_rng(seed)
    text = normalised(rng.standard_normal((T, C)))
    which = rng.integers(0, T, R)
    return text[which] + (2.0 / np.sqrt(C)) * rng.standard_normal((R, C)), text

"""float64 restatement of ov3d_vocab_score (include/ov3d_detect.h) and of the detection chain
around it (ov3d_amd.detect), with the seeded inputs and the error bars of
tests/test_detect_cpu.py and tests/test_detect_gpu.py.

Every bar is derived here and nothing is tuned to the kernel.  u = 2^-24 is half a float32 ulp
of 1, so 2u is a whole ulp, relative.

Score.  delta = (C + 2) * 2u * absdot with absdot = |scale| * sum_c |f_c text_c|: the float32 dot
product over C channels rounds every product and every addition at most once, a whole ulp each
(which covers truncating adders): open_vocab_ref.eps(C) = (C + 1) * 2u; the multiply by scale
is one more rounding.  Products of two bfloat16 values are exact in float32, so the same bar
holds for both dtypes.

Exact dot products (the exact family: the kernel's s_t equal the float64 ones bit for bit, and
so does m).  A probability e_t / Z and obj = F / Z take the relative bar (a + T + c) * 2u:
  a  the argument s_t - m of an exponential is a float32 difference and carries half an ulp of
     its own magnitude, u * |s_t - m|, which the exponential turns into a relative error of
     the same size; counted at a whole ulp here.  For a probability a is its own |s_t - m| plus
     the softmax-weighted mean of |s_t - m| over Z's terms (the share of Z's relative error
     that comes from its terms' arguments); for obj it is that mean over F's terms plus the one
     over Z's.  |s_t - m| is capped at A_CAP = 104 > 150 ln 2, past which float32 expf returns
     0 and the term is covered by the floor below.  A streamed evaluation that rescales its
     running sum by expf(m_old - m_new) splits s_t - m into pieces whose magnitudes add up to
     |s_t - m| (the running maximum only rises), so its argument errors stay inside a.
  T  the sum of T non-negative terms in any order: at most T - 1 roundings of u each, counted
     at 2u; the other T * u cover the rescalings of a streamed sum (one expf, 2u, and one
     multiply, u, per tile that raises the maximum; with tiles at least 4 wide that is under
     0.75 T u).
  c  C_FN = 4 ulp for the library functions, at the bounds the HIP math API documentation
     gives for ROCm's device library: expf 1 ulp (once in the numerator, once in each of the
     denominator's terms), logf 1 ulp, and the float32 division 0.5 ulp (correctly rounded
     under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt): 1 + 1 + 0.5 for a
     probability or obj, rounded up.
The absolute floor FLOOR = 2^-126, the smallest normal float32: a term below it may be flushed
or lose all of its precision.  A probability takes one floor (Z >= 1 up to rounding, the
largest term being expf(0) = 1), obj takes T of them.

lse = m + logf(Z): absolute bar (a + T + c) * 2u for ln Z (a: the weighted mean over Z's terms)
plus 2u * |ln Z| for logf and 2u * |lse| for the final addition.

Rounded dot products.  Every s_t moves by at most delta_t, so a ratio of sums of exp(s_t) moves
by a factor within exp(+-2 d), d = max_t delta_t: exp(2 d) - 1 is added to the relative bars
(compounded), and lse, 1-Lipschitz in the largest score change, takes d more.

Objectness interval.  obj = 1 / (1 + r) with r = e_bg / F, and r moves by a factor within
exp(+-2 d): obj_interval returns [1 / (1 + r exp(2 d)), 1 / (1 + r exp(-2 d))] widened by the
exact relative bar.  It lies inside the relative bar above: the width a float32 objectness
can really have near 1, where the relative bar is loose.  The chain tests' separation
preconditions (separated_all) use the relative bar itself.
"""
import numpy as np

import open_vocab_ref as OVR

U = 2.0 ** -24
A_CAP = 104.0
C_FN = 4.0
FLOOR = 2.0 ** -126
CHAIN_SEED = 0      # of chain_case: chosen on the CPU so that separated_all and top1_clear hold

normal_case = OVR.normal_case
prototype_case = OVR.prototype_case
rounded = OVR.rounded


def exact_shift(C):
    """the power of two k of exact_case: an integer feature in [-4, 4] has mean square 60 / 9,
    an integer text element in [-3, 3] mean square 4, so a dot product over C channels has
    standard deviation sqrt(C * 80 / 3) = 5.16 sqrt(C); k = round(log2 of that) brings it into
    [0.71, 1.41]"""
    return max(0, int(round(np.log2(np.sqrt(C * 80.0 / 3.0)))))


def exact_case(R, C, T, seed=0):
    """open_vocab_ref.exact_case (integers: features in [-4, 4], text in [-3, 3]) with the
    features times 2^-ceil(k / 2) and the text times 2^-floor(k / 2), k = exact_shift(C): the
    dot products are integers below 2^24 times 2^-k, exact in float32 in any order of
    accumulation and exact in bfloat16 inputs; a row's scores spread over order 1 and ties are
    plentiful"""
    feat, text = OVR.exact_case(R, C, T, seed)
    k = exact_shift(C)
    return feat * 2.0 ** -((k + 1) // 2), text * 2.0 ** -(k // 2)


def score(feat, text, bg, scale, K):
    """feat (R, C), text (T, C) float64 -> dict: s (R, T) = scale * feat @ text.T, absdot,
    m, e = exp(s - m), F, Z, obj, lse (R), top_cls (R, K) int32, top_prob (R, K); ties go to
    the smaller index; a row with a non-finite score takes obj 0, lse NaN, classes -1 and
    probabilities 0"""
    f, t = np.asarray(feat, dtype=np.float64), np.asarray(text, dtype=np.float64)
    R, T = f.shape[0], t.shape[0]
    with np.errstate(all="ignore"):
        s = scale * (f @ t.T)
        absdot = abs(scale) * (np.abs(f) @ np.abs(t).T)
    ok = np.isfinite(s).all(1)
    ss = np.where(ok[:, None], s, 0.0)
    fg = np.arange(T) != bg
    m = ss.max(1)
    e = np.exp(ss - m[:, None])
    F = (e * fg).sum(1)
    Z = F + (e[:, bg] if bg >= 0 else 0.0)
    obj = np.where(ok, F / Z, 0.0)
    lse = np.where(ok, m + np.log(Z), np.nan)
    key = np.where(fg, ss, -np.inf)
    order = np.argsort(-key, axis=1, kind="stable")[:, :K]
    nfg = T - (bg >= 0)
    top_cls = np.full((R, K), -1, np.int32)
    top_prob = np.zeros((R, K))
    n = min(K, nfg)
    top_cls[:, :n] = order[:, :n]
    top_prob[:, :n] = np.take_along_axis(e, order[:, :n], 1) / Z[:, None]
    top_cls[~ok] = -1
    top_prob[~ok] = 0.0
    return {"s": s, "absdot": absdot, "ok": ok, "m": m, "e": e, "F": F, "Z": Z, "obj": obj, "lse": lse,
            "top_cls": top_cls, "top_prob": top_prob, "fg": fg, "bg": bg}


def delta(ref, C):
    """(R, T): the bar of every float32 score against its float64 value"""
    return (C + 2) * 2 * U * ref["absdot"]


def _means(ref):
    """the softmax-weighted means of a = min(m - s, A_CAP) over Z's and over F's terms, and a"""
    a = np.minimum(ref["m"][:, None] - np.where(ref["ok"][:, None], ref["s"], 0.0), A_CAP)
    with np.errstate(all="ignore"):
        az = (a * ref["e"]).sum(1) / ref["Z"]
        af = np.where(ref["F"] > 0, (a * ref["e"] * ref["fg"]).sum(1) / np.where(ref["F"] > 0, ref["F"], 1.0), 0.0)
    return a, az, af


def bars(ref, C, cls=None, rounded_dots=False):
    """-> dict of bars for the rows of ref: prob_rel (R, K) for the classes cls (default: the
    restatement's own top_cls; -1 slots get 0), prob_floor, obj_rel (R), obj_floor, lse_abs (R),
    d (R) = max_t delta (0 for exact dot products)"""
    T = ref["s"].shape[1]
    cls = ref["top_cls"] if cls is None else cls
    a, az, af = _means(ref)
    at = np.take_along_axis(a, np.maximum(cls, 0).astype(np.int64), 1)
    prob_rel = (at + az[:, None] + T + C_FN) * 2 * U
    obj_rel = (af + az + T + C_FN) * 2 * U
    with np.errstate(all="ignore"):
        lse_abs = (az + T + C_FN) * 2 * U + 2 * U * (np.abs(np.log(ref["Z"])) + np.abs(ref["lse"]))
    d = delta(ref, C).max(1) if rounded_dots else np.zeros(len(az))
    g = np.expm1(2 * d)
    prob_rel = (1 + g[:, None]) * (1 + prob_rel) - 1
    obj_rel = (1 + g) * (1 + obj_rel) - 1
    return {"prob_rel": np.where(cls >= 0, prob_rel, 0.0), "prob_floor": FLOOR, "obj_rel": obj_rel,
            "obj_floor": T * FLOOR, "lse_abs": lse_abs + d, "d": d}


def obj_interval(ref, C, rounded_dots=True):
    """-> (lo, hi) (R): where a float32 objectness computed from float32 scores may lie"""
    T = ref["s"].shape[1]
    _, az, af = _means(ref)
    rel = (af + az + T + C_FN) * 2 * U
    d = delta(ref, C).max(1) if rounded_dots else np.zeros(len(az))
    with np.errstate(all="ignore"):
        r = np.where(ref["F"] > 0, (ref["Z"] - ref["F"]) / np.where(ref["F"] > 0, ref["F"], 1.0), np.inf)
        lo, hi = 1.0 / (1.0 + r * np.exp(2 * d)), 1.0 / (1.0 + r * np.exp(-2 * d))
    return lo * (1 - rel) - T * FLOOR, hi * (1 + rel) + T * FLOOR


def softmax_direct(s, bg):
    """the plain softmax over one row's scores -> (probabilities (T), obj = 1 - p_bg or 1)"""
    s = np.asarray(s, dtype=np.float64)
    p = np.exp(s - np.log(np.exp(s).sum()))
    return p, (1.0 - p[bg] if bg >= 0 else 1.0)


# ---------------------------------------------------------------- the detection chain

def nms(boxes, thr, old_type=False, samecls=True, valid=None):
    """greedy NMS over rows [x1, y1, z1, x2, y2, z2, score(, class)] in float64 -> keep (K) bool.
    Boxes are visited by descending score, among equal scores the larger index first; a visited
    box that is still alive is kept and kills every later one whose overlap with it exceeds thr
    (intersection over union, or over the later box's own volume for old_type; with samecls
    only boxes of its class)."""
    b = np.asarray(boxes, dtype=np.float64)
    K = len(b)
    alive = np.ones(K, bool) if valid is None else np.asarray(valid, bool).copy()
    vol = np.prod(b[:, 3:6] - b[:, 0:3], axis=1)
    order = sorted(range(K), key=lambda i: (-b[i, 6], -i))
    keep = np.zeros(K, bool)
    for pos, i in enumerate(order):
        if not alive[i]:
            continue
        keep[i] = True
        rest = np.array([j for j in order[pos + 1:] if alive[j]], dtype=np.int64)
        if not len(rest):
            continue
        side = np.maximum(0.0, np.minimum(b[i, 3:6], b[rest, 3:6]) - np.maximum(b[i, 0:3], b[rest, 0:3]))
        inter = side.prod(1)
        with np.errstate(all="ignore"):
            o = inter / vol[rest] if old_type else inter / (vol[i] + vol[rest] - inter)
        if samecls:
            o = o * (b[rest, 7] == b[i, 7])
        alive[rest[o > thr]] = False
    return keep


def nms_table(corners, obj, cls, use_3d=True):
    """corners (Q, 8, 3) float32, obj (Q), cls (Q) -> the float64 NMS rows of one scene:
    the corners' bounding box, obj and the class, or (use_3d False) the bird's-eye rectangle
    of x and z as a box of unit depth"""
    c = np.asarray(corners, dtype=np.float64)
    lo, hi = c.min(1), c.max(1)
    if use_3d:
        return np.concatenate([lo, hi, np.asarray(obj, np.float64)[:, None], np.asarray(cls, np.float64)[:, None]], 1)
    z, o = np.zeros(len(c)), np.ones(len(c))
    return np.stack([lo[:, 0], z, lo[:, 2], hi[:, 0], o, hi[:, 2], np.asarray(obj, np.float64)], 1)


def chain(ref, corners, counts, cfg, Q):
    """the detection chain of ov3d_amd.detect.detect on the float64 scoring `ref` of B * Q rows:
    corners (B, Q, 8, 3), counts (B, Q) the points inside every box (None without the empty-box
    filter) -> (keep (B, Q) bool, det (B, Q) bool)"""
    B = corners.shape[0]
    obj = ref["obj"].reshape(B, Q)
    cls = ref["top_cls"][:, 0].reshape(B, Q)
    keep = np.zeros((B, Q), bool)
    for b in range(B):
        if cfg["remove_empty_box"]:
            nonempty = counts[b] >= 5
            if not nonempty.any():
                nonempty[np.argmax(obj[b])] = True
        else:
            nonempty = np.ones(Q, bool)
        if cfg.get("no_nms", False):
            keep[b] = nonempty
        elif not cfg["use_3d_nms"]:
            keep[b] = nms(nms_table(corners[b], obj[b], cls[b], False), cfg["nms_iou"], cfg["use_old_type_nms"],
                          samecls=False, valid=nonempty)
        else:
            keep[b] = nms(nms_table(corners[b], obj[b], cls[b]), cfg["nms_iou"], cfg["use_old_type_nms"],
                          samecls=cfg["cls_nms"], valid=nonempty)
    return keep, keep & (obj > cfg["conf_thresh"])


def separated_all(ref, C, conf_thresh, B, Q):
    """the separation preconditions of the chain tests, on the float64 values: no two objectness
    values of a scene are closer than the sum of their rounded bars and none is within its bar of
    conf_thresh -> (ok, offending pairs, offending thresholds)"""
    b = bars(ref, C, rounded_dots=True)
    obj = ref["obj"].reshape(B, Q)
    bar = (b["obj_rel"] * ref["obj"] + b["obj_floor"]).reshape(B, Q)
    close = np.abs(obj[:, :, None] - obj[:, None, :]) <= bar[:, :, None] + bar[:, None, :]
    pairs = (int(close.sum()) - B * Q) // 2
    thr = int((np.abs(obj - conf_thresh) <= bar).sum())
    return pairs == 0 and thr == 0, pairs, thr


def chain_case(seed, B=2, Q=64, C=64, T=11, num_points=2000):
    """synthetic model outputs: the boxes and point cloud of tests/golden/eval_cases.py (boxes
    around the scene's objects and elsewhere in the room, many of them empty), float32 query
    embeddings ~ N(0.3, 1) and a float32 text table ~ N(0, 0.1^2) whose last row, the
    background, has mean 0.135: the background score then sits near the foreground's
    log-sum-exp (ln 10 + 0.32 against 0.3 * 64 * 0.135) and the objectness values spread over
    (0, 1) instead of crowding at 1"""
    from eval_cases import make_batches
    bt = make_batches(num_batches=1, batch=B, K=Q, num_points=num_points, num_classes=20, seed=seed)[0]
    rng = np.random.default_rng(7919 * seed + 13)
    text = 0.1 * rng.standard_normal((T, C))
    text[-1] += 0.135
    return {"visual": (0.3 + rng.standard_normal((B, Q, C))).astype(np.float32), "text": text.astype(np.float32),
            "corners": bt["pred_corners"].astype(np.float32), "points": bt["point_clouds"].astype(np.float32)}


def top1_clear(ref, C):
    """(R) bool: the best foreground score leads the second by more than 2 max_t delta, so a
    float32 evaluation cannot name another top-1 class (rows with one foreground class pass)"""
    key = np.sort(np.where(ref["fg"], ref["s"], -np.inf), axis=1)
    if key.shape[1] < 2 or not np.isfinite(key[:, -2]).all():
        return np.ones(len(key), bool)
    return key[:, -1] - key[:, -2] > 2 * delta(ref, C).max(1)

"""Detecting with any vocabulary on the GPU (csrc/vocabscore.hip behind include/ov3d_detect.h,
ov3d_amd.detect) against the float64 restatement and its derived bars
(tests/vocab_score_ref.py): exact integer cases at the shapes where the tiling can go wrong,
rounded cases inside the bars, the special rows, independence bit for bit, the guard-band case
(tests/guard.py), the launch census and a hipGraph capture (a synchronisation raises there),
the training vocabulary against the existing parse_predictions path, and a vocabulary swap on
a real model.

The vocabulary swap.  The eval fixture (tests/golden/model_sun_eval.npz) carries no state dict,
so the model is built as tests/test_eval_forward_gpu.py builds it (full_fixture.build) rather
than through helpers.build_model_from_fixture.  Its weights are a random initialisation, and the
query embeddings of such a model are all but one vector: over the fixture's float64 outputs the
rows have norm 4.57 and lie 0.054 from their mean, and under the model's own table the 256
objectness values span 0.95519 .. 0.95543, 2e-6 apart on average, while the interval a float32
objectness may lie in (vocab_score_ref.obj_interval) is 4.6e-5 wide.  No separation
precondition can hold there, under any vocabulary: which box the NMS visits first is inside the
rounding error, so a comparison of detections against a float64 chain would be unsound.  The
swap is therefore pinned in two sound halves that meet at the kernel's outputs: those outputs
against float64 inside the rounded bars with tolerant class validity (as the rounded cases),
and the chain after them, exactly: the numpy restatement of the chain (its NMS checked on the
CPU against tests/golden/nms.npz) and the existing parse_predictions, both fed the kernel's own
objectness and probabilities, must give detect()'s detections and scores bit for bit.  The
point counts of the empty-box filter come from the existing ov3d_box_points_count launch, which
tests/test_evaldet_gpu.py pins against the reference.
"""
import functools

import numpy as np
import pytest
import torch

import guard
import vocab_score_ref as V
from guard import In, Out
from helpers import ov3d  # noqa: F401

pytestmark = pytest.mark.gpu

# the entries this file's cases run between guard bands (tests/guard_cases.py)
ENTRIES = ("ov3d_vocab_score",)

TILE = 256                      # OV3D_DETECT_TILE_T, the kernel's vocabulary tile width
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DT = list(DTYPES)


@pytest.fixture(scope="module")
def D(ov3d):
    from ov3d_amd import detect
    assert detect.TILE_T == TILE
    return detect


def host(t):
    return t.cpu().numpy()


def bg_row(where, T):
    return {"last": T - 1, "first": 0, "mid": T // 2, "none": -1}[where]


def run(D, cuda, feat, vocab, K, ld=None):
    """feat (R, C) host tensor -> host arrays obj, lse, top_cls, top_prob; ld: the rows live in a
    wider buffer and are passed as a strided view"""
    if ld is None:
        f = feat.to(cuda)
    else:
        buf = torch.full((feat.shape[0], ld), float("nan"), dtype=feat.dtype, device=cuda)
        buf[:, :feat.shape[1]] = feat.to(cuda)
        f = buf[:, :feat.shape[1]]
        assert not f.is_contiguous() or feat.shape[0] == 1
    out = D.score_queries(f, vocab.to(cuda), K)
    obj, lse, cls, prob = (host(o) for o in out)
    R = feat.shape[0]
    assert obj.shape == lse.shape == (R,) and cls.shape == prob.shape == (R, K)
    assert obj.dtype == lse.dtype == prob.dtype == np.float32 and cls.dtype == np.int32
    return obj, lse, cls, prob


def within(got, want, rel, floor):
    return np.abs(got.astype(np.float64) - want) <= rel * np.abs(want) + floor


# ---------------------------------------------------------------- exact cases

# R around the 16-row wave tile, the 64-row workgroup and the 4096-row switch between the two
# four-wave workgroup shapes; C around the 128-byte chunk of either element size; T in one, two
# and sixteen tiles, around the tile width and in every accumulator count (1, 2, 4, 8, 16 blocks
# of 16); K at both ends and on both sides of 8, above which one wave takes the row group alone;
# every background
# (R, C, T, K, background, extra row pitch, scale)
EXACT = [(1, 1, 1, 1, "last", 0, 1.0), (1, 1, 1, 5, "none", 0, 1.0), (63, 8, 2, 5, "first", 0, 1.0),
         (64, 13, 17, 16, "mid", 3, 1.0), (65, 13, 40, 5, "mid", 0, 1.0), (63, 8, 100, 8, "last", 0, 1.0),
         (65, 96, TILE - 1, 5, "last", 0, 1.0), (65, 520, TILE, 16, "none", 0, 1.0),
         (1000, 96, TILE + 1, 5, "mid", 0, 0.5), (1000, 640, 17, 1, "last", 0, 1.0),
         (1000, 96, 4096, 16, "last", 0, 1.0), (63, 640, 4096, 5, "first", 0, 1.0),
         (4100, 13, TILE + 1, 5, "last", 0, 1.0), (4100, 96, 40, 8, "mid", 0, 1.0), (4100, 96, 17, 8, "mid", 0, 1.0),
         (4100, 8, 2, 16, "last", 0, 1.0)]


@functools.lru_cache(maxsize=None)
def exact_ref(R, C, T, K, bg, scale):
    feat, text = V.exact_case(R, C, T)
    return feat, text, V.score(feat, text, bg, scale, K)


@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("R,C,T,K,where,extra,scale", EXACT)
def test_exact_cases_equal_float64(cuda, D, R, C, T, K, where, extra, scale, name):
    dtype, bg = DTYPES[name], bg_row(where, T)
    feat, text, ref = exact_ref(R, C, T, K, bg, scale)
    vocab = D.Vocabulary(text, background=None if bg < 0 else bg, dtype=dtype, scale=scale)
    assert np.array_equal(vocab.text.double().numpy(), text)
    obj, lse, cls, prob = run(D, cuda, torch.from_numpy(feat).to(dtype), vocab, K, ld=C + extra if extra else None)
    assert np.array_equal(cls, ref["top_cls"])                         # padding included
    bar = V.bars(ref, C)
    worst = max(np.max(np.abs(prob - ref["top_prob"]) / (bar["prob_rel"] * ref["top_prob"] + bar["prob_floor"])),
                np.max(np.abs(obj - ref["obj"]) / (bar["obj_rel"] * ref["obj"] + bar["obj_floor"])),
                np.max(np.abs(lse - ref["lse"]) / bar["lse_abs"]))
    print(f"exact R={R} C={C} T={T} K={K} bg={where} {name}: worst error / bar {worst:.3g}")
    assert within(prob, ref["top_prob"], bar["prob_rel"], bar["prob_floor"]).all()
    assert within(obj, ref["obj"], bar["obj_rel"], bar["obj_floor"]).all()
    assert within(lse, ref["lse"], 0.0, bar["lse_abs"]).all()
    assert (prob[cls < 0] == 0).all() and (cls[:, min(K, T - (bg >= 0)):] == -1).all()
    if bg < 0:
        assert (obj == 1.0).all()
    if T == 1 and bg == 0:
        assert (obj == 0.0).all() and (cls == -1).all()
    if T >= TILE and R >= 1000:
        top = np.take_along_axis(ref["s"], np.maximum(ref["top_cls"], 0).astype(np.int64), 1)
        assert (top[:, 1:] == top[:, :-1]).any()                       # ties inside the top-K were there


# ---------------------------------------------------------------- rounded cases

@functools.lru_cache(maxsize=None)
def rounded_ref(family, name, T):
    from ov3d_amd import detect as D
    dtype = DTYPES[name]
    feat, text = getattr(V, family + "_case")(4096, 640, T)
    ft, fv = V.rounded(feat, dtype)
    vocab = D.Vocabulary(text, dtype=dtype)
    return ft, vocab, V.score(fv, vocab.text.double().numpy(), T - 1, 1.0, 5)


def check_rounded(ref, C, bg, obj, lse, cls, prob, what):
    """the rounded bars and the tolerant validity of the classes; prints the worst error / bar"""
    R, K = cls.shape
    rows = np.arange(R)[:, None]
    bar = V.bars(ref, C, cls=cls, rounded_dots=True)
    d = bar["d"]
    assert ((cls >= 0) & (cls < ref["s"].shape[1]) & (cls != bg)).all()
    assert (np.sort(cls, 1)[:, 1:] != np.sort(cls, 1)[:, :-1]).all()          # distinct
    got = ref["s"][rows, cls]
    best = -np.sort(-np.where(ref["fg"], ref["s"], -np.inf), axis=1)[:, :K]
    assert (got >= best - 2 * d[:, None]).all()                       # no lower than the j-th largest
    assert (got[:, 1:] <= got[:, :-1] + 2 * d[:, None]).all()         # non-increasing
    want = ref["e"][rows, cls] / ref["Z"][:, None]
    worst = max(np.max(np.abs(prob - want) / (bar["prob_rel"] * want + bar["prob_floor"])),
                np.max(np.abs(obj - ref["obj"]) / (bar["obj_rel"] * ref["obj"] + bar["obj_floor"])),
                np.max(np.abs(lse - ref["lse"]) / bar["lse_abs"]))
    print(f"{what}: worst error / bar {worst:.3g}, classes differing from float64 "
          f"{(cls != ref['top_cls']).any(1).sum()} rows of {R}")
    assert within(lse, ref["lse"], 0.0, bar["lse_abs"]).all()         # the scores, through lse
    assert within(obj, ref["obj"], bar["obj_rel"], bar["obj_floor"]).all()
    assert within(prob, want, bar["prob_rel"], bar["prob_floor"]).all()


@pytest.mark.parametrize("T", [19, 1204])
@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("family", ["normal", "prototype"])
def test_rounded_cases_stay_inside_the_derived_bar(cuda, D, family, name, T):
    ft, vocab, ref = rounded_ref(family, name, T)
    obj, lse, cls, prob = run(D, cuda, ft, vocab, 5)
    check_rounded(ref, 640, T - 1, obj, lse, cls, prob, f"{family} {name} T={T}")


# ---------------------------------------------------------------- special rows

@pytest.mark.parametrize("name", DT)
def test_special_rows(cuda, D, name):
    dtype = DTYPES[name]
    R, C, T, K = 130, 40, 19, 5
    feat, text = V.exact_case(R, C, T, seed=1)
    text[:, 0] = 0.0
    text[T - 1, 0] = 0.5                               # the background alone sees channel 0
    clean = feat.copy()
    nan, inf, zero, dom = 5, 17, 20, 33                # rows of the first three 16-row workgroups
    feat[nan, 7] = np.nan
    feat[inf, 3] = np.inf
    feat[zero] = 0.0
    feat[dom] = 0.0
    feat[dom, 0] = 256.0                               # s_bg = 128, every other score 0
    vocab = D.Vocabulary(text, dtype=dtype)
    obj, lse, cls, prob = run(D, cuda, torch.from_numpy(feat).to(dtype), vocab, K)
    ref = V.score(feat, text, T - 1, 1.0, K)
    for r in (nan, inf):
        assert obj[r] == 0 and np.isnan(lse[r]) and (cls[r] == -1).all() and (prob[r] == 0).all()
    assert cls[zero].tolist() == [0, 1, 2, 3, 4] and (prob[zero] == prob[zero, 0]).all()
    assert abs(prob[zero, 0] - 1 / 19) <= 2.0 ** -22 / 19 and abs(obj[zero] - 18 / 19) <= 2.0 ** -22 and \
        abs(lse[zero] - np.log(19)) <= 2.0 ** -21
    assert ref["s"][dom, T - 1] - ref["s"][dom, :T - 1].max() > 104
    assert obj[dom] == 0 and (prob[dom] == 0).all() and lse[dom] == 128 and cls[dom].tolist() == [0, 1, 2, 3, 4]
    # everything else, the neighbours in the same workgroups included, is as without the special rows
    others = np.setdiff1d(np.arange(R), [nan, inf, zero, dom])
    assert np.array_equal(cls[others], ref["top_cls"][others])
    bar = V.bars(ref, C)
    assert within(prob, ref["top_prob"], bar["prob_rel"], bar["prob_floor"])[others].all()
    base = run(D, cuda, torch.from_numpy(clean).to(dtype), vocab, K)
    for a, b in zip((obj, lse, cls, prob), base):
        assert np.array_equal(a[others].view(np.int32), b[others].view(np.int32))


# ---------------------------------------------------------------- independence

@pytest.mark.parametrize("name", DT)
def test_a_row_depends_on_its_values_alone(cuda, D, name):
    """alone, at the end of a 65-row launch, inside a 1000-row launch, inside launches of the
    other two workgroup shapes, and through strided views: bit for bit"""
    dtype = DTYPES[name]
    R, C, T, K = 1000, 200, 300, 5
    feat, text = V.normal_case(R, C, T, seed=7)
    ft = V.rounded(feat, dtype)[0]
    vocab = D.Vocabulary(text, dtype=dtype, background=17)
    base = run(D, cuda, ft, vocab, K)
    bits = lambda out: [np.ascontiguousarray(o).view(np.int32) for o in out]          # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))   # noqa: E731
    for r in (0, 777, R - 1):
        assert same(run(D, cuda, ft[r:r + 1], vocab, K), [o[r:r + 1] for o in base])
    assert same([o[-1:] for o in run(D, cuda, ft[713:778], vocab, K)], [o[777:778] for o in base])
    assert same(run(D, cuda, ft, vocab, K, ld=C + 3), base)
    big = run(D, cuda, ft.repeat(5, 1)[:4100], vocab, K)               # four waves, 64 rows
    assert same([o[3000:4000] for o in big], base)
    deep = run(D, cuda, ft, vocab, 16)                                 # one wave, 16 rows
    assert same([deep[0], deep[1], deep[2][:, :K], deep[3][:, :K]], base)
    # the last layer of a stacked (L, B, Q, C) output, and a channel slice of a wider one
    stacked = torch.zeros(3, 4, 250, C, dtype=dtype, device=cuda)
    stacked[-1] = ft.to(cuda).view(4, 250, C)
    out = D.score_queries(stacked[-1], vocab.to(cuda), K)
    assert out[0].shape == (4, 250) and out[2].shape == (4, 250, K)
    assert same([host(o).reshape((R,) + o.shape[2:]) for o in out], base)
    wide = torch.zeros(4, 250, C + 8, dtype=dtype, device=cuda)
    wide[..., :C] = ft.to(cuda).view(4, 250, C)
    out = D.score_queries(wide[..., :C], vocab.to(cuda), K)
    assert same([host(o).reshape((R,) + o.shape[2:]) for o in out], base)
    assert len(np.unique(base[2][:, 0])) > 50


# ---------------------------------------------------------------- guard bands

@pytest.mark.parametrize("name", DT)
def test_guard_vocab_score(cuda, ov3d, name):
    dtype = DTYPES[name]
    R, C, T, K = 65, 13, TILE + 1, 16
    feat, text = V.exact_case(R, C, T, seed=2)
    ref = V.score(feat, text, T - 1, 1.0, K)
    specs = {"feat": In(torch.from_numpy(feat).to(dtype), ld=C + 3), "text": In(torch.from_numpy(text).to(dtype)),
             "obj": Out((R,), torch.float32), "lse": Out((R,), torch.float32),
             "cls": Out((R, K), torch.int32), "prob": Out((R, K), torch.float32)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_vocab_score", t["feat"], {"f32": 0, "bf16": 1}[name], R, C, C + 3, t["text"], T, T - 1, 1.0, K,
        t["obj"], t["lse"], t["cls"], t["prob"], like=t["feat"]))
    bar = V.bars(ref, C)
    assert np.array_equal(host(out["cls"]), ref["top_cls"])
    assert within(host(out["prob"]), ref["top_prob"], bar["prob_rel"], bar["prob_floor"]).all()
    assert within(host(out["obj"]), ref["obj"], bar["obj_rel"], bar["obj_floor"]).all()
    assert within(host(out["lse"]), ref["lse"], 0.0, bar["lse_abs"]).all()


@pytest.mark.parametrize("bad", [dict(K=17), dict(T=0)])
def test_guard_rejected_calls_write_nothing(cuda, ov3d, bad):
    R, C, T, K = 65, 13, TILE + 1, 16
    feat, text = V.exact_case(R, C, T, seed=2)
    a = dict(T=T, K=K)
    a.update(bad)
    specs = {"feat": In(torch.from_numpy(feat).float(), ld=C + 3), "text": In(torch.from_numpy(text).float()),
             "obj": Out((R,), torch.float32), "lse": Out((R,), torch.float32),
             "cls": Out((R, K), torch.int32), "prob": Out((R, K), torch.float32)}
    guard.run_case(cuda, specs, lambda t: guard.raw_call(
        "ov3d_vocab_score", t["feat"], 0, R, C, C + 3, t["text"], a["T"], -1, 1.0, a["K"], t["obj"], t["lse"],
        t["cls"], t["prob"], like=t["feat"]), expect_reject=True)


# ---------------------------------------------------------------- the chain

class _Cfg:
    def __init__(self, c):
        self.num_semcls = c


def chain_inputs(cuda, c):
    out = {"visual_embeds": torch.from_numpy(c["visual"]).to(cuda), "box_corners": torch.from_numpy(c["corners"]).to(cuda),
           "sem_cls_prob": torch.full((2, 64, 10), float("nan"), device=cuda),          # never read
           "objectness_prob": torch.full((2, 64), float("nan"), device=cuda)}
    return out, torch.from_numpy(c["points"]).to(cuda)


def triples(dets, corners):
    """per-scene lists of (class, corners, score) -> [(scene, class, query)], [score]"""
    where = [{corners[b, q].tobytes(): q for q in range(corners.shape[1])} for b in range(len(corners))]
    assert all(len(w) == corners.shape[1] for w in where)              # the boxes tell the queries apart
    tri = [(b, int(c), where[b][np.ascontiguousarray(box, np.float32).tobytes()])
           for b, scene in enumerate(dets) for c, box, _ in scene]
    return tri, np.array([s for scene in dets for _, _, s in scene], dtype=np.float64)


# ---------------------------------------------------------------- census and capture

def test_one_launch_and_nothing_synchronises(cuda, D):
    """the census of entry calls, and score_queries and detect inside a hipGraph capture, where a
    synchronisation or a read-back raises; the replay gives the eager results"""
    from ov3d_amd import _native
    c = V.chain_case(V.CHAIN_SEED)
    out, points = chain_inputs(cuda, c)
    vocab = D.Vocabulary(c["text"], device=cuda)
    rows = out["visual_embeds"].view(128, 64)

    def both():
        det = D.detect(out, vocab, points, topk=10)
        return D.score_queries(rows, vocab, 7) + (det.keep, det.cls, det.score, det.obj)

    _native.census_start()
    D.score_queries(rows, vocab, 7)
    assert _native.census_stop() == {"ov3d_vocab_score": 1}
    _native.census_start()
    D.detect(out, vocab, points, topk=10)
    assert _native.census_stop() == {"ov3d_vocab_score": 1, "ov3d_box_points_count": 1,
                                     "ov3d_nms_boxes_from_corners": 1, "ov3d_nms3d": 1}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside the capture
        eager = [t.clone() for t in both()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = both()
    for t in got:
        t.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    assert len(got) == 8 and bool(eager[4].any()) and bool((eager[5] >= 0).any())
    for g, e in zip(got, eager):
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                           e.view(torch.int32) if e.dtype == torch.float32 else e)


# ---------------------------------------------------------------- the training vocabulary

@pytest.mark.parametrize("ap", [dict(), dict(use_3d_nms=False), dict(no_nms=True)], ids=["nms3d", "nms2d", "no_nms"])
def test_training_vocabulary_reproduces_parse_predictions(cuda, D, ap):
    """synthetic outputs under the table the probabilities were made from: detect(topk=10) gives
    the (scene, class, query) triples of the existing parse_predictions in its order, the scores
    within the bar"""
    from ov3d_amd import ap_calculator as apc
    B, Q, C, T = 2, 64, 64, 11
    c = V.chain_case(V.CHAIN_SEED)
    ref = V.score(c["visual"].reshape(B * Q, C), c["text"], T - 1, 1.0, T - 1)
    # the preconditions, on the float64 values
    ok, pairs, thr = V.separated_all(ref, C, 0.05, B, Q)
    assert ok and V.top1_clear(ref, C).all(), (pairs, thr)
    p64 = ref["e"] / ref["Z"][:, None]
    sem = torch.from_numpy(p64[:, :T - 1].reshape(B, Q, T - 1)).float().to(cuda)
    objp = torch.from_numpy((1.0 - p64[:, T - 1]).reshape(B, Q)).float().to(cuda)
    out, points = chain_inputs(cuda, c)
    conf = apc.get_ap_config_dict(dataset_config=_Cfg(T - 1), **ap)
    want = apc.parse_predictions(out["box_corners"], sem, objp, points, conf)
    got = D.detect(out, D.Vocabulary(c["text"], device=cuda), points, topk=T - 1, config=conf).to_list()
    tw, sw = triples(want, c["corners"])
    tg, sg = triples(got, c["corners"])
    assert len(tw) > 100 and tg == tw
    # the score of a (query, class): top_prob * obj, one float32 product of two values inside their bars
    bar = V.bars(ref, C, cls=np.tile(np.arange(T - 1), (B * Q, 1)), rounded_dots=True)
    rows = np.array([b * Q + q for b, _, q in tw])
    cls = np.array([k for _, k, _ in tw])
    rel = (1 + bar["prob_rel"][rows, cls]) * (1 + bar["obj_rel"][rows]) * (1 + 2 * V.U) - 1
    exact = p64[rows, cls] * ref["obj"][rows]
    floor = bar["prob_floor"] + bar["obj_floor"]
    print(f"{len(tw)} proposals, worst score error / bar {np.max(np.abs(sg - exact) / (rel * exact + floor)):.3g}")
    assert (np.abs(sg - exact) <= rel * exact + floor).all()
    # and against the existing path's own float32 scores: its two casts and its product, an ulp each
    assert (np.abs(sg - sw) <= (rel + 3 * 2 * V.U) * exact + floor).all()
    n_kept = sum(len({q for bb, _, q in tw if bb == b}) for b in range(B))
    assert 10 < n_kept < B * Q                                          # the filters removed something


# ---------------------------------------------------------------- a vocabulary swap on a real model

def test_vocabulary_swap_on_a_real_model(cuda, D):
    """see the module docstring for what is compared and why"""
    import full_fixture as F
    from ov3d_amd import ap_calculator as apc
    torch.backends.cuda.matmul.allow_tf32 = False
    name, name_eval, ds = F.EVAL_CASES[0]
    fx = F.eval_fixture(name, name_eval)
    model, cfg, _ = F.build(fx, cuda, ds, train=False)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batch = F.eval_batch(fx, cuda)
    inputs = {k: batch[k] for k in F.INPUT_KEYS}
    own_out = F.eval_forward(model, batch)["outputs"]
    visual, corners = own_out["visual_embeds"], own_out["box_corners"]
    B, Q, C = visual.shape
    assert (B, Q, C) == (2, 128, 640) and visual.dtype == torch.float32
    v64, c32 = host(visual).astype(np.float64).reshape(B * Q, C), host(corners)
    counts = host(apc.box_points_count(batch["point_clouds"][..., 0:3], corners))
    conf = apc.get_ap_config_dict()

    def check(det, vocab, k):
        """detect()'s result: the kernel's outputs against float64, then the chain, exactly"""
        T = vocab.T
        obj, lse, cls, prob = (host(o) for o in D.score_queries(visual, vocab, k))
        ref = V.score(v64, vocab.text.double().cpu().numpy(), vocab.bg, vocab.scale, k)
        check_rounded(ref, C, vocab.bg, obj.reshape(-1), lse.reshape(-1), cls.reshape(-1, k), prob.reshape(-1, k),
                      f"model embeddings T={T}")
        assert np.array_equal(host(det.obj), obj)
        mine = {"obj": obj.reshape(-1).astype(np.float64), "top_cls": cls.reshape(-1, k)}
        keep, hit = V.chain(mine, c32, counts.copy(), conf, Q)
        assert np.array_equal(host(det.keep), keep)
        want_score = np.where(hit[..., None] & (cls >= 0), prob * obj[..., None], -np.inf).astype(np.float32)
        assert np.array_equal(host(det.score), want_score)
        assert np.array_equal(host(det.cls), np.where(np.isfinite(want_score), cls, -1))
        return obj, cls, prob, hit

    # a 300-name vocabulary the model never saw
    rng = np.random.default_rng(300)
    names = [f"thing{i}" for i in range(300)] + ["no object"]
    swapped = D.Vocabulary(rng.standard_normal((301, C)) / np.sqrt(C), names=names, device=cuda)
    detector = D.Detector(model, swapped, topk=5)
    det = detector(inputs)
    assert det.cls.shape == (B, Q, 5) and det.vocab is detector.vocab
    _, _, _, hit = check(det, detector.vocab, 5)
    listed = det.to_list()
    assert [len(s) for s in listed] == (5 * hit.sum(1)).tolist() and hit.any()
    assert all(0 <= c < 300 and detector.vocab.name(c).startswith("thing") for s in listed for c, _, _ in s)
    assert all(s == sorted(s, key=lambda d: d[0]) for s in listed)
    # back to the model's own table: the existing path on the kernel's own probabilities
    own = D.Vocabulary(fx["text"], device=cuda)
    detector.topk = 10
    det = detector.set_vocabulary(own)(inputs)
    T = own.T
    obj, cls, prob, hit = check(det, own, 10)
    sem = np.zeros((B, Q, T - 1), np.float32)
    np.put_along_axis(sem, cls.astype(np.int64), prob, axis=2)
    conf_own = apc.get_ap_config_dict(dataset_config=cfg)
    want = apc.parse_predictions(corners, torch.from_numpy(sem).to(cuda), torch.from_numpy(obj).to(cuda),
                                 batch["point_clouds"], conf_own)
    tw, sw = triples(want, c32)
    tg, sg = triples(det.to_list(), c32)
    # a model has 20 classes and topk = 10 of them: the existing path's proposals of those classes
    kept = [(i, t) for i, t in enumerate(tw) if t[1] in cls[t[0], t[2]][:10].tolist()]
    assert [t for _, t in kept] == tg and len(tg) > 0
    assert np.array_equal(sw[[i for i, _ in kept]].astype(np.float32), sg.astype(np.float32))
    # the model is untouched
    after = model.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not model.training

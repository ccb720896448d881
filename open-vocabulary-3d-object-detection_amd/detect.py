"""Detect with any vocabulary: the model's per-query ``visual_embeds`` against a text table chosen
at inference time -> detections, on the device.

``Model3DETR._build_heads`` freezes the training text table into ``sem_cls_head``; every path
that makes detections (``ap_calculator.parse_predictions_device``, ``label_formatter``) reads the
``sem_cls_prob`` / ``objectness_prob`` computed from it.  Here the table is an argument.  The
kernel is csrc/vocabscore.hip behind include/ov3d_detect.h, which pins the semantics: float32 dot
products on MFMA as ``open_vocab`` forms them, a softmax streamed over the vocabulary in tiles
(the (R, T) scores never reach memory), ``obj = F / Z`` (1 - p_background without the
cancellation), the top-k foreground classes with the smaller index first among equal scores, and
a row with a non-finite score can never become a detection.  The reference has no such code: its
``compute_objectness_and_cls_prob`` asserts the training class count.

  Vocabulary     the prepared (T, C) table (``open_vocab.prepare_text``), its names, its "no
                 object" row and its temperature
  score_queries  (..., C) embeddings -> obj, lse, top_cls, top_prob; one launch and nothing else
  detect         the model's ``outputs["outputs"]`` -> Detections: ``parse_predictions_device``
                 step for step (empty-box filter, NMS, confidence threshold, per-class proposals
                 cut to k) with the new quantities in place of the old
  Detections     device tensors; ``to_list()`` is the one read-back
  Detector       a model and a vocabulary; ``set_vocabulary`` swaps the table, not the model

The scores have their plain meaning: query q against text row t.  A checkpoint trained under
``cls_logits_layout="reference"`` carries the reference's scrambled (query, class) layout
 in its weights; nothing is done about that here.

Nothing synchronises before ``to_list()``; everything up to it is legal inside a hipGraph
capture.
"""
import numpy as np
import torch

from . import _native as nat
from . import nms as _nms
from .ap_calculator import box_points_count, get_ap_config_dict
from .open_vocab import prepare_text

MAX_T, MAX_C, MAX_K = 4096, 4096, 16     # OV3D_DETECT_MAX_T, _MAX_C, _MAX_K
TILE_T = 256                             # OV3D_DETECT_TILE_T: text rows per vocabulary tile
DTYPES = {torch.float32: 0, torch.bfloat16: 1}   # OV3D_OPENVOCAB_F32, _BF16


class Vocabulary:
    """text (T, C) embeddings (numpy or torch), one row per name -> the table the kernel reads.

    background: the "no object" row as a Python index (default -1, the last row, where the
    reference's layout puts it); None: the table has no such row and every query's objectness
    is 1.  normalize=False and scale=1.0 reproduce the model's own scoring (raw text rows, no
    temperature); normalize=True divides every row by its L2 norm in float64 first, scale
    multiplies every score.  Refuses non-finite text, T or C outside the kernel's limits and
    names of the wrong length."""

    def __init__(self, text, names=None, background=-1, dtype=torch.float32, normalize=False, scale=1.0,
                 device=None):
        if dtype not in DTYPES:
            raise TypeError(f"dtype: expected float32 or bfloat16, got {dtype}")
        if isinstance(text, torch.Tensor):
            device = text.device if device is None else device
            text = text.detach().to(device="cpu", dtype=torch.float64).numpy()
        x = np.array(text, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError(f"text: expected (T, C), got {x.shape}")
        T, C = x.shape
        if not 1 <= T <= MAX_T or not 1 <= C <= MAX_C:
            raise ValueError(f"expected 1 <= T <= {MAX_T} and 1 <= C <= {MAX_C}, got T = {T}, C = {C}")
        if not np.isfinite(x).all():
            raise ValueError("text: non-finite embeddings")
        if names is not None:
            names = [str(n) for n in names]
            if len(names) != T:
                raise ValueError(f"names: expected {T}, one per text row, got {len(names)}")
        if background is None:
            bg = -1
        else:
            bg = int(background)
            if not -T <= bg < T:
                raise ValueError(f"background: row {background} of a table of {T}")
            bg %= T
        scale = float(scale)
        if not np.isfinite(scale):
            raise ValueError("scale: a finite factor expected")
        self.text = prepare_text(x, dtype, normalize=normalize, device=device)
        if not bool(torch.isfinite(self.text.float()).all()):
            raise ValueError(f"text: not finite in {dtype}")
        self.names, self.bg, self.scale, self.T, self.C = names, bg, scale, T, C

    def to(self, device):
        """the same vocabulary with its table on `device`"""
        if self.text.device == torch.device(device):
            return self
        other = object.__new__(Vocabulary)
        other.__dict__.update(self.__dict__)
        other.text = self.text.to(device)
        return other

    def name(self, cls):
        """the name of text row cls (its number where the vocabulary has no names)"""
        return str(int(cls)) if self.names is None else self.names[int(cls)]


def _rows(v, C):
    """(..., C) tensor -> (R, row pitch in elements) of the rows where they are, without a copy"""
    if v.stride(-1) != 1 and C > 1:
        raise ValueError("visual_embeds: the channels must be adjacent in memory")
    lead, strides = list(v.shape[:-1]), list(v.stride()[:-1])
    R = int(np.prod(lead)) if lead else 1
    dims = [(n, s) for n, s in zip(lead, strides) if n > 1]
    for (_, s0), (n1, s1) in zip(dims, dims[1:]):
        if s0 != s1 * n1:
            raise ValueError(f"visual_embeds: rows of shape {tuple(v.shape)} and strides {v.stride()} are not "
                             "evenly spaced; pass a contiguous tensor")
    ld = dims[-1][1] if dims else C
    if ld < C:
        raise ValueError(f"visual_embeds: rows {ld} elements apart overlap")
    return R, ld


def _check_queries(v, vocab, topk):
    """the host refusals of score_queries -> (R, ld); nothing is launched"""
    if not isinstance(vocab, Vocabulary):
        raise TypeError("vocab: a Vocabulary expected")
    if not isinstance(v, torch.Tensor):
        raise TypeError("visual_embeds: expected a tensor")
    if v.dtype not in DTYPES:
        raise TypeError(f"visual_embeds: expected float32 or bfloat16, got {v.dtype}")
    if v.dtype != vocab.text.dtype:
        raise TypeError(f"visual_embeds are {v.dtype}, the vocabulary {vocab.text.dtype}: build the "
                        "Vocabulary with dtype= the embeddings' type")
    if v.dim() < 1 or v.shape[-1] != vocab.C:
        raise ValueError(f"visual_embeds {tuple(v.shape)}: the vocabulary has {vocab.C} channels")
    topk = int(topk)
    if not 1 <= topk <= MAX_K:
        raise ValueError(f"topk: expected 1 <= k <= {MAX_K}, got k = {topk}")
    R, ld = _rows(v, vocab.C)
    if not 1 <= R < 2 ** 31:
        raise ValueError(f"expected 1 <= rows < 2^31, got {R}")
    nat.check_device(v, "visual_embeds")
    if vocab.text.device != v.device:
        raise ValueError(f"the vocabulary is on {vocab.text.device}, visual_embeds on {v.device}")
    return R, ld


@torch.no_grad()
def score_queries(visual_embeds, vocab, topk=5):
    """visual_embeds (..., C) float32 / bfloat16 on the device (a strided view of evenly spaced
    rows, such as the last layer of the stacked head outputs, is read where it is), vocab a
    Vocabulary of the same dtype and device -> (obj (...) f32, lse (...) f32, top_cls (..., k)
    int32, top_prob (..., k) f32) as include/ov3d_detect.h defines them: class indices are rows
    of the vocabulary's table, -1 and probability 0 beyond the foreground count or where a score
    is not finite.  One launch and nothing else."""
    R, ld = _check_queries(visual_embeds, vocab, topk)
    v, k = visual_embeds.detach(), int(topk)
    lead, dev = tuple(v.shape[:-1]), v.device
    obj = torch.empty(lead, dtype=torch.float32, device=dev)
    lse = torch.empty(lead, dtype=torch.float32, device=dev)
    top_cls = torch.empty(lead + (k,), dtype=torch.int32, device=dev)
    top_prob = torch.empty(lead + (k,), dtype=torch.float32, device=dev)
    nat.call("ov3d_vocab_score", v, DTYPES[v.dtype], R, vocab.C, ld, vocab.text, vocab.T, vocab.bg,
             vocab.scale, k, obj, lse, top_cls, top_prob, like=v)
    return obj, lse, top_cls, top_prob


class Detections:
    """detect()'s result, all on the device: keep (B, Q) bool, the queries left by the empty-box
    filter and the NMS; cls (B, Q, k) int32, the vocabulary rows a query is a detection of, -1
    where none; score (B, Q, k) f32, -inf where none; obj (B, Q) f32; corners (B, Q, 8, 3)."""

    def __init__(self, keep, cls, score, obj, corners, vocab):
        self.keep, self.cls, self.score, self.obj, self.corners, self.vocab = keep, cls, score, obj, corners, vocab

    def to_list(self):
        """per scene the list of (class, corners (8, 3), score), classes outer and boxes inner
        as parse_predictions orders its per-class proposals.  The one read-back (synchronises)."""
        B, Q, k = self.cls.shape
        packed = torch.cat([self.cls.double(), self.score.double(), self.corners.reshape(B, Q, 24).double()],
                           -1).cpu().numpy()
        cls, score = packed[..., :k].astype(np.int64), packed[..., k:2 * k].astype(np.float32)
        corners = packed[..., 2 * k:].astype(np.float32).reshape(B, Q, 8, 3)
        out = []
        for i in range(B):
            j, s = np.nonzero(np.isfinite(score[i]) & (cls[i] >= 0))
            order = np.lexsort((j, cls[i][j, s]))
            out.append([(int(cls[i, a, b]), corners[i, a], score[i, a, b]) for a, b in zip(j[order], s[order])])
        return out


@torch.no_grad()
def detect(outputs, vocab, point_cloud=None, topk=5, config=None):
    """outputs: the model's ``outputs["outputs"]`` dict (``visual_embeds`` (B, Q, C) and
    ``box_corners`` (B, Q, 8, 3) are read, its own ``sem_cls_prob`` / ``objectness_prob`` are
    not); config: a ``get_ap_config_dict(...)`` dict, by default one whose remove_empty_box
    follows whether a point cloud (B, N, >= 3) was given -> Detections.

    ``parse_predictions_device`` step for step: the empty-box filter (``box_points_count``, the
    most objectlike box kept where all are empty), the NMS table from the corners, obj and the
    top-1 class (``nms_boxes_from_corners``, ``nms3d_batched``; the bird's-eye table without
    use_3d_nms), a query is a detection iff it is kept and obj > conf_thresh, and a detection
    contributes its top-k classes with score top_prob * obj: the per-class proposals, cut to k
    (a config without per_class_proposal is refused).  The scores have their plain
    meaning, query against text row; the reference-layout quirk of a checkpoint's weights (Q8) is
    not undone.  One ov3d_vocab_score launch plus the existing ones; nothing synchronises."""
    visual, corners = outputs["visual_embeds"], outputs["box_corners"]
    cfg = get_ap_config_dict(remove_empty_box=point_cloud is not None) if config is None else config
    if not isinstance(corners, torch.Tensor) or corners.dim() != 4 or tuple(corners.shape[2:]) != (8, 3):
        raise ValueError("box_corners: expected a (B, Q, 8, 3) tensor")
    B, Q = corners.shape[:2]
    if isinstance(visual, torch.Tensor) and tuple(visual.shape[:-1]) != (B, Q):
        raise ValueError(f"visual_embeds {tuple(visual.shape)} against box_corners {tuple(corners.shape)}")
    if cfg["remove_empty_box"] and point_cloud is None:
        raise ValueError("remove_empty_box needs the point cloud")
    if not cfg["per_class_proposal"] or cfg["use_cls_confidence_only"]:
        raise ValueError("detect makes per-class proposals scored top_prob * obj: per_class_proposal=True, "
                         "use_cls_confidence_only=False")
    if not cfg.get("no_nms", False) and Q > _nms.MAX_K:
        raise ValueError(f"nms3d supports K <= {_nms.MAX_K} boxes per scene")
    _check_queries(visual, vocab, topk)
    obj, _, top_cls, top_prob = score_queries(visual, vocab, topk)
    corners = corners.detach().float().contiguous()
    dev = corners.device
    pred_cls = top_cls[..., 0]
    if cfg["remove_empty_box"]:
        nonempty = box_points_count(point_cloud[..., 0:3], corners) >= 5
        none = ~nonempty.any(1)                     # all empty -> keep the most objectlike
        first = torch.arange(Q, device=dev) == torch.argmax(obj, 1, keepdim=True)
        nonempty = nonempty | (none[:, None] & first)
    else:
        nonempty = torch.ones((B, Q), dtype=torch.bool, device=dev)
    if cfg.get("no_nms", False):
        keep = nonempty
    elif not cfg["use_3d_nms"]:
        c64 = corners.double()
        lo, hi = c64.amin(2), c64.amax(2)
        table = torch.stack([lo[..., 0], lo[..., 2], hi[..., 0], hi[..., 2], obj.double()], -1)
        keep = _nms.nms3d_batched(_nms.boxes2d_as_3d(table), cfg["nms_iou"], cfg["use_old_type_nms"],
                                  samecls=False, valid=nonempty).bool()
    else:
        boxes = _nms.nms_boxes_from_corners(corners, obj, pred_cls if cfg["cls_nms"] else None)
        keep = _nms.nms3d_batched(boxes, cfg["nms_iou"], cfg["use_old_type_nms"], samecls=cfg["cls_nms"],
                                  valid=nonempty).bool()
    det = keep & (obj > cfg["conf_thresh"])
    mine = det[..., None] & (top_cls >= 0)
    val = top_prob * obj[..., None]
    score = torch.where(mine, val, torch.full_like(val, -float("inf")))
    cls = torch.where(mine, top_cls, torch.full_like(top_cls, -1))
    return Detections(keep, cls, score, obj, corners, vocab)


class Detector:
    """a model and a vocabulary: ``detector(inputs)`` runs the eval-mode forward under no_grad
    and detect() on its outputs, with ``inputs["point_clouds"]`` as the point cloud of the
    empty-box filter.  ``set_vocabulary`` swaps the table; the model is never touched."""

    def __init__(self, model, vocab, topk=5, config=None):
        self.model, self.topk, self.config = model, topk, config
        self.set_vocabulary(vocab)

    def set_vocabulary(self, vocab):
        if not isinstance(vocab, Vocabulary):
            raise TypeError("vocab: a Vocabulary expected")
        param = next(self.model.parameters(), None)
        self.vocab = vocab if param is None else vocab.to(param.device)
        return self

    @torch.no_grad()
    def __call__(self, inputs):
        was_training = self.model.training
        self.model.eval()
        try:
            out = self.model(inputs)["outputs"]
        finally:
            self.model.train(was_training)
        wants_points = self.config is None or self.config["remove_empty_box"]
        return detect(out, self.vocab, inputs["point_clouds"] if wants_points else None, self.topk, self.config)

"""Open-vocabulary labels on the device: feature vectors against the text embeddings of a
vocabulary -> one class index per scan vertex or per frame pixel.

This is the step the reference leaves open: its loader carries ``# TODO: acquire semantic labels
using LSeg / OpenSeg + projection`` (``datasets/scannet.py:272``) and its tools read the
``<scan>.npy`` ``[x, y, z, label]`` files and the per-frame label dicts from directories filled
outside the code base.  The kernel is csrc/openvocab.hip behind include/ov3d_openvocab.h, which
pins the semantics: float32 dot products on MFMA (float32 features are not rounded), the
smallest index among the largest, NaN never wins, and a row of zeros (what
``projection.compose_features`` writes for a vertex no frame keeps) is ``unseen``.

  prepare_text               (T, C) embeddings -> L2-normalised in float64, rounded once
  classify_rows              (R, C) rows, the layout of compose_features(rows=True); one launch
  classify_frames            (F, C, H, W) channel-first maps -> (F, H, W); one launch
  vertex_labels_from_frames  classify the frames, then back-project the label map as a
                             one-channel feature: three launches, no (N, C) feature array
  save_vertex_labels         the (N, 4) file ``label_formatter`` and the ScanNet lifter load
  save_frame_labels          the per-frame dict ``assess_pseudo_label.py`` loads
  load_frame_labels          that script's two loading lines -> the array ``label_assess`` takes

Nothing here synchronises before the writers; everything up to them is legal inside a hipGraph
capture.  Producing the image features themselves (LSeg, CLIP) is out of scope.
"""
import numpy as np
import torch

from . import _native as nat
from .projection import compose_features

MAX_T, MAX_C = 256, 4096                 # OV3D_OPENVOCAB_MAX_T, _MAX_C
DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}   # OV3D_OPENVOCAB_F32, _BF16, _F16


def _round_to_odd_f32(x):
    """float64 -> float32 rounded to odd: a following round-to-nearest to a narrower type then
    equals one rounding of the float64 value"""
    f = x.astype(np.float32)
    back = f.astype(np.float64)
    inexact = np.isfinite(back) & (back != x)
    toward_zero = np.where(np.abs(back) > np.abs(x), np.nextafter(f, np.float32(0)), f).astype(np.float32)
    bits = toward_zero.view(np.uint32) | np.uint32(1)
    return np.where(inexact, bits.view(np.float32), f).astype(np.float32)


def prepare_text(text, dtype=torch.float32, normalize=True, device=None):
    """(T, C) text embeddings (numpy or torch) -> tensor of `dtype`: every row divided by its
    L2 norm in float64 (a zero row stays zero), then rounded once to `dtype`.  normalize=False:
    the cast alone.  device: where the result goes (default: the input's device, the host for
    numpy)."""
    if dtype not in DTYPES:
        raise TypeError(f"dtype: expected float32, bfloat16 or float16, got {dtype}")
    if isinstance(text, torch.Tensor):
        device = text.device if device is None else device
        text = text.detach().to(device="cpu", dtype=torch.float64).numpy()
    x = np.array(text, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f"text: expected (T, C), got {x.shape}")
    if normalize:
        n = np.sqrt((x * x).sum(axis=1, keepdims=True))
        x = np.divide(x, n, out=np.zeros_like(x), where=n > 0)
    if dtype == torch.float32:
        out = torch.from_numpy(x.astype(np.float32))
    elif dtype == torch.float16:
        with np.errstate(over="ignore"):
            out = torch.from_numpy(x.astype(np.float16))
    else:
        out = torch.from_numpy(_round_to_odd_f32(x)).to(torch.bfloat16)
    return out if device is None else out.to(device)


def _check(features, text, ndim, unseen, min_sim):
    """the host refusals shared by both layouts -> (T, C, unseen); nothing is launched"""
    if not isinstance(features, torch.Tensor) or not isinstance(text, torch.Tensor):
        raise TypeError("features, text: expected tensors")
    if features.dtype not in DTYPES:
        raise TypeError(f"features: expected float32, bfloat16 or float16, got {features.dtype}")
    if text.dtype != features.dtype:
        raise TypeError(f"text: expected the features' {features.dtype}, got {text.dtype} (see prepare_text)")
    if features.dim() != ndim or text.dim() != 2:
        raise ValueError(f"expected {ndim}-d features and (T, C) text, got {tuple(features.shape)} and "
                         f"{tuple(text.shape)}")
    T, C = text.shape
    if features.shape[1] != C:
        raise ValueError(f"features have {features.shape[1]} channels, the text {C}")
    if not 1 <= T <= MAX_T or not 1 <= C <= MAX_C:
        raise ValueError(f"expected 1 <= T <= {MAX_T} and 1 <= C <= {MAX_C}, got T = {T}, C = {C}")
    rows = features.numel() // C
    if not 1 <= rows < 2 ** 31:
        raise ValueError(f"expected 1 <= rows < 2^31, got {rows}")
    if text.device != features.device:
        raise ValueError(f"text is on {text.device}, the features on {features.device}")
    unseen = T if unseen is None else int(unseen)
    if not -2 ** 31 <= unseen < 2 ** 31:
        raise ValueError("unseen: an int32 expected")
    if min_sim is not None and not np.isfinite(float(min_sim)):
        raise ValueError("min_sim: a finite cosine expected")
    nat.check(features, "features")
    nat.check(text, "text")
    return T, C, unseen


def _classify(features, text, planes, R, C, P, T, unseen, min_sim):
    dev = features.device
    label = torch.empty(R, dtype=torch.int32, device=dev)
    score = torch.empty(R, dtype=torch.float32, device=dev)
    norm = torch.empty(R, dtype=torch.float32, device=dev)
    nat.call("ov3d_openvocab_classify", features, DTYPES[features.dtype], planes, R, C, P, text, T, unseen,
             label, score, norm, like=features)
    if min_sim is not None:
        label.masked_fill_(score < float(min_sim) * norm, unseen)
    return label, score, norm


@torch.no_grad()
def classify_rows(features, text, unseen=None, min_sim=None):
    """features (R, C) float32 / bfloat16 / float16 on the device, text (T, C) of the same dtype
    and device -> (label (R) int32, score (R) float32, norm (R) float32): the smallest index of
    the largest dot product, that dot product, and the row's L2 norm.  A row of zeros and a row
    without a winner (every product NaN) take label = unseen (default T) and score 0; with
    min_sim so does every row whose cosine score / norm lies below it (the label alone changes;
    torch ops on the device, no read-back).  One launch."""
    T, C, unseen = _check(features, text, 2, unseen, min_sim)
    return _classify(features, text, 0, features.shape[0], C, 0, T, unseen, min_sim)


@torch.no_grad()
def classify_frames(features, text, unseen=None, min_sim=None):
    """features (F, C, H, W), the channel-first maps the back-projection reads -> (label, score,
    norm), each (F, H, W); otherwise as classify_rows, to which it is bit-equal pixel by pixel.
    One launch, no transposed copy."""
    T, C, unseen = _check(features, text, 4, unseen, min_sim)
    F, _, H, W = features.shape
    out = _classify(features, text, 1, F * H * W, C, H * W, T, unseen, min_sim)
    return tuple(t.view(F, H, W) for t in out)


@torch.no_grad()
def vertex_labels_from_frames(points, depths, poses, features, text, unseen=None, min_sim=None,
                              projector=None):
    """points (N, 3), depths (F, H, W), poses (F, 4, 4) as compose_features takes them, features
    (F, C, H, W) and text (T, C) as classify_frames does -> (label (N) int32, frame (N) int32):
    every vertex takes the label of the pixel it lands on in the last frame that keeps it, and
    unseen (frame -1) where no frame does.  Equal to classify_rows over
    compose_features(..., rows=True) without forming the (N, C) features: the label map goes
    through ov3d_backproj_compose as a one-channel float32 feature.  Three launches."""
    label_map = classify_frames(features, text, unseen, min_sim)[0]
    unseen = text.shape[0] if unseen is None else int(unseen)
    lifted, frame = compose_features(points, depths, poses, label_map.to(torch.float32).unsqueeze(1),
                                     rows=True, projector=projector)
    label = lifted[:, 0].to(torch.int32).masked_fill_(frame < 0, unseen)
    return label, frame


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def save_vertex_labels(path, xyz, label):
    """the ``<scan>.npy`` file LabelFormatter and ScannetBoxLifter load: (N, 4) rows
    [x, y, z, label], float64 where xyz is float64 and float32 otherwise.  Reads the tensors
    back (synchronises)."""
    xyz, label = _host(xyz), _host(label)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or label.shape != (xyz.shape[0],):
        raise ValueError(f"expected xyz (N, 3) and label (N), got {xyz.shape} and {label.shape}")
    if label.dtype.kind not in "iu":
        raise TypeError(f"label: integers expected, got {label.dtype}")
    dt = np.float64 if xyz.dtype == np.float64 else np.float32
    out = np.empty((xyz.shape[0], 4), dtype=dt)
    out[:, :3] = xyz
    out[:, 3] = label
    np.save(path, out)
    return out


def save_frame_labels(path, frame_ids, maps):
    """the per-scan file ``assess_pseudo_label.py`` loads: a dict {int(frame id): (H, W) int16
    class map} saved with numpy (a pickled 0-d object array, which that script opens with
    ``allow_pickle=True``).  maps (F, H, W) integers, one per frame id.  Reads back."""
    maps = _host(maps)
    ids = [int(i) for i in frame_ids]
    if maps.ndim != 3 or maps.shape[0] != len(ids) or len(set(ids)) != len(ids):
        raise ValueError(f"expected (F, H, W) maps and F distinct frame ids, got {maps.shape} and {len(ids)} ids")
    if maps.dtype.kind not in "iu" or maps.size and (maps.min() < -2 ** 15 or maps.max() >= 2 ** 15):
        raise TypeError("maps: integers within int16 expected")
    np.save(path, {i: np.ascontiguousarray(m, dtype=np.int16) for i, m in zip(ids, maps)})


def load_frame_labels(path, frame_ids):
    """``assess_pseudo_label.py:32-33``: the dict written by save_frame_labels -> (F, H, W)
    int64, the pseudo_frames argument of label_assess.match / frame_confusion / assess"""
    x = np.load(path, allow_pickle=True)
    return np.stack([x.item()[int(i)].astype(np.int64) for i in frame_ids])

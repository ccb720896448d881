"""Cases of tests/golden/pseudo_label.npz (shared by make_pseudo_label_golden.py and the tests):
per-vertex-labelled scans and the model outputs of every step, regenerated bit-identically from
numpy PCG64 seeds (integers and random() only).

Construction: one spatial blob per class (centres 3/4 apart, half extent 1/2, so neighbouring
blobs overlap), vertex coordinates on a 1/64 grid, about a tenth of the labels replaced by
ignored values (18, 23, -100).  A query's box is centred on the blob of its own class (about 70 %)
or on a neighbouring class's blob; centres and sizes lie on a 1/32 grid, so that box faces pass
exactly through vertices.  On top come the hand-made queries of `_specials` in a far-away empty
region of the scan."""
import numpy as np

NUM_CLASSES = 18
Q = 16
F32 = np.float32

# case: seed, (vertices, dtype) per scan, the scans of every step (B = 2), thresholds
CASES = {
    "mixed": dict(seed=101,
                  scans=[(1000, np.float32), (63, np.float64), (257, np.float32), (1, np.float64),
                         (1000, np.float64), (257, np.float32)],
                  steps=[(0, 1), (2, 3), (4, 0)],      # the last step repeats scan 0; 5: no boxes
                  th_s=0.9, th_o=0.5),
    "small": dict(seed=202, scans=[(1000, np.float32), (257, np.float64)], steps=[(0, 1), (1, 0)],
                  th_s=0.9, th_o=0.3),
}


def scan_name(i):
    return "scene%04d_00" % i


def blob(c):
    return np.array([(c % 6) * 0.75, (c // 6) * 0.75, 0.5])


def _scan(rng, n, dtype, classes):
    cls = classes[rng.integers(0, len(classes), n)]
    off = rng.integers(-32, 33, (n, 3)) / 64.0
    xyz = np.stack([blob(c) for c in cls]) + off
    lab = cls.astype(np.float64)
    swap = rng.random(n) < 0.1
    lab[swap] = np.array([18.0, 23.0, -100.0])[rng.integers(0, 3, n)][swap]
    return np.concatenate([xyz, lab[:, None]], 1).astype(dtype)


def _specials(raw, f64):
    """hand-made vertices (overwriting the scan's last rows) and queries, 10 and more units away
    from the blobs: -> [(centre, size, class row of sem_cls_prob)]"""
    rows, queries = [], []

    def row(cls, other=None):
        p = np.zeros(NUM_CLASSES, F32)
        p[cls] = F32(0.95)
        if other is not None:
            p[other] = F32(0.95)
        return p

    def verts(cx, labels):
        for j, l in enumerate(labels):
            rows.append([cx + (j - 1) / 64.0, j / 64.0, 0.0, l])
    # a tie between the box's class and a smaller label: the mode is the smaller, dropped
    verts(10.0, [3, 3, 7, 7])
    queries.append(([10.0, 0.0, 0.0], [0.5, 0.5, 0.5], row(7)))
    # a tie between the box's class and a larger label: kept
    verts(12.0, [3, 3, 7, 7])
    queries.append(([12.0, 0.0, 0.0], [0.5, 0.5, 0.5], row(3)))
    # a zero-size box on the grid plane z = 0: its vertices are inside (closed intervals)
    verts(14.0, [4, 4, 18])
    queries.append(([14.0, 0.0, 0.0], [0.5, 0.5, 0.0], row(4)))
    # two equal maxima: the first index (5) is the label, and the blob there is 5
    verts(18.0, [5, 5, 11])
    queries.append(([18.0, 0.0, 0.0], [0.25, 0.25, 0.25], row(5, 11)))
    if f64:
        # a vertex at lo - 2^-40: outside in double, on the face once rounded to float32, where
        # it would tie the vote 9 : 2 and the smaller label would win
        rows.append([16.0, 0.0, 0.0, 9])
        rows.append([15.75 - 2.0 ** -40, 0.0, 0.0, 2])
        queries.append(([16.0, 0.0, 0.0], [0.5, 0.5, 0.5], row(9)))
    raw[len(raw) - len(rows):] = np.array(rows, raw.dtype)
    assert not f64 or raw[-1, 0] != 15.75
    return queries


def make(name):
    """-> (scans: list of (n, 4) arrays, steps: list of (outputs dict, scan_idx) numpy)"""
    cs = CASES[name]
    rng = np.random.Generator(np.random.PCG64(cs["seed"]))
    scans, classes, special = [], [], {}
    for i, (n, dt) in enumerate(cs["scans"]):
        cl = np.sort(rng.permutation(NUM_CLASSES)[:6 if n >= 257 else 2])   # few vertices: few blobs
        raw = _scan(rng, n, dt, cl)
        if n >= 1000:
            special[i] = _specials(raw, dt == np.float64)
        classes.append(cl)
        scans.append(raw)
    scores = np.array([0.97, 0.93, F32(0.9), 0.85, 0.5], F32)
    objs = np.array([0.99, 0.8, 0.5, 0.2], F32)
    steps = []
    for scan_idx in cs["steps"]:
        B = len(scan_idx)
        prob = (rng.random((B, Q, NUM_CLASSES)) * 0.04).astype(F32)
        obj = objs[rng.integers(0, len(objs), (B, Q))]
        ctr = np.zeros((B, Q, 3), F32)
        size = np.zeros((B, Q, 3), F32)
        for b, s in enumerate(scan_idx):
            cl = classes[s]
            for q in range(Q):
                c = cl[rng.integers(0, len(cl))]
                at = c if rng.random() < 0.7 else cl[(list(cl).index(c) + 1) % len(cl)]
                if cs["scans"][s][0] == 1:
                    # the one-vertex scan: boxes on its vertex, all of another class
                    at, c = int(scans[s][0, 3]) % NUM_CLASSES, (int(scans[s][0, 3]) + 1) % NUM_CLASSES
                    ctr[b, q] = scans[s][0, :3] + rng.integers(-2, 3, 3) / 32.0
                else:
                    ctr[b, q] = blob(at) + rng.integers(-8, 9, 3) / 32.0
                size[b, q] = rng.integers(1, 17, 3) / 32.0
                prob[b, q, c] = scores[rng.integers(0, len(scores))]
            for q, (c0, s0, row) in enumerate(special.get(s, [])):
                ctr[b, q], size[b, q], prob[b, q], obj[b, q] = c0, s0, row, F32(0.99)
        steps.append(({"sem_cls_prob": prob, "objectness_prob": obj, "center_unnormalized": ctr,
                       "size_unnormalized": size}, np.array(scan_idx, np.int64)))
    return scans, steps

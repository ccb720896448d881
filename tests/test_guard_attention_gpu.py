"""Guard-band cases of the attention kernels (csrc/attn.hip; key tiles of 64, query blocks of
128 forward / 64 for dK, dV; Lq % 32 == 0) at the smallest ragged key counts, every operand
between guard bands (tests/guard.py).  q, k and v are column ranges of wider rows (strides
larger than H * 64, a non-zero column offset); dq, dk and dv are column ranges of banded
buffers whose other columns must keep their sentinel.  Values: the fp32 softmax with the
boolean mask and the keep mask rebuilt from the documented hash, test_attention_gpu.py's
reference and bars (relative Frobenius error 1e-2 forward, 2e-2 gradients)."""
import ctypes

import numpy as np
import pytest
import torch

import guard
from guard import In, Out
from helpers import ov3d  # noqa: F401
from test_attention_gpu import _drop_key, _ref_masked, _rel, keep_mask

pytestmark = pytest.mark.gpu

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
ENTRIES = ("ov3d_attn_fwd", "ov3d_attn_bwd", "ov3d_attn_fwd_masked", "ov3d_attn_bwd_masked",
           "ov3d_attn_bwd_dkdv_batch", "ov3d_attn_dropgen", "ov3d_attn_fwd_pregen",
           "ov3d_attn_mask_pack")

B, H = 2, 2
E = H * 64
PAD = 8                        # column offset of q / k / dq / dk in their wider rows
SQ, SKV = E + 2 * PAD, 2 * E + 2 * PAD
SO = E + PAD
SCALE = 0.125
SEED, SITE = 20241, 11


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 15485863 * int(k) for i, k in enumerate(key)) % (1 << 31))
    return g


def _seed():
    return In(torch.tensor([SEED], dtype=torch.int64), index=(3, 5))


def _scratch(n):
    return Out((n,), F32, full=False, compare=False, finite=False)


def _lib():
    from ov3d_amd import _native
    return _native.load()


def _pack(cuda, am):
    """(nb, Lq, Lk) bool -> packed words (int32, on the host) by a plain call"""
    nb, Lq, Lk = am.shape
    src = am.to(cuda).to(torch.uint8).contiguous()
    words = torch.empty(_lib().ov3d_attn_maskbits_words(nb, Lq, Lk), dtype=I32, device=cuda)
    guard.call("ov3d_attn_mask_pack", src, 0, 0.0, nb, Lq, Lk, words, like=src)
    return words.cpu()


def _cols(rows, width, lo, hi):
    m = torch.zeros(rows, width, dtype=torch.bool)
    m[:, lo:hi] = True
    return m


class Problem:
    """one attention problem: data on the host, the fp32 reference computed once"""

    def __init__(self, cuda, Lq, Lk, masked, p, key=0, nb=B):
        g = _gen(Lq, Lk, masked, int(p * 10), key, nb)
        self.cuda, self.Lq, self.Lk, self.p, self.nb = cuda, Lq, Lk, p, nb
        self.qs = (torch.randn(Lq, nb, SQ, generator=g) * 1.5).to(BF)
        self.kvs = torch.randn(Lk, nb, SKV, generator=g)
        self.kvs[..., :PAD + E] *= 1.5
        self.kvs = self.kvs.to(BF)
        self.dout = torch.randn(Lq * nb, E, generator=g).to(BF)
        self.am = None
        if masked:
            self.am = torch.rand(nb, Lq, Lk, generator=g) < 0.7
            self.am[:, :, 0] = False                    # every query attends to something
        self.words = _pack(cuda, self.am) if masked else None
        self.nbits = _lib().ov3d_attn_dropbits_words(nb, H, Lq, Lk) if p > 0 else 0
        assert p == 0 or self.nbits == 4 * ((Lk + 63) // 64) * nb * H * Lq

    def reference(self):
        cuda = self.cuda
        q = self.qs[..., PAD:PAD + E].to(cuda).float().requires_grad_()
        k = self.kvs[..., PAD:PAD + E].to(cuda).float().requires_grad_()
        v = self.kvs[..., PAD + E:PAD + 2 * E].to(cuda).float().requires_grad_()
        am = self.am.to(cuda) if self.am is not None else torch.zeros(
            self.nb, self.Lq, self.Lk, dtype=torch.bool, device=cuda)
        keep = keep_mask(SEED, SITE, self.nb, H, self.Lq, self.Lk, self.p, cuda) if self.p > 0 else None
        ref = _ref_masked(q, k, v, H, am, self.p, keep)
        ref.backward(self.dout.to(cuda).float().view(self.Lq, self.nb, E))
        return ref.detach().reshape(-1, E), q.grad.reshape(-1, E), k.grad.reshape(-1, E), \
            v.grad.reshape(-1, E)

    def qkv(self, t):
        return (t["qs"][..., PAD:PAD + E], t["kvs"][..., PAD:PAD + E], t["kvs"][..., PAD + E:PAD + 2 * E])

    def forward(self, nsplit=1, entry=None, bits=None):
        """the guarded forward -> its outputs (o, lse, bits)"""
        Lq, Lk, p, nb = self.Lq, self.Lk, self.p, self.nb
        nws = _lib().ov3d_attn_fwd_workspace(nb, H, Lq, Lk, nsplit)
        assert (nws > 0) == (nsplit > 1)
        if entry is None:
            entry = "ov3d_attn_fwd" if self.words is None and p == 0 else "ov3d_attn_fwd_masked"
        specs = {"qs": In(self.qs), "kvs": In(self.kvs), "seed": _seed() if p > 0 else None,
                 "mask": In(self.words) if self.words is not None else None,
                 "o": Out((Lq * nb, E), BF, ld=SO), "lse": Out((nb * H, Lq), F32),
                 "bits": (Out((self.nbits,), I32, init=bits, full=bits is None) if p > 0 else None),
                 "ws": _scratch(nws) if nws else None}

        def call(t):
            q, k, v = self.qkv(t)
            args = [q, k, v, SQ, SKV, SKV, nb, H, Lq, Lk, SCALE, float(p), t["seed"], SITE, t["o"], SO,
                    t["lse"], t["bits"], t["ws"], nsplit]
            if entry != "ov3d_attn_fwd":
                args.append(t["mask"])
            guard.call(entry, *args, like=q)
        return guard.run_case(self.cuda, specs, call)

    def backward(self, fwd, nsplit=1, kv=True):
        """the guarded backward from the forward's outputs -> dq, dkv (dk | dv columns), dvec"""
        Lq, Lk, p, nb = self.Lq, self.Lk, self.p, self.nb
        nws = _lib().ov3d_attn_fwd_workspace(nb, H, Lq, Lk, nsplit)
        entry = "ov3d_attn_bwd" if self.words is None and p == 0 else "ov3d_attn_bwd_masked"
        specs = {"qs": In(self.qs), "kvs": In(self.kvs), "o": In(fwd["o"].cpu(), ld=SO),
                 "dout": In(self.dout, ld=SO), "lse": In(fwd["lse"].cpu()),
                 "bits": In(fwd["bits"].cpu()) if p > 0 else None,
                 "mask": In(self.words) if self.words is not None else None,
                 "dvec": Out((nb * H, Lq), F32, full=False),
                 "dq": Out((Lq * nb, SQ), BF, full=_cols(Lq * nb, SQ, PAD, PAD + E)),
                 "dkv": Out((Lk * nb, SKV), BF, full=_cols(Lk * nb, SKV, PAD, PAD + 2 * E)) if kv else None,
                 "ws": _scratch(nws) if nws else None}

        def call(t):
            q, k, v = self.qkv(t)
            dk = t["dkv"][:, PAD:PAD + E] if kv else None
            dv = t["dkv"][:, PAD + E:PAD + 2 * E] if kv else None
            args = [q, k, v, SQ, SKV, SKV, t["o"], SO, t["dout"], SO, t["lse"], nb, H, Lq, Lk, SCALE,
                    float(p), t["bits"], t["dvec"], t["dq"][:, PAD:PAD + E], SQ, dk, SKV, dv, SKV,
                    t["ws"], nsplit]
            if entry != "ov3d_attn_bwd":
                args.append(t["mask"])
            guard.call(entry, *args, like=q)
        return guard.run_case(self.cuda, specs, call)


def _one_key_scales(pr):
    """Lk == 1: the softmax is the constant 1, so dS = P (dP - D) cancels to exactly zero in
    the reference and dq = dk = 0 there: a relative error against them is undefined.  The
    kernel's D = rowsum(dout o) comes from the bf16-rounded o, so its dS is rounding noise of
    the two terms that cancel.  -> the norms of dq and dk built from |dP| alone, the scale the
    2e-2 bar is then taken of."""
    assert pr.Lk == 1
    q = pr.qs[..., PAD:PAD + E].float().view(pr.Lq, pr.nb, H, 64)
    k = pr.kvs[..., PAD:PAD + E].float().view(1, pr.nb, H, 64)
    v = pr.kvs[..., PAD + E:PAD + 2 * E].float().view(1, pr.nb, H, 64)
    dP = (pr.dout.float().view(pr.Lq, pr.nb, H, 64) * v).sum(-1).abs() / (1 - pr.p)
    return (SCALE * dP[..., None] * k.abs()).norm().item(), \
        (SCALE * (dP[..., None] * q.abs()).sum(0)).norm().item()


def _check_grad(got, ref, zero_scale):
    if float(ref.norm()) == 0:
        assert float(got.float().norm()) <= 2e-2 * zero_scale
    else:
        assert _rel(got, ref) < 2e-2


def _check_grads(pr, out, ref):
    _, rq, rk, rv = ref
    sq, sk = _one_key_scales(pr) if pr.Lk == 1 else (None, None)
    _check_grad(out["dq"][:, PAD:PAD + E], rq, sq)
    _check_grad(out["dkv"][:, PAD:PAD + E], rk, sk)
    assert _rel(out["dkv"][:, PAD + E:PAD + 2 * E], rv) < 2e-2


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Lk", [1, 63, 65, 200])
@pytest.mark.parametrize("Lq", [32, 96, 160])
def test_attention_fwd_bwd(cuda, Lq, Lk, masked, p):
    """forward and backward, one key split; short unmasked attentions (Lq, Lk <= 128) run the
    backward in both settings of ov3d_attn_small_bwd (one launch / two launches)"""
    pr = Problem(cuda, Lq, Lk, masked, p)
    ref = pr.reference()
    fwd = pr.forward()
    assert _rel(fwd["o"], ref[0]) < 1e-2
    short = not masked and Lq <= 128 and Lk <= 128
    prev = _lib().ov3d_attn_small_bwd(-1)
    try:
        for setting in ((1, 0) if short else (prev,)):
            _lib().ov3d_attn_small_bwd(setting)
            _check_grads(pr, pr.backward(fwd), ref)
    finally:
        _lib().ov3d_attn_small_bwd(prev)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_attention_key_splits(cuda, p):
    """4 key splits with the fp32 partials in a workspace of exactly ov3d_attn_fwd_workspace floats"""
    pr = Problem(cuda, 128, 512, False, p)
    ref = pr.reference()
    fwd = pr.forward(nsplit=4)
    assert _rel(fwd["o"], ref[0]) < 1e-2
    _check_grads(pr, pr.backward(fwd, nsplit=4), ref)


def test_attention_dkdv_batch(cuda):
    """2 jobs of one shape write different column blocks of ONE dK and ONE dV buffer; dQ and D
    come from ov3d_attn_bwd with dk = dv = NULL"""
    from ov3d_amd import _native
    Lq, Lk, p = 64, 65, 0.3
    probs = [Problem(cuda, Lq, Lk, False, p, key=j) for j in range(2)]
    refs = [pr.reference() for pr in probs]
    fwds = [pr.forward() for pr in probs]
    dqs = [pr.backward(f, kv=False) for pr, f in zip(probs, fwds)]
    for d, r in zip(dqs, refs):
        assert _rel(d["dq"][:, PAD:PAD + E], r[1]) < 2e-2
    W = 2 * E + 2 * PAD
    specs = {"dk": Out((Lk * B, W), BF, full=_cols(Lk * B, W, PAD, PAD + 2 * E)),
             "dv": Out((Lk * B, W), BF, full=_cols(Lk * B, W, PAD, PAD + 2 * E))}
    for j, (pr, f, d) in enumerate(zip(probs, fwds, dqs)):
        specs.update({f"qs{j}": In(pr.qs), f"kvs{j}": In(pr.kvs), f"dout{j}": In(pr.dout, ld=SO),
                      f"lse{j}": In(f["lse"].cpu()), f"dvec{j}": In(d["dvec"].cpu()),
                      f"bits{j}": In(f["bits"].cpu())})
    J = _native.struct("ov3d_attn_dkdv_job")

    def call(t):
        jobs = []
        for j in range(2):
            q = t[f"qs{j}"][..., PAD:PAD + E]
            k, v = t[f"kvs{j}"][..., PAD:PAD + E], t[f"kvs{j}"][..., PAD + E:PAD + 2 * E]
            c0 = PAD + j * E
            jobs.append(J(q.data_ptr(), SQ, k.data_ptr(), SKV, v.data_ptr(), SKV, t[f"dout{j}"].data_ptr(),
                          SO, t[f"lse{j}"].data_ptr(), t[f"dvec{j}"].data_ptr(), t[f"bits{j}"].data_ptr(),
                          t["dk"][:, c0:c0 + E].data_ptr(), W, t["dv"][:, c0:c0 + E].data_ptr(), W))
        arr = (J * 2)(*jobs)
        guard.call("ov3d_attn_bwd_dkdv_batch", ctypes.addressof(arr), 2, B, H, Lq, Lk, SCALE, float(p),
                   like=t["dk"])
    out = guard.run_case(cuda, specs, call)
    for j, r in enumerate(refs):
        c0 = PAD + j * E
        assert _rel(out["dk"][:, c0:c0 + E], r[2]) < 2e-2
        assert _rel(out["dv"][:, c0:c0 + E], r[3]) < 2e-2


SMALL = [(32, 1), (96, 200)]


@pytest.mark.parametrize("Lq,Lk", SMALL)
@pytest.mark.parametrize("nb", [1, 3])
def test_dropgen_and_pregen_forward(cuda, nb, Lq, Lk):
    """ov3d_attn_dropgen writes exactly ov3d_attn_dropbits_words words, the bits of the hashing
    forward; ov3d_attn_fwd_pregen reading them gives that forward's output and lse bit for bit
    (test_forward_with_drop_bits_ahead_equals_hashing_forward) and leaves the words alone"""
    p = 0.3
    pr = Problem(cuda, Lq, Lk, True, p, nb=nb)
    hashed = pr.forward()
    assert _rel(hashed["o"], pr.reference()[0]) < 1e-2
    specs = {"seed": _seed(), "bits": Out((pr.nbits,), I32)}
    gen = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_attn_dropgen", nb, H, Lq, Lk, float(p), t["seed"], SITE, t["bits"], like=t["bits"]))["bits"]
    assert torch.equal(gen, hashed["bits"])
    pre = pr.forward(entry="ov3d_attn_fwd_pregen", bits=gen.cpu())
    assert torch.equal(pre["o"], hashed["o"]) and torch.equal(pre["lse"], hashed["lse"])
    assert torch.equal(pre["bits"], gen)


def _decode(words, nb, Lq, Lk):
    """both layouts of packed mask words -> (nb, Lq, nkt * 64) bool each (test_mask_pack_layouts)"""
    w = words.cpu().numpy().view(np.uint32)
    nkt = (Lk + 63) // 64
    W = nkt * nb * Lq * 2
    wq = w[:W].reshape(nkt, nb, Lq, 2)
    wk = w[W:].reshape(Lq // 32, nb, nkt * 64)
    dec_q = np.zeros((nb, Lq, nkt * 64), bool)
    dec_k = np.zeros((nb, Lq, nkt * 64), bool)
    for n in range(32):
        for h in range(2):
            kk = np.arange(nkt) * 64 + _drop_key(n, h)
            dec_q[:, :, kk] = ((wq[:, :, :, h] >> n) & 1).transpose(1, 2, 0).astype(bool)
        dec_k[:, n::32, :] = ((wk >> n) & 1).transpose(1, 0, 2).astype(bool)
    return dec_q, dec_k


@pytest.mark.parametrize("Lq,Lk", SMALL)
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_mask_pack(cuda, kind, nb, Lq, Lk):
    """exactly ov3d_attn_maskbits_words words, both layouts decoding to the mask bit for bit and
    zero past Lk"""
    g = _gen(kind, nb, Lq, Lk)
    thr = 0.8
    if kind == 0:
        m = torch.rand(nb, Lq, Lk, generator=g) < 0.4
        src = In(m.to(torch.uint8), index=(0, 1))        # bands: valid mask bytes, A != B
    else:
        d = torch.rand(nb, Lq, Lk, generator=g) * 2 - (0.2 if kind == 2 else 0)
        m = (d >= thr) if kind == 1 else (d.clamp_min(0).sqrt() >= thr)
        src = In(d)
    n = _lib().ov3d_attn_maskbits_words(nb, Lq, Lk)
    assert n == 4 * ((Lk + 63) // 64) * nb * Lq
    specs = {"src": src, "words": Out((n,), I32)}
    words = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_attn_mask_pack", t["src"], kind, thr, nb, Lq, Lk, t["words"], like=t["words"]))["words"]
    for dec in _decode(words, nb, Lq, Lk):
        assert np.array_equal(dec[:, :, :Lk], m.numpy()) and not dec[:, :, Lk:].any()


@pytest.mark.parametrize("nb", [1, 3])
def test_mask_pack_points(cuda, nb):
    """kind 3 (L = 96): the bits of packing torch.cdist's distances (test_point_mask_equals_cdist_mask)"""
    L, thr = 96, 0.8
    xyz = torch.rand(nb, L, 3, generator=_gen(nb, L)) * 2
    xyz[:, 7] = xyz[:, 3]                                # coincident points
    xg = xyz.to(cuda)                                    # the norms as attention.pack_mask_points forms them
    pts = torch.cat([xg, xg.pow(2).sum(-1, keepdim=True)], -1).contiguous().cpu()
    n =_lib().ov3d_attn_maskbits_words(nb, L, L)
    specs = {"src": In(pts), "words": Out((n,), I32)}
    words = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_attn_mask_pack", t["src"], 3, thr, nb, L, L, t["words"], like=t["words"]))["words"]
    dist = torch.cdist(xyz.to(cuda), xyz.to(cuda), p=2)
    ref = torch.empty(n, dtype=I32, device=cuda)
    guard.call("ov3d_attn_mask_pack", dist.contiguous(), 1, thr, nb, L, L, ref, like=ref)
    assert torch.equal(words, ref)

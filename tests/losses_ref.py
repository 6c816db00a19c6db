"""Float64 references of the loss, warp, mask, normalisation and Adam kernels (loss_misc.hip and the
warp / mask part of pool_warp.hip), the inputs of their GPU tests and the bounds those tests apply.

tests/test_gpu_losses.py compares the HIP kernels with these references; tests/test_losses_ref.py
checks, without a GPU, the references against the oracle (oracle/reconet_ref.py) and torch.optim.Adam,
and that the float32 CPU rendition of every operation meets the bound its GPU test applies, on the
very inputs that test uses -- so no bound here is taken from the code under test.

Everything is float64 torch-CPU, with one exception: the warp's source coordinates are the oracle's
float32 `_sample_coords`.  That op order is the definition of the operation (a float64 coordinate
floors differently at integer positions); everything after the coordinates is float64.
"""
import zlib

import numpy as np
import torch

from oracle import reconet_ref as R

F64 = torch.float64
LUM = (0.2126, 0.7152, 0.0722)
U23 = 2.0 ** -23

# bounds (derivations: the docstrings of the margin functions below)
LOSS_REL = 1e-5
ELEM_REL, ELEM_ABS = 1e-5, 1e-6
MASK_THR, MASK_BAND, MASK_BAND_SHARE = 2.0, 1e-4, 0.01

# Adam moments: no clean bound exists for m + (1-b1)(g-m) (it cancels), so the bound is 4x the error
# of torch.optim.Adam run in float32 on the CPU against `adam` below, on ADAM_CASE's own inputs, as
#   |err| / (|ref| + max_t |g_t gscale|)    for m,   |err| / (|ref| + max_t (g_t gscale)^2)   for v
# (4x: the kernel's lerp form m + (1-b1)(g-m) rounds differently from mul_/add_).  Measured maxima
# over both gscale values and all K steps: m 6.42e-08, v 3.05e-08 (tests/test_losses_ref.py asserts
# the measurement stays between bound/8 and bound/4).
ADAM_M_BOUND = 2.6e-7
ADAM_V_BOUND = 1.25e-7


def _d(t):
    return t.detach().to(F64)


# ------------------------------------------------------------------ margins (<= 1 passes)
def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0 and x / 0 = inf (a zero bound demands an exact zero)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
    r = np.where((bound == 0) & (err > 0), np.inf, r)
    return float(r.max()) if r.size else 0.0


def loss_margin(x, ref):
    """Loss scalars, 1e-5 relative: before the finisher's double accumulation each partial is at most
    ceil(work / 262144) + 6 + 4 float32 additions of same-sign terms; with the per-term rounding that
    is below 20 * 2^-24 = 1.2e-6, so 1e-5 leaves about 8x.  A zero reference demands an exact zero."""
    return _ratio(abs(float(x) - float(ref)), LOSS_REL * abs(float(ref)))


def elem_margin(x, ref):
    """Elementwise results: per element |err| <= 1e-5 |ref| + 1e-6 max|ref| (not the max-norm alone:
    one wrong small element would hide under it; the absolute term is for the OTL ot - it
    cancellation)."""
    x, ref = _d(x).numpy(), _d(ref).numpy()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return _ratio(np.abs(x - ref), ELEM_REL * np.abs(ref) + ELEM_ABS * np.abs(ref).max())


def warp_margin(x, ref, A, n):
    """Warp forward / backward: per element |err| <= (n + 8) 2^-23 A with A = sum |w| |g| and n the
    number of products (4 for the forward, the source pixel's list length for the backward, given per
    (b, pixel)): the standard bound of a sequential float32 sum of n products, plus three roundings in
    each weight, times two.  An element with an empty list has A = 0 and must be exactly 0."""
    x, ref, A = _d(x).numpy(), _d(ref).numpy(), _d(A).numpy()
    n = np.asarray(n, dtype=np.float64)
    if n.ndim:  # (B, HW) -> broadcast over channels
        n = n.reshape(x.shape[0], 1, *x.shape[2:])
    return _ratio(np.abs(x - ref), (n + 8) * U23 * A)


def adam_margins(p, m, v, ref, gmax, K):
    """(p, m, v) margins of one step against `adam`'s (p, m, v); gmax = max_t |g_t gscale| per element.
    p: |err| <= K 2^-23 max(1, |p|)."""
    rp, rm, rv = (r.numpy() for r in ref)
    p, m, v, gmax = _d(p).numpy(), _d(m).numpy(), _d(v).numpy(), _d(gmax).numpy()
    return (_ratio(np.abs(p - rp), K * U23 * np.maximum(1.0, np.abs(rp))),
            _ratio(np.abs(m - rm), ADAM_M_BOUND * (np.abs(rm) + gmax)),
            _ratio(np.abs(v - rv), ADAM_V_BOUND * (np.abs(rv) + gmax ** 2)))


def adam_moment_errors(m, v, ref, gmax):
    """The normalised m / v errors ADAM_M_BOUND / ADAM_V_BOUND are expressed in (maxima)."""
    _, rm, rv = (r.numpy() for r in ref)
    m, v, gmax = _d(m).numpy(), _d(v).numpy(), _d(gmax).numpy()
    return (float((np.abs(m - rm) / (np.abs(rm) + gmax)).max()),
            float((np.abs(v - rv) / (np.abs(rv) + gmax ** 2)).max()))


# ------------------------------------------------------------------ temporal losses
def _masked(a, b, it, m, count, weight):
    """weight * sum(m (a - b - it)^2) / count and its gradients w.r.t. a and b (autograd, float64).
    count == 0 (an all-zero mask): the library defines the loss as 0 and the gradients as 0 (its
    finisher divides by 1 instead, and every term carries the zero mask), so that is returned."""
    a, b = _d(a).requires_grad_(True), _d(b).requires_grad_(True)
    if count == 0:
        return 0.0, 0, torch.zeros_like(a), torch.zeros_like(b)
    loss = torch.sum(m * (a - b - it) ** 2) * weight / count
    loss.backward()
    return loss.item(), count, a.grad, b.grad


def ftl(a, b, mask, weight):
    """Feature temporal loss (oracle/reconet_ref.py:286-292): weight sum(m (a-b)^2) / (C nnz(m)),
    m = (mask > 0); mask (N, 1, H, W).  Returns (loss, count, d/da, d/db)."""
    m = (mask > 0).to(F64)
    return _masked(a, b, 0.0, m, a.shape[1] * int(m.count_nonzero()), weight)


def otl(s2, ws1, i2, wi1, mask, weight):
    """Output temporal loss (oracle/reconet_ref.py:293-298): the mask VALUE weights each term, `it` is
    the luminance of i2 - wi1, the count is 3 nnz(mask != 0).  Returns (loss, count, d/ds2, d/dws1)."""
    it = _d(i2) - _d(wi1)
    it = (LUM[0] * it[:, 0] + LUM[1] * it[:, 1] + LUM[2] * it[:, 2]).unsqueeze(1)
    return _masked(s2, ws1, it, _d(mask), 3 * int(mask.count_nonzero()), weight)


# ------------------------------------------------------------------ plain reductions
def mse(a, b, weight):
    """weight * mean((a - b[i % nb])^2), b broadcast over a's leading dim.  (loss, d/da, d/db)."""
    a, b = _d(a).requires_grad_(True), _d(b).requires_grad_(True)
    loss = ((a.reshape(-1, b.numel()) - b.reshape(1, -1)) ** 2).mean() * weight
    loss.backward()
    return loss.item(), a.grad, b.grad


def _tv_terms(s):
    return ((s[:, :, :-1, 1:] - s[:, :, :-1, :-1]) ** 2, (s[:, :, 1:, :-1] - s[:, :, :-1, :-1]) ** 2)


def tv(s, weight):
    """weight * sum(dx^2 + dy^2) over [:, :, :-1, :-1] (oracle/reconet_ref.py:306-308).  (loss, d/ds)."""
    s = _d(s).requires_grad_(True)
    r1, r2 = _tv_terms(s)
    loss = weight * torch.sum(r1 + r2)
    loss.backward()
    return loss.item(), s.grad


def tv_sqrt(s, weight):
    """weight * mean(sqrt(clamp(dx^2 + dy^2, min=1e-8))), RT/train.py's regulariser.  (loss, d/ds)."""
    s = _d(s).requires_grad_(True)
    r1, r2 = _tv_terms(s)
    loss = torch.sqrt((r1 + r2).clamp(min=1e-8)).mean() * weight
    loss.backward()
    return loss.item(), s.grad


def sum_scaled(x, weight):
    return float(_d(x).sum() * weight)


# ------------------------------------------------------------------ Adam
def adam(p, m, v, grads, first_step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0):
    """`oracle.reconet_ref.adam_step`'s arithmetic in float64 for len(grads) consecutive steps, from the
    given moments, the first step being number `first_step`; the gradient of a step is g * gscale.
    Returns [(p, m, v) after each step]."""
    p, m, v = _d(p).clone(), _d(m).clone(), _d(v).clone()
    out = []
    for k, g in enumerate(grads):
        t = first_step + k
        g = _d(g) * gscale
        m = m * b1 + g * (1 - b1)
        v = v * b2 + g * g * (1 - b2)
        denom = v.sqrt() / np.sqrt(1 - b2 ** t) + eps
        p = p - (lr / (1 - b1 ** t)) * m / denom
        out.append((p.clone(), m.clone(), v.clone()))
    return out


# ------------------------------------------------------------------ warp
def warp_taps(flo, H, W):
    """For each output pixel the four source taps (nw, ne, sw, se) of the bilinear warp:
    (idx (B, 4, HW) int64 flat source index, clamped where invalid; valid (B, 4, HW) bool;
    w (B, 4, HW) float64).  The coordinates are the oracle's float32 ones."""
    sx, sy = R._sample_coords(flo.detach().float(), H, W)
    assert sx.dtype == torch.float32
    B = flo.shape[0]
    sx, sy = sx.to(F64).reshape(B, H * W), sy.to(F64).reshape(B, H * W)
    x0, y0 = torch.floor(sx), torch.floor(sy)
    wx1, wy1 = sx - x0, sy - y0
    idx, valid, w = [], [], []
    for dy, wy in ((0, 1 - wy1), (1, wy1)):
        for dx, wx in ((0, 1 - wx1), (1, wx1)):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            valid.append((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H))
            idx.append(yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1))
            w.append(wx * wy)
    return torch.stack(idx, 1), torch.stack(valid, 1), torch.stack(w, 1)


def warp_fwd(x, flo):
    """(out, A): out = sum of the valid taps w x[src]; A = sum |w| |x[src]| (for `warp_margin`, n = 4)."""
    B, C, H, W = x.shape
    idx, valid, w = warp_taps(flo, H, W)
    w = w * valid
    flat = _d(x).reshape(B, C, H * W)
    out, A = torch.zeros_like(flat), torch.zeros_like(flat)
    for k in range(4):
        v = flat.gather(2, idx[:, k:k + 1].expand(B, C, H * W))
        out += v * w[:, k:k + 1]
        A += v.abs() * w[:, k:k + 1].abs()
    return out.reshape(B, C, H, W), A.reshape(B, C, H, W)


def warp_bwd(gout, flo):
    """(gx, A, n): the adjoint of warp_fwd as a float64 scatter-add, A = sum |w| |g| per element and
    n (B, HW) the number of taps that land on each source pixel (its list length)."""
    B, C, H, W = gout.shape
    idx, valid, w = warp_taps(flo, H, W)
    w = w * valid
    g = _d(gout).reshape(B, C, H * W)
    gx, A = torch.zeros_like(g), torch.zeros_like(g)
    n = torch.zeros(B, H * W, dtype=torch.int64)
    for k in range(4):
        e = idx[:, k:k + 1].expand(B, C, H * W)
        gx.scatter_add_(2, e, g * w[:, k:k + 1])
        A.scatter_add_(2, e, g.abs() * w[:, k:k + 1].abs())
        n.scatter_add_(1, idx[:, k], valid[:, k].long())
    return gx.reshape(B, C, H, W), A.reshape(B, C, H, W), n


def flow_mask_err(flo01, flo10):
    """|warp(grid + flo01, flo10) - grid|_1 in float64, (B, H, W): the forward-backward consistency
    error before the threshold (oracle/reconet_ref.py:213-220)."""
    B, _, H, W = flo01.shape
    grid = torch.stack(torch.meshgrid(torch.arange(W, dtype=F64), torch.arange(H, dtype=F64), indexing="xy"))
    fw, _ = warp_fwd(grid.unsqueeze(0) + _d(flo01), flo10)
    return (fw - grid).abs().sum(1)


# ------------------------------------------------------------------ normalisation / ConvTanh
def _std():
    return torch.tensor(R.IMAGENET_STD, dtype=F64).view(1, 3, 1, 1)


def vgg_normalize(x):
    """((x / 255 - mean) / std, x / 255): the output and what the in-place form leaves in x."""
    x = _d(x) / 255
    return (x - torch.tensor(R.IMAGENET_MEAN, dtype=F64).view(1, 3, 1, 1)) / _std(), x


def vgg_normalize_bwd(gout, gscaled=None):
    """Gradient w.r.t. the input from `gout` (on the output) and, for the in-place form, `gscaled` (on
    the mutated input x / 255): (gout / std[c] + gscaled) / 255."""
    g = _d(gout) / _std()
    return (g if gscaled is None else g + _d(gscaled)) / 255


def tanh_out_bwd(gy, t, prenorm):
    """ConvTanh backward from the saved tanh value: gy 150 (1 - t^2) / 255, preceded by the fused
    vgg_normalize backward gy / std[c] / 255 when prenorm."""
    gy, t = _d(gy), _d(t)
    if prenorm:
        gy = gy / _std() / 255
    return gy * 150 * (1 - t * t) / 255


# ====================================================================== inputs of the GPU tests
def _gen(*key):
    """A torch.Generator seeded from the case's name."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


TEMPORAL_SHAPES = {0: [(2, 5, 7, 9), (1, 3, 1, 1)], 1: [(2, 3, 7, 9), (1, 3, 1, 1)]}
TEMPORAL_BIG = {0: (1, 2, 513, 512), 1: (1, 3, 513, 512)}  # N HW = 262,656 > 1024 blocks x 256 threads
TEMPORAL_MASKS = ("binary", "signed", "zero")
TEMPORAL_BIG_MASKS = ("tail", "random")
TEMPORAL_WEIGHT = {0: 2.5, 1: 0.75}
GOUT = 0.5  # upstream gradient of every loss test (a kernel that ignored it would be off by 2x)


def temporal_case(mode, shape, mask_kind):
    """(a, b, c, d, mask, weight): c / d (the frames of the luminance term) are None in mode 0.
    Masks: "binary" 0/1; "signed" fractional with zeros and negative entries (mode 0 must treat <= 0
    as 0, mode 1 weights by the value and counts != 0); "zero"; for the grid-stride shapes "tail"
    (non-zero only in the last 600 pixels, so the strided second pass carries the whole result) and
    "random"."""
    g = _gen("temporal", mode, *shape, mask_kind)
    N, C, H, W = shape
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    c = d = None
    if mode == 1:
        c, d = torch.randn(N, 3, H, W, generator=g), torch.randn(N, 3, H, W, generator=g)
    u = torch.rand(N, 1, H, W, generator=g)
    val = torch.rand(N, 1, H, W, generator=g) * 0.9 + 0.1
    if mask_kind == "binary":
        mask = (u > 0.4).float()
        if mask.numel() == 1:
            mask.fill_(1.0)
    elif mask_kind == "signed":
        # 20% zeros, 15% negative (small, so the sum stays dominated by the positive terms), 65% in (0.1, 1)
        mask = torch.where(u < 0.2, torch.zeros_like(u), torch.where(u < 0.35, -0.3 * val, val))
        if mask.numel() == 1:
            mask.fill_(-0.625)
    elif mask_kind == "zero":
        mask = torch.zeros(N, 1, H, W)
    elif mask_kind == "tail":
        mask = torch.zeros(N * H * W)
        mask[-600:] = 1.0 if mode == 0 else 0.75
        mask = mask.view(N, 1, H, W)
    elif mask_kind == "random":
        mask = (u > 0.5).float() if mode == 0 else torch.where(u > 0.3, val, torch.zeros_like(u))
    else:
        raise ValueError(mask_kind)
    return a, b, c, d, mask, TEMPORAL_WEIGHT[mode]


def temporal_ref(mode, a, b, c, d, mask, weight):
    return ftl(a, b, mask, weight) if mode == 0 else otl(a, b, c, d, mask, weight)


BIG_N = 262144 + 257  # just past 1024 blocks x 256 threads
MSE_CASES = {"broadcast": (1000, 250), "full": (1000, 1000), "big": (BIG_N, BIG_N)}
MSE_WEIGHT = 3.0


def mse_case(name):
    n, nb = MSE_CASES[name]
    g = _gen("mse", name)
    return torch.randn(n // nb, nb, generator=g), torch.randn(nb, generator=g)


TV_SHAPES = [(2, 3, 2, 2), (1, 2, 2, 17), (1, 2, 17, 2), (2, 3, 10, 13), (1, 1, 514, 513)]
TV_WEIGHT = 0.5


def tv_case(shape, flat):
    """Pixel values in [0, 255).  flat: a constant patch (a whole plane of the 2 x 2 shape), which
    takes tv_sqrt's clamp branch."""
    s = torch.rand(shape, generator=_gen("tv", *shape)) * 255
    if flat and shape == (2, 3, 2, 2):
        s[1, 2] = 7.0
    elif flat and min(shape[2:]) >= 3:
        s[0, 0, :3, :3] = 7.0
    return s


SUM_SIZES = [1003, BIG_N]
SUM_WEIGHT = 0.25


def sum_case(n):
    return torch.rand(n, generator=_gen("sum", n)) + 0.1


ADAM_K, ADAM_FIRST = 4, 7
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_GSCALES = (1.0, 1.0 / 1024)


def adam_case(gscale):
    """n = 1003 (no multiple of 256 or 4), K = 4 steps from step 7, p ~ U(-1, 1), gradient magnitudes
    10^U(-6, 1) per element, non-zero moments of the size six earlier steps of such gradients leave.
    Returns (p, m, v, [g_1..g_K], gmax) with gmax = max_t |g_t gscale| per element."""
    g = _gen("adam", int(round(1 / gscale)))
    n = 1003
    p = torch.rand(n, generator=g) * 2 - 1
    mag = 10 ** (torch.rand(n, generator=g) * 7 - 6)
    grads = [mag * torch.randn(n, generator=g) for _ in range(ADAM_K)]
    eff = mag * gscale
    m = 0.4 * eff * torch.randn(n, generator=g)
    v = 0.006 * eff ** 2 * (0.5 + torch.rand(n, generator=g))
    gmax = torch.stack([(x * gscale).abs() for x in grads]).max(0).values
    return p, m, v, grads, gmax


def adam_first_case():
    """n = 5, step 1 from zero moments."""
    g = _gen("adam1")
    p = torch.rand(5, generator=g) * 2 - 1
    grad = torch.tensor([1e-6, -3e-3, 0.25, -10.0, 1.5]) * (0.5 + torch.rand(5, generator=g))
    return p, torch.zeros(5), torch.zeros(5), [grad], grad.abs()


# ---- warp
WARP_SHAPES = [(2, 5, 12, 20), (1, 19, 10, 24), (2, 3, 1, 7), (1, 2, 9, 1)]
WARP_FLOWS = ("random", "outside", "integer")
# backward only: flows chosen for the tiers of the gather form's list sort
WARP_TIER_CASES = {
    "mid": (1, 3, 12, 36),         # 3.3x zoom-in: lists of 9..16 (register tier) and 17..512 (LDS rank tier)
    "insertion": (1, 9, 24, 32),   # converging: lists over 512 (insertion tier)
    "scan": (1, 1, 1025, 1024),    # 1,049,600 pixels = 1025 scan blocks: the carry loop of the totals scan
}
WG_REG, WG_NET, WG_LONG, WS_BLOCK, SCAN_CHUNK = 8, 16, 512, 1024, 1024  # pool_warp.hip's tiers


def _coords_axis(cand, pos, n, axis):
    """The oracle's float32 source coordinate along one axis for flow values cand (K, n) at positions
    0..n-1."""
    K = cand.shape[0]
    if axis == 0:
        flo = torch.zeros(K, 2, 1, n)
        flo[:, 0, 0] = cand
        return R._sample_coords(flo, 1, n)[0][:, 0]
    flo = torch.zeros(K, 2, n, 1)
    flo[:, 1, :, 0] = cand
    return R._sample_coords(flo, n, 1)[1][:, :, 0]


def integral_axis_flow(n, axis, g):
    """Flow values f[0..n) (float32) for which the oracle's float32 source coordinate of position i
    is EXACTLY an in-bounds integer: solved from `_sample_coords` -- (i + f) = (t + 0.5) (n-1) / n for
    a target t -- then searched over neighbouring float32 values (and further targets where the
    float32 op chain skips the integer) until the oracle's own coordinate is integral."""
    pos = torch.arange(n, dtype=F64)
    tgt0 = torch.randperm(n, generator=g)
    out = torch.zeros(n)
    found = torch.zeros(n, dtype=torch.bool)
    ks = torch.arange(-48, 49, dtype=torch.int32).view(-1, 1)
    for shift in range(n):
        tgt = (tgt0 + shift) % n
        base = ((tgt.to(F64) + 0.5) * max(n - 1, 1) / n - pos).float()
        cand = (base.view(torch.int32).view(1, n) + ks).view(torch.float32)
        cand = torch.where(torch.isfinite(cand), cand, base.view(1, n).expand_as(cand))
        s = _coords_axis(cand, pos, n, axis)
        ok = s == tgt.float().view(1, n)
        first = ok.float().argmax(0)
        hit = ok.any(0) & ~found
        out = torch.where(hit, cand.gather(0, first.view(1, n))[0], out)
        found |= hit
        if bool(found.all()):
            return out
    raise AssertionError(f"no integral source coordinate for axis length {n}")


def warp_flow(kind, shape):
    """The flow (B, 2, H, W) of a warp case."""
    B, _, H, W = shape
    g = _gen("flow", kind, *shape)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    r = torch.rand(B, 2, H, W, generator=g)
    if kind == "random":
        return r * 8 - 4
    if kind == "random3":
        return r * 6 - 3
    if kind == "outside":  # every sample more than one pixel outside: right of the image on even rows, left on odd
        u = torch.where(ys % 2 == 0, W + 2 + r[:, 0], -xs - 3 - r[:, 0])
        return torch.stack([u, r[:, 1] * 2 - 1], 1)
    if kind == "integer":
        u = integral_axis_flow(W, 0, g).view(1, 1, W).expand(B, H, W)
        v = integral_axis_flow(H, 1, g).view(1, H, 1).expand(B, H, W)
        return torch.stack([u, v], 1).contiguous()
    if kind == "mid":  # 3.3x zoom-in
        return torch.stack([xs / 3.3 - xs + 4, ys / 3.3 - ys + 2], 1) + 0.3 * r
    if kind == "insertion":  # everything samples near column 5 / row 4
        return torch.stack([5.3 - xs, 4.6 - ys], 1) + 0.2 * r
    raise ValueError(kind)


WARP_FWD_CASES = [(f, s) for s in WARP_SHAPES for f in WARP_FLOWS]
WARP_BWD_CASES = WARP_FWD_CASES + [("mid", WARP_TIER_CASES["mid"]), ("insertion", WARP_TIER_CASES["insertion"]),
                                   ("random3", WARP_TIER_CASES["scan"])]
WARP_ATOMIC_CASES = [("mid", WARP_TIER_CASES["mid"]), ("random", (1, 19, 10, 24))]


def warp_case(kind, shape):
    """(x or gout, flo) of a warp forward / backward case."""
    return torch.randn(shape, generator=_gen("warpx", kind, *shape)), warp_flow(kind, shape)


MASK_SHAPES = [(2, 12, 20), (1, 1, 7), (1, 9, 1)]
# A sample with all four taps out of bounds has err = x + y exactly, so at x + y = 2 it ties with the
# threshold and lies in the guard band; on the one-row / one-column shapes most samples are out of
# bounds, so their seeds are chosen to keep pixel 2 in bounds (the band's share is asserted <= 1% by
# tests/test_losses_ref.py from the reference alone).
MASK_SEEDS = {(2, 12, 20): 0, (1, 1, 7): 4, (1, 9, 1): 10}


def mask_case(shape):
    """Random +-3 forward and backward flows (B, 2, H, W)."""
    B, H, W = shape
    g = _gen("fwm", *shape, MASK_SEEDS[shape])
    return torch.rand(B, 2, H, W, generator=g) * 6 - 3, torch.rand(B, 2, H, W, generator=g) * 6 - 3


def mask_check(mask, err64):
    """(wrong, band share): pixels outside the guard band |err64 - thr| <= 1e-4 where the mask is not
    (err64 < thr), and the share of pixels inside the band (either value is accepted there)."""
    mask, err64 = _d(mask).numpy(), err64.numpy()
    band = np.abs(err64 - MASK_THR) <= MASK_BAND
    wrong = (mask != (err64 < MASK_THR)) & ~band
    return int(wrong.sum()), float(band.mean())


NORM_SHAPES = [(2, 3, 5, 7), (1, 3, 1, 1)]


def norm_case(shape):
    """(x in [0, 255), gout, gscaled)."""
    g = _gen("norm", *shape)
    return torch.rand(shape, generator=g) * 255, torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def tanh_case():
    """(gy, t): t = tanh of a pre-activation, up to about 0.999 (1 - t^2 cancels there: the bound's
    absolute term)."""
    g = _gen("tanh")
    return torch.randn(2, 3, 5, 7, generator=g), torch.tanh(1.5 * torch.randn(2, 3, 5, 7, generator=g))

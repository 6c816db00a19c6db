"""Float64 references of the InstanceNorm and channel-sum kernels (csrc/norm.hip), the inputs of their
GPU tests and the bounds those tests apply.

tests/test_gpu_norm.py compares the HIP kernels with these references; tests/test_norm_ref.py checks,
without a GPU, the references against float64 torch autograd, and that the plain float32 form of every
formula meets the bound its GPU test applies, on the very inputs that test uses -- so no bound here
is taken from the code under test.  Everything is float64 torch on the CPU.

Bounds (per element, u = 2^-24, from the float64 statistics of the test's own inputs):

    dx    = |xhat| + |mean| rstd
    Y_pre = u (K_Y dx |w| + |b|)
    Y     = Y_pre + u |y|  (+ u |res| when a residual is added)
    GX    = min( K_G  u rstd |w| (|g| + |mean g| + dx |mean(g xhat)|),
                 K_GS u rstd |w| (|g| + |mean g| (1 + |xhat| |mean| rstd) + dx |mean(g xhat)|) )

They follow from two facts: the kernels keep the plane moments in fp64 and round mean and rstd to fp32
once each (u relative: through xhat that is u |mean| rstd and u |xhat|), and `in_affine` and the gx
expression add three roundings each.  The second form of GX has one term more: the fp32 mean shifts
every xhat of a plane by the same (mean - mean32) rstd, which moves mean(g xhat) by that shift times
mean(g) and gx by |xhat| times that.  On "offset" planes (|mean| rstd = 50) the first form has to pay
for it with its constant, on the others the second form's constant is the larger one: both are bounds,
so the smaller holds.  The constants are measured on the plain float32 form (`plain_forward` /
`plain_backward`: fp64 moments, mean and rstd rounded to fp32, everything else fp32 torch on the CPU),
not on the kernels: the worst error / (bound at K = 1) over every input below, times 4, rounded up to
one significant digit (the factor the Adam moment bounds of tests/losses_ref.py use: room for another
equally valid rounding order, none for a wrong term).  tests/test_norm_ref.py prints the ratios and
asserts K / 8 < ratio <= K / 4.  Measured:

    y                  worst ratio  1.78 ("near",   HW = 32768)  ->  K_Y  = 8
    gx, first form     worst ratio 13.7  ("offset", HW = 32761)  ->  K_G  = 60
    gx, second form    worst ratio  4.44 ("near",   HW = 32768)  ->  K_GS = 20

gw: |err| <= 4u sum |g xhat| + u sum over the planes of |mean| rstd |sum g|; gb: |err| <= 4u sum |g| (sums
over the channel's terms).  Bounds, not estimates: the per-plane partials are fp32-rounded fp64 sums (u
each), the sum over n is rounded once more (u), and the LDS route adds fp32 sums of four first (2u).
gw's second term is the mean shift again, times the plane's sum of g: it is in gw whatever the summation
does, and at HW = 35 on "offset" planes the plain float32 form misses 4u sum |g xhat| alone by 2.9x.
gc (the producing conv's bias gradient, sum of gx, analytically 0): against the float64 sum of the gx
the kernel wrote, 4u sum |gx|; against 0, the sum over the channel's elements of GX.
Accumulating entries: the same bound plus one ulp (2^-23) of old + ref.

Statistics: mean and rstd are fp32 roundings of fp64 values, |err| <= u |ref| plus what D64 = 128
float64 roundings of the sums can move them (the kernels add at most 32 terms in sequence per lane and
a tree of 16 levels above them, the reference sums pairwise; both together stay below 128):
    d mean <= D64 2^-53 mean|x|,   d var <= D64 2^-53 (E x^2 + 2 |mean| E|x|),   d rstd <= rstd d var / (2 (var + eps)).

Guard bands (either answer is accepted inside; tests/test_norm_ref.py asserts each holds <= 1 % of a
case): the ReLU decision where |pre64| <= Y_pre, and a byte of the fused tail where the float64 image
value lies within dimg = 127.5 (1 - t^2) Y_pre + 127.5 * 4u (1 + |t|) + 510u of an integer (the
pre-activation's error through tanh's slope, four roundings of tanhf's result and of t + 1, and two
roundings of an image value of at most 255).
"""
import zlib

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
EPS = 1e-5
D64 = 128

K_Y = 8.0
K_G = 60.0
K_GS = 20.0
BAND_SHARE = 0.01


def _d(t):
    return t.detach().to(F64)


def _gen(*key):
    """A torch.Generator seeded from the case's name."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0 and x / 0 = inf (a zero bound demands an exact zero)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
    r = np.where((bound == 0) & (err > 0), np.inf, r)
    r = np.where(np.isfinite(err), r, np.inf)
    return float(r.max()) if r.size else 0.0


def margin(x, ref, bound):
    """max |x - ref| / bound over the elements; <= 1 passes, a non-finite x never does."""
    x, ref, bound = _d(x).numpy(), _d(ref).numpy(), _d(bound).numpy()
    assert x.shape == ref.shape == bound.shape, (x.shape, ref.shape, bound.shape)
    return _ratio(np.abs(x - ref), bound)


# ====================================================================== references
def stats(x, eps=EPS):
    """(mean, var, rstd), each (N, C, 1, 1): biased variance as E[x^2] - mean^2 clamped at 0, the form
    the kernels use, rstd = 1 / sqrt(var + eps)."""
    x = _d(x).flatten(2)
    mean = x.mean(2)
    var = ((x * x).mean(2) - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return tuple(t.view(*t.shape, 1, 1) for t in (mean, var, rstd))


def _cw(v):
    return _d(v).view(1, -1, 1, 1)


def forward(x, w, b, relu=False, res=None, eps=EPS):
    """(pre, y): pre = xhat w + b, y = [relu](pre) [+ res]."""
    mean, _, rstd = stats(x, eps)
    pre = (_d(x) - mean) * rstd * _cw(w) + _cw(b)
    y = pre.clamp_min(0) if relu else pre.clone()
    if res is not None:
        y = y + _d(res)
    return pre, y


def backward(gy, x, w, mask=None, eps=EPS):
    """(gx, gw, gb, gc) with the ReLU mask an input (None: no ReLU): g = gy mask,
    gx = rstd w (g - mean(g) - xhat mean(g xhat)), gw = sum g xhat, gb = sum g, gc = sum gx (sums over
    n, h, w)."""
    mean, _, rstd = stats(x, eps)
    xhat = (_d(x) - mean) * rstd
    g = _d(gy) if mask is None else _d(gy) * _d(mask)
    mg = g.mean((2, 3), keepdim=True)
    mgx = (g * xhat).mean((2, 3), keepdim=True)
    gx = rstd * _cw(w) * (g - mg - xhat * mgx)
    return gx, (g * xhat).sum((0, 2, 3)), g.sum((0, 2, 3)), gx.sum((0, 2, 3))


def chunk_bounds(HW, S, k):
    """Elements [lo, hi) of chunk k of S of a plane (norm.hip's rule: whole float4s when HW % 4 == 0)."""
    if HW % 4 == 0:
        n4 = HW // 4
        return n4 * k // S * 4, n4 * (k + 1) // S * 4
    return HW * k // S, HW * (k + 1) // S


def tanh_frames(x, w, b, bgr, eps=EPS):
    """(img, frames): img = clamp((tanh(pre) + 1) / 2 * 255, 0, 255) in float64 and its truncation to
    uint8, both (N, H, W, 3), channels reversed if bgr."""
    pre, _ = forward(x, w, b, eps=eps)
    img = ((torch.tanh(pre) + 1) / 2 * 255).clamp(0, 255).permute(0, 2, 3, 1)
    if bgr:
        img = img.flip(-1)
    img = img.contiguous()
    return img, img.to(torch.uint8)


def channel_sum(x):
    """x (N, C, HW) -> (C,)."""
    return _d(x).sum((0, 2))


# ====================================================================== bounds
def _dx(x, eps):
    mean, _, rstd = stats(x, eps)
    return ((_d(x) - mean) * rstd).abs() + mean.abs() * rstd


def forward_bounds(x, w, b, relu=False, res=None, K=K_Y, eps=EPS):
    """(Y_pre, Y) of the module docstring."""
    _, y = forward(x, w, b, relu, None, eps)
    y_pre = U * (K * _dx(x, eps) * _cw(w).abs() + _cw(b).abs())
    Y = y_pre + U * y.abs()
    if res is not None:
        Y = Y + U * _d(res).abs()
    return y_pre, Y


def backward_bounds(gy, x, w, mask=None, K=K_G, K_shift=K_GS, eps=EPS):
    """(GX per element, GW (C,), GB (C,)) of the module docstring; K / K_shift None leaves that form of GX
    out (tests/test_norm_ref.py measures each alone)."""
    mean, _, rstd = stats(x, eps)
    xhat = (_d(x) - mean) * rstd
    g = _d(gy) if mask is None else _d(gy) * _d(mask)
    mg = g.mean((2, 3), keepdim=True).abs()
    mgx = (g * xhat).mean((2, 3), keepdim=True).abs()
    dx = _dx(x, eps)
    k = U * rstd * _cw(w).abs()
    shift = xhat.abs() * mean.abs() * rstd
    both = [K * k * (g.abs() + mg + dx * mgx)] if K is not None else []
    if K_shift is not None:
        both.append(K_shift * k * (g.abs() + mg * (1 + shift) + dx * mgx))
    GX = both[0] if len(both) == 1 else torch.minimum(*both)
    # gw: the fp32 mean shifts every xhat of a plane by the same (mean - mean32) rstd, at most u |mean| rstd,
    # and that shift times the plane's sum of g is in gw whatever the summation does
    shift_gw = (U * mean.abs() * rstd * g.sum((2, 3), keepdim=True).abs()).sum((0, 2, 3))
    return GX, 4 * U * (g * xhat).abs().sum((0, 2, 3)) + shift_gw, 4 * U * g.abs().sum((0, 2, 3))


def stats_bounds(x, eps=EPS):
    """(d mean, d rstd), each (N, C, 1, 1), of the module docstring."""
    x64 = _d(x).flatten(2)
    mean, var, rstd = stats(x, eps)
    sh = mean.shape
    e1, e2 = x64.abs().mean(2).view(sh), (x64 * x64).mean(2).view(sh)
    f = D64 * 2.0 ** -53
    dvar = f * (e2 + 2 * mean.abs() * e1)
    return U * mean.abs() + f * e1, U * rstd + rstd * dvar / (2 * (var + eps))


def gc_sum_bound(gx):
    """4u sum |gx| per channel, for gc against the float64 sum of the gx that was written."""
    return 4 * U * _d(gx).abs().sum((0, 2, 3))


def ulp_sum(old, ref):
    """One fp32 ulp of old + ref (the rounding of an accumulating store)."""
    return 2.0 ** -23 * (_d(old) + _d(ref)).abs()


def relu_band(pre, y_pre):
    """Elements whose ReLU decision fp32 rounding may flip: |pre64| <= Y_pre."""
    return pre.abs() <= y_pre


def relu_wrong(y, pre, sure):
    """Number of elements outside the guard band where (y > 0) differs from (pre64 > 0)."""
    return int((((_d(y) > 0) != (pre > 0)) & sure).sum())


def frame_dimg(x, w, b, bgr, eps=EPS):
    """dimg (N, H, W, 3), laid out as `tanh_frames` lays out the image."""
    pre, _ = forward(x, w, b, eps=eps)
    y_pre, _ = forward_bounds(x, w, b, eps=eps)
    t = torch.tanh(pre)
    d = 127.5 * (1 - t * t) * y_pre + 127.5 * 4 * U * (1 + t.abs()) + 510 * U
    d = d.permute(0, 2, 3, 1)
    return (d.flip(-1) if bgr else d).contiguous()


def frames_check(frames, img, dimg):
    """(wrong, band share, differing share) of uint8 frames against the float64 image: a byte must equal
    trunc(img), except that where img lies within dimg of an integer it may differ from it by 1."""
    want = img.to(torch.uint8).to(torch.int16)
    got = frames.cpu().to(torch.int16)
    assert got.shape == want.shape, (got.shape, want.shape)
    band = (img - torch.round(img)).abs() <= dimg
    diff = (got - want).abs()
    wrong = ((diff > 0) & ~band) | (diff > 1)
    return int(wrong.sum()), float(band.double().mean()), float((diff > 0).double().mean())


def channel_sum_bound(x, ref, old=None):
    """|err| <= 2^-24 |ref| + n 2^-53 sum |x| (n = N HW terms per channel), plus one ulp of old + ref when
    accumulating."""
    x = _d(x)
    n = x.shape[0] * x.shape[2]
    bound = U * ref.abs() + n * 2.0 ** -53 * x.abs().sum((0, 2))
    return bound if old is None else bound + ulp_sum(old, ref)


# ====================================================================== the plain float32 form
def plain_stats(x, eps=EPS):
    """fp64 moments, mean and rstd rounded to fp32 (each (N, C, 1, 1))."""
    mean, _, rstd = stats(x, eps)
    return mean.float(), rstd.float()


def plain_forward(x, w, b, relu=False, res=None, eps=EPS):
    """(pre, y) in fp32 torch from `plain_stats`."""
    mean, rstd = plain_stats(x, eps)
    pre = (x - mean) * rstd * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    y = pre.clamp_min(0) if relu else pre.clone()
    return pre, (y if res is None else y + res)


def plain_backward(gy, x, w, mask=None, eps=EPS):
    """(gx, gw, gb, gc): xhat and gx in fp32 torch, the plane means of g and g xhat fp64 sums of the
    fp32 terms rounded to fp32, the per-plane partials of gw / gb / gc fp32-rounded fp64 sums, their sum
    over n rounded to fp32 once more."""
    mean, rstd = plain_stats(x, eps)
    xhat = (x - mean) * rstd
    g = gy if mask is None else gy * mask.float()
    sg = g.double().sum((2, 3), keepdim=True)
    sgx = (g.double() * xhat.double()).sum((2, 3), keepdim=True)
    HW = x.shape[2] * x.shape[3]
    mg, mgx = (sg / HW).float(), (sgx / HW).float()
    gx = (rstd * w.view(1, -1, 1, 1)) * (g - mg - xhat * mgx)
    over_n = lambda p: p.float().double().sum(0).float().flatten()
    return gx, over_n(sgx), over_n(sg), over_n(gx.double().sum((2, 3), keepdim=True))


def plain_tanh_frames(x, w, b, bgr, eps=EPS):
    """frames_elem.h's steps in fp32 torch on `plain_forward`'s pre-activation: (N, H, W, 3) uint8."""
    pre, _ = plain_forward(x, w, b, eps=eps)
    img = (((torch.tanh(pre) + 1.0) / 2.0) * 255.0).clamp(0, 255).permute(0, 2, 3, 1)
    return (img.flip(-1) if bgr else img).contiguous().to(torch.uint8)


def plain_channel_sum(x, old=None):
    """fp64 plane sums rounded to fp32, summed over n in fp64, rounded to fp32 [and added to old in fp32]."""
    s = x.double().sum(2).float().double().sum(0).float()
    return s if old is None else old + s


# ====================================================================== inputs of the GPU tests
KINDS = ("near", "offset", "const")


def planes(shape, seed, kind):
    """(N, C, H, W) float32 planes.  "near": per-plane mean within +-4 std, std in [0.5, 2]; "offset":
    mean = +-50 std (the fp32-rounded mean then costs |mean| rstd = 50 ulps of xhat, and a float
    accumulation of the moments would lose the variance); "const": every element 1.5 (the fp64 moments
    are exact: var == 0, rstd = eps^-1/2, xhat == 0)."""
    N, C, H, W = shape
    if kind == "const":
        return torch.full(shape, 1.5)
    g = _gen("planes", *shape, seed, kind)
    std = 0.5 + 1.5 * torch.rand(N, C, 1, 1, generator=g)
    if kind == "near":
        mean = (8 * torch.rand(N, C, 1, 1, generator=g) - 4) * std
    elif kind == "offset":
        mean = 50 * std * (2.0 * (torch.rand(N, C, 1, 1, generator=g) < 0.5) - 1)
    else:
        raise ValueError(kind)
    return torch.randn(N, C, H, W, generator=g) * std + mean


def affine(C, *key):
    """w = 1 + 0.3 randn, b = 0.3 randn, distinct per channel; the last channel's w is negative."""
    g = _gen("affine", C, *key)
    w = 1.0 + 0.3 * torch.randn(C, generator=g)
    b = 0.3 * torch.randn(C, generator=g)
    w[-1] = -w[-1].abs()
    return w, b


# (N, C, H, W): HW and what it exercises
SHAPES = [
    (2, 3, 1, 1),       # 1: var = 0, scalar route
    (1, 2, 1, 4),       # 4: one float4, 511 idle threads
    (2, 3, 5, 7),       # 35: scalar two-pass route, HW < NT
    (1, 2, 61, 68),     # 4148: n4 = 1037, third register slot partly filled, fourth empty
    (2, 3, 64, 128),    # 8192: register route exactly full
    (1, 2, 3, 2732),    # 8196: first size on <1024,8> forward and the LDS backward
    (1, 2, 128, 256),   # 32768: LDS route exactly full
    (1, 2, 3, 10924),   # 32772: n4 = 8193, float4 two-pass, only thread 0 takes the tail `if (i < n4)`
    (1, 2, 181, 181),   # 32761: scalar two-pass, several strides per thread
    # 36864: n4 = 9216 = 4 * 2048 + 1024, float4 two-pass: the second load of thread 0's fifth pair would be
    # the float4 one past the plane (a pair loop running to `i + NT <= n4` reads the next plane's there)
    (1, 2, 3, 12288),
]
BY_HW = {s[2] * s[3]: s for s in SHAPES}
EDGE_HW = (35, 8192, 8196, 32772, 32761)  # one per kernel body: "offset" and "const" run here
CASES = [(s, "near") for s in SHAPES] + [(BY_HW[hw], k) for k in ("offset", "const") for hw in EDGE_HW]
ACC_HW = (35, 8192, 8196, 32772)  # one per backward kernel
MISALIGNED_HW = (35, 32761, 4148, 8196, 32772)  # scalar route; then HW % 4 == 0 on each vector route
RELU_RES = [(False, False), (True, False), (False, True), (True, True)]

# The host routes of vst_instnorm_fwd / vst_instnorm_bwd as data: (kernel, needs HW % 4 == 0 and 16-byte
# aligned tensors, largest HW or None), first match wins.
FWD_ROUTES = (("in_fwd_reg_kernel<512,4>", True, 8192), ("in_fwd_reg_kernel<1024,8>", True, 32768),
              ("in_fwd_kernel<1024>", False, None))
BWD_ROUTES = (("in_bwd_reg_kernel<512,4,true>", True, 8192), ("in_bwd_lds_kernel", True, 32768),
              ("in_bwd_kernel<1024>", False, None))
# what each named shape is there for: (forward kernel, backward kernel, body of a two-pass kernel)
INTENDED = {
    1: ("in_fwd_kernel<1024>", "in_bwd_kernel<1024>", "scalar"),
    4: ("in_fwd_reg_kernel<512,4>", "in_bwd_reg_kernel<512,4,true>", None),
    35: ("in_fwd_kernel<1024>", "in_bwd_kernel<1024>", "scalar"),
    4148: ("in_fwd_reg_kernel<512,4>", "in_bwd_reg_kernel<512,4,true>", None),
    8192: ("in_fwd_reg_kernel<512,4>", "in_bwd_reg_kernel<512,4,true>", None),
    8196: ("in_fwd_reg_kernel<1024,8>", "in_bwd_lds_kernel", None),
    32768: ("in_fwd_reg_kernel<1024,8>", "in_bwd_lds_kernel", None),
    32772: ("in_fwd_kernel<1024>", "in_bwd_kernel<1024>", "float4"),
    32761: ("in_fwd_kernel<1024>", "in_bwd_kernel<1024>", "scalar"),
    36864: ("in_fwd_kernel<1024>", "in_bwd_kernel<1024>", "float4"),
}


def route(routes, HW, aligned=True):
    """(kernel, body): body is "float4" / "scalar" for the two-pass kernels (which choose it themselves
    by the same HW % 4 and alignment test), None for the others."""
    vec = HW % 4 == 0 and aligned
    for name, need_vec, limit in routes:
        if (vec or not need_vec) and (limit is None or HW <= limit):
            return name, (None if need_vec else ("float4" if vec else "scalar"))
    raise AssertionError(HW)


def case(shape, kind):
    """The inputs of one (shape, kind): x, w, b, gy, res (float32)."""
    N, C, H, W = shape
    g = _gen("case", *shape, kind)
    w, b = affine(C, *shape, kind)
    return dict(x=planes(shape, 1, kind), w=w, b=b, gy=torch.randn(shape, generator=g),
                res=torch.randn(shape, generator=g))


# split-plane apply: (shape, S); those of tests/test_gpu_rtnstv_inference.py's `_split_cases` are left out
APPLY_CASES = [((2, 3, 5, 7), 2), ((2, 3, 5, 7), 3), ((2, 3, 5, 7), 7), ((2, 3, 5, 7), 256),
               ((1, 3, 36, 52), 3), ((1, 3, 36, 52), 256), ((1, 2, 1, 8), 7)]
APPLY_MISALIGNED = ((1, 3, 36, 52), 3)  # res offset by one float: the scalar body at HW % 4 == 0
# fused tail: (shape, S), S = None is the host rule's choice (1 at these sizes)
TAIL_CASES = [((2, 3, 5, 7), 3), ((2, 3, 36, 52), None), ((2, 3, 36, 52), 2), ((2, 3, 36, 52), 7),
              ((1, 3, 33, 257), 5)]


def apply_case(shape):
    """x, w, b, res of a split-plane apply case."""
    w, b = affine(shape[1], "apply", *shape)
    return planes(shape, 17, "near"), w, b, torch.randn(shape, generator=_gen("applyres", *shape))


def tail_case(shape):
    """z = planes * 3 (the spread of conv4's output), w, b."""
    w, b = affine(3, "tail", *shape)
    return planes(shape, 29, "near") * 3, w, b


# channel_sum: (N, C, HW).  4100: HW4 = 1025, thread 0 alone takes the tail; 8196: several iterations
# plus a tail; C = 260: two blocks of sum_over_n_kernel, the second ragged; 6144: HW4 = 1536 = 1024 + 512, the
# second load of thread 0's second pair would be the float4 one past the plane
CSUM_SHAPES = [(2, 3, 1), (2, 3, 35), (3, 5, 4100), (1, 2, 8196), (2, 260, 8), (1, 2, 6144)]


def csum_case(shape):
    """(x with mean 3 so that cancellation does not hide a dropped element, old (C,) for the
    accumulating call)."""
    g = _gen("csum", *shape)
    return 3.0 + torch.randn(shape, generator=g), 10.0 * torch.randn(shape[1], generator=g)


def misaligned(t, pad=8, fill=float("nan")):
    """(view, buffer): a copy of t that starts one float past a 16-byte boundary, inside a buffer filled with
    `fill` that extends `pad` - 1 floats past its end (for a look at what lies around an output)."""
    buf = torch.full((t.numel() + pad,), fill, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v, buf


def untouched_around(buf, n):
    """The floats of `misaligned`'s buffer outside the n-element view still hold the NaN fill."""
    return bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + n:]).all())

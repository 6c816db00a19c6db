"""The reflect-pad-1 3x3 data gradient on the exact grid (vst_conv_dgrad_reflect3, the RT form of
csrc/conv_halo_kernel.h) against float64 autograd and the padded-grid path it replaces.

dx[ci,i,j] = sum_co sum_{kh,kw} w[co,ci,kh,kw] sum_{y in R_kh(i)} sum_{x in C_kw(j)} dy[co,y,x], with
R_kh(i) = {i+1-kh} u ({0} if i == 1 and kh == 0) u ({H-1} if i == H-2 and kh == 2) and C_kw(j) likewise:
the zero-pad transposed conv plus the border's reflected taps, which the kernel adds as extra MFMAs
from the patch it has staged.  The reference is float64 autograd of conv2d(pad(x, reflect)); the bars
are the per-mode bars of tests/test_gpu_halo.py for this operation.  Outside rows {1, H-2} and columns
{1, W-2} the unsplit launch sums the same products in the same order as vst_conv_dgrad_padout +
vst_fold_border, so those pixels are compared bitwise.

Shapes: H, W in {2, 3, 4} (rows 1 and H-2 coincide or swap); W in {32, 33, 34} (column W-2 the last
lane of a tile, its source column in the next tile, lane 0 of a ragged tile); H in {5, 8, 9, 10, 17}
(row H-2 on either side of the 4- and 8-row tile boundaries); Cin in {64, 128, 192, 256} (every block
shape); Cin = 96 (the form does not apply: the padded-grid path stays).  Split-K engages from six
channel blocks on these small grids (Cout = 96)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from vst._lib import VstError, lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16X3, BF16, BF16X6, F16 = 1, 2, 3, 4
KBLOCK, PERTAP, NOSPLIT = 16, 32, 64
GM_TRANSPOSED = 2
EPI_MASK, EPI_PADOUT = 8, 128

# output error vs fp64 (max-norm relative) by product precision
TOL = {BF16X6: 5e-6, BF16X3: 1e-4, F16: 2e-3, BF16: 2e-2}
MODES = [BF16X6, F16, BF16, BF16X3]


def _dims(M, K):
    mp, kp = ctypes.c_int(), ctypes.c_int()
    assert lib.vst_conv_pack_dims(M, K, ctypes.byref(mp), ctypes.byref(kp)) == 0
    return mp.value, kp.value


def _pack(w, mode, transposed=False):
    Cout, Cin, KH, KW = w.shape
    M = Cin if transposed else Cout
    Mpad, Kpad = _dims(M, KH * KW * (Cout if transposed else Cin))
    n = Mpad * Kpad * 3 // 2 if (mode & 7) == BF16X6 else Mpad * Kpad
    p = torch.empty(n, device=DEV)
    lib.vst_pack_weight(w.data_ptr(), p.data_ptr(), Cout, Cin, KH, KW, int(transposed), 0, Mpad, Kpad, mode,
                        torch.cuda.current_stream().cuda_stream)
    return p


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _P(t):
    return None if t is None else t.data_ptr()


def _exact(dy, wp, Cin, mode, mask=None, ws=True):
    """vst_conv_dgrad_reflect3 into a NaN-filled dx; ws: supply the split-K workspace it asks for."""
    N, Cout, H, W = dy.shape
    dx = torch.full((N, Cin, H, W), float("nan"), device=DEV)
    nb = lib.vst_conv_dgrad_reflect3_workspace(N, Cout, Cin, H, W, mode)
    assert nb >= 0, "the exact-grid form must apply here"
    nb = nb if ws else 0
    wsb = torch.empty((nb + 3) // 4, device=DEV) if nb else None
    lib.vst_conv_dgrad_reflect3(dy.data_ptr(), wp.data_ptr(), _P(mask), dx.data_ptr(), N, Cout, Cin, H, W, _P(wsb), nb,
                                mode, torch.cuda.current_stream().cuda_stream)
    return dx


def _padout(dy, wp, Cin, mode, mask=None):
    """The padded-grid path: vst_conv_dgrad_padout + vst_fold_border (unsplit unless mode allows)."""
    N, Cout, H, W = dy.shape
    st = torch.cuda.current_stream().cuda_stream
    dx = torch.full((N, Cin, H, W), float("nan"), device=DEV)
    border = torch.zeros(N, Cin, H + 2, W + 2, device=DEV)
    nb = lib.vst_conv_splitk_workspace(N, Cout, Cin, H + 2, W + 2, 3, 3, GM_TRANSPOSED, 1, 0, 0, 1,
                                       EPI_PADOUT | (EPI_MASK if mask is not None else 0), 0, mode)
    wsb = torch.empty((nb + 3) // 4, device=DEV) if nb else None
    lib.vst_conv_dgrad_padout(dy.data_ptr(), wp.data_ptr(), _P(mask), dx.data_ptr(), border.data_ptr(), N, Cout, H, W,
                              Cin, H, W, 3, 1, _P(wsb), nb, mode, st)
    lib.vst_fold_border(border.data_ptr(), _P(mask), dx.data_ptr(), N * Cin, H, W, 1, st)
    return dx


def _ref64(dy, w, Cin, mask=None):
    N, _, H, W = dy.shape
    x = torch.zeros(N, Cin, H, W, dtype=torch.float64, device=DEV, requires_grad=True)
    F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w.double()).backward(dy.double())
    return x.grad * (mask > 0).double() if mask is not None else x.grad


def _rel(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def _unaffected(H, W):
    """Pixels no reflected tap reaches: outside rows {1, H-2} and columns {1, W-2}."""
    keep = torch.ones(H, W, dtype=torch.bool, device=DEV)
    keep[[1, H - 2], :] = False
    keep[:, [1, W - 2]] = False
    return keep


def _check(N, Cout, Cin, H, W, mode, masked=False):
    """Unsplit launch: fp64 bar, bitwise equality with the padded-grid path off the affected rows and
    columns, no untouched pixel, determinism, batch independence."""
    dy = _rand(N, Cout, H, W, seed=8)
    w = _rand(Cout, Cin, 3, 3, seed=9, scale=0.05)
    mask = _rand(N, Cin, H, W, seed=10) if masked else None
    m = mode | KBLOCK | NOSPLIT
    wp = _pack(w, m, transposed=True)
    dx = _exact(dy, wp, Cin, m, mask)
    old = _padout(dy, wp, Cin, m, mask)
    again = _exact(dy, wp, Cin, m, mask)
    alone = _exact(dy[N - 1:].contiguous(), wp, Cin, m, None if mask is None else mask[N - 1:].contiguous())
    torch.cuda.synchronize()
    ref = _ref64(dy, w, Cin, mask)
    err, err_old = _rel(dx, ref), _rel(old, ref)
    print(f"reflect3 N{N} Cout{Cout} Cin{Cin} {H}x{W} mode {mode} masked {masked}: err {err:.3e} "
          f"(padded-grid path {err_old:.3e})")
    assert not torch.isnan(dx).any()
    if masked:
        assert torch.equal(dx[~(mask > 0)], torch.zeros_like(dx[~(mask > 0)]))
    keep = _unaffected(H, W)
    assert torch.equal(dx[:, :, keep], old[:, :, keep]), float((dx - old)[:, :, keep].abs().max())
    assert err < TOL[mode], err
    assert torch.equal(dx, again)
    assert torch.equal(dx[N - 1:], alone), float((dx[N - 1:] - alone).abs().max())
    return dx


@pytest.mark.parametrize("mode", [BF16X6, F16])
@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("H", [2, 3, 4])
def test_reflect3_tiny_grids(H, W, mode):
    _check(2, 16, 64, H, W, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [32, 33, 34])
def test_reflect3_column_tile_edges(W, mode):
    _check(2 if W == 33 else 1, 32, 64, 6, W, mode, masked=W == 33)


@pytest.mark.parametrize("mode", [BF16X6, F16])
@pytest.mark.parametrize("Cin", [64, 128, 192, 256])
@pytest.mark.parametrize("H", [5, 8, 9, 10, 17])
def test_reflect3_row_tile_edges(H, Cin, mode):
    _check(2, 16, Cin, H, 9, mode, masked=H == 9)


@pytest.mark.parametrize("mode", [BF16X3, BF16])
@pytest.mark.parametrize("Cin", [128, 192, 256])
def test_reflect3_block_shapes_other_modes(Cin, mode):
    _check(1, 16, Cin, 10, 34, mode)


def test_reflect3_image_in_batch_of_three():
    dy = _rand(3, 32, 9, 33, seed=11)
    w = _rand(32, 192, 3, 3, seed=12, scale=0.05)
    m = BF16X6 | KBLOCK | NOSPLIT
    wp = _pack(w, m, transposed=True)
    batch = _exact(dy, wp, 192, m)
    for n in range(3):
        alone = _exact(dy[n:n + 1].contiguous(), wp, 192, m)
        assert torch.equal(batch[n:n + 1], alone), n


@pytest.mark.parametrize("mode", [BF16X6, F16])
@pytest.mark.parametrize("shape", [(2, 64, 3, 3), (1, 64, 6, 33), (2, 192, 9, 9), (1, 128, 17, 9), (1, 256, 8, 34),
                                   (2, 192, 4, 32)])
def test_reflect3_split_k(shape, mode):
    """Six channel blocks (Cout = 96): the plan splits K on these grids; the slices' sums (each with its
    border terms inside) match the unsplit launch within fp32 summation-order rounding."""
    N, Cin, H, W = shape
    Cout = 96
    dy = _rand(N, Cout, H, W, seed=13)
    w = _rand(Cout, Cin, 3, 3, seed=14, scale=0.05)
    mask = _rand(N, Cin, H, W, seed=15) if H == 9 else None
    m = mode | KBLOCK
    assert lib.vst_conv_dgrad_reflect3_workspace(N, Cout, Cin, H, W, m) > 0, "split-K must be on for this case"
    assert lib.vst_conv_dgrad_reflect3_workspace(N, Cout, Cin, H, W, m | NOSPLIT) == 0
    wp = _pack(w, m, transposed=True)
    split = _exact(dy, wp, Cin, m, mask)
    split2 = _exact(dy, wp, Cin, m, mask)
    unsplit = _exact(dy, wp, Cin, m | NOSPLIT, mask)
    nows = _exact(dy, wp, Cin, m, mask, ws=False)  # no workspace: runs unsplit
    torch.cuda.synchronize()
    ref = _ref64(dy, w, Cin, mask)
    d, err = _rel(split, unsplit), _rel(split, ref)
    print(f"reflect3 split N{N} Cin{Cin} {H}x{W} mode {mode}: vs unsplit {d:.3e}, vs fp64 {err:.3e}")
    assert not torch.isnan(split).any()
    if mask is not None:
        assert torch.equal(split[~(mask > 0)], torch.zeros_like(split[~(mask > 0)]))
    assert d < 1e-5, d
    assert err < TOL[mode], err
    assert torch.equal(split, split2)
    assert torch.equal(nows, unsplit)


def test_reflect3_plan_says_no():
    """Where the halo form does not apply the query says so, the entry refuses, and ops.conv_dgrad still
    returns the gradient through the padded-grid path."""
    from vst import ops

    q = lib.vst_conv_dgrad_reflect3_workspace
    m = BF16X6 | KBLOCK
    assert q(2, 32, 192, 8, 40, m) >= 0
    assert q(2, 32, 96, 8, 40, m) == -1          # a 96-row pack: the 128-row M tile does not divide it
    assert q(2, 32, 192, 8, 40, KBLOCK) == -1    # strict fp32
    assert q(2, 32, 192, 8, 40, m | PERTAP) == -1
    assert q(2, 32, 192, 8, 40, BF16X6) == -1    # no channel-blocked K order
    assert q(2, 24, 192, 8, 40, m) == -1         # Cout % 16
    assert q(2, 32, 192, 1, 40, m) == -1 and q(2, 32, 192, 8, 1, m) == -1
    N, Cout, Cin, H, W = 2, 32, 96, 9, 33
    dy = _rand(N, Cout, H, W, seed=16)
    w = _rand(Cout, Cin, 3, 3, seed=17, scale=0.05)
    wp = _pack(w, m, transposed=True)
    dx = torch.zeros(N, Cin, H, W, device=DEV)
    with pytest.raises(VstError):
        lib.vst_conv_dgrad_reflect3(dy.data_ptr(), wp.data_ptr(), None, dx.data_ptr(), N, Cout, Cin, H, W, None, 0, m,
                                    torch.cuda.current_stream().cuda_stream)
    old = ops.POLICY_NAME[0] or ops.DEFAULT_POLICY
    ops.use_policy("bf16x6")
    try:
        got = ops.conv_dgrad(dy, w, (N, Cin, H, W), 3, 1, 1, "reflect", 1)
    finally:
        ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)
    err = _rel(got, _ref64(dy, w, Cin))
    assert err < TOL[BF16X6], err


_CHILD = r"""
import sys
import torch
sys.path[:0] = [{repo!r}, {pkg!r}]
sys.path.insert(0, {tests!r})
import test_gpu_dgrad_reflect as T
from vst import ops
assert not ops.DGRAD_EXACT
ops.use_policy("bf16x6")
N, Cout, Cin, H, W = 2, 96, 192, 9, 33
dy = T._rand(N, Cout, H, W, seed=18)
w = T._rand(Cout, Cin, 3, 3, seed=19, scale=0.05)
mask = T._rand(N, Cin, H, W, seed=20)
for mk in (None, mask):
    got = ops.conv_dgrad(dy, w, (N, Cin, H, W), 3, 1, 1, "reflect", 1, dmask=mk)
    m = T.BF16X6 | T.KBLOCK
    old = T._padout(dy, T._pack(w, m, transposed=True), Cin, m, mk)
    torch.cuda.synchronize()
    assert torch.equal(got, old)
print("child ok")
"""


def test_reflect3_python_route():
    """ops.conv_dgrad takes the exact-grid path and equals the direct library call bitwise (split-K as
    the plan says, masked and not); with VST_DGRAD_EXACT=0 (a child process) it equals the old path."""
    from vst import ops

    N, Cout, Cin, H, W = 2, 96, 192, 9, 33
    dy = _rand(N, Cout, H, W, seed=18)
    w = _rand(Cout, Cin, 3, 3, seed=19, scale=0.05)
    mask = _rand(N, Cin, H, W, seed=20)
    old = ops.POLICY_NAME[0] or ops.DEFAULT_POLICY
    ops.use_policy("bf16x6")
    try:
        assert ops.DGRAD_EXACT
        for mk in (None, mask):
            got = ops.conv_dgrad(dy, w, (N, Cin, H, W), 3, 1, 1, "reflect", 1, dmask=mk)
            m = BF16X6 | KBLOCK
            direct = _exact(dy, _pack(w, m, transposed=True), Cin, m, mk)
            torch.cuda.synchronize()
            assert torch.equal(got, direct)
            assert _rel(got, _ref64(dy, w, Cin, mk)) < TOL[BF16X6]
    finally:
        ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)
    tests = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests)
    code = _CHILD.format(repo=repo, pkg=os.path.join(repo, "video-style-transfer_amd"), tests=tests)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VST_DGRAD_EXACT="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr

"""The row-tiled weight gradient (`wgrad2_kernel`, csrc/wgrad_gemm.hip) with its software-pipelined k loop:
every block shape the dispatch can select, 1 / 2 / 3 / 4 / 5 / 7 k-tiles per block (one tile: only the
past-the-end load / store path runs), border / mixed / interior gather windows, ragged M and J, several
split-K chunks with a short last one, stride 2, the 9x9 first conv, the nearest-x2 / row-split / Gram
entry points (the non-S1 instantiations) and the two-tiles-per-stage single-product modes -- against
float64, against itself (determinism, accumulate) and, bitwise, against the digests recorded with the
kernel before the loop was pipelined (tools/wgrad_digest.py holds the cases and the recipe; the k-tile
order, the MFMA sequence, the split arithmetic and the slab order did not change, so every bit stays).
VST_GEMM_PERTAP is set in every call's mode: the row-tiled kernel runs whatever the policy would pick."""
import importlib.util
import json
import os

import pytest
import torch

from vst._lib import lib

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("wgrad_digest", os.path.join(os.path.dirname(_HERE), "tools",
                                                                            "wgrad_digest.py"))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

# max |err| / max |dW| vs float64: test_gpu_wgrad_halo.py's TOL; bf16x3 from test_gpu_halo.py's TOL and
# f32 from test_gpu_parity.py's CONV_TOL
TOL = {D.BF16X6: 5e-6, D.F16: 3e-3, D.BF16: 2e-2, D.BF16X3: 1e-4, D.F32: 1e-4}
CASES = D.cases()
DIGESTS = json.load(open(os.path.join(_HERE, "golden", "wgrad_pipe_digests.json")))["digests"]


def _ref(c, dy, x):
    """float64 on the CPU: conv2d_weight on the padded input (as test_gpu_wgrad_halo._ref)."""
    F = torch.nn.functional
    if c["kind"] == "gram":
        f = x.cpu().double()
        return 0.25 * f @ f.transpose(1, 2)
    x64, dy, K = x.cpu().double(), dy.cpu(), c.get("K", 3)
    if c["kind"] == "up2":
        x64 = F.interpolate(x64, scale_factor=2, mode="nearest")
    p = K // 2
    reflect = c["kind"] != "conv" or c["gmode"] == 0
    xp = F.pad(x64, (p, p, p, p), mode="reflect" if reflect else "constant")
    return torch.nn.grad.conv2d_weight(xp, (dy.shape[1], x.shape[1], K, K), dy.double(), stride=c.get("stride", 1))


@pytest.fixture(scope="module")
def results():
    """Every case once: (first call, second call, float64 reference), computed on first use and shared."""
    cache = {}

    def get(c):
        k = D.case_id(c)
        if k not in cache:
            dy, x = D.inputs(c)
            a = D.run(lib, c, dy, x)
            b = D.run(lib, c, dy, x)
            torch.cuda.synchronize()
            cache[k] = (a, b, _ref(c, dy, x))
        return cache[k]

    return get


def test_case_list_reaches_every_block_and_tile_count():
    """The block named next to each conv case is the one wgrad_gemm.hip's dispatch selects (wsel /
    run_wg, restated here), all eight are reached, and the cases that claim a k-tile count per block get
    it from the split-K planner (through the workspace query: floats = N * S * Mpad * Jpad)."""
    seen = set()
    for c in D.CONV:
        M, J = c["Cout"], c["K"] * c["K"] * c["Cin"]
        Jpad = (J + 127) // 128 * 128
        if M <= 32:
            blk, bm = "W32", 32
        elif M <= 64:
            blk, bm = "W64", 64
        elif M <= 96:
            blk, bm = "W96", 96
        elif M % 192 == 0 and M % 128 != 0:
            blk, bm = "W192", 192
        else:
            blk, bm = "W128", 128
        if blk in ("W64", "W96") and J > 128 and Jpad % 256 == 0:
            blk += "N"
        if blk == "W64" and J <= 64:
            blk = "W64H"
        assert blk == c["block"], c
        seen.add(blk)
        if "tiles" in c:
            HWo, Mpad = c["H"] * c["W"], (M + bm - 1) // bm * bm
            S = lib.vst_wgrad_workspace(c["N"], M, J, HWo) // (c["N"] * Mpad * Jpad)
            chunk = ((HWo + S - 1) // S + 15) // 16 * 16
            assert chunk // 16 == c["tiles"] and HWo % chunk == 0, (c, S)
    assert seen == {"W32", "W64", "W96", "W128", "W192", "W64N", "W96N", "W64H"}
    assert sorted(DIGESTS) == sorted(D.case_id(c) for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=D.case_id)
def test_wgrad_pipe_vs_fp64_deterministic_and_parent_bits(c, results):
    a, b, ref = results(c)
    assert torch.isfinite(a).all()
    err = float((a.cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print(D.case_id(c), "err", err)
    assert err < TOL[c["mode"]], err
    assert torch.equal(a, b)  # fixed slab order: bitwise reproducible
    assert D.digest(a) == DIGESTS[D.case_id(c)]  # ... and bitwise what the un-pipelined loop computed


@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] != "gram" and c["mode"] == D.BF16X6], ids=D.case_id)
def test_wgrad_pipe_accumulate(c, results):
    plain = results(c)[0]
    g = torch.Generator().manual_seed(5)
    base = torch.randn(*plain.shape, generator=g).to(D.DEV)
    dy, x = D.inputs(c)
    acc = D.run(lib, c, dy, x, out=base.clone())
    torch.cuda.synchronize()
    assert float((acc - (plain + base)).abs().max()) <= 1e-6 * float(acc.abs().max())

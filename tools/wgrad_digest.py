#!/usr/bin/env python
"""The row-tiled weight gradient's bitwise record: the cases of tests/test_gpu_wgrad_pipe.py (raw C ABI,
VST_GEMM_PERTAP in the mode so `wgrad2_kernel` runs whatever the policy would pick), their seeded
CPU-generator inputs, and a sha256 of each result's bytes.

    python tools/wgrad_digest.py --write tests/golden/wgrad_pipe_digests.json    # record (on a GPU)
    python tools/wgrad_digest.py --check tests/golden/wgrad_pipe_digests.json    # compare

The committed digests were recorded with the library built from the commit before the k loop was
software-pipelined: a change of the kernel that keeps the k-tile order, the per-k-tile MFMA sequence, the
split arithmetic and the slab order reproduces every one of them.  A digest that differs means one of
those moved -- fix the kernel, do not re-record."""
import argparse
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "video-style-transfer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = "cuda"
F32, BF16X3, BF16, BF16X6, F16, PERTAP = 0, 1, 2, 3, 4, 32
MODE_NAME = {F32: "f32", BF16X3: "bf16x3", BF16: "bf16", BF16X6: "bf16x6", F16: "f16"}

# ---- cases ------------------------------------------------------------------------------------------
# conv: (N, Cin, H, W, Cout, K, gmode, stride).  H, W are the OUTPUT grid; the source is stride times
# that.  gmode 0 reflect, 1 zero.  The block `wgrad2_kernel` runs on follows from M = Cout and
# J = K*K*Cin (wgrad_gemm.hip wsel / run_wg); `block` names it and the test checks the name against
# the same rule, so the list below provably reaches every block shape the dispatch can select.
#   W32   Cout <= 32                     W64H  Cout <= 64,  J <= 64
#   W64   Cout <= 64                     W64N  Cout <= 64,  128 < J, Jpad % 256 == 0
#   W96   Cout <= 96                     W96N  Cout <= 96,  128 < J, Jpad % 256 == 0
#   W192  Cout % 192 == 0, % 128 != 0    W128  everything else
CONV = [
    # tiles per block 1 (only the past-the-end load/store path runs) and 2; width 16: every window on a border
    # (one row: zero gather -- a reflect pad of 1 needs two rows)
    dict(N=1, Cin=3, H=1, W=16, Cout=32, gmode=1, block="W32"),
    dict(N=3, Cin=7, H=1, W=16, Cout=64, gmode=1, block="W64H"),
    dict(N=1, Cin=96, H=1, W=16, Cout=192, gmode=1, block="W192"),
    dict(N=1, Cin=16, H=2, W=16, Cout=128, block="W128"),
    dict(N=3, Cin=96, H=2, W=16, Cout=192, block="W192"),
    dict(N=1, Cin=7, H=2, W=16, Cout=48, block="W64H"),     # ragged M, J = 63
    # 3 x 16: two chunks, 2 + 1 tiles
    dict(N=1, Cin=16, H=3, W=16, Cout=64, block="W64N"),    # J = 144 (not a multiple of 128)
    dict(N=1, Cin=24, H=3, W=16, Cout=96, block="W96N"),    # J = 216
    dict(N=3, Cin=24, H=3, W=16, Cout=192, block="W192"),
    # width 32 (border and mixed windows) and 48 (mostly interior)
    dict(N=1, Cin=96, H=7, W=32, Cout=64, block="W64"),     # J = 864, Jpad 896
    dict(N=1, Cin=96, H=7, W=32, Cout=96, block="W96"),
    dict(N=3, Cin=96, H=7, W=32, Cout=192, block="W192"),
    dict(N=1, Cin=96, H=7, W=32, Cout=48, block="W64"),     # ragged M
    dict(N=1, Cin=3, H=5, W=48, Cout=32, block="W32"),
    dict(N=1, Cin=16, H=5, W=48, Cout=128, block="W128"),
    dict(N=3, Cin=7, H=5, W=48, Cout=96, block="W96"),      # J = 63 on a 96-row tile
    dict(N=1, Cin=24, H=5, W=48, Cout=192, block="W192"),
    dict(N=1, Cin=96, H=5, W=48, Cout=192, gmode=1, block="W192"),
    dict(N=1, Cin=16, H=7, W=32, Cout=64, gmode=1, block="W64N"),
    dict(N=3, Cin=3, H=3, W=16, Cout=32, gmode=1, block="W32"),
    # tall: split-K gives several chunks with a short last one
    dict(N=1, Cin=32, H=70, W=16, Cout=64, block="W64"),    # J = 288, Jpad 384
    # 3, 4, 5 and 7 k-tiles per block: 64 chunks (the planner's cap) over 64-pixel rows
    dict(N=1, Cin=3, H=48, W=64, Cout=32, block="W32", tiles=3),
    dict(N=1, Cin=7, H=64, W=64, Cout=64, block="W64H", tiles=4),
    dict(N=1, Cin=16, H=80, W=64, Cout=192, block="W192", tiles=5),
    dict(N=1, Cin=16, H=112, W=64, Cout=128, gmode=1, block="W128", tiles=7),
    # stride 2 (conv2-like, Cin 16 -> Cout 32 on an 8 x 32 input) and the 9 x 9 conv1-like case
    dict(N=1, Cin=16, H=4, W=16, Cout=32, stride=2, block="W32"),
    dict(N=3, Cin=16, H=4, W=16, Cout=32, stride=2, gmode=1, block="W32"),
    dict(N=1, Cin=3, H=12, W=32, Cout=48, K=9, block="W64N"),  # J = 243, Jpad 256
]
for _c in CONV:
    _c.setdefault("K", 3)
    _c.setdefault("gmode", 0)
    _c.setdefault("stride", 1)
    _c["kind"] = "conv"
# the non-S1 instantiations and the Gram matrix, once each at their smallest legal shape
OTHER = [
    dict(kind="up2", N=1, Cin=8, H=2, W=15, Cout=8),        # nearest-x2 phase GEMM: M = 32, 3 x 16 grid
    dict(kind="rowsplit", N=1, Cin=8, H=5, W=16, Cout=3, K=9),  # M = 27 rows (co, kh), 13 x 16 grid
    dict(kind="gram", N=1, C=64, HW=48),                     # J = 64: the 64 x 64 block
    dict(kind="gram", N=3, C=96, HW=16),
]
# the KD = 2 paths (bf16, f16: two k-tiles per stage) and the other arithmetic modes: stages 1 (one and
# two tiles), 2 (three and four tiles), odd tile counts (a short last stage), and a stride-2 gather
SUBSET = [CONV[0], CONV[4], CONV[9], CONV[21], CONV[23], CONV[25]]


def cases():
    out = []
    for c in CONV + OTHER:
        out.append(dict(c, mode=BF16X6))
    for m in (F32, BF16X3, BF16, F16):
        for c in SUBSET:
            out.append(dict(c, mode=m))
    return out


def case_id(c):
    m = MODE_NAME[c["mode"]]
    if c["kind"] == "conv":
        return (f"conv-n{c['N']}-ci{c['Cin']}-{c['H']}x{c['W']}-co{c['Cout']}-k{c['K']}-g{c['gmode']}"
                f"-s{c['stride']}-{m}")
    if c["kind"] == "gram":
        return f"gram-n{c['N']}-c{c['C']}-hw{c['HW']}-{m}"
    return f"{c['kind']}-n{c['N']}-ci{c['Cin']}-{c['H']}x{c['W']}-co{c['Cout']}-{m}"


def _rand(shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def inputs(c):
    """(dy, x) of a case (x alone for a Gram matrix): CPU generator, fixed seeds."""
    if c["kind"] == "gram":
        return None, _rand((c["N"], c["C"], c["HW"]), 31, 1.0)
    N, Cin, H, W, Cout = c["N"], c["Cin"], c["H"], c["W"], c["Cout"]
    if c["kind"] == "up2":
        return _rand((N, Cout, 2 * H, 2 * W), 2, 0.5), _rand((N, Cin, H, W), 1, 2.0)
    s = c.get("stride", 1)
    return _rand((N, Cout, H, W), 2, 0.5), _rand((N, Cin, H * s, W * s), 1, 2.0)


def run(lib, c, dy, x, out=None):
    """One call of the case through the C ABI; out given: accumulate onto it."""
    st = torch.cuda.current_stream().cuda_stream
    acc = int(out is not None)
    mode = c["mode"] | PERTAP
    if c["kind"] == "gram":
        N, C, HW = c["N"], c["C"], c["HW"]
        ws = torch.empty(lib.vst_wgrad_workspace(N, C, C, HW), device=DEV)
        g = torch.full((N, C, C), float("nan"), device=DEV)
        assert lib.vst_gram(x.data_ptr(), g.data_ptr(), ws.data_ptr(), N, C, HW, 0.25, mode, st) == 0
        return g
    N, Cin, H, W, Cout = c["N"], c["Cin"], c["H"], c["W"], c["Cout"]
    K = c.get("K", 3)
    dw = torch.full((Cout, Cin, K, K), float("nan"), device=DEV) if out is None else out
    if c["kind"] == "up2":
        ws = torch.empty(lib.vst_conv_wgrad_up2_workspace(N, Cin, H, W, Cout), device=DEV)
        assert lib.vst_conv_wgrad_up2(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, Cin, H, W, Cout,
                                      acc, mode, st) == 0
    elif c["kind"] == "rowsplit":
        ws = torch.empty(lib.vst_wgrad_workspace(N, Cout * K, K * Cin, (H + K - 1) * W), device=DEV)
        assert lib.vst_conv_wgrad_rowsplit(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, Cin, H, W,
                                           Cout, K, acc, mode, st) == 0
    else:
        s, g = c["stride"], c["gmode"]
        nf = lib.vst_conv_wgrad_workspace(N, Cin, H * s, W * s, Cout, H, W, K, K, g, s, K // 2, 1, mode)
        assert nf > 0
        ws = torch.empty(nf, device=DEV)
        assert lib.vst_conv_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), nf, N, Cin, H * s, W * s,
                                  Cout, H, W, K, K, g, s, K // 2, 1, acc, mode, st) == 0
    return dw


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def all_digests(lib):
    out = {}
    for c in cases():
        dy, x = inputs(c)
        r = run(lib, c, dy, x)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(r).all()), case_id(c)
        out[case_id(c)] = digest(r)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", help="record the digests of the loaded library into this JSON file")
    ap.add_argument("--check", help="compare the loaded library's digests with this JSON file")
    a = ap.parse_args()
    from vst._lib import lib

    got = all_digests(lib)
    if a.write:
        with open(a.write, "w") as f:
            json.dump({"build_id": lib.build_id, "digests": got}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"{len(got)} digests written to {a.write} (library {lib.build_id})")
    if a.check:
        want = json.load(open(a.check))["digests"]
        bad = [k for k in want if got.get(k) != want[k]]
        print(f"{len(want) - len(bad)} of {len(want)} digests reproduced" + (": differ " + ", ".join(bad) if bad else ""))
        return 1 if bad or set(want) != set(got) else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())

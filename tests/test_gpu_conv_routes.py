"""The dispatch behind vst.ops' route functions: for every route of every kind, at the smallest geometry
the route function returns it for, one conv forward + backward is run under a recorder of the library
calls.  The entry points called are the ones the route names, and every weight pack is made in the mode
of the launch that reads it.  No numeric assertion: the parity and bitwise tests keep theirs."""
import pytest
import torch

from vst import _lib, ops

pytestmark = pytest.mark.gpu

# the entry point only this route calls (None: the plain conv GEMM, i.e. none of the others')
FWD = {"rowsplit": "vst_rowsplit_reduce", "cin3": "vst_conv_cin3_k3", "up2": "vst_conv_up2_fwd", "kwu": "vst_unfold_kw",
       "gemm": None}
DGRAD = {"tapsum": "vst_tapsum", "thin": "vst_conv_dgrad_thin", "zero": None, "phase2": "vst_conv_dgrad_s2",
         "padout_kwu": "vst_conv_dgrad_padout_kwu", "reflect3": "vst_conv_dgrad_reflect3",
         "padout": "vst_conv_dgrad_padout", "ring": "vst_dgrad_ring", "fold": "vst_fold_reflect"}
WGRAD = {"up2": "vst_conv_wgrad_up2", "rowsplit": "vst_conv_wgrad_rowsplit", "gemm": "vst_conv_wgrad"}
PACKS = ("vst_pack_weight", "vst_pack_weight_kwu", "vst_pack_weight_phase2", "vst_pack_weight_upsum")
LAUNCHES = ("vst_conv_gemm_padx", "vst_conv_up2_fwd", "vst_conv_dgrad_s2", "vst_conv_dgrad_padout",
            "vst_conv_dgrad_padout_kwu", "vst_conv_dgrad_reflect3")

# policy, Cin, Cout, ks, H, W, stride, pad, pad_mode, up, act, x is a ReLU output (mask_dx), the routes
CASES = [
    ("f32", 16, 16, 3, 8, 16, 1, 1, "reflect", 1, None, False, ("gemm", "padout", "gemm")),
    ("bf16x6", 64, 16, 3, 8, 16, 1, 1, "reflect", 1, "relu", True, ("gemm", "reflect3", "rowsplit")),
    ("f32", 16, 3, 9, 16, 16, 1, 4, "reflect", 1, "tanh", False, ("rowsplit", "padout_kwu", "rowsplit")),
    ("f32", 3, 16, 9, 16, 16, 1, 4, "reflect", 1, None, False, ("kwu", "padout", "gemm")),
    ("f32", 3, 16, 3, 8, 16, 1, 1, "zero", 1, "relu", False, ("cin3", "tapsum", "gemm")),
    ("f32", 16, 16, 3, 8, 16, 1, 1, "zero", 1, "relu", True, ("gemm", "zero", "gemm")),
    ("f32", 16, 16, 3, 8, 16, 1, 1, "reflect", 2, None, False, ("up2", "ring", "up2")),
    ("f32", 16, 16, 3, 8, 16, 2, 1, "reflect", 1, None, False, ("gemm", "phase2", "gemm")),
    ("f32", 16, 3, 3, 8, 16, 1, 1, "reflect", 1, None, True, ("rowsplit", "thin", "gemm")),
    ("f32", 16, 16, 1, 8, 16, 1, 0, "reflect", 1, None, False, ("gemm", "fold", "gemm")),
    # a one-row plane with <= 4 outputs: the thin kernels need two rows, so the library's answer keeps it off them
    ("f32", 16, 3, 3, 1, 16, 1, 1, "zero", 1, None, False, ("gemm", "zero", "gemm")),
]


@pytest.fixture
def recorder(monkeypatch):
    """Every library call as (entry name, arguments), in issue order."""
    calls = []

    def getattr_(self, name):
        fn = getattr(self.load(), name)

        def call(*args):
            calls.append((name, args))
            rc = fn(*args)
            if fn.restype is _lib.ctypes.c_int and rc != 0:
                raise _lib.VstError(f"{name} failed (rc={rc})")
            return rc

        return call

    monkeypatch.setattr(_lib._Lib, "__getattr__", getattr_)
    return calls


def test_cases_cover_every_route():
    for i, table in enumerate((FWD, DGRAD, WGRAD)):
        assert {c[-1][i] for c in CASES} == set(table)
    assert set(FWD) == set(ops._FWD) and set(DGRAD) == set(ops._DGRAD)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(c[-1] + (("onerow",) if c[4] == 1 else ())))
def test_dispatch_follows_route(case, recorder):
    policy, Cin, Cout, ks, H, W, stride, pad, pad_mode, up, act, masked, want = case
    ops.gemm_role("fwd")  # (applies the environment's policy first, so it is the one restored)
    old = ops.POLICY_NAME[0]
    ops.use_policy(policy)
    try:
        Ho, Wo = ops.conv_out_hw(H, W, ks, stride, pad, up)
        dmode, wmode = ops.gemm_role("dgrad"), ops.gemm_role("wgrad")
        assert ops.conv_fwd_route(Cin, Cout, H, W, ks, stride, pad, pad_mode, up, act) == want[0]
        assert ops.conv_dgrad_route(1, Cin, Cout, H, W, Ho, Wo, ks, (ks, ks), stride, pad, pad_mode, up, masked,
                                    dmode)[0] == want[1]
        assert ops.conv_wgrad_route(Cin, Cout, W, ks, stride, pad, pad_mode, up, wmode, H=H)[0] == want[2]
        g = torch.Generator().manual_seed(5)
        x = torch.randn(1, Cin, H, W, generator=g).relu_().cuda().requires_grad_(True)
        w = (torch.randn(Cout, Cin, ks, ks, generator=g) * 0.1).cuda().requires_grad_(True)
        y = ops.conv2d(x, w, None, stride, pad, pad_mode, up, act, mask_dx=masked)
        n_fwd = len(recorder)
        y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
    finally:
        ops.use_policy(old if old in ops.POLICIES else ops.DEFAULT_POLICY)
    fwd, bwd = [n for n, _ in recorder[:n_fwd]], [n for n, _ in recorder[n_fwd:]]
    for table, route, names in ((FWD, want[0], fwd), (DGRAD, want[1], bwd), (WGRAD, want[2], bwd)):
        for r, entry in table.items():
            if entry is not None:
                assert (entry in names) == (r == route), (r, route, names)
    assert "vst_conv_gemm_padx" in fwd or want[0] in ("cin3", "up2")
    # a pack is read by the next launch: same mode (a launch may add the PERTAP kernel choice to it)
    pending = None
    for name, args in recorder:
        if name in PACKS:
            assert pending is None, f"{pending} packed and never launched"
            pending = (name, args[-2])
        elif name in LAUNCHES:
            if pending is not None:
                assert args[-2] & ~ops.PERTAP == pending[1], (pending, name, args[-2])
            pending = None
    assert pending is None

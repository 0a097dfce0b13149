"""CPU checks of the class-balanced box-map loss: the fp64 reference of tests/_box_loss_ref.py against torch and against the closed-form
gradient of include/dd_hotpath.h, the hparams / command-line surface (spatial.box_loss_config), and the refusals of the three entry points
of csrc/box_loss.hip (no GPU: nothing is launched here).  The GPU tests (test_gpu_box_loss.py) then hold the kernels to the reference."""
import ctypes
from argparse import ArgumentParser, Namespace

import pytest
import torch
import torch.nn.functional as F

import _box_loss_ref as ref


def ragged_inputs():
    """B = 3, P = 1028: sample 1 has an empty target, sample 2 is all ones."""
    return ref.inputs(3, 1028, salt=1, empty=(1,), full=(2,))


# ------------------------------------------------------------------------------------------------ 1. the BCE term is torch's weighted BCE
@pytest.mark.parametrize("pos_weight", [None, 7.5, "auto"])
def test_reference_bce_is_torchs_weighted_bce(pos_weight):
    p, t = ragged_inputs()
    p, t = p.double(), t.double()
    w = ref.weights(t, pos_weight)
    want = F.binary_cross_entropy(p, t, weight=1 + (w - 1) * t)
    l_bce, _ = ref.terms(p, t, pos_weight)
    assert abs(float(l_bce) - float(want)) <= 1e-12 * abs(float(want))
    if pos_weight == "auto":
        assert w.flatten().tolist() == [(1028 - float(t[0].sum())) / float(t[0].sum()), 1028.0, 0.0]


# ------------------------------------------------------------------------------------------------ 2. closed form == autograd
@pytest.mark.parametrize("eps", [1.0, 0.0])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)])
@pytest.mark.parametrize("pos_weight", [None, 7.5, "auto"])
def test_closed_form_gradient_is_autograds(pos_weight, alpha, beta, eps):
    p, t = ragged_inputs()
    _, _, _, auto = ref.loss_and_grad(p, t, pos_weight, alpha, beta, eps)
    closed = ref.closed_form_grad(p, t, pos_weight, alpha, beta, eps)
    assert float((auto - closed).abs().max()) <= 1e-12 * float(closed.abs().max())


def test_reference_at_the_clamps():
    p, t = ref.inputs(2, 1028, salt=2)
    p[0, :4] = torch.tensor([0.0, 0.0, 1.0, 1.0])
    t[0, :4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    total, l_bce, _, g = ref.loss_and_grad(p, t, 7.5, 1.0, 0.0)
    assert torch.isfinite(total) and torch.isfinite(g).all()
    want = F.binary_cross_entropy(p.double(), t.double(), weight=1 + 6.5 * t.double())      # torch clamps at -100 too
    assert abs(float(l_bce) - float(want)) <= 1e-12 * float(want)
    # p = 0: the log p term has no slope, the other gives (1 - t) / (1 - 0); p = 1 likewise
    scale = 1.0 / (2 * 1028)
    assert g[0, :4].tolist() == pytest.approx([scale, 0.0, 0.0, -7.5 * scale], abs=1e-18)
    closed = ref.closed_form_grad(p, t, 7.5, 1.0, 0.0)
    assert float((g - closed).abs().max()) <= 1e-12 * float(closed.abs().max())


# ------------------------------------------------------------------------------------------------ 3. hparams
def test_box_loss_config():
    from driving_dirty_amd.spatial import box_loss_config
    assert box_loss_config(Namespace()) is None
    assert box_loss_config(Namespace(box_pos_weight=None, box_bce_weight=1.0, box_ts_weight=0.0, box_ts_eps=1.0, mse_loss=True)) is None
    assert box_loss_config(Namespace(box_pos_weight="auto")) == {"pos_weight": "auto", "bce_weight": 1.0, "ts_weight": 0.0, "ts_eps": 1.0}
    assert box_loss_config(Namespace(box_pos_weight="3.5"))["pos_weight"] == 3.5
    got = box_loss_config(Namespace(box_pos_weight=2, box_ts_weight=0.5, box_ts_eps=0))
    assert got == {"pos_weight": 2.0, "bce_weight": 1.0, "ts_weight": 0.5, "ts_eps": 0.0} and isinstance(got["pos_weight"], float)
    assert box_loss_config(Namespace(box_ts_weight=1.0)) == {"pos_weight": None, "bce_weight": 1.0, "ts_weight": 1.0, "ts_eps": 1.0}
    assert box_loss_config(Namespace(box_bce_weight=0.5))["bce_weight"] == 0.5
    for bad in (0, -1, "car", "-2", float("nan"), float("inf")):
        with pytest.raises(ValueError, match="box_pos_weight"):
            box_loss_config(Namespace(box_pos_weight=bad))
    with pytest.raises(ValueError, match="box_ts_eps"):
        box_loss_config(Namespace(box_ts_eps=-1))
    with pytest.raises(ValueError, match="box_ts_eps"):
        box_loss_config(Namespace(box_pos_weight="auto", box_ts_eps=-1))
    with pytest.raises(ValueError, match="box_ts_weight"):
        box_loss_config(Namespace(box_ts_weight=-0.5))
    with pytest.raises(ValueError, match="box_bce_weight"):
        box_loss_config(Namespace(box_bce_weight=-1))
    with pytest.raises(ValueError, match="constant"):
        box_loss_config(Namespace(box_bce_weight=0))
    for on in ({"box_pos_weight": "auto"}, {"box_pos_weight": 2.0}, {"box_ts_weight": 1.0}, {"box_bce_weight": 0.5}):
        with pytest.raises(ValueError, match="mse_loss"):
            box_loss_config(Namespace(mse_loss=True, **on))


def test_a_bad_value_fails_when_the_module_is_built():
    from driving_dirty_amd.autoencoder import BasicAE
    from driving_dirty_amd.joint import JointRoadMapBBox
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    for cls in (BBSpatialRoadMap, JointRoadMapBBox):
        base = dict(pretrained_ae=BasicAE(Namespace(hidden_dim=16, latent_dim=8)), unfreeze_epoch_no=5, learning_rate=1e-3, output_img_freq=500)
        assert cls(Namespace(**base)).box_loss is None
        assert cls(Namespace(box_pos_weight="auto", box_ts_weight=1.0, **base)).box_loss == {"pos_weight": "auto", "bce_weight": 1.0, "ts_weight": 1.0,
                                                                                               "ts_eps": 1.0}
        with pytest.raises(ValueError, match="box_pos_weight"):
            cls(Namespace(box_pos_weight="car", **base))


# ------------------------------------------------------------------------------------------------ 4. command line
def test_command_line_flags_default_to_off():
    from driving_dirty_amd.spatial import BBSpatialRoadMap, box_loss_config
    parser = BBSpatialRoadMap.add_model_specific_args(ArgumentParser(add_help=False))
    args = parser.parse_args([])
    assert (args.box_pos_weight, args.box_bce_weight, args.box_ts_weight, args.box_ts_eps) == (None, 1.0, 0.0, 1.0)
    assert box_loss_config(args) is None
    args = parser.parse_args(["--box_pos_weight", "auto", "--box_ts_weight", "1", "--box_ts_eps", "0.5", "--box_bce_weight", "2"])
    assert box_loss_config(args) == {"pos_weight": "auto", "bce_weight": 2.0, "ts_weight": 1.0, "ts_eps": 0.5}
    assert box_loss_config(parser.parse_args(["--box_pos_weight", "3.5"]))["pos_weight"] == 3.5


# ------------------------------------------------------------------------------------------------ 5. the ABI without a GPU
def test_entry_points_are_exported_and_refuse_on_the_host():
    from driving_dirty_amd import _lib
    from driving_dirty_amd.build import LIB
    handle = ctypes.CDLL(LIB)
    for name in ("dd_box_loss_workspace_bytes", "dd_box_loss_fwd", "dd_box_loss_bwd"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.dd_box_loss_workspace_bytes(2) >= 2 * 5 * 8 and lib.dd_box_loss_workspace_bytes(2) % 8 == 0
    assert lib.dd_box_loss_workspace_bytes(0) == -1
    UNSUPPORTED, BAD_ARG = 1, 2
    # aligned addresses that are never read: every call below is refused by the host-side validation, before any device call
    # (DD_ERR_LAUNCH = 3 would mean that one got as far as a launch)
    a = ctypes.c_void_p(1 << 20)
    good = dict(probs=a, target=a, dtype=0, batch=2, per=1028, pw=1.0, alpha=1.0, beta=0.0, eps=1.0, loss=a, stats=a, coef=a, ws=a)

    def fwd(**change):
        k = dict(good, **change)
        return lib.dd_box_loss_fwd(k["probs"], k["target"], k["dtype"], k["batch"], k["per"], k["pw"], k["alpha"], k["beta"], k["eps"], k["loss"],
                                   k["stats"], k["coef"], k["ws"], None)

    assert fwd(per=6) == UNSUPPORTED and b"multiple of 4" in lib.dd_last_error()
    assert fwd(dtype=2) == UNSUPPORTED
    for change in (dict(batch=0), dict(pw=0.0), dict(pw=-2.0), dict(pw=float("nan")), dict(eps=-1.0), dict(alpha=-1.0), dict(beta=-0.5), dict(probs=None),
                   dict(target=None), dict(loss=None), dict(stats=None), dict(coef=None), dict(ws=None), dict(per=0),
                   dict(probs=ctypes.c_void_p((1 << 20) + 4)), dict(target=ctypes.c_void_p((1 << 20) + 4)), dict(coef=ctypes.c_void_p((1 << 20) + 8))):
        assert fwd(**change) == BAD_ARG, change
    assert b"box_loss_fwd" in lib.dd_last_error()
    # a byte target needs 4-byte alignment only; the automatic weight's sentinel is no error by itself (the NULL pointer is)
    assert fwd(dtype=1, target=ctypes.c_void_p((1 << 20) + 2)) == BAD_ARG
    assert fwd(pw=-1.0, ws=None) == BAD_ARG and b"NULL" in lib.dd_last_error()

    def bwd(probs=a, target=a, dtype=0, batch=2, per=1028, coef=a, dprobs=a):
        return lib.dd_box_loss_bwd(probs, target, dtype, batch, per, coef, 1.0, dprobs, None)

    assert bwd(per=6) == UNSUPPORTED
    for change in (dict(batch=0), dict(probs=None), dict(coef=None), dict(dprobs=None), dict(dprobs=ctypes.c_void_p((1 << 20) + 4))):
        assert bwd(**change) == BAD_ARG, change


def test_python_surface_refuses_on_the_host():
    from driving_dirty_amd import _lib, ops
    with pytest.raises(_lib.HotpathError, match="probs"):
        ops.box_loss(torch.zeros(2, 8), torch.zeros(2, 8))      # CPU tensors: there is no CPU fallback
    with pytest.raises(_lib.HotpathError, match=r"\[B, P\]"):
        ops.box_loss(torch.zeros(16), torch.zeros(16))

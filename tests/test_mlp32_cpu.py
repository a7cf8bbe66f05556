"""Host side of the fused deformation MLP with a 32-feature trunk (csrc/deform_mlp.hip at KT = 1; dnerf/eulerian_150_16: two HexPlane
levels of 16 channels, net_width 64, defor_depth 0): which models Deformation routes to it, the *_n entry points of the C ABI and
what they and ops.DeformMLPFunction refuse.  No GPU needed: every refused call is refused before anything is launched."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

pkg = "iclr2025_3d-mom_amd"
ops = importlib.import_module(pkg + ".ops")
N = importlib.import_module(pkg + "._native")
Deformation = importlib.import_module(pkg + ".scene.deformation").Deformation
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HP16:        # the network of eulerian_150_16 on a small field
    net_width = 64; timebase_pe = 4; defor_depth = 0; posebase_pe = 10; scale_rotation_pe = 2; opacity_pe = 2
    timenet_width = 64; timenet_output = 32; bounds = 1.6; plane_tv_weight = 0.0001; time_smoothness_weight = 0.01
    l1_time_planes = 0.0001
    kplanes_config = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [8, 8, 8, 5]}
    multires = [1, 2]; no_dx = False; no_grid = False; no_ds = False; no_dr = False; no_do = True; no_dshs = True
    empty_voxel = False; grid_pe = 0; static_mlp = False; apply_rotation = False


class HP32(HP16):  # the shipped field: two levels of 32 channels
    kplanes_config = dict(HP16.kplanes_config, output_coordinate_dim=32)


def _net(base, W=64, D=0, **over):
    return Deformation(W=W, D=D, args=type("HPv", (base,), over))


def test_the_two_fields_of_two_levels_take_the_fused_mlp_and_only_the_32_channel_one_the_fused_paths():
    d16, d32 = _net(HP16), _net(HP32)
    assert d16.grid.feat_dim == 32 and len(d16.grid.grids) == 2 and d16.feature_out[0].weight.shape == (64, 32)
    assert d16._mlp_fusable() and not d16._fusable()          # the fused step / autograd / render pool keep declining it
    assert d32.grid.feat_dim == 64 and d32._mlp_fusable() and d32._fusable()


@pytest.mark.parametrize("base", [HP16, HP32])
@pytest.mark.parametrize("what,kw", [("W=128", dict(W=128)), ("D=1", dict(D=1)), ("no_do=False", dict(no_do=False)),
                                     ("static_mlp", dict(static_mlp=True)), ("apply_rotation", dict(apply_rotation=True))])
def test_any_other_network_keeps_its_linear_modules(base, what, kw):
    d = _net(base, **kw)
    assert not d._mlp_fusable() and not d._fusable(), what


def test_four_levels_of_16_channels_keep_their_linear_modules():
    d = _net(HP16, multires=[1, 2, 4, 8])                    # 64 features, but not from two levels
    assert d.grid.feat_dim == 64 and not d._mlp_fusable() and not d._fusable()
    d = _net(HP16, multires=[1, 2, 4])                       # dynerf / hypernerf: 48 features
    assert d.grid.feat_dim == 48 and not d._mlp_fusable() and not d._fusable()
    d = _net(HP32, multires=[1])                             # 32 features from ONE level of 32 channels
    assert d.grid.feat_dim == 32 and not d._mlp_fusable() and not d._fusable()


NEW = ("mom_deform_forward_n", "mom_deform_forward_activated_n", "mom_deform_backward_n", "mom_deform_backward_split_n")


def test_the_n_entry_points_are_exported_with_the_declared_argument_lists():
    """Each *_n entry takes its namesake's arguments with `int in_features` after P: header, binding and library agree."""
    lib = N.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mom4d.h")).read(), flags=re.S)

    def declared(name):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/mom4d.h"
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    for name in NEW:
        assert name in N.EXPORTS
        fn, old = getattr(lib, name), getattr(lib, name[:-2])
        args, args_old = declared(name), declared(name[:-2])
        assert args[2] == "int in_features" and args[:2] + args[3:] == args_old, name
        assert len(fn.argtypes) == len(args) == len(old.argtypes) + 1
        assert list(fn.argtypes) == list(old.argtypes[:2]) + [C.c_int] + list(old.argtypes[2:]), name


def _fake_desc():
    fake = 1 << 20          # a non-null pointer value; the calls are refused before it could be followed
    w = N.MomDeformMLP()
    for name, ctype in N.MomDeformMLP._fields_:
        setattr(w, name, fake if ctype is C.c_void_p else ctype(fake, fake, fake))
    return w, fake


@pytest.mark.parametrize("n_in", [0, 16, 31, 33, 48, 128, -32])
def test_a_trunk_width_other_than_32_or_64_is_einval(n_in, monkeypatch):
    monkeypatch.delenv("MOM_MLP_BWD", raising=False)
    lib = N.lib()
    w, f = _fake_desc()
    assert lib.mom_deform_forward_n(C.byref(w), 32, n_in, f, f, f, f, f, 0.5, f, f, f, f, None) == N.MOM_EINVAL
    assert lib.mom_deform_forward_activated_n(C.byref(w), 32, n_in, f, f, f, f, f, 0.5, f, f, f, f, f, f, f, f, None) == N.MOM_EINVAL
    assert lib.mom_deform_backward_n(C.byref(w), 32, n_in, f, f, f, f, f, f, f, None) == N.MOM_EINVAL
    assert lib.mom_deform_backward_split_n(C.byref(w), 32, n_in, f, f, f, f, f, f, f, None, None) == N.MOM_EINVAL


@pytest.mark.parametrize("n_in", [32, 64])
def test_an_unknown_backward_form_is_einval_for_either_width(n_in, monkeypatch):
    """MOM_MLP_BWD names a form of the 64-feature backward.  32 features have the f32 form only and take it under every valid
    name, but a name that is refused at 64 is refused at 32 as well."""
    lib = N.lib()
    w, f = _fake_desc()
    for bad in ("fused", "f32", "Split", "b", "split "):
        monkeypatch.setenv("MOM_MLP_BWD", bad)
        assert lib.mom_deform_backward_n(C.byref(w), 32, n_in, f, f, f, f, f, f, f, None) == N.MOM_EINVAL, bad
        assert lib.mom_deform_backward_split_n(C.byref(w), 32, n_in, f, f, f, f, f, f, f, None, None) == N.MOM_EINVAL, bad


def test_no_work_and_missing_pointers_at_32_features():
    lib = N.lib()
    w, f = _fake_desc()
    assert lib.mom_deform_forward_n(C.byref(w), 0, 32, None, None, None, None, None, 0.5, None, None, None, None, None) == N.MOM_OK
    assert lib.mom_deform_forward_n(C.byref(w), -1, 32, f, f, f, f, f, 0.5, f, f, f, f, None) == N.MOM_EINVAL
    assert lib.mom_deform_forward_n(C.byref(w), 32, 32, None, f, f, f, f, 0.5, f, f, f, f, None) == N.MOM_EINVAL
    assert lib.mom_deform_forward_n(None, 32, 32, f, f, f, f, f, 0.5, f, f, f, f, None) == N.MOM_EINVAL
    # opacity_act without opacity_raw
    assert lib.mom_deform_forward_activated_n(C.byref(w), 32, 32, f, f, f, f, f, 0.5, f, f, f, f, None, None, None, f, None) == N.MOM_EINVAL
    assert lib.mom_deform_backward_n(C.byref(w), 0, 32, None, None, None, None, None, None, None, None) == N.MOM_OK
    assert lib.mom_deform_backward_n(C.byref(w), 32, 32, f, f, f, f, f, f, None, None) == N.MOM_EINVAL       # no scratch
    w.dW0 = None
    assert lib.mom_deform_backward_n(C.byref(w), 32, 32, f, f, f, f, f, f, f, None) == N.MOM_EINVAL          # no gradient buffer


def _params(n_in):
    ps = [torch.zeros(64, n_in), torch.zeros(64)]
    for nout in (3, 3, 4):
        ps += [torch.zeros(64, 64), torch.zeros(64), torch.zeros(nout, 64), torch.zeros(nout)]
    return ps


def test_the_autograd_function_checks_every_shape_it_hands_to_the_kernels():
    check = ops.DeformMLPFunction.check_shapes
    assert check(torch.zeros(5, 32), _params(32)) == 32 and check(torch.zeros(5, 64), _params(64)) == 64
    assert check(torch.zeros(0, 32), _params(32)) == 32
    for width in (16, 48, 128):
        with pytest.raises(N.MomError):
            check(torch.zeros(5, width), _params(width))
    with pytest.raises(N.MomError):
        check(torch.zeros(5, 32), _params(64))              # W0 [64,64] with feat [P,32]: the kernel would read feat 64 wide
    with pytest.raises(N.MomError):
        check(torch.zeros(5, 64), _params(32))
    with pytest.raises(N.MomError):
        check(torch.zeros(5, 32, 1), _params(32))
    for i in range(1, 14):                                   # each of the other 13 tensors, one element short
        ps = _params(32)
        ps[i] = ps[i].reshape(-1)[:-1]
        with pytest.raises(N.MomError):
            check(torch.zeros(5, 32), ps)
    with pytest.raises(N.MomError):
        check(torch.zeros(5, 32), _params(32)[:-1])
    ps = _params(32)
    ps[2] = ps[2].double()
    with pytest.raises(N.MomError):
        check(torch.zeros(5, 32), ps)

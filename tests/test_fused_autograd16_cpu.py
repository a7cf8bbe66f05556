"""Which models gradient-mode render() runs as one autograd node (fused_autograd.node_width, NODE_WIDTHS): the shipped 32 x 2 field
at 64 features, a 16 x 2 field (dnerf/eulerian_150_16) at 32 while 32 is in NODE_WIDTHS, nothing else -- and the same width the
fused step would take (fused_step.step_features) wherever both take the model.  Real Deformation modules; no GPU needed."""
import importlib

import pytest

from test_field16_cpu import HP16, HP32, _net

pkg = "iclr2025_3d-mom_amd"
FA = importlib.import_module(pkg + ".fused_autograd")
FS = importlib.import_module(pkg + ".fused_step")


def _big():
    """tests/test_field16_cpu.py's `big` field: level 1 is 1026 texels along x, beyond Deformation.FIELD16_MAX_RES."""
    return _net(HP16, kplanes_config=dict(HP16.kplanes_config, resolution=[513, 8, 8, 5]))


CASES = [("16 x 2", lambda: _net(HP16), 32), ("32 x 2", lambda: _net(HP32), 64),
         ("16 x 4", lambda: _net(HP16, multires=[1, 2, 4, 8]), 0), ("net_width 128", lambda: _net(HP16, W=128), 0),
         ("32 x 2, net_width 128", lambda: _net(HP32, W=128), 0), ("a 1026-texel plane", _big, 0)]


@pytest.mark.parametrize("what,make,want", CASES, ids=[c[0] for c in CASES])
def test_node_width_of_real_modules(monkeypatch, what, make, want):
    monkeypatch.setattr(FA, "NODE_WIDTHS", (64, 32))
    d = make()
    got = FA.node_width(d)
    assert got == want, what
    if got:
        assert got == FS.step_features(d) == d.grid.feat_dim, what
    else:
        assert not d._fusable() and (what != "a 1026-texel plane" or d._mlp_fusable())
    assert FA.node_width(d) == want                  # the cached answer


def test_without_32_in_node_widths_a_16_x_2_model_goes_op_by_op(monkeypatch):
    d16, d32 = _net(HP16), _net(HP32)
    monkeypatch.setattr(FA, "NODE_WIDTHS", (64, 32))
    assert FA.node_width(d16) == 32 and FA.node_width(d32) == 64
    monkeypatch.setattr(FA, "NODE_WIDTHS", (64,))            # read at every call: the module's cached width does not pin the answer
    assert FA.node_width(d16) == 0 and FA.node_width(d32) == 64
    assert FS.step_features(d16) == 32                       # the fused step's own routing is not touched by the constant


def test_the_modules_answer_is_cached_until_a_parameter_object_is_replaced(monkeypatch):
    """_field16_fusable() walks every plane: asked once per set of parameter objects, not per frame."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", (64, 32))
    d = _net(HP16)
    calls = []
    real = d._field16_fusable
    d.__dict__["_field16_fusable"] = lambda: calls.append(1) or real()
    for _ in range(3):
        assert FA.node_width(d) == 32
    assert len(calls) == 1
    planes, mlp = d._fa_params[2], d._fa_params[3]
    assert len(planes) == 12 and len(mlp) == 14 and planes[0] is d.grid.grids[0][0]
    import torch
    d.grid.grids[0][0] = torch.nn.Parameter(d.grid.grids[0][0].detach().clone())       # what a densify round does to a parameter
    assert FA.node_width(d) == 32 and len(calls) == 2
    assert d._fa_params[2][0] is d.grid.grids[0][0]

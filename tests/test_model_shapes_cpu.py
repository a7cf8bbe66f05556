"""The package's deform_network on the CPU oracle backend against the g16 fixtures: the reference's own deform_network at the
model shapes it ships besides the dnerf one (dynerf: net_width 128 with the opacity and SH heads live; hypernerf: three levels,
net_width 128; the bare defaults: 32 channels x 4 levels; defor_depth 1 builds the same one-layer trunk as 0) and at five switches of Deformation.forward_dynamic
(static_mlp mask, apply_rotation, grid_pe, a deeper trunk, the opacity head alone).  All of them take the general branch of
forward_dynamic.  Tolerances: tests/test_golden_cpu.py::test_g2_deform_network_mirror_matches_reference."""
import numpy as np
import pytest

import model_shapes_cases as M
from oracle import cpu_backend, param_fill


def test_param_fill_is_a_closed_form_of_the_indices():
    """Integer hash -> 24 bits -> float32, exactly: multiples of 2^-23 in [-1, 1), the same for the same indices, spread out."""
    u = param_fill.unit(3, 4096)
    assert u.dtype == np.float32 and np.array_equal(u, param_fill.unit(3, 4096)) and np.array_equal(u[:100], param_fill.unit(3, 100))
    assert np.array_equal(u * 2.0 ** 23, np.round(u * 2.0 ** 23)) and float(u.min()) >= -1.0 and float(u.max()) < 1.0
    assert not np.array_equal(u, param_fill.unit(4, 4096))
    assert abs(float(u.mean())) < 0.05 and 0.5 < float(u.std()) < 0.65 and len(np.unique(u)) > 4000
    # pinned values: the harness that wrote the fixtures and every later reader compute these bits
    np.testing.assert_array_equal(param_fill.unit(0, 3), np.array([7379374, -5317567, -3826456], np.float32) * np.float32(2.0 ** -23))
    assert param_fill.rule("deformation_net.grid.aabb", (2, 3)) is None and param_fill.rule("pos_poc", (10,)) is None
    assert param_fill.rule("deformation_net.pos_deform.1.weight", (64, 64)) == (0.0, 0.25)
    assert param_fill.rule("deformation_net.grid.grids.1.4", (1, 16, 5, 12)) == (0.75, 1.0)
    assert param_fill.rule("deformation_net.pos_deform.3.bias", (3,)) == (0.0, 0.03125)
    assert param_fill.rule("deformation_net.rotations_deform.3.bias", (4,)) == (0.0, 0.5)
    assert param_fill.rule("deformation_net.static_mlp.3.weight", (1, 64)) == (0.0, 0.03125)
    assert param_fill.rule("deformation_net.pos_deform.3.weight", (3, 64)) == (0.0, 0.03125)


def test_fixture_settings_are_the_shipped_shapes():
    for name, (levels, channels, width, depth) in M.EXPECT.items():
        st = M.settings(name, name)
        assert (len(st["multires"]), st["kplanes_config"]["output_coordinate_dim"], st["net_width"], st["defor_depth"]) == \
            (levels, channels, width, depth), (name, st)
    assert M.settings("hypernerf", "hypernerf")["batch_size"] == 2 and M.settings("dynerf", "dynerf")["batch_size"] == 1
    st = M.settings("dynerf", "dynerf")
    assert not st["no_do"] and not st["no_dshs"]
    assert M.dead_groups(st) == {"timenet"} and M.dead_groups(M.settings("bare", "bare")) == {"timenet", "opacity_deform", "shs_deform"}


@pytest.mark.parametrize("fname,case", M.CASES)
def test_g16_mirror_matches_reference(fname, case):
    d = M.load(fname)
    st = M.settings(fname, case)
    with cpu_backend.installed():
        net = M.build(fname, case)
        dn = net.deformation_net
        assert not dn._fusable() and not dn._mlp_fusable() and not dn._field16_fusable()
        for triple in M.TRIPLES:
            tag = M.tag(triple)
            has_grads = triple == M.TRIPLES[1]
            outs, dins, dpar = M.run(net, fname, triple, backward=has_grads, tensor_time=True)      # [n,1] times, as the reference passes
            for k in M.OUTPUTS:
                np.testing.assert_allclose(outs[k].detach().numpy(), d[f"{case}__{k}_{tag}"], rtol=1e-6, atol=1e-7, err_msg=f"{k} {tag}")
            if not has_grads:
                continue
            np.testing.assert_allclose(dins["xyz"].numpy(), d[f"{case}__dxyz_{tag}"], rtol=1e-5, atol=1e-6)
            for k in M.INPUTS[1:]:
                # g2 holds d/d scaling and d/d rotation to rtol 1e-6 because they ARE the loss weights there (the inputs are passed
                # through and added to); so they are here, except under the static_mlp mask and for apply_rotation's quaternion
                # product, where they are computed by the network like d/d xyz: rtol 1e-5 as for that one, with an absolute part
                # of 2e-9 (2e-6 of the loss weights' scale, 2^-10) for the elements a cancelling sum leaves small
                if st["static_mlp"] or (k == "rotation" and st["apply_rotation"]):
                    np.testing.assert_allclose(dins[k].numpy(), d[f"{case}__d{k}_{tag}"], rtol=1e-5, atol=2e-9, err_msg=k)
                else:
                    np.testing.assert_allclose(dins[k].numpy(), d[f"{case}__d{k}_{tag}"], rtol=1e-6, err_msg=k)
            stored = sorted(k.split("__", 2)[2] for k in d.files if k.startswith(f"{case}__grad_{tag}__"))
            assert stored == sorted(dpar)                                   # the reference's parameter names
            dead, live = set(), 0
            for k, g in dpar.items():
                ref = d[f"{case}__grad_{tag}__{k}"]
                assert (g is None) == (ref.size == 0), (k, "None-ness differs from the reference")
                if g is None:
                    dead.add(k.split(".")[0] if k.startswith("timenet") else k.split(".")[1])
                else:
                    live += 1
                    assert float(np.abs(ref).max()) > 0, k
                    np.testing.assert_allclose(g.numpy(), ref, rtol=1e-5, atol=1e-7, err_msg=k)
            # timenet is dead everywhere; opacity_deform / shs_deform exactly where no_do / no_dshs say so ("grid": the frozen box)
            assert dead - {"grid"} == M.dead_groups(st), (dead, M.dead_groups(st))
            assert live >= 6 * len(st["multires"]) + 2 * max(st["defor_depth"], 1) + 4 * (5 - len(M.dead_groups(st)) + 1)

"""tests/deform_mlp_cases.py checked without a GPU: its float64 restatement against torch autograd in float64 on the same layers,
its builder's condition (no ambiguous ReLU left in any case the GPU tests run), and its bounds against the one fp32 evaluation
there is on the CPU: oracle.torch_ref.deform_mlp and its autograd must themselves lie inside the fp32 bounds, element by element,
with the structural units' exact zeros."""
import numpy as np
import pytest
import torch

import deform_mlp_cases as dc
from oracle import torch_ref as tr


def _torch_run(c, dtype):
    """oracle.torch_ref.deform_mlp and autograd in `dtype` on case c: (outputs + a0, dfeat, 14 parameter gradients), numpy."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    ps = [t(p).requires_grad_(True) for p in c["params"]]
    feat = t(c["feat"]).requires_grad_(True)
    o = tr.deform_mlp(feat, t(c["xyz"]), t(c["scal"]), t(c["rot"]), t(c["flow"]), dc.FLOW_COEF, ps)
    sum((a * t(w)).sum() for a, w in zip(o, c["douts"])).backward()
    a0 = torch.relu(torch.nn.functional.linear(feat, ps[0], ps[1])).detach()
    return [x.detach().numpy() for x in o] + [a0.numpy()], feat.grad.numpy(), [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("kind", ["dense", "needle", "wide"])
@pytest.mark.parametrize("n_in", [64, 32])
@pytest.mark.parametrize("P", [33, 2049])
def test_restatement_equals_torch_autograd_in_float64(P, n_in, kind):
    c = dc.case(P, n_in, kind)
    outs, dfeat, grads = _torch_run(c, torch.float64)
    v, _ = dc.forward(c["params"], c["feat"], c["xyz"], c["scal"], c["rot"], c["flow"])
    g, _ = dc.backward(c["params"], c["feat"], v["a0"], c["douts"])
    pairs = list(zip(dc.OUT_NAMES, outs)) + [("dfeat", dfeat)] + list(zip(dc.GRAD_NAMES, grads))
    for name, want in pairs:
        got = v[name] if name in v else g[name]
        assert got.shape == want.shape, name
        scale = float(np.abs(want).max())
        assert scale > 0, name
        err = float(np.abs(got - want).max())
        assert err <= 1e-12 * scale, (name, err, scale)


@pytest.mark.parametrize("n_in", [64, 32])
def test_every_case_is_built_without_an_ambiguous_relu(n_in):
    """The condition the backward comparisons rest on, checked apart from the builder's own assertion: no pre-activation of a
    non-structural unit within MARGIN bounds of zero (2 composed bounds), in any case the GPU tests run."""
    exempt = dc._exempt()
    for P, width, kind, redraw in dc.all_cases():
        if width != n_in or not redraw:
            continue
        c = dc.case(P, n_in, kind, redraw)
        left = int(dc.ambiguous_rows(c["params"], c["feat"], c["bf16"], dc.MARGIN, 2.0, exempt).sum())
        print("P=%d in=%d %s: redrawn %.1f %% of the rows, ambiguous rows left: %d" % (P, n_in, kind, 100 * c["redrawn"], left))
        assert left == 0 and c["ambiguous"] == 0, (P, n_in, kind, left)
        if kind == "needle":
            rows = np.flatnonzero(np.any(c["douts"][0] != 0, axis=1))
            assert np.array_equal(rows, dc.needle_rows(P)), (P, rows)
        if kind == "wide":
            assert int((np.abs(c["feat"]).max(1) == 0).sum()) >= 1


def _check_struct(c, grads, a0, what):
    for layer, unit in dc.STRUCT["zero"] + dc.STRUCT["dead"]:
        if layer == 0:
            assert not a0[:, unit].any(), (what, "a0 column", unit)
    for name, idx in dc.struct_zero_checks(c["n_in"]):
        assert not np.asarray(grads[name])[idx].any(), (what, name, idx)
    for layer, unit in dc.STRUCT["live"]:
        assert np.abs(grads["db1_%d" % (layer - 1)][unit]) > 0, (what, "live unit")


@pytest.mark.parametrize("n_in", [64, 32])
@pytest.mark.parametrize("P", [p for p in dc.SIZES_BACKWARD if p <= 8193])
def test_the_fp32_cpu_reference_is_inside_every_bound(P, n_in):
    """Forward and autograd in fp32 on the CPU against float64 under the composed fp32 bounds (the backward inherits the error
    of the forward's own a0): every element of every output and gradient, no row left out."""
    c = dc.case(P, n_in, "dense")
    outs, dfeat, grads = _torch_run(c, torch.float32)
    v, e = dc.forward_ref(P, n_in, "dense", True, False)
    g, ge = dc.backward(c["params"], c["feat"], v["a0"], c["douts"], False, e_a0=e["a0"])
    got = dict(zip(dc.OUT_NAMES, outs), dfeat=dfeat, **dict(zip(dc.GRAD_NAMES, grads)))
    for name in dc.OUT_NAMES + ("dfeat",) + dc.GRAD_NAMES:
        want, bound = (v[name], e[name]) if name in v else (g[name], ge[name])
        s = dc.share(got[name], want, bound)
        print("P=%d in=%d %-6s largest share of the bound %.3f" % (P, n_in, name, s))
        assert s <= 1.0, (name, s)
    _check_struct(c, got, got["a0"], "fp32 CPU reference")

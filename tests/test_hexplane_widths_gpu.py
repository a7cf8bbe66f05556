"""Both instantiations of the HexPlane kernel templates (csrc/hexplane.hip, C = 32 and C = 16) through the same cases, at the point
counts where the group arithmetic that follows from C can go wrong.

A wave holds 64 / C groups; the chunked forward and the gather deal a 32-point chunk out as 32 / (64 / C) points per group, the
scatter prepares C sorted positions per group and chunk and consumes them in batches of 16.  So, per point count P:

      1   one point: every group but the first is empty
      9   16 channels: the gather's second group gets a single point
     17   the second half-wave gets a single point; 32 channels: the scatter's second batch holds one position; 16 channels: a
          second scatter group starts
     33   the second gather chunk, and the second scatter group at 32 channels
     63   ragged everywhere
  20000   many points per texel and several workgroups

Tolerances are those of tests/test_hexplane16_gpu.py, whose helpers these tests use (gradients: rtol 2e-4 / atol 2e-5 max(1, |ref|max);
features against the oracle: rtol 2e-5 / atol 5e-6); forward features of the three forms are compared bit for bit."""
import numpy as np
import pytest
import torch

from test_hexplane16_gpu import _close, _field, _oracle, _points, ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [1, 9, 17, 33, 63, 20000])
@pytest.mark.parametrize("channels", [16, 32])
def test_two_pass_backward_equals_generic_backward_on_shared_cells(channels, P, monkeypatch):
    """8 x 8 x 8 cells and up to 20 000 points: many points per texel, several workgroups, a ragged last chunk and last group.  The
    32-channel field runs in the six-row form (lane-per-channel gather + scatter<false>), the counterpart of the 16-channel kernels."""
    if channels == 32:
        monkeypatch.setenv("MOM_HEX_GATHER", "5")
    t = 0.3
    f = _field((8, 8, 8, 5), (1, 2), channels=channels)
    assert f.feat_dim == 2 * channels
    pts = _points(P)
    w = torch.randn(P, f.feat_dim, generator=torch.Generator().manual_seed(3))
    ref = _oracle(f, pts, t, w)
    fg = f.cuda()
    levels = [list(g) for g in fg.grids]
    host = fg.aabb_host()

    def run(two_pass):
        fg.zero_grad()
        p = pts.cuda().requires_grad_(True)
        order = ops.morton_order(p)
        po = ops.hexplane_orders(p, levels, fg.aabb, aabb_host=host) if two_pass else None
        feat = ops.hexplane_features(p, t, fg.aabb, levels, order=order, aabb_host=host, plane_orders=po)
        (feat * w.cuda()).sum().backward()
        torch.cuda.synchronize()
        return p.grad.cpu().numpy(), [[q.grad.cpu().numpy().copy() for q in g] for g in fg.grids]

    two, gen = run(True), run(False)
    for got, what in ((two, "two-pass"), (gen, "generic")):
        _close(got[0], ref[1], what + " dxyz")
        for l in range(2):
            for i in range(6):
                assert got[1][l][i].shape == ref[2][l][i].shape
                _close(got[1][l][i], ref[2][l][i], f"{what} plane {l} {i}")
    _close(two[0], gen[0], "two-pass vs generic dxyz")
    for l in range(2):
        for i in range(6):
            _close(two[1][l][i], gen[1][l][i], f"two-pass vs generic plane {l} {i}")


@pytest.mark.parametrize("P", [33, 257])
@pytest.mark.parametrize("channels", [16, 32])
def test_forward_features_are_the_same_bits_in_every_form(channels, P):
    """Morton order and identity order (the chunked forward, fwd4) and per-point timestamps (the generic forward): one set of
    features, bit for bit, and the oracle's to rounding.  Three levels of unequal sizes, so that a width taken for a height shows."""
    t = 0.3
    f = _field((16, 12, 10, 7), (1, 2, 4), channels=channels)
    pts = _points(P)
    with torch.no_grad():
        want = _oracle_features(f, pts, t)
        fg = f.cuda()
        levels = [list(g) for g in fg.grids]
        host = fg.aabb_host()
        p = pts.cuda()
        morton = ops.hexplane_features(p, t, fg.aabb, levels, order=ops.morton_order(p), aabb_host=host)
        ident = ops.hexplane_features(p, t, fg.aabb, levels, order=torch.arange(P, dtype=torch.int32, device="cuda"), aabb_host=host)
        per_point = ops.hexplane_features(p, torch.full((P, 1), t, device="cuda"), fg.aabb, levels, order=ops.morton_order(p), aabb_host=host)
        torch.cuda.synchronize()
    morton = morton.cpu().numpy()
    assert morton.shape == (P, 3 * channels) and float(np.abs(morton).max()) > 0
    np.testing.assert_allclose(morton, want, rtol=2e-5, atol=5e-6)
    np.testing.assert_array_equal(ident.cpu().numpy(), morton)
    np.testing.assert_array_equal(per_point.cpu().numpy(), morton)


def _oracle_features(f, pts, t):
    from oracle import torch_ref as tr
    return tr.hexplane_features(pts, t, f.aabb.detach(), [[q.detach().clone().contiguous() for q in g] for g in f.grids]).numpy()

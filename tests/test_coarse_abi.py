"""The coarse stage's additions to the C ABI (MomRasterArgs.params_raw, the statistics epilogue of MomRasterGrads) are checked
before anything reaches the GPU: every invalid combination is refused with MOM_EINVAL on a machine without one."""
import ctypes as C
import importlib

N = importlib.import_module("iclr2025_3d-mom_amd._native")
FAKE = 1 << 20          # a non-null pointer value; every call below is refused before it could be followed


def _args(**kw):
    a = N.MomRasterArgs()
    a.P, a.D, a.M, a.W, a.H = 10, 0, 16, 32, 32
    for name in ("background", "means3D", "shs", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "campos"):
        setattr(a, name, FAKE)
    a.params_raw = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grads(**kw):
    g = N.MomRasterGrads()
    for name in ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        setattr(g, name, FAKE)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_abi_version_8_and_struct_sizes():
    lib = N.lib()
    assert N.ABI_VERSION == 8 == lib.mom_abi_version()
    assert lib.mom_abi_sizeof(0) == C.sizeof(N.MomRasterArgs)
    assert lib.mom_abi_sizeof(1) == C.sizeof(N.MomRasterGrads)
    assert [n for n, _ in N.MomRasterArgs._fields_][-1] == "params_raw"
    assert [n for n, _ in N.MomRasterGrads._fields_][-4:] == ["stats_max_radii2D", "stats_grad_accum", "stats_denom",
                                                              "stats_skip_if_nonzero"]


def test_params_raw_with_inputs_it_cannot_activate_is_refused():
    lib = N.lib()
    for bad in (dict(cov3D_precomp=FAKE), dict(scales=None), dict(rotations=None), dict(scales=None, rotations=None, cov3D_precomp=FAKE)):
        a = _args(**bad)
        assert lib.mom_raster_forward_geometry(C.byref(a), FAKE, FAKE, FAKE, FAKE, None, None) == N.MOM_EINVAL, bad
        assert lib.mom_raster_forward_render(C.byref(a), FAKE, FAKE, 16, FAKE, FAKE, FAKE, None, None) == N.MOM_EINVAL, bad
        assert lib.mom_raster_backward(C.byref(a), FAKE, FAKE, FAKE, 16, FAKE, FAKE, None, C.byref(_grads()), None) == N.MOM_EINVAL, bad
    # (P == 0 as well: the flag describes the call, not the data)
    a = _args(cov3D_precomp=FAKE, P=0)
    assert lib.mom_raster_forward_geometry(C.byref(a), None, None, None, FAKE, None, None) == N.MOM_EINVAL


def test_params_raw_together_with_act_rotations_raw_is_refused():
    lib = N.lib()
    a = _args()
    g = _grads(act_rotations_raw=FAKE)
    assert lib.mom_raster_backward(C.byref(a), FAKE, FAKE, FAKE, 16, FAKE, FAKE, None, C.byref(g), None) == N.MOM_EINVAL
    assert lib.mom_raster_backward_geometry(C.byref(a), FAKE, FAKE, C.byref(g), None) == N.MOM_EINVAL


def test_statistics_pointers_given_in_part_are_refused():
    lib = N.lib()
    names = ("stats_max_radii2D", "stats_grad_accum", "stats_denom")
    parts = [dict(zip(names[:k], [FAKE] * k)) for k in (1, 2)] + [{names[1]: FAKE}, {names[2]: FAKE},
                                                                    {names[0]: FAKE, names[2]: FAKE},
                                                                    {"stats_skip_if_nonzero": FAKE}]
    for raw in (0, 1):
        a = _args(params_raw=raw)
        for part in parts:
            g = _grads(**part)
            assert lib.mom_raster_backward(C.byref(a), FAKE, FAKE, FAKE, 16, FAKE, FAKE, None, C.byref(g), None) == N.MOM_EINVAL, part
            assert lib.mom_raster_backward_geometry(C.byref(a), FAKE, FAKE, C.byref(g), None) == N.MOM_EINVAL, part

"""CPU tests of the RK45 integrator's boundary (mvf_integrate_rk45): declared in the header and exported, every invalid
argument rejected through the status + mvf_last_error channel before anything is launched, and integrate_field's
argument checks made before any device object exists."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mvf.h")


def test_header_declares_and_library_exports_rk45():
    from spateo_amd import _lib

    text = open(HEADER).read()
    assert re.search(r"\bint mvf_integrate_rk45\s*\(", text)
    assert "trajectory.py:61-110" in text.split("mvf_integrate_rk45(")[0].rsplit("*/", 2)[-2]  # its Replaces: line
    for name, val in (("MVF_RK45_UNIFORM_TIME", _lib.RK45_UNIFORM_TIME), ("MVF_RK45_ARC_LENGTH", _lib.RK45_ARC_LENGTH)):
        assert int(re.search(rf"{name} = (\d+)", text).group(1)) == val
    lib = _lib.load()
    assert hasattr(lib, "mvf_integrate_rk45") and "mvf_integrate_rk45" in _lib.SIGNATURES
    assert lib.mvf_version() == 7  # an additive entry point


def _call(**over):
    """mvf_integrate_rk45 with fake (never dereferenced) device pointers and valid arguments, `over` replacing some."""
    from spateo_amd import _lib

    fake = ctypes.c_void_p(0x1000)
    world = (ctypes.c_double * 6)(1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
    a = dict(x4=fake, n=4, ctrl4=fake, m=3, beta=0.1, C=fake, affine=None, d=3, world=world, t_bound=10.0, rtol=1e-3,
             atol=1e-6, max_step=0.5, max_steps=1000, sampling=_lib.RK45_ARC_LENGTH, n_out=5, t=fake, traj=fake,
             stats=fake, dtype=_lib.MVF_F64, stream=None)
    a.update(over)
    lib = _lib.load()
    rc = lib.mvf_integrate_rk45(*a.values())
    return rc, lib.mvf_last_error().decode()


@pytest.mark.parametrize("over,msg", [
    (dict(rtol=0.0), "rtol"), (dict(rtol=-1e-3), "rtol"), (dict(rtol=float("nan")), "rtol"),
    (dict(rtol=float("inf")), "rtol"), (dict(atol=0.0), "atol"), (dict(atol=float("nan")), "atol"),
    (dict(atol=float("inf")), "atol"), (dict(max_step=0.0), "max_step"), (dict(max_step=-1.0), "max_step"),
    (dict(max_step=float("nan")), "max_step"), (dict(n_out=1), "n_out"), (dict(n_out=0), "n_out"), (dict(d=0), "d must"),
    (dict(d=4), "d must"), (dict(max_steps=0), "max_steps"), (dict(sampling=2), "sampling"), (dict(t_bound=0.0), "t_bound"),
    (dict(t_bound=float("nan")), "t_bound"), (dict(beta=0.0), "beta"), (dict(dtype=7), "dtype"), (dict(n=-1), "shape"),
    (dict(world=None), "world"), (dict(x4=None), "null pointer"), (dict(t=None), "null pointer"),
    (dict(traj=None), "null pointer"), (dict(stats=None), "null pointer"), (dict(C=None), "null pointer"),
])
def test_invalid_arguments_are_rejected_before_any_launch(over, msg):
    rc, err = _call(**over)
    assert rc != 0 and "mvf_integrate_rk45" in err and msg in err, (over, err)


def test_zero_scale_in_world_map_is_rejected():
    world = (ctypes.c_double * 6)(1.0, 0.0, 1.0, 0.0, 0.0, 0.0)
    rc, err = _call(world=world)
    assert rc != 0 and "world" in err


def test_empty_problem_launches_nothing():
    # n == 0 with null outputs: no pointer is needed and nothing is launched (this passes on a machine without a GPU)
    rc, err = _call(n=0, x4=None, t=None, traj=None, stats=None)
    assert rc == 0, err


@pytest.mark.parametrize("kw,msg", [
    (dict(integrator="rk5"), "integrator"), (dict(integrator="rk45", rtol=0.0), "rtol"),
    (dict(integrator="rk45", atol=-1.0), "atol"), (dict(integrator="rk45", rtol=float("nan")), "rtol"),
    (dict(integrator="rk45", max_steps=0), "max_steps"), (dict(integrator="rk45", t_end=-1.0), "t_end"),
])
def test_integrate_field_validates_before_touching_a_device(monkeypatch, kw, msg):
    from spateo_amd import _trajectory

    def no_device(*a, **k):
        raise AssertionError("a kernel object was created before the arguments were checked")

    monkeypatch.setattr(_trajectory, "_shared_kernels", no_device)
    rng = np.random.default_rng(0)
    vf = dict(X_ctrl=rng.standard_normal((5, 3)), C=rng.standard_normal((5, 3)), beta=0.1, method="sparsevfc",
              X=rng.standard_normal((5, 3)), V=rng.standard_normal((5, 3)))
    kw = dict(kw)
    t_end = kw.pop("t_end", 10.0)
    with pytest.raises(ValueError, match=msg):
        _trajectory.integrate_field(vf, vf["X"][:2], t_end=t_end, **kw)

"""fmmbem_options.stokes_batch_width (the multi-vector near field of Stokes plans) without a device: the default, the range
check of the create calls that take options, the Python mirrors of the struct, and the host-only plans on which the option is
accepted without effect (include/fmmbem.h).

fmmbem_plan_create_like takes a base plan and no options: the width it inherits was range-checked when its base was created, and a
base refused with FMMBEM_ERR_INVALID leaves no handle to create a like plan from (checked here)."""
import ctypes as C

import numpy as np
import pytest

OK, INVALID, NO_DEVICE = 0, 1, 2


def _default_options(fb):
    from fmm_bem_relaxed_amd import _capi
    o = _capi.Options()
    fb.lib().fmmbem_options_default(C.byref(o))
    return o


def _panels(fb, rec=2):
    return np.ascontiguousarray(fb.unit_sphere(rec), dtype=np.float64).reshape(-1, 9)


def test_defaults(fb):
    assert _default_options(fb).stokes_batch_width == 0
    assert fb.FMMOptions().stokes_batch_width == 0


def test_struct_size_is_the_librarys(fb):
    """fmmbem_options_default clears sizeof(fmmbem_options) bytes before it writes the defaults: on a buffer of 0xFF bytes the
    extent it touched is the library's size of the struct -- the ctypes mirror must have exactly that size; the new field is its
    last, directly behind near_f32_max_p."""
    from fmm_bem_relaxed_amd import _capi
    size = C.sizeof(_capi.Options)
    buf = (C.c_ubyte * (size + 64))(*([0xFF] * (size + 64)))
    fb.lib().fmmbem_options_default(C.cast(buf, C.POINTER(_capi.Options)))
    touched = [i for i, b in enumerate(buf) if b != 0xFF]
    assert touched[-1] + 1 == size, (touched[-1] + 1, size)
    assert _capi.Options.stokes_batch_width.offset == _capi.Options.near_f32_max_p.offset + 4
    assert size - 8 < _capi.Options.stokes_batch_width.offset + 4 <= size       # nothing but alignment padding behind it


@pytest.mark.parametrize("bad", [-1, 5])
@pytest.mark.parametrize("kernel", ["laplace", "stokes"])
def test_out_of_range_is_invalid_from_create(fb, bad, kernel):
    from fmm_bem_relaxed_amd import _capi
    o = _default_options(fb)
    o.host_only = 1
    o.stokes_batch_width = bad
    if kernel == "stokes":
        o.kernel = _capi.KERNEL_STOKES_BEM
    v = _panels(fb)
    h = C.c_void_p()
    assert fb.lib().fmmbem_plan_create(C.byref(o), len(v), v.ctypes.data_as(C.c_void_p), None, C.byref(h)) == INVALID
    assert not h.value
    # no base plan came out of the refused create; create_like has nothing to inherit a bad width from
    like = C.c_void_p()
    assert fb.lib().fmmbem_plan_create_like(h, None, C.byref(like)) == INVALID and not like.value
    K = fb.LaplaceSphericalBEM(5, 3) if kernel == "laplace" else fb.StokesSphericalBEM(5, 3)
    with pytest.raises(fb.FmmBemError) as e:
        fb.FMM_plan(K, fb.unit_sphere(2), host_only=True, stokes_batch_width=bad)
    assert e.value.status == INVALID
    opts = fb.FMMOptions()
    opts.stokes_batch_width = bad                       # ... and through FMMOptions
    with pytest.raises(fb.FmmBemError) as e:
        fb.FMM_plan(K, fb.unit_sphere(2), opts, host_only=True)
    assert e.value.status == INVALID


@pytest.mark.parametrize("bad", [-1, 5])
def test_out_of_range_is_invalid_from_create_targets(fb, bad):
    o = _default_options(fb)
    o.host_only = 1
    o.stokes_batch_width = bad
    v = _panels(fb)
    pts = np.ascontiguousarray(np.random.default_rng(1).normal(size=(10, 3)) * 2.0)
    h = C.c_void_p()
    rc = fb.lib().fmmbem_plan_create_targets(C.byref(o), len(v), v.ctypes.data_as(C.c_void_p), None, len(pts),
                                             pts.ctypes.data_as(C.c_void_p), None, C.byref(h))
    assert rc == INVALID and not h.value
    with pytest.raises(fb.FmmBemError) as e:
        fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), fb.unit_sphere(2), host_only=True, targets=pts, stokes_batch_width=bad)
    assert e.value.status == INVALID


def test_create_like_of_a_host_only_base_is_refused_as_before(fb):
    o = _default_options(fb)
    o.host_only = 1
    o.stokes_batch_width = 3
    v = _panels(fb)
    h, like = C.c_void_p(), C.c_void_p()
    assert fb.lib().fmmbem_plan_create(C.byref(o), len(v), v.ctypes.data_as(C.c_void_p), None, C.byref(h)) == OK
    assert fb.lib().fmmbem_plan_create_like(h, None, C.byref(like)) == NO_DEVICE and not like.value
    fb.lib().fmmbem_plan_destroy(h)


@pytest.mark.parametrize("width", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kernel", ["laplace", "stokes"])
def test_accepted_on_host_only_plans_whose_width_is_one(fb, kernel, width):
    K = fb.LaplaceSphericalBEM(5, 3) if kernel == "laplace" else fb.StokesSphericalBEM(5, 3)
    v = fb.unit_sphere(3)
    pl = fb.FMM_plan(K, v, host_only=True, stokes_batch_width=width)
    assert pl.batch_width() == 1
    ref = fb.FMM_plan(K, v, host_only=True)
    s, r = pl.stats(), ref.stats()
    for key in ("n_panels", "n_boxes", "n_leaves", "near_nnz", "m2l_pairs", "p2p_pairs", "n_devices"):
        assert s[key] == r[key]                                  # the option does not touch the tree or the lists


def test_target_plan_accepts_the_option(fb):
    pts = np.random.default_rng(2).normal(size=(50, 3)) * 2.0
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(5, 3), fb.unit_sphere(3), host_only=True, targets=pts, stokes_batch_width=4)
    assert pl.batch_width() == 1


def test_first_layout_of_the_struct_still_works_under_the_plain_names(fb):
    """A program compiled against the header before stokes_batch_width holds 120 bytes of options and calls the plain symbols:
    fmmbem_options_default writes exactly those 120 bytes, and the create calls neither read the bytes behind them (0xFF here:
    a width of -1 if they did) nor refuse the plan.  Python itself calls the _r2 entry points (fmm_bem_relaxed_amd._capi.lib)."""
    from fmm_bem_relaxed_amd import _capi
    raw = C.CDLL(_capi.LIB_PATH)                      # the library's own names, without the rebinding of _capi.lib()
    first = _capi.Options.stokes_batch_width.offset
    assert first == 120 and C.sizeof(_capi.Options) == 128
    buf = (C.c_ubyte * (first + 64))(*([0xFF] * (first + 64)))
    raw.fmmbem_options_default.restype = None
    raw.fmmbem_options_default(buf)
    assert all(b == 0xFF for b in buf[first:]) and any(b != 0xFF for b in buf[:first])
    o = _capi.Options.from_buffer(buf)
    assert o.p_max == 10 and o.ncrit == 64 and o.near_f32_max_p == 0 and o.stokes_batch_width == -1     # -1: never written
    o.host_only = 1
    v = _panels(fb)
    pts = np.ascontiguousarray(np.random.default_rng(3).normal(size=(10, 3)) * 2.0)
    vp = C.c_void_p
    raw.fmmbem_plan_create.argtypes = [vp, C.c_size_t, vp, vp, C.POINTER(vp)]
    raw.fmmbem_plan_create_targets.argtypes = [vp, C.c_size_t, vp, vp, C.c_size_t, vp, vp, C.POINTER(vp)]
    raw.fmmbem_plan_batch_width.argtypes = [vp, C.POINTER(C.c_int)]
    raw.fmmbem_plan_destroy.argtypes = [vp]
    raw.fmmbem_plan_destroy.restype = None
    h, t, w = vp(), vp(), C.c_int(0)
    assert raw.fmmbem_plan_create(C.addressof(o), len(v), v.ctypes.data_as(vp), None, C.byref(h)) == OK and h.value
    assert raw.fmmbem_plan_create_targets(C.addressof(o), len(v), v.ctypes.data_as(vp), None, len(pts), pts.ctypes.data_as(vp),
                                          None, C.byref(t)) == OK and t.value
    assert raw.fmmbem_plan_batch_width(h, C.byref(w)) == OK and w.value == 1
    raw.fmmbem_plan_destroy(h)
    raw.fmmbem_plan_destroy(t)
    # the same struct through the entry points of today's layout IS read to its end
    assert fb.lib().fmmbem_plan_create(C.byref(o), len(v), v.ctypes.data_as(vp), None, C.byref(h)) == INVALID

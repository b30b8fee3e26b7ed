"""The field quantities of one plan beside each other (fmmbem_plan_execute_gradient, _pressure, _velocity_gradient): the plan keeps
one set of buffers per quantity, allocated at the quantity's first call, and one launcher serves all three, so a crossed buffer or
launcher would show only where the quantities are mixed on one plan.  The values are held to their references by
test_gpu_field_gradient.py, test_gpu_field_pressure.py and test_gpu_field_velocity_gradient.py; here, on the two_r3 case of those
tests (ten coincident targets: the per-point buffers are live), two fresh plans that meet the quantities in opposite orders
give, call by call, the same bits as each other and as every repeat, at orders 2, 12 and 13 -- the first order the velocity gradient
launches, the last unrolled order and the first run-time order -- the host form equals the torch form, and execute_stress is its
formula of the two.  A result of each quantity is also held to that quantity's own composed reference at order 12, relative L2
<= 1e-12 -- the bound of the three test files above for these kernels on this case -- so that a launcher that served another
quantity's kernel, or a buffer read at another quantity's width, shows as a wrong value."""
import numpy as np
import pytest
import torch

import field_gradient_reference as G
import field_pressure_reference as Q
import field_velocity_gradient_reference as V

pytestmark = pytest.mark.gpu

ORDERS = (2, 12, 13)


def stokes_record(fb, first):
    """A fresh Stokes field plan of two_r3; `first`: the quantity it meets first.  Every result of the sequence, by name."""
    ref = Q.reference("two_r3")
    assert len(ref.tree) < len(ref.given)                  # some targets coincide
    K, plan = Q.host_plan(fb, ref.v, ref.pts, ref.c["ncrit"], p_max=16, host_only=False)
    x = ref.vector("x")
    xd = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to("cuda:0")
    calls = {"pressure": lambda: plan.execute_pressure(x), "velocity_gradient": lambda: plan.execute_velocity_gradient(x),
             "velocity": lambda: plan.execute(x)}
    rec = {}
    K.set_p(8)
    for name in (first, "velocity_gradient" if first == "pressure" else "pressure"):       # allocation order
        rec["first", name] = calls[name]()
    for sweep in range(2):
        for p in ORDERS:
            K.set_p(p)
            for k, name in enumerate(("pressure", "velocity_gradient", "velocity", "pressure")):
                out = calls[name]()
                if (p, name) in rec:                       # every repeat of a call: identical bits
                    assert np.array_equal(out, rec[p, name]), (first, sweep, p, k, name)
                rec[p, name] = out
    for p in ORDERS:
        K.set_p(p)
        q, g = rec[p, "pressure"], rec[p, "velocity_gradient"]
        assert q.shape == (len(ref.pts),) and g.shape == (len(ref.pts), 3, 3) and rec[p, "velocity"].shape == (len(ref.pts), 3)
        assert np.array_equal(plan.execute_pressure_torch(xd).cpu().numpy(), q), (first, p)
        assert np.array_equal(plan.execute_velocity_gradient_torch(xd).cpu().numpy(), g), (first, p)
        assert np.array_equal(plan.execute_stress(x), -q[:, None, None] * np.eye(3)[None] + K.Mu * (g + g.transpose(0, 2, 1))), (first, p)
    # each quantity is ITS quantity: the composed references of the pressure and of the velocity gradient at order 12
    assert np.array_equal(V.reference("two_r3").vector("x"), x)
    for name, want in (("pressure", ref.pressure(12)), ("velocity_gradient", V.reference("two_r3").gradient(12))):
        rel = float(np.linalg.norm(rec[12, name] - want) / np.linalg.norm(want))
        print("%s first, %s at p = 12: rel L2 %.2e" % (first, name, rel))
        assert rel <= 1e-12, (first, name, rel)
    return rec


def test_stokes_quantities_interleaved_on_two_plans(fb):
    a, b = stokes_record(fb, "pressure"), stokes_record(fb, "velocity_gradient")
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def laplace_record(fb, first):
    """A fresh Laplace target plan of two_r3; `first`: the execute it meets first."""
    ref = G.reference("two_r3")
    assert len(ref.tree) < len(ref.given)
    opts = fb.FMMOptions()
    opts.set_mac_theta(G.THETA)
    opts.set_max_per_box(ref.c["ncrit"])
    K = fb.LaplaceSphericalBEM(8, G.K)
    plan = fb.FMM_plan(K, ref.v, opts, p_max=16, targets=ref.pts, target_bc=ref.flags)
    x = ref.vector("x")
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    calls = {"gradient": lambda: plan.execute_gradient(x), "potential": lambda: plan.execute(x)}
    rec = {}
    K.set_p(8)
    for name in (first, "potential" if first == "gradient" else "gradient"):
        rec["first", name] = calls[name]()
    for sweep in range(2):
        for p in (1,) + ORDERS:
            K.set_p(p)
            for k, name in enumerate(("gradient", "potential", "gradient")):
                out = calls[name]()
                if (p, name) in rec:
                    assert np.array_equal(out, rec[p, name]), (first, sweep, p, k, name)
                rec[p, name] = out
    for p in (1,) + ORDERS:
        K.set_p(p)
        assert rec[p, "gradient"].shape == (len(ref.pts), 3)
        assert np.array_equal(plan.execute_gradient_torch(xd).cpu().numpy(), rec[p, "gradient"]), (first, p)
    want = ref.gradient(12)                               # the composed reference, flag by flag as test_gpu_field_gradient.py holds it
    for f in (0, 1):
        s = ref.flags == f
        rel = float(np.linalg.norm(rec[12, "gradient"][s] - want[s]) / np.linalg.norm(want[s]))
        print("%s first, gradient at p = 12, flag %d: rel L2 %.2e" % (first, f, rel))
        assert rel <= 1e-12, (first, f, rel)
    return rec


def test_laplace_gradient_interleaved_on_two_plans(fb):
    a, b = laplace_record(fb, "gradient"), laplace_record(fb, "potential")
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), key

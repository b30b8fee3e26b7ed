"""Inputs and the CPU reference shared by tests/test_m2l_form_cases_host.py and tests/test_gpu_m2l_forms.py: geometries whose M2L lists
reach every path of the double-sum M2L kernels (csrc/kernels_m2l.hip: m2l_small_kernel at p <= 4, m2l_kernel<P, NS, NSLOT> above),
which a plan runs at every order under FMMBEM_M2L_ROT=0.

What each case is for (the host test holds the figures, so a changed generator cannot empty a case):

  two_r54          targets of up to 64, of 65-128 and of more than 128 sources: one, two and three rounds of m2l_small_kernel's
                   lane-strided source loop; fewer than 512 targets: one block of the XCD remap of m2l_kernel
  soup2500         more than 1 024 targets: the third block of 512 workgroups of the XCD remap partly filled; a ragged tree
  tiny48           a nearly empty launch: 7 targets of 1-4 sources
  stokes_r43       the Stokes passes (four slots per pass, two at p = 11 and 12; eleven slots one per pass with mixed flags)
  stokes_soup1500  more than 512 targets with four slots per pass

The reference is the CPU oracle with the complete L2L list (the device's default; l2l_skipped is 0 on all five, so the two rules
coincide), its expansions and its matvec; computed once per (case, flag set, order) and per process, shared, never written to."""
import numpy as np

from near_form_cases import _soup

STOKES_K, STOKES_KFINE, STOKES_MU = 4, 19, 1e-3
LAPLACE_K = 3

# name: (kind, ncrit, theta); the figures: boxes, M2L pairs, distinct M2L targets, (fewest, most) sources of a target, targets of
# <= 64 / 65-128 / > 128 sources, levels -- measured with the CPU oracle, held by tests/test_m2l_form_cases_host.py
CASES = {
    "two_r54": ("laplace", 16, 0.4),
    "soup2500": ("laplace", 8, 0.4),
    "tiny48": ("laplace", 8, 0.5),
    "stokes_r43": ("stokes", 16, 0.4),
    "stokes_soup1500": ("stokes", 8, 0.4),
}
FIGURES = {
    "two_r54": dict(boxes=474, pairs=18936, targets=463, sources=(4, 161), le64=417, le128=45, gt128=1, levels=6),
    "soup2500": dict(boxes=1120, pairs=91305, targets=1109, sources=(2, 191), le64=305, le128=711, gt128=93, levels=8),
    "tiny48": dict(boxes=13, pairs=10, targets=7, sources=(1, 4), le64=7, le128=0, gt128=0, levels=4),
    "stokes_r43": dict(boxes=146, pairs=4072, targets=139, sources=(4, 55), le64=139, le128=0, gt128=0, levels=5),
    "stokes_soup1500": dict(boxes=672, pairs=40120, targets=660, sources=(1, 142), le64=373, le128=285, gt128=2, levels=8),
}
LAPLACE_FLAG_SETS = ("potential", "normal_deriv", "mixed")
STOKES_FLAG_SETS = ("velocity", "mixed3")


def vertices(O, name):
    """O: the oracle module (its generators are the project's own on the host)"""
    if name == "two_r54":
        return np.concatenate([O.unit_sphere(5), O.unit_sphere(4, center=(2.5, 0.3, -0.2))])
    if name == "soup2500":
        return _soup(11, 2500, 5, 3.0, 2.0)
    if name == "tiny48":
        return np.concatenate([O.unit_sphere(1), O.unit_sphere(1, center=(6.0, 0.5, 0.25)), O.unit_sphere(2, center=(0.3, 7.0, -1.0))])
    if name == "stokes_r43":
        return np.concatenate([O.unit_sphere(4), O.unit_sphere(3, center=(2.6, 0.2, -0.3))])
    if name == "stokes_soup1500":
        return _soup(11, 1500, 5, 3.0, 2.0)
    raise KeyError(name)


def is_stokes(name):
    return CASES[name][0] == "stokes"


def flags(name, flag_set, n):
    """None (all POTENTIAL / VELOCITY: expansion slot 0, Stokes slots 0..3), or the flags.  normal_deriv: slot 1 alone is live, so the
    kernels' slot table starts with 1; mixed: seeded, both slots; mixed3: panel i is TRACTION where i % 3 == 0, eleven slots"""
    if flag_set in ("potential", "velocity"):
        return None
    if flag_set == "normal_deriv":
        return np.ones(n, dtype=np.uint8)
    if flag_set == "mixed":
        return (np.random.default_rng(29).random(n) < 0.5).astype(np.uint8)
    if flag_set == "mixed3":
        return (np.arange(n) % 3 == 0).astype(np.uint8)
    raise KeyError(flag_set)


def live_slots(name, flag_set):
    return {"potential": (0,), "normal_deriv": (1,), "mixed": (0, 1), "velocity": (0, 1, 2, 3), "mixed3": tuple(range(11))}[flag_set]


def density(name, n, k=None):
    """the case's input vector ((n,), Stokes (n, 3)); k: a batch of k further vectors, (k, ...)"""
    rng = np.random.default_rng(41)
    shape = (n, 3) if is_stokes(name) else (n,)
    x = rng.standard_normal(shape)
    return x if k is None else rng.standard_normal((k,) + shape)


def make_oracle(O, name, flag_set):
    kind, ncrit, theta = CASES[name]
    v = vertices(O, name)
    bc = flags(name, flag_set, len(v))
    if kind == "laplace":
        return O.Oracle(v, bc=bc, K=LAPLACE_K, theta=theta, ncrit=ncrit, complete_l2l=True)
    assert bc is None, "the oracle's Stokes far field is the velocity branch only"
    return O.StokesOracle(v, K=STOKES_K, K_fine=STOKES_KFINE, mu=STOKES_MU, theta=theta, ncrit=ncrit, complete_l2l=True)


def m2l_figures(o):
    """the figures of FIGURES from an oracle's lists; pairs are (source box, target box)"""
    st = o.stats()
    pairs = o.pairs("m2l")
    per_target = np.bincount(pairs[:, 1], minlength=st["boxes"]) if len(pairs) else np.zeros(st["boxes"], dtype=np.int64)
    have = per_target[per_target > 0]
    return dict(boxes=st["boxes"], pairs=len(pairs), targets=len(have), sources=(int(have.min()), int(have.max())),
                le64=int(np.count_nonzero(have <= 64)), le128=int(np.count_nonzero((have > 64) & (have <= 128))),
                gt128=int(np.count_nonzero(have > 128)), levels=st["levels"]), st


def make_plan_args(fb, name, flag_set, p_max):
    """(args, kw) of fb.FMM_plan for a case, and the kernel object"""
    kind, ncrit, theta = CASES[name]
    v = vertices(fb, name)
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    opts.set_max_per_box(ncrit)
    if kind == "laplace":
        K = fb.LaplaceSphericalBEM(p_max, LAPLACE_K)
    else:
        K = fb.StokesSphericalBEM(p_max, STOKES_K, STOKES_MU)
        K.set_Kfine(STOKES_KFINE)
    return K, (K, v, opts), dict(bc=flags(name, flag_set, len(v)), p_max=p_max)


_ORACLES, _RESULTS = {}, {}


def reference(O, name, flag_set, p):
    """dict(y, L) of the oracle at order p: the matvec of density(name) and the local expansions of every box after it"""
    key = (name, flag_set)
    if key not in _ORACLES:
        _ORACLES[key] = make_oracle(O, name, flag_set)
    if key + (p,) not in _RESULTS:
        o = _ORACLES[key]
        y = o.matvec(density(name, o.n), p)
        L = o.expansions(p, "L")
        for a in (y, L):
            a.setflags(write=False)
        _RESULTS[key + (p,)] = dict(y=y, L=L)
    return _RESULTS[key + (p,)]

"""Host-side mirror of the reference's operator interface for the FMM matvec path.

Reference surface (C++ templates) -> here:
    FMMOptions                              include/FMMOptions.hpp:9-60        -> FMMOptions
    LaplaceSphericalBEM(p, k) / set_p(p)    kernel/LaplaceSphericalBEM.hpp:131-140 -> LaplaceSphericalBEM
    FMM_plan<K>(K, panels, opts)            include/FMM_plan.hpp:34-43         -> FMM_plan(K, panels, opts)
    plan.execute(charges) -> results        include/FMM_plan.hpp:75-90         -> FMM_plan.execute
    plan.kernel() / plan.options()          include/FMM_plan.hpp:66-71, 94-96  -> .kernel() / .options()
Same names, same argument meaning; errors are exceptions (FmmBemError) instead of exit()/printf.
All arithmetic happens in libfmmbem_hip.so on the GPU; this file only marshals arrays.
"""
import ctypes as C
import os

import numpy as np

from . import _capi


class FMMOptions:
    """include/FMMOptions.hpp:9-60 (fields the hot path reads)."""

    def __init__(self):
        self.lazy_evaluation = True     # FMMOptions.hpp:41
        # FMMOptions.hpp:18,91 (`-eval FMM|TREE`): "FMM" or "TREECODE" -- with lazy_evaluation the far field by M2L, L2L and L2P, or
        # every long-range pair by M2P (include/fmmbem.h FMMBEM_EVAL_TREECODE; Laplace, one device)
        self.evaluator = "FMM"
        self.local_evaluation = False
        self.sparse_local = True        # examples/LaplaceBEM.cpp:81 forces it
        self.block_diagonal = False
        self.theta = 0.5                # DefaultMAC(0.5), FMMOptions.hpp:45
        self.ncrit = 64                 # NCRIT_, FMMOptions.hpp:46
        # not in the reference: True applies exactly the L2L edges the reference's lazy evaluator queues, which on
        # adaptive trees leaves some boxes without their ancestors' far field (include/fmmbem.h, fmmbem_l2l_rule)
        self.reference_l2l = False
        # not in the reference: share of the near-field pairs kept as a matrix; < 1: the rest is recomputed every matvec by the
        # same kernel between its streamed items (include/fmmbem.h, fmmbem_options.near_stream_fraction)
        self.near_stream_fraction = 1.0
        # not in the reference: vectors one near-field pass of a Stokes plan serves in a batch (0, 1: off; 2, 3, 4;
        # include/fmmbem.h, fmmbem_options.stokes_batch_width)
        self.stokes_batch_width = 0

    def set_mac_theta(self, theta):     # FMMOptions.hpp:50-52
        self.theta = float(theta)

    def set_max_per_box(self, ncrit):   # FMMOptions.hpp:58-60
        self.ncrit = int(ncrit)

    def max_per_box(self):
        return self.ncrit


class _SingleOperators:
    """The translation operators one at a time -- P2M, M2M, M2L, L2L, L2P of kernel/KernelSkeleton.hpp:62-212 as the BEM kernels
    define them (kernel/LaplaceSphericalBEM.hpp:307-476, kernel/StokesSphericalBEM.hpp:391-530) -- run by the device kernels of
    the matvec on a two-box plan (fmmbem_ops_*, csrc/ops.hip).  Argument order and the "+=" into the last argument are the
    reference's; an expansion is a complex array (slots, p (p + 1) / 2), slots = 2 (Laplace: G, dG/dn) or 4 (Stokes: the stokeslet
    group M[0]); panels are (n, 3, 3) vertex arrays with one boundary-condition flag each (None: all 0)."""
    _ops = None
    device = 0

    def _handle(self):
        if self._ops is None or self._ops[1] != (self.K, getattr(self, "Mu", None), self.device):
            self._close()
            o = _capi.Options()
            _capi.lib().fmmbem_options_default(C.byref(o))
            o.p_max, o.quad_k, o.device = _capi.PMAX, self.K, int(self.device)
            if isinstance(self, StokesSphericalBEM):
                o.kernel, o.mu = _capi.KERNEL_STOKES_BEM, self.Mu
            h = C.c_void_p()
            _capi.check(_capi.lib().fmmbem_ops_create(C.byref(o), C.byref(h)))
            self._ops = (h, (self.K, getattr(self, "Mu", None), self.device))
        return self._ops[0]

    def _close(self):
        if self._ops is not None:
            _capi.lib().fmmbem_ops_destroy(self._ops[0])
            self._ops = None

    def __del__(self):
        try:
            self._close()
        except Exception:
            pass

    def slots(self):
        """expansions per box that P2M writes and L2P reads (multipole_type's size)"""
        return 4 if isinstance(self, StokesSphericalBEM) else 2

    def init_multipole(self, slots=None):
        """a zeroed multipole_type / local_type at the current order (init_multipole / init_local, LaplaceSphericalBEM.hpp:143-156)"""
        return np.zeros((self.slots() if slots is None else slots, self.P * (self.P + 1) // 2), dtype=np.complex128)

    init_local = init_multipole

    def _expansion(self, E, writable):
        S = self.P * (self.P + 1) // 2
        if not (isinstance(E, np.ndarray) and E.dtype == np.complex128 and E.ndim == 2 and E.shape[1] == S and E.flags.c_contiguous):
            raise ValueError("an expansion is a C-contiguous complex128 array (slots, p (p + 1) / 2) at the kernel's current p")
        if writable and not E.flags.writeable:
            raise ValueError("the target expansion must be writable")
        return E

    @staticmethod
    def _panels(panels, bc):
        v = np.ascontiguousarray(panels, dtype=np.float64).reshape(-1, 9)
        b = None
        if bc is not None:
            b = np.ascontiguousarray(bc, dtype=np.uint8)
            if b.shape != (len(v),):
                raise ValueError("one boundary-condition flag per panel")
        return v, b

    def P2M(self, sources, charges, center, M, bc=None):
        """M += the moments of the sources about center (P2M(source, charge, center, M), vectorised over the sources)"""
        v, b = self._panels(sources, bc)
        M = self._expansion(M, True)
        if M.shape[0] != self.slots():
            raise ValueError("P2M writes %d expansions" % self.slots())
        q = np.ascontiguousarray(charges, dtype=np.float64).reshape(-1)
        if q.size != len(v) * (3 if isinstance(self, StokesSphericalBEM) else 1):
            raise ValueError("one charge per source")
        c = np.ascontiguousarray(center, dtype=np.float64)
        vp = C.c_void_p
        _capi.check(_capi.lib().fmmbem_ops_p2m(self._handle(), self.P, len(v), v.ctypes.data_as(vp), None if b is None else b.ctypes.data_as(vp),
                                                q.ctypes.data_as(vp), c.ctypes.data_as(vp), M.ctypes.data_as(vp)))

    def _shift(self, fn, source, target, translation):
        source, target = self._expansion(source, False), self._expansion(target, True)
        if source.shape != target.shape:
            raise ValueError("source and target expansions differ in shape")
        t = np.ascontiguousarray(translation, dtype=np.float64)
        vp = C.c_void_p
        _capi.check(fn(self._handle(), self.P, source.shape[0], source.ctypes.data_as(vp), target.ctypes.data_as(vp), t.ctypes.data_as(vp)))

    def M2M(self, Msource, Mtarget, translation):
        """Mtarget += the source multipole moved by translation = centre(target) - centre(source)"""
        self._shift(_capi.lib().fmmbem_ops_m2m, Msource, Mtarget, translation)

    def M2L(self, Msource, Ltarget, translation):
        self._shift(_capi.lib().fmmbem_ops_m2l, Msource, Ltarget, translation)

    def L2L(self, Lsource, Ltarget, translation):
        self._shift(_capi.lib().fmmbem_ops_l2l, Lsource, Ltarget, translation)

    def L2P(self, L, center, targets, result, bc=None):
        """result += the local expansion about center evaluated at the targets' centroids (L2P(L, center, target, result))"""
        v, b = self._panels(targets, bc)
        L = self._expansion(L, False)
        if L.shape[0] != self.slots():
            raise ValueError("L2P reads %d expansions" % self.slots())
        dof = 3 if isinstance(self, StokesSphericalBEM) else 1
        if not (isinstance(result, np.ndarray) and result.dtype == np.float64 and result.size == len(v) * dof and result.flags.c_contiguous):
            raise ValueError("result must be a C-contiguous float64 array with one value (Stokes: three) per target")
        c = np.ascontiguousarray(center, dtype=np.float64)
        vp = C.c_void_p
        _capi.check(_capi.lib().fmmbem_ops_l2p(self._handle(), self.P, L.ctypes.data_as(vp), c.ctypes.data_as(vp), len(v), v.ctypes.data_as(vp),
                                                None if b is None else b.ctypes.data_as(vp), result.ctypes.data_as(vp)))


class LaplaceSphericalBEM(_SingleOperators):
    """Kernel descriptor: expansion order p and Gauss rule key k (kernel/LaplaceSphericalBEM.hpp:131)."""
    POTENTIAL, NORMAL_DERIV = _capi.BC_POTENTIAL, _capi.BC_NORMAL_DERIV

    def __init__(self, p=5, k=3):
        if not 1 <= int(p) <= _capi.PMAX:
            raise ValueError("p must be in 1..%d" % _capi.PMAX)
        self.P = int(p)
        self.K = int(k)

    def set_p(self, p):                 # kernel/LaplaceSphericalBEM.hpp:137-140
        if not 1 <= int(p) <= _capi.PMAX:
            raise ValueError("p must be in 1..%d" % _capi.PMAX)
        self.P = int(p)


class StokesSphericalBEM(_SingleOperators):
    """Kernel descriptor of kernel/StokesSphericalBEM.hpp:131-141: order p, Gauss key k, viscosity mu and the
    near-regime rule K_fine (ctor default 25; examples/StokesBEM.cpp:128-129,218 uses 19).  Only the VELOCITY
    boundary condition (stokeslet single layer, the operator the solve uses) is built; charges and results are
    Vec<3,double> per panel, i.e. arrays of shape (N, 3)."""
    VELOCITY, TRACTION = 0, 1

    def __init__(self, p=5, k=3, mu=1e-3):
        if not 1 <= int(p) <= _capi.PMAX:
            raise ValueError("p must be in 1..%d" % _capi.PMAX)
        self.P, self.K, self.Mu, self.K_fine = int(p), int(k), float(mu), 25

    def set_p(self, p):
        if not 1 <= int(p) <= _capi.PMAX:
            raise ValueError("p must be in 1..%d" % _capi.PMAX)
        self.P = int(p)

    def set_Kfine(self, k):
        self.K_fine = int(k)


def unit_sphere(recursions, center=(0.0, 0.0, 0.0)):
    """Triangulation::UnitSphere (examples/BEM/Triangulation.hpp:105-121) -> (N, 3, 3) vertex array."""
    n = C.c_size_t(0)
    _capi.check(_capi.lib().fmmbem_mesh_unit_sphere(recursions, None, C.byref(n)))
    v = np.empty((n.value, 3, 3), dtype=np.float64)
    _capi.check(_capi.lib().fmmbem_mesh_unit_sphere(recursions, v.ctypes.data_as(C.c_void_p), C.byref(n)))
    if any(center):
        v += np.asarray(center, dtype=np.float64)
    return v


def quadrature(key):
    """Triangle Gauss rule of examples/BEM/GaussQuadrature.hpp: (barycentric points (n, 3), weights (n,))."""
    pts, w, n = np.empty((_capi.MAX_QUAD, 3)), np.empty(_capi.MAX_QUAD), C.c_int(0)
    _capi.check(_capi.lib().fmmbem_quadrature(int(key), pts.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), C.byref(n)))
    return pts[:n.value].copy(), w[:n.value].copy()


def red_blood_cell(recursions):
    """Triangulation::RedBloodCell, identity rotation, zero shift (examples/BEM/Triangulation.hpp:184-255)."""
    n = C.c_size_t(0)
    _capi.check(_capi.lib().fmmbem_mesh_red_blood_cell(recursions, None, C.byref(n)))
    v = np.empty((n.value, 3, 3), dtype=np.float64)
    _capi.check(_capi.lib().fmmbem_mesh_red_blood_cell(recursions, v.ctypes.data_as(C.c_void_p), C.byref(n)))
    return v


def red_blood_cells(recursions, cells, placement=None):
    """Triangulation::MultipleRedBloodCell (examples/BEM/Triangulation.hpp:260-321).  placement: (cells, 6) rows of
    alpha, beta, gamma, shift x, y, z; None: the reference's own drand48-driven orientations and offsets."""
    pl = None
    if placement is not None:
        placement = np.ascontiguousarray(placement, dtype=np.float64)
        if placement.shape != (cells, 6):
            raise ValueError("placement must be (cells, 6)")
        pl = placement.ctypes.data_as(C.c_void_p)
    n = C.c_size_t(0)
    _capi.check(_capi.lib().fmmbem_mesh_red_blood_cells(recursions, cells, pl, None, C.byref(n)))
    v = np.empty((n.value, 3, 3), dtype=np.float64)
    _capi.check(_capi.lib().fmmbem_mesh_red_blood_cells(recursions, cells, pl, v.ctypes.data_as(C.c_void_p), C.byref(n)))
    return v


def kernel_entries(K, targets, sources, target_bc=None, device=0):
    """K(target_i, source_i) for n panel pairs -- Kernel::operator() of kernel/LaplaceSphericalBEM.hpp:273-297 /
    kernel/StokesSphericalBEM.hpp:377-389, evaluated on the device.  targets, sources: (n, 3, 3) vertices;
    target_bc: n flags (the target's flag selects G vs dG/dn).  Returns (n,) or (n, 3, 3)."""
    t = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 9)
    s = np.ascontiguousarray(sources, dtype=np.float64).reshape(-1, 9)
    if t.shape != s.shape:
        raise ValueError("one source per target")
    o = _capi.Options()
    _capi.lib().fmmbem_options_default(C.byref(o))
    o.quad_k, o.device = K.K, int(device)
    stokes = isinstance(K, StokesSphericalBEM)
    if stokes:
        o.kernel, o.mu, o.quad_k_fine = _capi.KERNEL_STOKES_BEM, K.Mu, K.K_fine
    bcp = None
    if target_bc is not None:
        target_bc = np.ascontiguousarray(target_bc, dtype=np.uint8)
        if target_bc.shape != (len(t),):
            raise ValueError("target_bc must have one flag per pair")
        bcp = target_bc.ctypes.data_as(C.c_void_p)
    out = np.empty((len(t), 3, 3) if stokes else len(t))
    _capi.check(_capi.lib().fmmbem_kernel_entries(C.byref(o), len(t), t.ctypes.data_as(C.c_void_p), bcp,
                                                  s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def kernel_gradient_entries(K, targets, sources, target_bc=None, device=0):
    """gamma(target_i, source_i) of the field gradient for n pairs (fmmbem_kernel_gradient_entries): the gradient, with respect to
    the target point, of the panel integral the target's flag picks, by the function FMM_plan.execute_gradient's near kernel calls.
    targets, sources: (n, 3, 3) vertices -- the target POINT is the target panel's centroid; target_bc: n flags.  Laplace only.
    Returns (n, 3)."""
    return _laplace_pair_entries("fmmbem_kernel_gradient_entries", (3,), K, targets, sources, target_bc, device)


def kernel_hessian_entries(K, targets, sources, target_bc=None, device=0):
    """eta(target_i, source_i) of the field Hessian for n pairs (fmmbem_kernel_hessian_entries): the derivative, with respect to the
    target point, of kernel_gradient_entries' gamma, by the function FMM_plan.execute_hessian's near kernel calls.  targets, sources:
    (n, 3, 3) vertices -- the target POINT is the target panel's centroid; target_bc: n flags.  Laplace only.  Returns (n, 3, 3),
    symmetric bit for bit."""
    return _laplace_pair_entries("fmmbem_kernel_hessian_entries", (3, 3), K, targets, sources, target_bc, device)


def _laplace_pair_entries(symbol, tail, K, targets, sources, target_bc, device):
    t = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 9)
    s = np.ascontiguousarray(sources, dtype=np.float64).reshape(-1, 9)
    if t.shape != s.shape:
        raise ValueError("one source per target")
    o = _capi.Options()
    _capi.lib().fmmbem_options_default(C.byref(o))
    o.quad_k, o.device = K.K, int(device)
    if isinstance(K, StokesSphericalBEM):
        o.kernel = _capi.KERNEL_STOKES_BEM                 # refused by the library (status 6)
    bcp = None
    if target_bc is not None:
        target_bc = np.ascontiguousarray(target_bc, dtype=np.uint8)
        if target_bc.shape != (len(t),):
            raise ValueError("target_bc must have one flag per pair")
        bcp = target_bc.ctypes.data_as(C.c_void_p)
    out = np.empty((len(t),) + tail)
    _capi.check(getattr(_capi.lib(), symbol)(C.byref(o), len(t), t.ctypes.data_as(C.c_void_p), bcp,
                                             s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def kernel_pressure_entries(K, targets, sources, device=0):
    """pi(target_i, source_i) of the field pressure for n pairs (fmmbem_kernel_pressure_entries): the row vector with q += pi . x_j,
    by the function FMM_plan.execute_pressure's near kernel calls.  targets, sources: (n, 3, 3) vertices -- the target POINT is the
    target panel's centroid.  Stokes only.  Returns (n, 3)."""
    t = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 9)
    s = np.ascontiguousarray(sources, dtype=np.float64).reshape(-1, 9)
    if t.shape != s.shape:
        raise ValueError("one source per target")
    o = _capi.Options()
    _capi.lib().fmmbem_options_default(C.byref(o))
    o.quad_k, o.device = K.K, int(device)
    if isinstance(K, StokesSphericalBEM):
        o.kernel, o.mu, o.quad_k_fine = _capi.KERNEL_STOKES_BEM, K.Mu, K.K_fine
    out = np.empty((len(t), 3))
    _capi.check(_capi.lib().fmmbem_kernel_pressure_entries(C.byref(o), len(t), t.ctypes.data_as(C.c_void_p),
                                                           s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def kernel_velocity_gradient_entries(K, targets, sources, device=0):
    """Gamma(target_i, source_i) of the field velocity gradient for n pairs (fmmbem_kernel_velocity_gradient_entries): the tensor
    with G[k][m] += sum_e Gamma[k][m][e] x_j[e], the 1/(2 mu) included, by the function FMM_plan.execute_velocity_gradient's near
    kernel calls.  targets, sources: (n, 3, 3) vertices -- the target POINT is the target panel's centroid.  Stokes only.
    Returns (n, 3, 3, 3)."""
    t = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 9)
    s = np.ascontiguousarray(sources, dtype=np.float64).reshape(-1, 9)
    if t.shape != s.shape:
        raise ValueError("one source per target")
    o = _capi.Options()
    _capi.lib().fmmbem_options_default(C.byref(o))
    o.quad_k, o.device = K.K, int(device)
    if isinstance(K, StokesSphericalBEM):
        o.kernel, o.mu, o.quad_k_fine = _capi.KERNEL_STOKES_BEM, K.Mu, K.K_fine
    out = np.empty((len(t), 3, 3, 3))
    _capi.check(_capi.lib().fmmbem_kernel_velocity_gradient_entries(C.byref(o), len(t), t.ctypes.data_as(C.c_void_p),
                                                                    s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


class Direct:
    """Direct::matvec (include/Direct.hpp:232-302) on the device: y_i = sum_j K(t_i, s_j) x_j over ALL the panels, every entry the
    one kernel_entries gives for that pair (fmmbem_direct_*, csrc/kernels_direct.hip).  Laplace and Stokes; no tree, no matrix.

    panels: (N, 3, 3) source triangles; they carry no flags -- the TARGET's flag picks the operator (Laplace G / dG/dn; Stokes
    velocity / the double layer with the source's normal).  The order of addition is fixed (chunks of .chunk sources, ascending),
    so a result's bits do not depend on how many targets a call holds.  The same handle sums the field quantities at points:
    gradient (Laplace), pressure, velocity_gradient and stress (Stokes) -- what FMM_plan.execute_gradient / execute_pressure /
    execute_velocity_gradient / execute_stress approximate.
    """

    def __init__(self, K, panels, device=0):
        v = np.ascontiguousarray(panels, dtype=np.float64).reshape(-1, 9)
        self._K = K
        self.n = v.shape[0]
        self.device = int(device)
        self.dof = 3 if isinstance(K, StokesSphericalBEM) else 1
        o = _capi.Options()
        _capi.lib().fmmbem_options_default(C.byref(o))
        o.quad_k, o.device = K.K, self.device
        if self.dof == 3:
            o.kernel, o.mu, o.quad_k_fine = _capi.KERNEL_STOKES_BEM, K.Mu, K.K_fine
        h = C.c_void_p()
        self._h = None
        _capi.check(_capi.lib().fmmbem_direct_create(C.byref(o), self.n, v.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._h = h

    @property
    def chunk(self):
        """sources per partial sum (fmmbem_direct_chunk)"""
        return _capi.lib().fmmbem_direct_chunk()

    def kernel(self):
        return self._K

    def _targets(self, targets, target_bc):
        if targets is None:
            t, m = None, self.n
        else:
            t = np.asarray(targets, dtype=np.float64)
            if t.ndim == 3 and t.shape[1:] == (3, 3):
                t = (t[:, 0] + t[:, 1] + t[:, 2]) / 3          # a Panel target: its centre, as FMM_plan(targets=...) takes it
            if t.ndim != 2 or t.shape[1] != 3:
                raise ValueError("targets must be (M, 3) points or (M, 3, 3) triangles")
            t, m = np.ascontiguousarray(t), t.shape[0]
        if target_bc is not None:
            target_bc = np.ascontiguousarray(target_bc, dtype=np.uint8)
            if target_bc.shape != (m,):
                raise ValueError("target_bc must have one flag per target")
        return t, target_bc, m

    def matvec(self, x, targets=None, target_bc=None):
        """x: (N,) -- (N, 3) for Stokes.  targets: (M, 3) points or (M, 3, 3) triangles standing for their centroids; None: the
        symmetric form, the targets are the panels' own centroids and target_bc their flags.  Returns (M,) or (M, 3).  numpy in,
        numpy out (host)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        want = (self.n,) if self.dof == 1 else (self.n, 3)
        if x.shape != want:
            raise ValueError("x must have shape %r" % (want,))
        t, bc, m = self._targets(targets, target_bc)
        y = np.empty((m,) if self.dof == 1 else (m, 3))
        vp = C.c_void_p
        _capi.check(_capi.lib().fmmbem_direct_apply(self._h, m, None if t is None else t.ctypes.data_as(vp),
                                                    None if bc is None else bc.ctypes.data_as(vp), x.ctypes.data_as(vp), y.ctypes.data_as(vp)))
        return y

    def matvec_torch(self, x, targets=None, target_bc=None, out=None):
        """The same sum on device tensors, asynchronous on torch's current stream.  x: contiguous float64 CUDA tensor of N * dof
        values; targets: contiguous float64 CUDA tensor (M, 3) or None; target_bc: uint8 CUDA tensor (M,) or None."""
        import torch
        if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.numel() != self.n * self.dof:
            raise ValueError("x must be a contiguous float64 CUDA tensor with dof values per panel")
        if x.device.index != self.device:
            raise ValueError("x lives on cuda:%s but the Direct sum was built on device %d" % (x.device.index, self.device))
        m = self.n
        if targets is not None:
            if (targets.dtype != torch.float64 or targets.device != x.device or not targets.is_contiguous() or targets.dim() != 2
                    or targets.shape[1] != 3):
                raise ValueError("targets must be a contiguous float64 tensor (M, 3) on x's device")
            m = targets.shape[0]
        if target_bc is not None and (target_bc.dtype != torch.uint8 or target_bc.device != x.device or not target_bc.is_contiguous()
                                      or tuple(target_bc.shape) != (m,)):
            raise ValueError("target_bc must be a contiguous uint8 tensor (M,) on x's device")
        shape = (m,) if self.dof == 1 else (m, 3)
        if out is None:
            out = x.new_empty(shape)
        elif out.dtype != torch.float64 or out.device != x.device or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError("out must be a contiguous float64 tensor of shape %r on x's device" % (shape,))
        vp = C.c_void_p
        _capi.check(_capi.lib().fmmbem_direct_apply_device(
            self._h, m, None if targets is None else vp(targets.data_ptr()), None if target_bc is None else vp(target_bc.data_ptr()),
            vp(x.data_ptr()), vp(out.data_ptr()), vp(torch.cuda.current_stream(x.device).cuda_stream)))
        return out

    # ---- the field quantities at points (include/fmmbem.h, "Direct sum: field quantities"): the all-pairs sums that
    # FMM_plan.execute_gradient / execute_pressure / execute_velocity_gradient approximate, every pair's value the one
    # kernel_gradient_entries / kernel_pressure_entries / kernel_velocity_gradient_entries gives, the order of addition fixed ----
    def _field_host(self, symbol, x, targets, target_bc, tail, flags):
        x = np.ascontiguousarray(x, dtype=np.float64)
        want = (self.n,) if self.dof == 1 else (self.n, 3)
        if x.shape != want:
            raise ValueError("x must have shape %r" % (want,))
        if targets is None:
            raise ValueError("targets must be (M, 3) points or (M, 3, 3) triangles (the field quantities have no symmetric form)")
        t, bc, m = self._targets(targets, target_bc)
        out = np.empty((m,) + tail)
        vp = C.c_void_p
        args = [self._h, m, t.ctypes.data_as(vp)] + ([None if bc is None else bc.ctypes.data_as(vp)] if flags else [])
        _capi.check(getattr(_capi.lib(), symbol)(*args, x.ctypes.data_as(vp), out.ctypes.data_as(vp)))
        return out

    def _field_torch(self, symbol, x, targets, target_bc, out, tail, flags):
        import torch
        if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.numel() != self.n * self.dof:
            raise ValueError("x must be a contiguous float64 CUDA tensor with dof values per panel")
        if x.device.index != self.device:
            raise ValueError("x lives on cuda:%s but the Direct sum was built on device %d" % (x.device.index, self.device))
        if (targets is None or targets.dtype != torch.float64 or targets.device != x.device or not targets.is_contiguous()
                or targets.dim() != 2 or targets.shape[1] != 3):
            raise ValueError("targets must be a contiguous float64 tensor (M, 3) on x's device")
        m = targets.shape[0]
        if target_bc is not None and (target_bc.dtype != torch.uint8 or target_bc.device != x.device or not target_bc.is_contiguous()
                                      or tuple(target_bc.shape) != (m,)):
            raise ValueError("target_bc must be a contiguous uint8 tensor (M,) on x's device")
        shape = (m,) + tail
        if out is None:
            out = x.new_empty(shape)
        elif out.dtype != torch.float64 or out.device != x.device or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError("out must be a contiguous float64 tensor of shape %r on x's device" % (shape,))
        vp = C.c_void_p
        args = [self._h, m, vp(targets.data_ptr())] + ([None if target_bc is None else vp(target_bc.data_ptr())] if flags else [])
        _capi.check(getattr(_capi.lib(), symbol)(*args, vp(x.data_ptr()), vp(out.data_ptr()),
                                                 vp(torch.cuda.current_stream(x.device).cuda_stream)))
        return out

    def gradient(self, x, targets, target_bc=None):
        """(N,) charges -> (M, 3): g_i = sum_j gamma(t_i, s_j) x_j over ALL panels, gamma that of FMM_plan.execute_gradient, picked by
        target_bc[i] (None: all 0).  Laplace only: FmmBemError (status 6) on a Stokes kernel.  numpy in, numpy out (host)."""
        return self._field_host("fmmbem_direct_gradient", x, targets, target_bc, (3,), True)

    def gradient_torch(self, x, targets, target_bc=None, out=None):
        """The same sum on device tensors, asynchronous on torch's current stream; returns (M, 3)."""
        return self._field_torch("fmmbem_direct_gradient_device", x, targets, target_bc, out, (3,), True)

    def hessian(self, x, targets, target_bc=None):
        """(N,) charges -> (M, 3, 3): H_i[a][b] = sum_j eta_ab(t_i, s_j) x_j over ALL panels, eta that of FMM_plan.execute_hessian,
        picked by target_bc[i] (None: all 0); symmetric bit for bit.  Laplace only: FmmBemError (status 6) on a Stokes kernel.  numpy
        in, numpy out (host)."""
        return self._field_host("fmmbem_direct_hessian", x, targets, target_bc, (3, 3), True)

    def hessian_torch(self, x, targets, target_bc=None, out=None):
        """The same sum on device tensors, asynchronous on torch's current stream; returns (M, 3, 3)."""
        return self._field_torch("fmmbem_direct_hessian_device", x, targets, target_bc, out, (3, 3), True)

    def pressure(self, x, targets):
        """(N, 3) traction density -> (M,): q_i = sum_j pi(t_i, s_j) . x_j over ALL panels, in the scaling of
        FMM_plan.execute_pressure (the physical pressure is q / 4 pi).  Stokes only: FmmBemError (status 6) on a Laplace kernel."""
        return self._field_host("fmmbem_direct_pressure", x, targets, None, (), False)

    def pressure_torch(self, x, targets, out=None):
        """The same sum on device tensors, asynchronous on torch's current stream; returns (M,)."""
        return self._field_torch("fmmbem_direct_pressure_device", x, targets, None, out, (), False)

    def velocity_gradient(self, x, targets):
        """(N, 3) traction density -> (M, 3, 3): G_i[k][m] = d u'_k / d t_m over ALL panels, in the scaling of
        FMM_plan.execute_velocity_gradient (the 1/(2 mu) included).  Stokes only: FmmBemError (status 6) on a Laplace kernel."""
        return self._field_host("fmmbem_direct_velocity_gradient", x, targets, None, (3, 3), False)

    def velocity_gradient_torch(self, x, targets, out=None):
        """The same sum on device tensors, asynchronous on torch's current stream; returns (M, 3, 3)."""
        return self._field_torch("fmmbem_direct_velocity_gradient_device", x, targets, None, out, (3, 3), False)

    def stress(self, x, targets):
        """(N, 3) traction density -> (M, 3, 3): sigma_i[k][m] = -q_i delta_km + mu (G_i[k][m] + G_i[m][k]), q of pressure and G of
        velocity_gradient, composed as FMM_plan.execute_stress composes it (the physical stress is the result / 4 pi)."""
        q = self.pressure(x, targets)
        g = self.velocity_gradient(x, targets)
        return -q[:, None, None] * np.eye(3)[None] + self._K.Mu * (g + g.transpose(0, 2, 1))

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().fmmbem_direct_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _read(fn, *paths):
    n = C.c_size_t(0)
    args = [os.fsencode(p) for p in paths]
    _capi.check(fn(*args, None, C.byref(n)))
    v = np.empty((n.value, 3, 3), dtype=np.float64)
    _capi.check(fn(*args, v.ctypes.data_as(C.c_void_p), C.byref(n)))
    return v


def read_msh(path):
    """MeshIO::readMsh (examples/BEM/MshReader.hpp:18-94): gmsh v2 ASCII triangles -> (N, 3, 3)."""
    return _read(_capi.lib().fmmbem_mesh_read_msh, path)


def read_vert_face(vert_path, face_path):
    """MeshIO::ReadVertFace (examples/BEM/VertFaceReader.hpp:17-76) -> (N, 3, 3)."""
    return _read(_capi.lib().fmmbem_mesh_read_vert_face, vert_path, face_path)


def write_vert_face(vert_path, face_path, panels):
    """The .vert/.face dump of the generators (examples/BEM/Triangulation.hpp:124-134), readable by read_vert_face."""
    v = np.ascontiguousarray(panels, dtype=np.float64).reshape(-1, 9)
    _capi.check(_capi.lib().fmmbem_mesh_write_vert_face(os.fsencode(vert_path), os.fsencode(face_path),
                                                        v.ctypes.data_as(C.c_void_p), len(v)))


class FMM_plan:
    """FMM_plan<LaplaceSphericalBEM> (include/FMM_plan.hpp:16-128).

    panels: (N, 3, 3) triangle vertices (the arguments of Panel(p0, p1, p2)); bc: N boundary flags.
    p_max: largest order later set through kernel().set_p (defaults to K.P, or 16 if the caller
    intends to relax p upward).

    targets: the reference's FMM_plan(K, sources, targets, opts) (include/FMM_plan.hpp:45-55) -- (M, 3) points, or (M, 3, 3)
    triangles standing for their centroids; target_bc: M flags (default POTENTIAL).  execute then returns the M values
    y_i = sum_j K(t_i, s_j) x_j, the target's flag picking G or dG/dn (fmmbem_plan_create_targets; Laplace only -- the field of
    either kernel at points: field_plan).

    near_f32_max_p: not in the reference.  0: off; 1..16: executes at an order p <= this value stream a float copy of the
    assembled near matrix (fmmbem_options.near_f32_max_p); stats() reports near_f32_bytes (0: not active on this plan) and
    last_near_f32.

    stokes_batch_width: not in the reference.  0 or 1: off; 2, 3, 4: on a Stokes plan one pass over the near matrix serves that
    many vectors of execute_batch / gmres_capi_batch (fmmbem_options.stokes_batch_width), every result the bits of its single
    execute; batch_width() reports it where it is active.  None (default): opts.stokes_batch_width.
    """

    def __init__(self, K, panels, opts=None, bc=None, p_max=None, device=0, shard=(0, 1), host_only=False,
                 shard_upward=False, devices=None, replicate_upward=False, targets=None, target_bc=None, near_f32_max_p=0,
                 stokes_batch_width=None):
        opts = opts if opts is not None else FMMOptions()
        # executor/make_executor.hpp:24-60: lazy_evaluation wins, then local_evaluation, then block_diagonal; the
        # non-lazy upward/interact/downward evaluators compute the same operator as the lazy ones
        which = getattr(opts, "evaluator", "FMM")
        if which not in ("FMM", "TREECODE"):
            raise ValueError('FMMOptions.evaluator is "FMM" or "TREECODE"')
        evaluator = _capi.EVAL_TREECODE if which == "TREECODE" else _capi.EVAL_FMM
        if not opts.lazy_evaluation:
            evaluator = _capi.EVAL_FMM                 # local_evaluation and block_diagonal have no far field to choose
            if opts.local_evaluation:
                evaluator = _capi.EVAL_LOCAL
            elif opts.block_diagonal:
                evaluator = _capi.EVAL_BLOCK_DIAGONAL
        self._K = K
        self._opts = opts
        v = np.ascontiguousarray(panels, dtype=np.float64).reshape(-1, 9)
        self.n = v.shape[0]
        o = _capi.Options()
        _capi.lib().fmmbem_options_default(C.byref(o))
        o.p_max = int(p_max if p_max is not None else K.P)
        o.quad_k = K.K
        o.theta = opts.theta
        o.ncrit = opts.ncrit
        o.sparse_local = 1 if opts.sparse_local else 0
        o.host_only = 1 if host_only else 0
        o.evaluator = evaluator
        o.l2l_rule = _capi.L2L_REFERENCE if getattr(opts, "reference_l2l", False) else _capi.L2L_COMPLETE
        o.near_stream_fraction = float(getattr(opts, "near_stream_fraction", 1.0))
        o.near_f32_max_p = int(near_f32_max_p)
        o.stokes_batch_width = int(getattr(opts, "stokes_batch_width", 0) if stokes_batch_width is None else stokes_batch_width)
        o.device = int(device)
        self.device = int(device)
        if devices is not None and len(devices) > 1:
            # one plan over several devices of this process (fmmbem_options.n_devices): vectors live on devices[0]
            if len(devices) > 8:
                raise ValueError("at most 8 devices per plan")
            o.n_devices = len(devices)
            for i, dv in enumerate(devices):
                o.devices[i] = int(dv)
            o.device = self.device = int(devices[0])
        self.dof = 1
        if isinstance(K, StokesSphericalBEM):
            o.kernel = _capi.KERNEL_STOKES_BEM
            o.mu = K.Mu
            o.quad_k_fine = K.K_fine
            self.dof = 3
        o.shard_rank, o.shard_world = int(shard[0]), int(shard[1])
        self._shard_world = int(shard[1])
        # shard_upward: False / True (1: all-gather of the multipoles) / 2 (all-to-all of the ones each receiver reads)
        o.shard_upward = (2 if shard_upward == 2 else 1) if (shard_upward and int(shard[1]) > 1) else 0
        if o.n_devices > 1:                    # inside a multi-device plan: owners + selective exchange, or every device repeats the upward pass
            o.shard_upward = 0 if replicate_upward else 2
        self.shard_upward = bool(o.shard_upward)
        self.exchange_mode = int(o.shard_upward)
        self.p_max = o.p_max
        bcp = None
        if bc is not None:
            bc = np.ascontiguousarray(bc, dtype=np.uint8)
            if bc.shape != (self.n,):
                raise ValueError("bc must have one flag per panel")
            bcp = bc.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        self.n_targets = None
        self._created_from = (v, o)                        # what field_plan builds its plan from
        if targets is None:
            if target_bc is not None:
                raise ValueError("target_bc without targets")
            _capi.check(_capi.lib().fmmbem_plan_create(C.byref(o), self.n, v.ctypes.data_as(C.c_void_p), bcp, C.byref(h)))
        else:
            t, target_bc, tbcp = self._target_points(targets, target_bc)
            self._targets = (t, target_bc)                 # kept alive with the plan
            _capi.check(_capi.lib().fmmbem_plan_create_targets(C.byref(o), self.n, v.ctypes.data_as(C.c_void_p), bcp, t.shape[0],
                                                               t.ctypes.data_as(C.c_void_p), tbcp, C.byref(h)))
            self.n_targets = t.shape[0]
        self._h = h

    @staticmethod
    def _target_points(targets, target_bc):
        t = np.asarray(targets, dtype=np.float64)
        if t.ndim == 3 and t.shape[1:] == (3, 3):
            t = (t[:, 0] + t[:, 1] + t[:, 2]) / 3              # a Panel target: its centre (LaplaceSphericalBEM.hpp:64-97)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("targets must be (M, 3) points or (M, 3, 3) triangles")
        t = np.ascontiguousarray(t)
        tbcp = None
        if target_bc is not None:
            target_bc = np.ascontiguousarray(target_bc, dtype=np.uint8)
            if target_bc.shape != (t.shape[0],):
                raise ValueError("target_bc must have one flag per target")
            tbcp = target_bc.ctypes.data_as(C.c_void_p)
        return t, target_bc, tbcp

    def field_plan(self, points, target_bc=None):
        """The field of a layer on this plan's panels at points of their own (fmmbem_plan_create_field), either kernel: a plan over
        the same kernel object, panels and options whose execute takes (N,) -- Stokes (N, 3) -- charges and returns
        y_i = sum_j K(t_i, s_j) x_j as (M,) -- Stokes (M, 3).  points: (M, 3), or (M, 3, 3) triangles standing for their centroids;
        target_bc: M flags (default 0) -- the TARGET's flag picks the operator (Stokes: VELOCITY the single layer, TRACTION the double
        layer with the source's normal), the panels' own flags do not enter.  execute_torch, execute_batch(_torch), set_graphs,
        target_info, target_boxes, target_perm, pairs and boxes work as on a targets= plan.  FmmBemError (status 6) on a plan that is
        itself a target plan, and on a treecode, LOCAL, BLOCK_DIAGONAL, matrix-free, sharded or device-list plan."""
        if self.n_targets is not None:
            raise _capi.FmmBemError(_capi.ERR_UNSUPPORTED, "field_plan: this plan is itself a plan over separate targets")
        v, o = self._created_from
        t, target_bc, tbcp = self._target_points(points, target_bc)
        h = C.c_void_p()
        _capi.check(_capi.lib().fmmbem_plan_create_field(C.byref(o), self.n, v.ctypes.data_as(C.c_void_p), t.shape[0],
                                                         t.ctypes.data_as(C.c_void_p), tbcp, C.byref(h)))
        other = object.__new__(type(self))                 # this plan's attributes with the new handle, as like()
        other.__dict__.update(self.__dict__, _h=h)
        other._targets = (t, target_bc)
        other.n_targets = t.shape[0]
        return other

    def like(self, bc, K=None):
        """A plan of the same panels and options with other boundary-condition flags (fmmbem_plan_create_like): shares this
        plan's tree, lists and tables; builds only the near-matrix values, P2M moments and expansions.  The drivers'
        right-hand-side plan (examples/LaplaceBEM.cpp:218-232).  K: the kernel object the new plan reads its order from
        (default: this plan's)."""
        bcp = None
        if bc is not None:
            bc = np.ascontiguousarray(bc, dtype=np.uint8)
            if bc.shape != (self.n,):
                raise ValueError("bc must have one flag per panel")
            bcp = bc.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        _capi.check(_capi.lib().fmmbem_plan_create_like(self._h, bcp, C.byref(h)))
        other = object.__new__(type(self))             # this plan's attributes with the new handle: never this plan's own
        other.__dict__.update(self.__dict__, _h=h)
        other._K = K if K is not None else self._K
        return other

    # ---- reference surface ----
    def kernel(self):
        return self._K

    def options(self):
        return self._opts

    def execute(self, charges):
        """results = plan.execute(charges) at the kernel's current p. numpy in, numpy out (host)."""
        x = np.ascontiguousarray(charges, dtype=np.float64)
        want = (self.n,) if self.dof == 1 else (self.n, self.dof)
        if x.shape != want:
            raise ValueError("charges must have shape %r" % (want,))
        y = np.empty(want if self.n_targets is None else self._target_shape())
        _capi.check(_capi.lib().fmmbem_plan_execute(self._h, self._K.P, x.ctypes.data_as(C.c_void_p),
                                                    y.ctypes.data_as(C.c_void_p)))
        return y

    def _target_shape(self):
        return (self.n_targets,) if self.dof == 1 else (self.n_targets, self.dof)

    def __call__(self, x, y):
        """Preconditioner-style operator()(x, y) adapter (examples/BEM/Preconditioner.hpp:11-15)."""
        y[...] = self.execute(x)

    # ---- device-resident variant (torch tensors or raw device pointers) ----
    def execute_device(self, x_ptr, y_ptr, stream=0, p=None):
        _capi.check(_capi.lib().fmmbem_plan_execute_device(self._h, self._K.P if p is None else int(p),
                                                           C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_void_p(stream)))

    # ---- split execute of a plan that shards the upward pass (include/fmmbem.h) ----
    def exchange_counts(self, p=None):
        """shard_upward = 2: (send, recv) int64 arrays of doubles per peer shard at order p (fmmbem_plan_exchange_counts)."""
        w = self._shard_world
        send, recv = np.zeros(w, dtype=np.int64), np.zeros(w, dtype=np.int64)
        _capi.check(_capi.lib().fmmbem_plan_exchange_counts(self._h, self._K.P if p is None else int(p),
                                                             send.ctypes.data_as(C.c_void_p), recv.ctypes.data_as(C.c_void_p)))
        return send, recv

    def exchange_doubles(self, p=None):
        n = C.c_size_t(0)
        _capi.check(_capi.lib().fmmbem_plan_exchange_doubles(self._h, self._K.P if p is None else int(p), C.byref(n)))
        return n.value

    def upward_device(self, x_ptr, send_ptr, stream=0, p=None):
        _capi.check(_capi.lib().fmmbem_plan_upward_device(self._h, self._K.P if p is None else int(p), C.c_void_p(x_ptr),
                                                          C.c_void_p(send_ptr), C.c_void_p(stream)))

    def downward_device(self, recv_ptr, y_ptr, stream=0, p=None):
        _capi.check(_capi.lib().fmmbem_plan_downward_device(self._h, self._K.P if p is None else int(p), C.c_void_p(recv_ptr),
                                                            C.c_void_p(y_ptr), C.c_void_p(stream)))

    def near_split_device(self, y_ptr, stream=0):
        _capi.check(_capi.lib().fmmbem_plan_near_split_device(self._h, C.c_void_p(y_ptr), C.c_void_p(stream)))

    # ---- results as tree-order slices (multi-GPU all-gather instead of all-reduce, include/fmmbem.h) ----
    def set_result_slices(self, on=True):
        _capi.check(_capi.lib().fmmbem_plan_set_result_slices(self._h, 1 if on else 0))

    def shard_rows(self, world):
        cut = np.empty(world + 1, dtype=np.int64)
        _capi.check(_capi.lib().fmmbem_plan_shard_rows(self._h, cut.ctypes.data_as(C.c_void_p)))
        return cut

    def assemble_slices_device(self, slices_ptr, chunk_doubles, y_ptr, stream=0):
        _capi.check(_capi.lib().fmmbem_plan_assemble_slices_device(self._h, C.c_void_p(slices_ptr), int(chunk_doubles),
                                                                  C.c_void_p(y_ptr), C.c_void_p(stream)))

    def near_device(self, x_ptr, y_ptr, stream=0):
        _capi.check(_capi.lib().fmmbem_plan_near_device(self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_void_p(stream)))

    def execute_torch(self, x, out=None, p=None):
        """x: float64 CUDA tensor (N,), ORIGINAL panel order. Runs on torch's current stream."""
        import torch
        if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.numel() != self.n * self.dof:
            raise ValueError("x must be a contiguous float64 CUDA tensor with dof values per panel")
        if x.device.index != self.device:
            raise ValueError("x lives on cuda:%s but the plan was built on device %d" % (x.device.index, self.device))
        if out is None:
            out = torch.empty_like(x) if self.n_targets is None else x.new_empty(self._target_shape())
        self.execute_device(x.data_ptr(), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream, p)
        return out

    # ---- field quantities at the points of a targets= plan or a field plan (include/fmmbem.h): the Laplace gradient, the pressure and
    # the velocity gradient of the Stokes single layer.  One form each for numpy (host), raw device pointers and torch ----
    def _field_rows(self):
        return self.n if self.n_targets is None else self.n_targets

    def _field_host(self, symbol, charges, tail, per):
        x = np.ascontiguousarray(charges, dtype=np.float64)
        if x.shape != (self.n * self.dof,) and x.shape != (self.n, self.dof):
            raise ValueError("charges must have %s per panel" % per)
        out = np.empty((self._field_rows(),) + tail)
        _capi.check(getattr(_capi.lib(), symbol)(self._h, self._K.P, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def _field_device(self, symbol, x_ptr, out_ptr, stream, p):
        _capi.check(getattr(_capi.lib(), symbol)(self._h, self._K.P if p is None else int(p), C.c_void_p(x_ptr), C.c_void_p(out_ptr),
                                                 C.c_void_p(stream)))

    def _field_torch(self, execute_device, x, out, p, tail, per):
        import torch
        if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.numel() != self.n * self.dof:
            raise ValueError("x must be a contiguous float64 CUDA tensor with %s per panel" % per)
        if x.device.index != self.device:
            raise ValueError("x lives on cuda:%s but the plan was built on device %d" % (x.device.index, self.device))
        shape = (self._field_rows(),) + tail
        if out is None:
            out = x.new_empty(shape)
        elif out.dtype != torch.float64 or out.device != x.device or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError("out must be a contiguous float64 tensor of shape %r on x's device" % (shape,))
        execute_device(x.data_ptr(), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream, p)
        return out

    def execute_gradient(self, charges):
        """(N,) charges -> (M, 3): g_i = sum_j gamma(t_i, s_j) x_j at the kernel's current p, gamma the gradient with respect to the
        target point of the integrand the target's flag picks (include/fmmbem.h, "Field gradient").  numpy in, numpy out (host).
        FmmBemError (status 6) on a plan that is not over separate targets, on a Stokes plan and on a host-only plan."""
        return self._field_host("fmmbem_plan_execute_gradient", charges, (3,), "one value")

    def execute_gradient_device(self, x_ptr, g_ptr, stream=0, p=None):
        self._field_device("fmmbem_plan_execute_gradient_device", x_ptr, g_ptr, stream, p)

    def execute_gradient_torch(self, x, out=None, p=None):
        """x: contiguous float64 CUDA tensor (N,), ORIGINAL panel order; returns (M, 3).  Runs on torch's current stream."""
        return self._field_torch(self.execute_gradient_device, x, out, p, (3,), "one value")

    def execute_hessian(self, charges):
        """(N,) charges -> (M, 3, 3): H_i[a][b] = sum_j eta_ab(t_i, s_j) x_j at the kernel's current p, the second derivatives with
        respect to the target point of what execute returns there (include/fmmbem.h, "Field Hessian"); H[a][b] and H[b][a] carry the
        same bits.  numpy in, numpy out (host).  FmmBemError (status 6) on a plan that is not over separate targets, on a Stokes plan
        and on a host-only plan."""
        return self._field_host("fmmbem_plan_execute_hessian", charges, (3, 3), "one value")

    def execute_hessian_device(self, x_ptr, h_ptr, stream=0, p=None):
        self._field_device("fmmbem_plan_execute_hessian_device", x_ptr, h_ptr, stream, p)

    def execute_hessian_torch(self, x, out=None, p=None):
        """x: contiguous float64 CUDA tensor (N,), ORIGINAL panel order; returns (M, 3, 3).  Runs on torch's current stream."""
        return self._field_torch(self.execute_hessian_device, x, out, p, (3, 3), "one value")

    def execute_pressure(self, charges):
        """(N, 3) or (3N,) traction density -> (M,): q_i = sum_j pi(t_i, s_j) . x_j at the kernel's current p, the pressure that
        belongs to the velocity execute returns (include/fmmbem.h, "Field pressure"; the physical pressure is q / 4 pi).  numpy in,
        numpy out (host).  FmmBemError (status 6) on a plan that is not over separate targets, on a Laplace plan, on a plan with a
        TRACTION target and on a host-only plan."""
        return self._field_host("fmmbem_plan_execute_pressure", charges, (), "dof values")

    def execute_pressure_device(self, x_ptr, q_ptr, stream=0, p=None):
        self._field_device("fmmbem_plan_execute_pressure_device", x_ptr, q_ptr, stream, p)

    def execute_pressure_torch(self, x, out=None, p=None):
        """x: contiguous float64 CUDA tensor with 3 values per panel, ORIGINAL panel order; returns (M,).  Runs on torch's current
        stream."""
        return self._field_torch(self.execute_pressure_device, x, out, p, (), "dof values")

    def execute_velocity_gradient(self, traction):
        """(N, 3) or (3N,) traction density -> (M, 3, 3): G_i[k][m] = d u'_k / d t_m at the kernel's current p, u' what execute
        returns (include/fmmbem.h, "Field velocity gradient"; the physical gradient is G / 4 pi).  numpy in, numpy out (host).
        FmmBemError (status 6) on a plan that is not over separate targets, on a Laplace plan, on a plan with a TRACTION target and
        on a host-only plan."""
        return self._field_host("fmmbem_plan_execute_velocity_gradient", traction, (3, 3), "dof values")

    def execute_velocity_gradient_device(self, x_ptr, g_ptr, stream=0, p=None):
        self._field_device("fmmbem_plan_execute_velocity_gradient_device", x_ptr, g_ptr, stream, p)

    def execute_velocity_gradient_torch(self, x, out=None, p=None):
        """x: contiguous float64 CUDA tensor with 3 values per panel, ORIGINAL panel order; returns (M, 3, 3).  Runs on torch's
        current stream."""
        return self._field_torch(self.execute_velocity_gradient_device, x, out, p, (3, 3), "dof values")

    # ---- the flow execute: velocity, pressure and velocity gradient on one far chain (include/fmmbem.h, "Flow execute") ----
    def execute_flow(self, traction, velocity=True, pressure=True, velocity_gradient=True):
        """(N, 3) or (3N,) traction density -> (u, q, G) at the kernel's current p: u (M, 3) what execute returns, q (M,) what
        execute_pressure returns, G (M, 3, 3) what execute_velocity_gradient returns, bit for bit, from ONE gather, P2M and far
        chain; None for what was not asked.  numpy in, numpy out (host).  FmmBemError (status 6) on a plan that is not over
        separate targets, on a Laplace plan, on a plan with a TRACTION target and on a host-only plan."""
        x = np.ascontiguousarray(traction, dtype=np.float64)
        if x.shape != (self.n * self.dof,) and x.shape != (self.n, self.dof):
            raise ValueError("traction must have dof values per panel")
        if not (velocity or pressure or velocity_gradient):
            raise ValueError("no output asked")
        rows = self._field_rows()
        u = np.empty((rows, 3)) if velocity else None
        q = np.empty((rows,)) if pressure else None
        g = np.empty((rows, 3, 3)) if velocity_gradient else None
        ptr = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in (u, q, g)]
        _capi.check(_capi.lib().fmmbem_plan_execute_flow(self._h, self._K.P, x.ctypes.data_as(C.c_void_p), *ptr))
        return u, q, g

    def execute_flow_device(self, x_ptr, u_ptr, q_ptr, g_ptr, stream=0, p=None):
        """raw device pointers; 0 for an output that is not asked"""
        _capi.check(_capi.lib().fmmbem_plan_execute_flow_device(
            self._h, self._K.P if p is None else int(p), C.c_void_p(x_ptr), C.c_void_p(u_ptr or None), C.c_void_p(q_ptr or None),
            C.c_void_p(g_ptr or None), C.c_void_p(stream)))

    def execute_flow_torch(self, x, velocity=True, pressure=True, velocity_gradient=True, p=None):
        """x: contiguous float64 CUDA tensor with 3 values per panel, ORIGINAL panel order; returns (u, q, G) of shapes (M, 3), (M,),
        (M, 3, 3), None for what was not asked.  Runs on torch's current stream."""
        tails = ((3,) if velocity else None, () if pressure else None, (3, 3) if velocity_gradient else None)
        if all(t is None for t in tails):
            raise ValueError("no output asked")
        first = next(k for k, t in enumerate(tails) if t is not None)
        outs = [None, None, None]

        def run(x_ptr, first_ptr, stream, p):                     # x is checked and the first output asked allocated by now
            for k, t in enumerate(tails):
                if t is not None and k != first:
                    outs[k] = x.new_empty((self._field_rows(),) + t)
            ptrs = [first_ptr if k == first else 0 if o is None else o.data_ptr() for k, o in enumerate(outs)]
            self.execute_flow_device(x_ptr, *ptrs, stream=stream, p=p)

        outs[first] = self._field_torch(run, x, None, p, tails[first], "dof values")
        return tuple(outs)

    # ---- the representation execute: both Laplace layers, value and gradient, on one far chain (include/fmmbem.h,
    # "Representation execute") ----
    def execute_representation(self, density, potential, value=True, gradient=True):
        """(N,) density sigma and (N,) surface potential mu -> (phi, grad) at the kernel's current p: phi (M,) = S[sigma] - D[mu] at
        the plan's points, grad (M, 3) its gradient, in execute's scaling (the physical values are the results / 4 pi); None for an
        output that was not asked.  density or potential None: that layer is left out.  The targets' own flags do not enter.  ONE
        gather, P2M per layer, far chain and near kernel where the four single executes on an all-0 and an all-1 plan run four.
        numpy in, numpy out (host).  FmmBemError (status 6) on a plan that is not over separate targets, on a Stokes plan and on a
        host-only plan."""
        if density is None and potential is None:
            raise ValueError("no layer given")
        if not (value or gradient):
            raise ValueError("no output asked")
        layers = []
        for name, a in (("density", density), ("potential", potential)):
            x = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            if x is not None and x.shape != (self.n * self.dof,) and x.shape != (self.n, self.dof):
                raise ValueError("%s must have one value per panel" % name)
            layers.append(x)
        rows = self._field_rows()
        phi = np.empty((rows,)) if value else None
        grad = np.empty((rows, 3)) if gradient else None
        ptr = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in (*layers, phi, grad)]
        _capi.check(_capi.lib().fmmbem_plan_execute_representation(self._h, self._K.P, *ptr))
        return phi, grad

    def execute_representation_device(self, density_ptr, potential_ptr, phi_ptr, grad_ptr, stream=0, p=None):
        """raw device pointers; 0 for a layer that is left out and for an output that is not asked"""
        _capi.check(_capi.lib().fmmbem_plan_execute_representation_device(
            self._h, self._K.P if p is None else int(p), C.c_void_p(density_ptr or None), C.c_void_p(potential_ptr or None),
            C.c_void_p(phi_ptr or None), C.c_void_p(grad_ptr or None), C.c_void_p(stream)))

    def execute_representation_torch(self, density, potential, value=True, gradient=True, p=None):
        """density, potential: contiguous float64 CUDA tensors (N,), ORIGINAL panel order, or None for a layer that is left out;
        returns (phi, grad) of shapes (M,), (M, 3), None for what was not asked.  Runs on torch's current stream."""
        if density is None and potential is None:
            raise ValueError("no layer given")
        if not (value or gradient):
            raise ValueError("no output asked")
        tails = (() if value else None, (3,) if gradient else None)
        first = 0 if value else 1
        outs = [None, None]
        lead = density if density is not None else potential    # checked by _field_torch; the other layer against it, below
        other = potential if density is not None else None

        def run(lead_ptr, first_ptr, stream, p):
            if other is not None and (other.dtype != lead.dtype or other.device != lead.device or not other.is_contiguous()
                                      or other.numel() != lead.numel()):
                raise ValueError("potential must be a contiguous float64 CUDA tensor with one value per panel on density's device")
            if value and gradient:
                outs[1] = lead.new_empty((self._field_rows(), 3))
            ptrs = [first_ptr if k == first else 0 if o is None else o.data_ptr() for k, o in enumerate(outs)]
            layer_ptrs = (lead_ptr, 0 if other is None else other.data_ptr()) if density is not None else (0, lead_ptr)
            self.execute_representation_device(*layer_ptrs, *ptrs, stream=stream, p=p)

        outs[first] = self._field_torch(run, lead, None, p, tails[first], "one value")
        return tuple(outs)

    def execute_stress(self, traction):
        """(N, 3) or (3N,) traction density -> (M, 3, 3): sigma_i[k][m] = -q_i delta_km + mu (G_i[k][m] + G_i[m][k]), q of
        execute_pressure and G of execute_velocity_gradient, in their scaling: the physical stress is the result / 4 pi.  ONE
        execute_flow(velocity=False): the pressure and the gradient on one far chain and one walk over the near lists, with the
        bits of the two single executes."""
        _, q, g = self.execute_flow(traction, velocity=False)
        return -q[:, None, None] * np.eye(3)[None] + self._K.Mu * (g + g.transpose(0, 2, 1))

    # ---- batched execute: k vectors, one near-field pass per batch_width() of them (fmmbem_plan_execute_batch) ----
    def execute_batch(self, charges):
        """(k, n) charges -- (k, n, 3) for Stokes -> (k, m) results ((k, m, 3)), m = n or the number of targets, at the
        kernel's current p.  Each row is bit for bit what execute gives for that row.  numpy in, numpy out (host)."""
        x = np.ascontiguousarray(charges, dtype=np.float64)
        want = (self.n,) if self.dof == 1 else (self.n, self.dof)
        if x.ndim != 1 + len(want) or x.shape[1:] != want or x.shape[0] < 1:
            raise ValueError("charges must have shape (k,) + %r with k >= 1" % (want,))
        k = x.shape[0]
        y = np.empty((k,) + (want if self.n_targets is None else self._target_shape()))
        ldx = self.n * self.dof
        ldy = ldx if self.n_targets is None else self.n_targets * self.dof
        _capi.check(_capi.lib().fmmbem_plan_execute_batch(self._h, self._K.P, k, x.ctypes.data_as(C.c_void_p), ldx,
                                                          y.ctypes.data_as(C.c_void_p), ldy))
        return y

    def execute_batch_device(self, k, x_ptr, ldx, y_ptr, ldy, stream=0, p=None):
        _capi.check(_capi.lib().fmmbem_plan_execute_batch_device(self._h, self._K.P if p is None else int(p), int(k), C.c_void_p(x_ptr),
                                                                 int(ldx), C.c_void_p(y_ptr), int(ldy), C.c_void_p(stream)))

    def execute_batch_torch(self, x, out=None, p=None):
        """x: contiguous float64 CUDA tensor (k, n * dof), ORIGINAL panel order. Returns (k, m * dof) (m: n or the number of
        targets). Runs on torch's current stream."""
        import torch
        if (x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.dim() != 2 or x.shape[0] < 1
                or x.shape[1] != self.n * self.dof):
            raise ValueError("x must be a contiguous float64 CUDA tensor of shape (k, n * dof)")
        if x.device.index != self.device:
            raise ValueError("x lives on cuda:%s but the plan was built on device %d" % (x.device.index, self.device))
        m = (self.n if self.n_targets is None else self.n_targets) * self.dof
        if out is None:
            out = x.new_empty((x.shape[0], m))
        elif (out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (x.shape[0], m)
              or out.device != x.device):
            raise ValueError("out must be a contiguous float64 tensor of shape (k, %d) on x's device" % m)
        self.execute_batch_device(x.shape[0], x.data_ptr(), x.shape[1], out.data_ptr(), m,
                                  torch.cuda.current_stream(x.device).cuda_stream, p)
        return out

    def batch_width(self):
        """Vectors one near-field pass of execute_batch serves on this plan (1: the batch runs vector by vector)."""
        w = C.c_int(0)
        _capi.check(_capi.lib().fmmbem_plan_batch_width(self._h, C.byref(w)))
        return w.value

    # ---- exact block-Jacobi preconditioner of a BLOCK_DIAGONAL plan (fmmbem_plan_block_inverse_*; not in the reference) ----
    def block_inverse_build(self):
        """Invert every leaf's self block on the device, once; execute keeps applying the blocks themselves.  A second call is
        a no-op.  Raises FmmBemError (status 1, the message names the leaf) when a block is singular."""
        _capi.check(_capi.lib().fmmbem_plan_block_inverse_build(self._h))

    def block_inverse_bytes(self):
        """HBM bytes of the inverses: what one apply streams (0 before block_inverse_build)."""
        b = C.c_int64(0)
        _capi.check(_capi.lib().fmmbem_plan_block_inverse_bytes(self._h, C.byref(b)))
        return b.value

    def block_inverse_apply(self, v):
        """z = M v, M the inverse of the block-diagonal operator.  v: (n,) -- (n, 3) for Stokes -- or k such vectors stacked in
        front; the same shape comes back.  numpy in, numpy out (host)."""
        x = np.ascontiguousarray(v, dtype=np.float64)
        want = (self.n,) if self.dof == 1 else (self.n, self.dof)
        if x.shape != want and (x.ndim != 1 + len(want) or x.shape[1:] != want or x.shape[0] < 1):
            raise ValueError("v must have shape %r, or (k,) + that with k >= 1" % (want,))
        k = 1 if x.shape == want else x.shape[0]
        z = np.empty_like(x)
        ld = self.n * self.dof
        _capi.check(_capi.lib().fmmbem_plan_block_inverse_apply(self._h, k, x.ctypes.data_as(C.c_void_p), ld,
                                                                z.ctypes.data_as(C.c_void_p), ld))
        return z

    def block_inverse_apply_torch(self, v, out=None):
        """The same on device tensors, asynchronous on torch's current stream.  v: contiguous float64 CUDA tensor of n * dof
        values, or (k, n * dof); out: a tensor of v's shape that does not overlap it."""
        import torch
        nd = self.n * self.dof
        if v.dtype != torch.float64 or not v.is_cuda or not v.is_contiguous() or v.numel() < nd or (v.numel() != nd and (v.dim() != 2 or v.shape[1] != nd)):
            raise ValueError("v must be a contiguous float64 CUDA tensor of n * dof values, or of shape (k, n * dof)")
        if v.device.index != self.device:
            raise ValueError("v lives on cuda:%s but the plan was built on device %d" % (v.device.index, self.device))
        if out is None:
            out = torch.empty_like(v)
        elif out.dtype != torch.float64 or out.device != v.device or not out.is_contiguous() or out.shape != v.shape or out.data_ptr() == v.data_ptr():
            raise ValueError("out must be a contiguous float64 tensor of v's shape on v's device, and not v itself")
        _capi.check(_capi.lib().fmmbem_plan_block_inverse_apply_device(
            self._h, v.numel() // nd, C.c_void_p(v.data_ptr()), nd, C.c_void_p(out.data_ptr()), nd,
            C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)))
        return out

    # ---- introspection ----
    def set_timing(self, on=True):
        """True / 1: HIP events around every stage; 2: around the near-field kernel only (an event record costs ~5 us of
        stream time, 85 us per fully instrumented matvec at N = 1M); False / 0: off."""
        _capi.check(_capi.lib().fmmbem_plan_set_timing(self._h, 2 if on == 2 else (1 if on else 0)))

    def set_graphs(self, on=True):
        """Replay each order's launch chain as a hipGraph from its second execute on (fmmbem_plan_set_graphs)."""
        _capi.check(_capi.lib().fmmbem_plan_set_graphs(self._h, 1 if on else 0))

    def stats(self):
        s = _capi.Stats()
        _capi.check(_capi.lib().fmmbem_plan_stats(self._h, C.byref(s)))
        return s.as_dict()

    def perm(self):
        out = np.empty(self.n, dtype=np.uint32)
        _capi.check(_capi.lib().fmmbem_plan_get_perm(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def boxes(self):
        nb = self.stats()["n_boxes"]
        d = dict(center=np.empty((nb, 3)), side=np.empty(nb))
        for k in ("level", "leaf", "parent", "bb", "be"):
            d[k] = np.empty(nb, dtype=np.int32)
        _capi.check(_capi.lib().fmmbem_plan_get_boxes(self._h, *[d[k].ctypes.data_as(C.c_void_p) for k in
                                                                 ("center", "side", "level", "leaf", "parent", "bb", "be")]))
        return d

    def target_info(self):
        """A plan over separate targets: counts of both trees (fmmbem_plan_target_info)."""
        s = _capi.TargetInfo()
        _capi.check(_capi.lib().fmmbem_plan_target_info(self._h, C.byref(s)))
        return s.as_dict()

    def target_boxes(self):
        """The target tree's boxes, as boxes() gives the source tree's."""
        nb = self.target_info()["n_target_boxes"]
        d = dict(center=np.empty((nb, 3)), side=np.empty(nb))
        for k in ("level", "leaf", "parent", "bb", "be"):
            d[k] = np.empty(nb, dtype=np.int32)
        _capi.check(_capi.lib().fmmbem_plan_get_target_boxes(self._h, *[d[k].ctypes.data_as(C.c_void_p) for k in
                                                                        ("center", "side", "level", "leaf", "parent", "bb", "be")]))
        return d

    def target_perm(self):
        """(target-tree position -> distinct point, given target -> distinct point)"""
        info = self.target_info()
        tree = np.empty(info["n_target_points"], dtype=np.uint32)
        given = np.empty(info["n_targets"], dtype=np.uint32)
        _capi.check(_capi.lib().fmmbem_plan_get_target_perm(self._h, tree.ctypes.data_as(C.c_void_p), given.ctypes.data_as(C.c_void_p)))
        return tree, given

    def pairs(self, which):
        idx = {"p2p": 0, "m2l": 1, "m2m": 2, "l2l": 3, "m2l_work": 4, "m2l_items": 5, "m2l_items_long": 6}[which]
        n = C.c_int64(0)
        _capi.check(_capi.lib().fmmbem_plan_get_pairs(self._h, idx, None, C.byref(n)))
        out = np.empty((n.value, 2), dtype=np.int32)
        _capi.check(_capi.lib().fmmbem_plan_get_pairs(self._h, idx, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def near_row(self, row, values=True):
        n = C.c_int64(0)
        _capi.check(_capi.lib().fmmbem_plan_get_near_row(self._h, row, None, None, C.byref(n)))
        cols = np.empty(n.value, dtype=np.uint32)
        vals = np.empty(n.value) if values else None
        _capi.check(_capi.lib().fmmbem_plan_get_near_row(
            self._h, row, cols.ctypes.data_as(C.c_void_p),
            vals.ctypes.data_as(C.c_void_p) if values else None, C.byref(n)))
        return cols, vals

    def diagonal(self):
        """K(s,s) of every unknown, original order (the entries Preconditioners::Diagonal inverts)."""
        out = np.empty(self.n * self.dof)
        _capi.check(_capi.lib().fmmbem_plan_get_diagonal(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def expansions(self, which, p=None):
        p = self._K.P if p is None else p
        nb = self.stats()["n_boxes"]
        out = np.empty((nb, self.stats()["expansion_slots"], p * (p + 1) // 2), dtype=np.complex128)   # Stokes: 8, 11 with TRACTION targets
        _capi.check(_capi.lib().fmmbem_plan_get_expansions(self._h, 0 if which == "M" else 1, p,
                                                           out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().fmmbem_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

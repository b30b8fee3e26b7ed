#!/usr/bin/env python3
"""The reference's potential-problem driver, examples/LaplaceBEM.cpp, on the MI355X library: same command-line flags
(:47-66, :98-160), same steps (sphere or gmsh mesh, right-hand side from the plan with flipped boundary conditions
:218-232, GMRES / FGMRES with relaxed p and the Identity / Diagonal / Local / block-diagonal preconditioners :276-316),
same report lines (timing, potential at the exterior point (3,3,3) :346-369, relative error against the analytic density
:372).  All matvecs run in libfmmbem_hip.so; this file is host glue.

    python examples/LaplaceBEM.py -recursions 6 -p 12 -theta 0.5

-field N (not a flag of the reference): after the solve, the same representation formula on N points of the sphere of radius 3
through a plan over those target points (FMM_plan(K, panels, targets=...), the reference's FMM_plan(K, sources, targets, opts)),
one more report line with its largest error against the exact exterior solution 1/|x|.
-near_f32 P (not a flag of the reference): the operator's matvecs at orders p <= P stream the float copy of the near matrix
(fmmbem_options.near_f32_max_p); the report lines are the same, plus one line that states the threshold.
-field_grad (not a flag of the reference): with -field N, one more line: the gradient of that formula at the same points
(FMM_plan.execute_gradient on the two plans over them), its largest error against the exact -x/|x|^3 relative to 1/9.
-field_hess (not a flag of the reference): with -field N, one more line: the Hessian of that formula at the same points
(FMM_plan.execute_hessian on the two plans over them, also when -field_one_pass is given), the Frobenius norm of its error against
the exact 3 x x^T / |x|^5 - I / |x|^3 relative to 2/27.  Like -field_grad it does nothing without -field.
-field_one_pass (not a flag of the reference): with -field N, the field line -- and with -field_grad the gradient line -- from ONE
plan over the points and ONE FMM_plan.execute_representation (fmmbem_plan_execute_representation: both layers folded into one
multipole set, one far chain, one kernel over the near pairs) where the lines otherwise take two plans and two or four executes;
the same lines, the same numbers to rounding.
-block_inverse (not a flag of the reference): GMRES with the exact block-Jacobi preconditioner -- the leaf blocks of the
block-diagonal operator inverted once on the device (solver.BlockInverse) where -fgmres -diagonal iterates on them; the same
report lines as the other modes.
"""
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fmm_bem_relaxed_amd as fb  # noqa: E402


def print_help_and_exit():
    print("serialBEM : FMM-BEM for Potential problems\n\nUsage: LaplaceBEM.py <options>\n\nFMM/Treecode Options:\n"
          "-theta <double> : Set MAC theta for treecode evaluators\n"
          "-eval {FMM,TREE} : Choose either FMM or treecode evaluator\n"
          "-ncrit <int> : Maximum # of particles per Octree box\n\nProblem & Solver Options:\n"
          "-p <double> : Number of terms in the Multipole / Local expansions\n"
          "-k {1,3,4,7} : Number of Gauss integration points used per panel\n"
          "-recursions <int> : number of recursive subdivisions to create a sphere - # panels = 2*4^recursions, default = 4\n"
          "-second_kind : enable 'second-kind' option to solve second-kind integral equations\n"
          "-fixed_p : enable 'non-relaxed' option\n"
          "-solver_tol <double> : Set the solver tolerance, default = 1e-5\n"
          "-max_iters <int>, -gmres, -fgmres, -local, -diagonal, -mesh <file.msh>\n"
          "-block_inverse : (not a flag of the reference) GMRES preconditioned by the exact inverse of the leaf-diagonal blocks\n"
          "-help : print this message")
    sys.exit(0)


class _Logged:
    """Prints the reference's per-iteration line (examples/BEM/GMRES.hpp:219-220) from the solver's log."""

    def __init__(self):
        self.rows = []

    def append(self, row):
        it, p, res = row
        self.rows.append(row)
        print("it: %03d, res: %.3e, fmm_req_p: %01d" % (it, res, p))


def exterior_potential(v, bc_flip, k, density, point):
    """Direct::matvec of the driver (:346-364) for ONE exterior target: far-regime Gauss quadrature of G or dG/dn over
    every panel (kernel/LaplaceSphericalBEM.hpp:199-205, 246-258; the point is far from every panel)."""
    pts, w = fb.quadrature(k)
    q = np.einsum("qa,nac->nqc", pts, v)                               # quadrature points (N, K, 3)
    e0, e1 = v[:, 2] - v[:, 0], v[:, 1] - v[:, 0]
    c = np.cross(e0, e1)
    area = 0.5 * np.linalg.norm(c, axis=1)
    normal = c / (2 * area)[:, None]
    dx = q - np.asarray(point)[None, None, :]
    r = np.linalg.norm(dx, axis=2)
    if bc_flip:                                                        # target POTENTIAL-side kernel: G
        kern = (w[None, :] * area[:, None] / r).sum(axis=1)
    else:
        kern = (w[None, :] * area[:, None] * np.einsum("nqc,nc->nq", dx, normal) / r ** 3).sum(axis=1)
    return float(kern @ density)


def exterior_direct(v, g_density, dgdn_density, point, k=3):
    """The driver's representation formula at one exterior point by Direct sums (:346-369): (sum G x - sum dG/dn c) / 4 pi"""
    return (exterior_potential(v, True, k, g_density, point) - exterior_potential(v, False, k, dgdn_density, point)) / 4 / math.pi


def exterior_fmm(fb_, v, g_density, dgdn_density, points, p, k=3, opts=None):
    """The same formula at many points: two executes over the target points, one with their flags POTENTIAL (G), one with
    them switched (dG/dn) -- the FMM in place of the two Direct sums"""
    m = len(points)
    K = fb_.LaplaceSphericalBEM(p, k)
    g = fb_.FMM_plan(K, v, opts, targets=points, target_bc=np.zeros(m, dtype=np.uint8))
    d = fb_.FMM_plan(K, v, opts, targets=points, target_bc=np.ones(m, dtype=np.uint8))
    out = (g.execute(g_density) - d.execute(dgdn_density)) / 4 / math.pi
    g.close()
    d.close()
    return out


def exterior_fmm_gradient(fb_, v, g_density, dgdn_density, points, p, k=3, opts=None):
    """The gradient of the same formula at the points: (grad of the single layer of g_density - grad of the double layer of
    dgdn_density) / 4 pi, by the gradient executes of the two plans over the points"""
    m = len(points)
    K = fb_.LaplaceSphericalBEM(p, k)
    g = fb_.FMM_plan(K, v, opts, targets=points, target_bc=np.zeros(m, dtype=np.uint8))
    d = fb_.FMM_plan(K, v, opts, targets=points, target_bc=np.ones(m, dtype=np.uint8))
    out = (g.execute_gradient(g_density) - d.execute_gradient(dgdn_density)) / 4 / math.pi
    g.close()
    d.close()
    return out


def exterior_fmm_hessian(fb_, v, g_density, dgdn_density, points, p, k=3, opts=None):
    """The Hessian of the same formula at the points: (Hessian of the single layer of g_density - Hessian of the double layer of
    dgdn_density) / 4 pi, by the Hessian executes of the two plans over the points; (M, 3, 3)"""
    m = len(points)
    K = fb_.LaplaceSphericalBEM(p, k)
    g = fb_.FMM_plan(K, v, opts, targets=points, target_bc=np.zeros(m, dtype=np.uint8))
    d = fb_.FMM_plan(K, v, opts, targets=points, target_bc=np.ones(m, dtype=np.uint8))
    out = (g.execute_hessian(g_density) - d.execute_hessian(dgdn_density)) / 4 / math.pi
    g.close()
    d.close()
    return out


def exterior_fmm_one_pass(fb_, v, g_density, dgdn_density, points, p, k=3, opts=None, gradient=False):
    """The formula, and with `gradient` its gradient, at the points from ONE plan over them and ONE representation execute (the
    points' flags do not enter): (phi, grad or None), each / 4 pi"""
    K = fb_.LaplaceSphericalBEM(p, k)
    plan = fb_.FMM_plan(K, v, opts, targets=points, target_bc=np.zeros(len(points), dtype=np.uint8))
    phi, grad = plan.execute_representation(g_density, dgdn_density, value=True, gradient=gradient)
    plan.close()
    return phi / 4 / math.pi, None if grad is None else grad / 4 / math.pi


def sphere_points(m, radius):
    """m points spread over a sphere (golden-angle spiral)"""
    i = np.arange(m) + 0.5
    z = 1 - 2 * i / m
    r = np.sqrt(1 - z * z)
    phi = math.pi * (3 - math.sqrt(5)) * i
    return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def main(argv):
    print("\nLaplaceBEM on a sphere")
    if len(argv) == 1:
        print_help_and_exit()
    theta, ncrit, p, k, recursions = 0.5, 64, 5, 3, 4
    second_kind, mesh, field, near_f32, evaluator = False, None, 0, 0, "FMM"
    field_grad = field_hess = field_one_pass = False
    so = fb.SolverOptions()
    max_iterations, solver, pc = 500, "gmres", "identity"
    print("parameters : \n============ ")
    i = 1
    while i < len(argv):
        a = argv[i]
        if a == "-theta":
            i += 1; theta = float(argv[i]); print("theta = %s" % argv[i])
        elif a == "-recursions":
            i += 1; recursions = int(argv[i]); print("N = %i" % (2 * 4 ** recursions))
        elif a == "-eval":                                 # FMMOptions.hpp:85-94 (the reference's driver prints no line for it)
            i += 1
            if argv[i] in ("FMM", "TREE"):
                evaluator = "TREECODE" if argv[i] == "TREE" else "FMM"
            else:
                print('[W]: Unknown evaluator type: "%s"' % argv[i])
        elif a == "-ncrit":
            i += 1; ncrit = int(argv[i]); print("ncrit = %s" % argv[i])
        elif a == "-printtree":
            pass
        elif a == "-p":
            i += 1; p = int(argv[i]); so.max_p = p; print("max-p = %i" % p)
        elif a == "-k":
            i += 1; k = int(argv[i])
        elif a == "-second_kind":
            second_kind = True; print("second-kind = True")
        elif a == "-fixed_p":
            so.variable_p = False; print("relaxed = False")
        elif a == "-solver_tol":
            i += 1; so.residual = float(argv[i]); print("solver_tol = %.2e" % so.residual)
        elif a == "-max_iters":
            i += 1; max_iterations = int(argv[i])
        elif a == "-gmres":
            solver = "gmres"
        elif a == "-fgmres":
            solver = "fgmres"
        elif a == "-local":
            solver, pc = "fgmres", "local"
        elif a == "-diagonal":
            pc = "diagonal"
        elif a == "-help":
            print_help_and_exit()
        elif a == "-mesh":
            i += 1; mesh = argv[i]
        elif a == "-field":
            i += 1; field = int(argv[i])
        elif a == "-field_grad":                           # not in the reference: FMM_plan.execute_gradient
            field_grad = True
        elif a == "-field_hess":                           # not in the reference: FMM_plan.execute_hessian
            field_hess = True
        elif a == "-field_one_pass":                       # not in the reference: FMM_plan.execute_representation
            field_one_pass = True
        elif a == "-block_inverse":                        # not in the reference: solver.BlockInverse
            solver, pc = "gmres", "block_inverse"
        elif a == "-near_f32":                             # not in the reference: fmmbem_options.near_f32_max_p
            i += 1; near_f32 = int(argv[i])
        else:
            print('[W]: Unknown command line arg: "%s"' % a)
            print_help_and_exit()
        i += 1
    if field_one_pass and field <= 0:
        print("[E]: -field_one_pass needs -field <N>: it chooses how the lines of -field are computed", file=sys.stderr)
        sys.exit(2)
    print("============")
    so.max_iters = so.restart = max_iterations
    so.max_p = p

    if mesh:
        print("reading mesh from: %s" % mesh)
        v = fb.read_msh(mesh)
    else:
        v = fb.unit_sphere(recursions)
    n = len(v)
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    opts.set_max_per_box(ncrit)
    opts.evaluator = evaluator                                         # the solve plan and the right-hand-side plan (:209-232)
    bc = np.full(n, 1 if second_kind else 0, dtype=np.uint8)           # panels switch_BC() for the second kind (:190-191)
    K = fb.LaplaceSphericalBEM(p, k)
    plan = fb.FMM_plan(K, v, opts, bc=bc, p_max=p, near_f32_max_p=near_f32)    # the operator of the solve; the right-hand side stays FP64
    if near_f32:
        print("float near field: matvecs at p <= %d stream %.3f GB of float entries" % (near_f32, plan.stats()["near_f32_bytes"] / 1e9))
    dev = torch.device("cuda", 0)
    charges = torch.ones(n, dtype=torch.float64, device=dev)

    tic = time.time()
    t2 = time.time()
    print("Flipping BC: %g" % (time.time() - t2))
    t2 = time.time()
    rhs_plan = fb.FMM_plan(fb.LaplaceSphericalBEM(p, k), v, opts, bc=1 - bc, p_max=p)
    print("Creating plan: %g" % (time.time() - t2))
    t2 = time.time()
    b = rhs_plan.execute_torch(charges)
    torch.cuda.synchronize()
    print("Executing plan: %g" % (time.time() - t2))
    rhs_plan.close()
    setup_time = time.time() - tic

    tic = time.time()
    x = torch.zeros(n, dtype=torch.float64, device=dev)
    print("2nd-kind equation being solved" if second_kind else "1st-kind equation being solved")
    log = _Logged()
    if solver == "gmres" and pc == "identity":
        print("Solver: GMRES\nPreconditioner: Identity")
        x, it, res = fb.gmres(plan, x, b, so, log=log)
    elif solver == "gmres" and pc == "diagonal":
        print("Solver: GMRES\nPreconditioner: Diagonal")
        x, it, res = fb.gmres(plan, x, b, so, M=fb.Diagonal(plan, dev), log=log)
    elif pc == "block_inverse":
        print("Solver: GMRES\nPreconditioner: Block inverse")
        x, it, res = fb.gmres(plan, x, b, so, M=fb.BlockInverse(fb, fb.LaplaceSphericalBEM(p, k), v, bc=bc, ncrit=ncrit), log=log)
    elif solver == "fgmres" and pc == "identity":
        print("Solver: FMRES\nPreconditioner: Identity")
        x, it, res = fb.fgmres(plan, x, b, so, lambda z: z, log=log)
    elif solver == "fgmres" and pc == "diagonal":
        print("Solver: FGMRES\nPreconditioner: Block Diagonal")
        x, it, res = fb.fgmres(plan, x, b, so, fb.BlockDiagonal(fb, fb.LaplaceSphericalBEM(p, k), v, bc=bc), log=log)
    else:
        print("Solver: FGMRES\nPreconditioner: Local solve")
        x, it, res = fb.fgmres(plan, x, b, so, fb.LocalInnerSolver(fb, fb.LaplaceSphericalBEM(p, k), v, bc=bc), log=log)
    torch.cuda.synchronize()
    print("Final residual: %.4e, after %d iterations" % (res, it))
    solve_time = time.time() - tic

    print("\nTIMING:\n\tsetup : %.4es\n\tsolve : %.4es" % (setup_time, solve_time))
    xs = x.cpu().numpy()
    # potential at an exterior point from the computed density and the prescribed data (:346-369)
    out = (3.0, 3.0, 3.0)
    # the driver's exterior target is a default (POTENTIAL) panel, then switch_BC(): G with x, dG/dn with the charges,
    # whichever equation was solved (:355-361)
    r2 = exterior_potential(v, True, k, xs, out)
    r1 = exterior_potential(v, False, k, np.ones(n), out)
    exact = 1.0 / math.sqrt(27.0)
    outside = (r2 - r1) / 4 / math.pi
    print("external phi: %.5g, exact: %.5g, error: %.4e" % (outside, exact, abs(outside - exact) / abs(exact)))
    e = float(((xs - 1.0) ** 2).sum())
    print("relative error: %.3e" % math.sqrt(e / n))
    if field > 0:
        pts = sphere_points(field, 3.0)
        opts.evaluator = "FMM"                             # plans over target points: the FMM evaluator only
        grad = None
        if field_one_pass:
            phi, grad = exterior_fmm_one_pass(fb, v, xs, np.ones(n), pts, p, k, opts, gradient=field_grad)
        else:
            phi = exterior_fmm(fb, v, xs, np.ones(n), pts, p, k, opts)
        err = np.abs(phi - 1.0 / 3.0) / (1.0 / 3.0)
        print("field: %d points at r = 3, max error: %.4e, rms error: %.4e" % (field, float(err.max()), float(np.sqrt((err ** 2).mean()))))
        if field_grad:
            if grad is None:
                grad = exterior_fmm_gradient(fb, v, xs, np.ones(n), pts, p, k, opts)
            exact_grad = -pts / np.linalg.norm(pts, axis=1)[:, None] ** 3
            gerr = np.linalg.norm(grad - exact_grad, axis=1) / (1.0 / 9.0)
            print("field gradient: %d points at r = 3, max error: %.4e, rms error: %.4e"
                  % (field, float(gerr.max()), float(np.sqrt((gerr ** 2).mean()))))
        if field_hess:
            hess = exterior_fmm_hessian(fb, v, xs, np.ones(n), pts, p, k, opts)
            rr = np.linalg.norm(pts, axis=1)
            exact_hess = 3 * pts[:, :, None] * pts[:, None, :] / rr[:, None, None] ** 5 - np.eye(3)[None] / rr[:, None, None] ** 3
            herr = np.linalg.norm((hess - exact_hess).reshape(field, 9), axis=1) / (2.0 / 27.0)
            print("field Hessian: %d points at r = 3, max error: %.4e, rms error: %.4e"
                  % (field, float(herr.max()), float(np.sqrt((herr ** 2).mean()))))
    return it, res, math.sqrt(e / n), abs(outside - exact) / abs(exact)


if __name__ == "__main__":
    main(sys.argv)

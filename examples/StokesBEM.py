#!/usr/bin/env python3
"""The reference's Stokes driver, examples/StokesBEM.cpp, on the MI355X library: same command-line flags (:80-97,
:147-212), same steps -- unit sphere / red blood cell / mesh, unit velocity (1,0,0) on every panel, the right-hand side
the driver ends up using (it computes A_traction * u by FMM, reports how far that is from 4 pi, and then OVERWRITES it with
the analytic (4 pi, 0, 0), :262-277; the reference's own traction far field is wrong, SURVEY.md section 8a -- here the
double-layer far field of csrc/kernels_far.hip evaluates that step, up to order 12), the first-
kind stokeslet system solved by the relaxed GMRES of GMRES_Stokes.hpp (:307-330), and the same report: timing, drag
against 6 pi mu, area and pointwise traction errors (:337-372).  All matvecs run in libfmmbem_hip.so.

    python examples/StokesBEM.py -recursions 4 -p 10

-near_f32 P (not a flag of the reference): the operator's matvecs at orders p <= P stream the float copy of the near matrix
(fmmbem_options.near_f32_max_p); the report lines are the same, plus one line that states the threshold.

-field N (not a flag of the reference): after the solve, the velocity of the single layer with the solved density on N points of the
sphere of radius 3, summed on the device by fb.Direct; prints the largest and the mean magnitude.

-field_fmm N (not a flag of the reference): the same velocity on the same N points by the FMM, through plan.field_plan
(fmmbem_plan_create_field) at order p; prints "field (FMM): ..." in the format of the "field:" line and, given together with
-field N, the relative L2 difference between the two.

-field_pressure (not a flag of the reference; with -field_fmm N): the pressure of the solved layer on the same N points by
fplan.execute_pressure (fmmbem_plan_execute_pressure), in the library's scaling q = 4 pi p; prints "field pressure (FMM): ..." in the
format of the "field (FMM):" line and, for the unit sphere, the largest deviation of q / (6 pi mu) from x / r^3 -- the exact pressure
of a translating sphere, p = (3/2) mu a U.x / r^3 -- relative to 1/9.

-field_stress (not a flag of the reference; with -field_fmm N): the velocity gradient of the solved layer on the same N points by
fplan.execute_velocity_gradient (fmmbem_plan_execute_velocity_gradient), in the library's scaling G = 4 pi grad u, and the stress by
fplan.execute_stress; prints "field velocity gradient (FMM): ..." and "field stress (FMM): ..." in the format of the "field (FMM):" line
and, for the unit sphere, the largest deviation of G / 4 pi from the exact velocity gradient of a translating sphere, relative to that
gradient's largest entry on the points.

With -field_fmm N and -field_pressure and/or -field_stress the field comes from ONE fplan.execute_flow_torch (fmmbem_plan_execute_flow):
the velocity, the pressure and the gradient on one far chain, each bit for bit what its single execute returns, so every line above
is what it was.

-field_direct (not a flag of the reference; with -field_fmm N and -field_pressure and/or -field_stress): the same quantities on the same
N points summed over all panels on the device by fb.Direct (pressure_torch, velocity_gradient_torch); after the "field pressure (FMM):"
and the "field velocity gradient (FMM):" line prints "... against Direct: relative L2 difference ...", the distance of the FMM's value
from the sum it approximates.

-block_inverse (not a flag of the reference): GMRES with the exact block-Jacobi preconditioner -- the leaf blocks of the
block-diagonal operator inverted once on the device (solver.BlockInverse) where -diagonal iterates on them; the same report lines.

-stokes_batch K (not a flag of the reference): the operator plan is created with fmmbem_options.stokes_batch_width = K (2, 3, 4): one
pass over the near matrix serves K vectors of a batch; the report lines are the same, plus one line that states the width.

-resistance (not a flag of the reference): after the report, the translational resistance matrix of the body -- the unit translations
e_x, e_y, e_z solved as ONE lockstep batch (gmres_capi_batch) on the operator plan, column j the force of translation e_j -- and its
largest deviation from 6 pi mu I, exact for the unit sphere, relative to 6 pi mu.  With -stokes_batch 3 the three matvecs of an
iteration share one near-field pass.
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
    print("StokesBEM : FMM-BEM for Stokes problems\n\nUsage: StokesBEM.py <options>\n\nOptions:\n"
          "-theta <double> : Set MAC theta for treecode evaluators\n"
          "-eval {FMM,TREE} : Choose either FMM or treecode evaluator (only FMM is built)\n"
          "-p <double> : Number of terms in the Multipole / Local expansions\n"
          "-k {1,3,4,7} : Number of Gauss integration points used per panel\n"
          "-ncrit <int> : Maximum # of particles per Octree box\n"
          "-recursions <int> : number of recursive subdivisions to create a sphere - # panels = 2*4^recursions\n"
          "-rbc <int> : number of recursive subdivisions to create a red blood cell - # panels = 2*4^recursions\n"
          "-cells <int> : number of red blood cells to generate\n"
          "-fixed_p : Disable relaxation\n"
          "-pmin <int>, -mu <double>, -kfine <int>, -solver_tol <double>, -mesh <file.msh>, -vert <f> -face <f>,\n"
          "-fgmres, -diagonal, -local\n"
          "-block_inverse : (not a flag of the reference) GMRES preconditioned by the exact inverse of the leaf-diagonal blocks\n"
          "-stokes_batch <int> : (not a flag of the reference) vectors one near-field pass of a batch serves: 2, 3 or 4\n"
          "-resistance : (not a flag of the reference) the 3 x 3 translational resistance matrix, three solves in one batch\n"
          "-field <int> : (not a flag of the reference) the solved layer's velocity on N points at r = 3, by the Direct sum\n"
          "-field_fmm <int> : (not a flag of the reference) the same velocity by the FMM (plan.field_plan)\n"
          "-field_pressure : (not a flag of the reference) with -field_fmm: the pressure on the same points (execute_pressure)\n"
          "-field_stress : (not a flag of the reference) with -field_fmm: the velocity gradient and stress on the same points\n"
          "-field_direct : (not a flag of the reference) with -field_fmm and -field_pressure / -field_stress: their difference from the Direct sum\n"
          "-help : print this message")
    sys.exit(0)


class _Logged(list):
    """The per-iteration line of GMRES_Stokes.hpp:253."""

    def append(self, row):
        super().append(row)
        print("it: %03d, res: %.3e, fmm_req_p: %01d" % (row[0], row[2], row[1]))


def sphere_points(m, radius):
    """m points spread over a sphere (golden-angle spiral), as LaplaceBEM.py -field places them"""
    i = np.arange(m) + 0.5
    z = 1 - 2 * i / m
    r = np.sqrt(1 - z * z)
    phi = math.pi * (3 - math.sqrt(5)) * i
    return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def main(argv):
    if len(argv) == 1:
        print_help_and_exit()
    recursions, p, k, kfine, cells, mu, p_min = 4, 8, 4, 19, 1, 1e-3, 5
    theta, ncrit = 0.5, 64
    mesh = vert = face = None
    rbc, near_f32, field, field_fmm = False, 0, 0, 0
    stokes_batch, resistance, field_pressure, field_stress, field_direct = 0, False, False, False, False
    so = fb.SolverOptions()
    solver, pc = "gmres", "identity"
    i = 1
    while i < len(argv):
        a = argv[i]
        if a == "-p":
            i += 1; p = int(argv[i])
        elif a == "-pmin":
            i += 1; p_min = int(argv[i])
        elif a == "-k":
            i += 1; k = int(argv[i])
        elif a == "-mu":
            i += 1; mu = float(argv[i])
        elif a == "-recursions":
            i += 1; recursions = int(argv[i])
        elif a == "-rbc":
            i += 1; recursions = int(argv[i]); rbc = True
        elif a == "-cells":
            i += 1; cells = int(argv[i])
        elif a == "-fixed_p":
            so.variable_p = False
        elif a == "-solver_tol":
            i += 1; so.residual = float(argv[i])
        elif a == "-mesh":
            i += 1; mesh = argv[i]
        elif a == "-fgmres":
            solver = "fgmres"
        elif a in ("-diagonal", "-diag"):
            solver, pc = "fgmres", "diagonal"
        elif a == "-local":
            solver, pc = "fgmres", "local"
        elif a == "-help":
            print_help_and_exit()
        elif a == "-kfine":
            i += 1; kfine = int(argv[i])
        elif a == "-vert":
            i += 1; vert = argv[i]
        elif a == "-face":
            i += 1; face = argv[i]
        elif a == "-theta":                                # get_options(), include/FMMOptions.hpp
            i += 1; theta = float(argv[i])
        elif a == "-ncrit":
            i += 1; ncrit = int(argv[i])
        elif a == "-eval":
            i += 1
        elif a == "-block_inverse":                        # not in the reference: solver.BlockInverse
            solver, pc = "gmres", "block_inverse"
        elif a == "-near_f32":                             # not in the reference: fmmbem_options.near_f32_max_p
            i += 1; near_f32 = int(argv[i])
        elif a == "-stokes_batch":                         # not in the reference: fmmbem_options.stokes_batch_width
            i += 1; stokes_batch = int(argv[i])
        elif a == "-resistance":                           # not in the reference: three unit translations as one batch solve
            resistance = True
        elif a == "-field":                                # not in the reference: the solved layer's velocity off the surface
            i += 1; field = int(argv[i])
        elif a == "-field_fmm":                            # not in the reference: the same velocity through plan.field_plan
            i += 1; field_fmm = int(argv[i])
        elif a == "-field_pressure":                       # not in the reference: the pressure through fplan.execute_pressure
            field_pressure = True
        elif a == "-field_stress":                         # not in the reference: fplan.execute_velocity_gradient / execute_stress
            field_stress = True
        elif a == "-field_direct":                         # not in the reference: those quantities against fb.Direct's all-pairs sums
            field_direct = True
        elif a == "-disable_sparse":
            raise SystemExit("-disable_sparse: the Stokes near field is only built in assembled form")
        i += 1                                             # unknown arguments are ignored, as the reference does (:207-211)
    so.max_p, so.p_min, so.max_iters, so.restart = p, p_min, 100, 100
    if field_pressure and field_fmm <= 0:
        raise SystemExit("-field_pressure: needs -field_fmm N (the pressure is evaluated on the field plan's points)")

    if field_stress and field_fmm <= 0:
        raise SystemExit("-field_stress: needs -field_fmm N (the stress is evaluated on the field plan's points)")

    if field_direct and (field_fmm <= 0 or not (field_pressure or field_stress)):
        raise SystemExit("-field_direct: needs -field_fmm N and -field_pressure and/or -field_stress (it compares those quantities with the Direct sum)")

    if vert or face:
        print("reading mesh from %s, %s" % (vert, face))
        v = fb.read_vert_face(vert, face)
    elif mesh:
        print("reading mesh from %s" % mesh)
        v = fb.read_msh(mesh)
    elif rbc:
        v = fb.red_blood_cell(recursions) if cells <= 1 else fb.red_blood_cells(recursions, cells)
    else:
        v = fb.unit_sphere(recursions)
    n = len(v)
    opts = fb.FMMOptions()
    opts.set_mac_theta(theta)
    opts.set_max_per_box(ncrit)
    dev = torch.device("cuda", 0)

    print("generating RHS")
    tic = time.time()
    def kernel():
        K = fb.StokesSphericalBEM(p, k, mu)
        K.set_Kfine(kfine)
        return K

    # the reference runs the traction-BC plan on u = (1,0,0) here (switch_BC on every panel), prints the summed relative
    # distance of the result from 4 pi, and replaces it by the analytic value (:266-278)
    b = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    if p <= 12:
        rhs_plan = fb.FMM_plan(kernel(), v, opts, p_max=p, bc=np.ones(n, dtype=np.uint8))
        u = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        u[:, 0] = 1.0
        bt = rhs_plan.execute_torch(u.reshape(-1)).reshape(n, 3)
        print("rhs error: %.4e" % float(((bt[:, 0] - 4 * math.pi).abs() / 4 / math.pi).sum()))
        rhs_plan.close()
    else:
        print("rhs error: not evaluated (the far field of TRACTION targets is built for p <= 12)")
    b[:, 0] = 4 * math.pi
    print("done")
    setup_time = time.time() - tic

    plan = fb.FMM_plan(kernel(), v, opts, p_max=p, near_f32_max_p=near_f32, stokes_batch_width=stokes_batch)
    if stokes_batch:
        print("batched near field: one pass serves %d vectors" % plan.batch_width())
    if near_f32:
        print("float near field: matvecs at p <= %d stream %.3f GB of float entries" % (near_f32, plan.stats()["near_f32_bytes"] / 1e9))
    # x(panels.size(), charge_type(1.)): Vec<3,double> with ONE argument is the zero vector
    x = torch.zeros(3 * n, dtype=torch.float64, device=dev)
    log = _Logged()
    tic = time.time()
    if pc == "block_inverse":
        print("Solver: GMRES, Preconditioner: Block inverse")
        x, it, res = fb.gmres(plan, x, b.reshape(-1), so, M=fb.BlockInverse(fb, kernel(), v, ncrit=ncrit), log=log, stokes=True)
    elif solver == "gmres":
        print("Solver: GMRES, Preconditioner: Identity")
        x, it, res = fb.gmres(plan, x, b.reshape(-1), so, log=log, stokes=True)
    elif pc == "identity":
        print("Solver: FGMRES, Preconditioner: Identity")
        x, it, res = fb.fgmres(plan, x, b.reshape(-1), so, lambda z: z, log=log, stokes=True)
    elif pc == "diagonal":
        print("Solver: FGMRES, Preconditioner: Block-Diagonal")
        x, it, res = fb.fgmres(plan, x, b.reshape(-1), so, fb.BlockDiagonal(fb, kernel(), v), log=log, stokes=True)
    else:
        print("Solver: FGMRES, Preconditioner: Local Solve")
        x, it, res = fb.fgmres(plan, x, b.reshape(-1), so, fb.LocalInnerSolver(fb, kernel(), v), log=log, stokes=True)
    torch.cuda.synchronize()
    solve_time = time.time() - tic
    print("\nTIMING:\n\tsetup : %.4es\n\tsolve : %.4es\n" % (setup_time, solve_time))

    t = x.reshape(n, 3).cpu().numpy()
    e0, e1 = v[:, 2] - v[:, 0], v[:, 1] - v[:, 0]
    area = 0.5 * np.linalg.norm(np.cross(e0, e1), axis=1)
    fx, fy, fz = (t * area[:, None]).sum(axis=0)
    t_exact = 1.5 * mu
    print("t_exact : %.4g" % t_exact)
    approx = t[:, 0] * area                                # the driver compares t_x * Area with t_exact (:349-351)
    e, e2 = float(((approx - t_exact) ** 2).sum()), n * t_exact * t_exact
    analytical, analytical_area = 6 * math.pi * mu, 4 * math.pi
    print("\n\nFx: %.5f, analytical: %.4g" % (fx, analytical))
    print("Fy: %.4g, Fz: %.4g" % (fy, fz))
    drag_error = abs(analytical - fx) / abs(analytical)
    print("error on a sphere: %.5e" % drag_error)
    print("\n\n\n\tdrag error per panel : %.5e, average panel area: %.5e" % (drag_error / n, area.sum() / n))
    print("\tArea error : %.5e" % (abs(area.sum() - analytical_area) / analytical_area))
    print("\n\nPOINTWISE ERRORS\n\terror: %.3e" % math.sqrt(e / e2))
    u = None
    if field > 0:
        direct = fb.Direct(kernel(), v)
        u = direct.matvec_torch(x, torch.from_numpy(sphere_points(field, 3.0)).to(dev)).cpu().numpy()
        direct.close()
        mag = np.linalg.norm(u, axis=1)
        print("field: %d points at r = 3, max |u|: %.6e, mean |u|: %.6e" % (field, float(mag.max()), float(mag.mean())))
    if field_fmm > 0:
        fplan = plan.field_plan(sphere_points(field_fmm, 3.0))       # VELOCITY targets: the single layer
        plan.kernel().set_p(p)                             # (the relaxed solve leaves the kernel at its last order)
        q = gu = sig = None
        if field_pressure or field_stress:
            # ONE flow execute (fmmbem_plan_execute_flow): the velocity, the pressure (the stress needs it too) and the gradient on
            # one far chain, each with the bits of its single execute; the stress by execute_stress's formula
            uf, q, gu = (a if a is None else a.cpu().numpy() for a in fplan.execute_flow_torch(x, True, True, field_stress))
            if field_stress:
                sig = -q[:, None, None] * np.eye(3)[None] + fplan.kernel().Mu * (gu + gu.transpose(0, 2, 1))
            if not field_pressure:
                q = None
        else:
            uf = fplan.execute_torch(x).cpu().numpy()
        fplan.close()
        q_direct = gu_direct = None
        if field_direct:
            direct = fb.Direct(kernel(), v)
            pts_d = torch.from_numpy(sphere_points(field_fmm, 3.0)).to(dev)
            q_direct = direct.pressure_torch(x, pts_d).cpu().numpy() if field_pressure else None
            gu_direct = direct.velocity_gradient_torch(x, pts_d).cpu().numpy() if field_stress else None
            direct.close()
        mag = np.linalg.norm(uf, axis=1)
        print("field (FMM): %d points at r = 3, max |u|: %.6e, mean |u|: %.6e" % (field_fmm, float(mag.max()), float(mag.mean())))
        if u is not None and field == field_fmm:
            print("field (FMM) against field: relative L2 difference %.3e" % float(np.linalg.norm(uf - u) / np.linalg.norm(u)))
        if q is not None:
            print("field pressure (FMM): %d points at r = 3, max |q|: %.6e, mean |q|: %.6e" % (field_fmm, float(np.abs(q).max()), float(np.abs(q).mean())))
            if q_direct is not None:
                print("field pressure (FMM) against Direct: relative L2 difference %.3e" % float(np.linalg.norm(q - q_direct) / np.linalg.norm(q_direct)))
            if not (rbc or mesh or vert or face):
                # a sphere of radius a translating with U: p = (3/2) mu a U.x / r^3; q = 4 pi p and the solve's U is e_x
                pts = sphere_points(field_fmm, 3.0)
                dev_q = np.abs(q / (6 * math.pi * mu) - pts[:, 0] / 27.0).max() * 9.0
                print("field pressure against the translating sphere's: largest deviation %.3e of 1/9" % float(dev_q))
        if gu is not None:
            print("field velocity gradient (FMM): %d points at r = 3, max |G|: %.6e, mean |G|: %.6e" % (field_fmm, float(np.abs(gu).max()), float(np.abs(gu).mean())))
            if gu_direct is not None:
                print("field velocity gradient (FMM) against Direct: relative L2 difference %.3e" % float(np.linalg.norm(gu - gu_direct) / np.linalg.norm(gu_direct)))
            print("field stress (FMM): %d points at r = 3, max |sigma|: %.6e, mean |sigma|: %.6e" % (field_fmm, float(np.abs(sig).max()), float(np.abs(sig).mean())))
            if not (rbc or mesh or vert or face):
                # a unit sphere translating with e_x: u = 3/4 (e_x / r + x x_1 / r^3) + 1/4 (e_x / r^3 - 3 x x_1 / r^5); its gradient
                # by central differences of that closed form (h = 1e-4: 1e-11 of it, far below the discretisation's error)
                def u_exact(y):
                    r = np.linalg.norm(y, axis=1)[:, None]
                    ex = np.zeros_like(y)
                    ex[:, 0] = 1
                    return 0.75 * (ex / r + y * y[:, 0:1] / r ** 3) + 0.25 * (ex / r ** 3 - 3 * y * y[:, 0:1] / r ** 5)
                pts = sphere_points(field_fmm, 3.0)
                ge = np.empty((field_fmm, 3, 3))
                for m_ in range(3):
                    e_ = np.zeros(3)
                    e_[m_] = 1e-4
                    ge[:, :, m_] = (u_exact(pts + e_) - u_exact(pts - e_)) / 2e-4
                dev_g = np.abs(gu / (4 * math.pi) - ge).max() / np.abs(ge).max()
                print("field velocity gradient against the translating sphere's: largest deviation %.3e of its largest entry" % float(dev_g))
    if resistance:
        # unit translation e_j on every panel: the right-hand side 4 pi e_j (as b above), the force of the solved traction
        B = torch.zeros((3, n, 3), dtype=torch.float64, device=dev)
        for j in range(3):
            B[j, :, j] = 4 * math.pi
        X = torch.zeros_like(B)
        plan.kernel().set_p(p)
        X, its, _, seconds = fb.gmres_capi_batch(plan, X, B, so, stokes=True)
        torch.cuda.synchronize()
        R = (X.cpu().numpy() * area[None, :, None]).sum(axis=1).T          # R[i][j]: force component i of translation e_j
        print("\nresistance matrix (3 translations in one batch of width %d, %s iterations, %.4es):" % (plan.batch_width(), its, seconds))
        for row in R:
            print("\t% .6e % .6e % .6e" % tuple(row))
        print("resistance deviation from 6 pi mu I: %.5e" % (float(np.abs(R - analytical * np.eye(3)).max()) / analytical))
    return it, res, drag_error, [row[1] for row in log]


if __name__ == "__main__":
    main(sys.argv)

"""A plan for an A/B comparison that owns its geometry.

fmmbem_plan_create recognises the vertices and options of a live plan and hands the new plan that plan's PlanShared
(csrc/plan.hip: geometry_cache_find / same_geometry_options).  same_geometry_options compares the fields of fmmbem_options only;
the plan-time environment switches below are read ONCE, into the shared PlanGeometry / HostPlan, by the plan that builds the
geometry, and fmmbem_plan::like rebuilds only what the boundary flags decide.  A plan created under such a switch while a plan of
the same vertices and options is alive -- in a fixture, a module cache, or on the right of `pl = FMM_plan(...)`, where the old
plan is still referenced -- runs the LIVE plan's kernels, and a comparison of the two compares a kernel with itself.

Geometry-level switches (an A/B plan must go through plan_under), and where each is read:

    FMMBEM_M2L_ROT                                      g.rot_max                      plan.hip, to_device_near (layout_options)
    FMMBEM_SHIFT_LANES, FMMBEM_SHIFT_LANES_MAX,
    FMMBEM_SHIFT_ROT, FMMBEM_SHIFT_ROT_MIN              g.shift_lanes ... g.shift_rot_min, the tree passes' form; plan.hip
    FMMBEM_STOKES_SYM, FMMBEM_NEAR_STREAM_FRACTION      near_layout                    plan.hip, to_device_near (layout_options)
    FMMBEM_ROT_ITEM_PASSES, FMMBEM_ROT_LONG_MAX,
    FMMBEM_ROT_LONG_ROUNDS                              the cut of M2L pairs to items  host_plan.cpp (HostPlan)

Not affected by the recognition: the per-plan switches, read by every plan for itself -- FMMBEM_P2M_TABLE and
FMMBEM_P2M_TABLE_POINTS (plan.hip, to_device_bc_end), FMMBEM_ASM_COLS, FMMBEM_GRAPH -- and the live ones of csrc/switches.hpp
(FMMBEM_NEAR_P2M, FMMBEM_P2M_STREAM, FMMBEM_L2P_SCATTER, FMMBEM_L2P_GENERIC, FMMBEM_OPS_GENERIC, FMMBEM_MULTI_ISSUE_THREADS),
read at every launch.

FMMBEM_PLAN_SHARE=0 switches the recognition off for the plans created under it: such a plan neither takes a live geometry nor
enters the cache, so no later plan takes its geometry either."""
GEOMETRY_SWITCHES = (
    "FMMBEM_M2L_ROT", "FMMBEM_SHIFT_LANES", "FMMBEM_SHIFT_LANES_MAX", "FMMBEM_SHIFT_ROT", "FMMBEM_SHIFT_ROT_MIN",
    "FMMBEM_STOKES_SYM", "FMMBEM_NEAR_STREAM_FRACTION", "FMMBEM_ROT_ITEM_PASSES", "FMMBEM_ROT_LONG_MAX", "FMMBEM_ROT_LONG_ROUNDS",
)


def under(monkeypatch, env, make, plan_of=None):
    """make() under FMMBEM_PLAN_SHARE=0 and `env`, both removed again; the plan it returns (the first of a tuple; plan_of(what it
    returns) where given) owns its geometry.  For plans that a helper of a test file creates."""
    env = dict(env or {})
    for name in env:
        assert name.startswith("FMMBEM_"), name
    with monkeypatch.context() as m:
        m.setenv("FMMBEM_PLAN_SHARE", "0")
        for name, value in env.items():
            m.setenv(name, str(value))
        made = make()
        plan = plan_of(made) if plan_of else made[0] if isinstance(made, tuple) else made
        assert plan.stats()["geometry_shared"] == 1
    return made


def plan_under(fb, monkeypatch, env, *args, **kw):
    """fb.FMM_plan(*args, **kw) created under the environment `env` (a dict, or None for the default path) as the only holder of
    its geometry: sets FMMBEM_PLAN_SHARE=0 and env, creates the plan, asserts stats()["geometry_shared"] == 1, removes what it
    set (what the caller had set before comes back), returns the plan."""
    return under(monkeypatch, env, lambda: fb.FMM_plan(*args, **kw))

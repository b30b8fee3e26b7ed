"""The near field and P2M as ONE launch (near_p2m_kernel, kernels_near.hip: the P2M workgroups queued behind the near field's in
one grid) against the two launches it replaces: y and M of every box, bit for bit.  FMMBEM_NEAR_P2M is read at every execute:
0 = two launches, 1 / unset = one launch where the execute is eligible, 2 = one launch or FMMBEM_ERR_UNSUPPORTED -- which is
how these tests know that the combined kernel ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 6


def _two_spheres(fb, r):
    return np.concatenate([fb.unit_sphere(r), fb.unit_sphere(r, center=(3.0, 0.0, 0.0))])


def _opts(fb, ncrit):
    o = fb.FMMOptions()
    o.set_max_per_box(ncrit)
    return o


def _run(pl, x, p):
    """(y, M of every box) of one execute at order p, as torch tensors on the host"""
    import torch
    y = pl.execute_torch(torch.from_numpy(x).cuda(), p=p)
    torch.cuda.synchronize()
    return y.cpu(), torch.from_numpy(pl.expansions("M", p))


def _same(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("first", ["2", "0"])
@pytest.mark.parametrize("p", [8, 10, 12])
def test_one_launch_gives_the_bits_of_two(fb, monkeypatch, p, first):
    """Two unit spheres of recursion 5 (4 096 panels, 64 to a leaf) at the orders the streaming P2M serves.  Either way round: a
    plan built and run combined first, and one run separately first; and each plan once more the other way."""
    v = _two_spheres(fb, 5)
    x = np.random.default_rng(41).standard_normal(len(v))
    second = "0" if first == "2" else "2"
    got = {}
    monkeypatch.setenv("FMMBEM_NEAR_P2M", first)
    a = fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v, _opts(fb, 64))
    got[first] = _run(a, x, p)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", second)
    b = fb.FMM_plan(fb.LaplaceSphericalBEM(p, 3), v, _opts(fb, 64))
    got[second] = _run(b, x, p)
    assert float(got["0"][1].abs().max()) > 0
    assert _same(got["2"], got["0"])
    assert _same(_run(a, x, p), got["0"])              # the first plan, now the second way
    monkeypatch.setenv("FMMBEM_NEAR_P2M", first)
    assert _same(_run(b, x, p), got["0"])


@pytest.mark.parametrize("graphs", [False, True])
def test_relaxed_sequence_on_one_plan(fb, monkeypatch, graphs):
    """The solver's relaxation of p on one plan: 10, 8, 12, 10, 3.  p = 3 is below the streaming P2M and silently takes the two
    launches.  With graphs: launch by launch, captured, replayed."""
    v = _two_spheres(fb, 5)
    x = np.random.default_rng(42).standard_normal(len(v))
    seq = (10, 8, 12, 10, 3)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    sep = fb.FMM_plan(fb.LaplaceSphericalBEM(12, 3), v, _opts(fb, 64))
    want = {p: _run(sep, x, p) for p in set(seq)}
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(12, 3), v, _opts(fb, 64))
    pl.set_graphs(graphs)
    for rep in range(3 if graphs else 1):
        for p in seq:
            assert _same(_run(pl, x, p), want[p]), (rep, p)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")          # and 3 is indeed not eligible, 10 is
    with pytest.raises(fb.FmmBemError) as e:
        _run(pl, x, 3)
    assert e.value.status == ERR_UNSUPPORTED
    assert _same(_run(pl, x, 10), want[10])


def test_p2m_workgroups_queue_behind_a_full_near_grid(fb, monkeypatch):
    """One sphere of recursion 7 (32 768 panels, 16 to a leaf) at p = 10.  Every leaf is at least one near-field work item (its
    own rows against itself), so more than 1 280 leaves are more than 1 280 items: the near part of the grid is the 1 280
    workgroups that fill the chip, and the P2M workgroups start only as those retire."""
    v = fb.unit_sphere(7)
    x = np.random.default_rng(43).standard_normal(len(v))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, _opts(fb, 16))
    st = pl.stats()
    assert st["n_leaves"] > 1280 and st["p2m_leaves"] > 1280
    one = _run(pl, x, 10)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    assert _same(one, _run(pl, x, 10))
    assert _same(one, _run(fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, _opts(fb, 16)), x, 10))


def test_last_p2m_workgroup_with_idle_wavefronts(fb, monkeypatch):
    """A P2M workgroup is four wavefronts, a leaf each: UnitSphere(5) without its last 28 panels has 271 leaves at 16 panels to
    a leaf, so the last workgroup has one wavefront without a leaf."""
    v = fb.unit_sphere(5)[:-28]
    x = np.random.default_rng(44).standard_normal(len(v))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, _opts(fb, 16))
    assert pl.stats()["p2m_leaves"] % 4 != 0, pl.stats()["p2m_leaves"]
    one = _run(pl, x, 10)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    two = _run(fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, _opts(fb, 16)), x, 10)
    assert float(two[1].abs().max()) > 0
    assert _same(one, two)


def test_stage_timing_keeps_the_two_launches(fb, monkeypatch):
    """With stage timing on, the events bracket the near kernel and P2M each alone: the execute takes the two launches, gives the
    same bits, and both stages report a time."""
    v = _two_spheres(fb, 5)
    x = np.random.default_rng(45).standard_normal(len(v))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, _opts(fb, 64))
    untimed = _run(pl, x, 10)
    pl.set_timing(1)
    assert _same(_run(pl, x, 10), untimed)
    st = pl.stats()
    assert st["ms_near"] > 0 and st["ms_p2m"] > 0
    pl.set_timing(2)
    assert _same(_run(pl, x, 10), untimed)
    assert pl.stats()["ms_near"] > 0
    pl.set_timing(False)
    assert _same(_run(pl, x, 10), untimed)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")          # timed executes are not eligible
    pl.set_timing(1)
    with pytest.raises(fb.FmmBemError) as e:
        _run(pl, x, 10)
    assert e.value.status == ERR_UNSUPPORTED
    pl.set_timing(False)
    assert _same(_run(pl, x, 10), untimed)


@pytest.mark.parametrize("kind", ["stokes", "targets"])
def test_plans_that_keep_the_two_launches(fb, monkeypatch, kind):
    """A Stokes plan and a plan over separate targets never take the combined launch: FMMBEM_NEAR_P2M=2 is the unsupported
    error there, and the plan goes on working."""
    import torch
    if kind == "stokes":
        v = fb.red_blood_cell(4)
        pl = fb.FMM_plan(fb.StokesSphericalBEM(8, 3, 1e-3), v)
        x = np.random.default_rng(46).standard_normal((len(v), 3))
    else:
        v = fb.unit_sphere(5)
        pts = 1.5 * np.random.default_rng(47).standard_normal((300, 3))
        pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, targets=pts)
        x = np.random.default_rng(46).standard_normal(len(v))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    before = torch.from_numpy(pl.execute(x))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")
    with pytest.raises(fb.FmmBemError) as e:
        pl.execute(x)
    assert e.value.status == ERR_UNSUPPORTED
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    assert torch.equal(torch.from_numpy(pl.execute(x)), before)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    assert torch.equal(torch.from_numpy(pl.execute(x)), before)


# ---- the edges of the eligibility rule (near form Pipe and P2M form Stream, launch_choice.hpp), each proved by FMMBEM_NEAR_P2M=2 ----

def _refused(fb, pl, x, p):
    with pytest.raises(fb.FmmBemError) as e:
        _run(pl, x, p)
    assert e.value.status == ERR_UNSUPPORTED


def test_order_edge_of_the_streaming_p2m(fb, monkeypatch):
    """p = 7 has 28 coefficients and keeps p2m_apply_kernel; p = 8 has 36, more than half a wavefront, and streams: on one plan
    the first is refused, the second runs, and both give the bits of the two launches."""
    v = _two_spheres(fb, 5)
    x = np.random.default_rng(48).standard_normal(len(v))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, _opts(fb, 64))
    before = {p: _run(pl, x, p) for p in (7, 8)}
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")
    _refused(fb, pl, x, 7)
    assert _same(_run(pl, x, 8), before[8])
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    assert _same(_run(pl, x, 7), before[7])


def test_p2m_stream_switch_is_read_at_every_launch(fb, monkeypatch):
    """FMMBEM_P2M_STREAM=0 takes the streaming P2M away from a live plan, so p = 10 is refused; unset again, p = 10 runs combined
    on the same plan.  The plan and the near-field launcher read the switch at the same call, through the same function."""
    v = _two_spheres(fb, 5)
    x = np.random.default_rng(49).standard_normal(len(v))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, _opts(fb, 64))
    before = _run(pl, x, 10)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")
    assert _same(_run(pl, x, 10), before)
    monkeypatch.setenv("FMMBEM_P2M_STREAM", "0")
    _refused(fb, pl, x, 10)
    monkeypatch.delenv("FMMBEM_P2M_STREAM")
    assert _same(_run(pl, x, 10), before)


def test_float_near_field_keeps_the_two_launches(fb, monkeypatch):
    """near_f32_max_p = 5: p = 4 streams the float copy (and is below the streaming P2M) and is refused; p = 8 takes the FP64
    matrix and runs combined."""
    v = _two_spheres(fb, 5)
    x = np.random.default_rng(50).standard_normal(len(v))
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "0")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(8, 3), v, _opts(fb, 64), near_f32_max_p=5)
    assert pl.stats()["near_f32_bytes"] > 0
    before = {p: _run(pl, x, p) for p in (4, 8)}
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")
    _refused(fb, pl, x, 4)
    assert _same(_run(pl, x, 8), before[8])
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    assert _same(_run(pl, x, 4), before[4])
    assert pl.stats()["last_near_f32"] == 1


def test_hybrid_plan_keeps_the_two_launches(fb, monkeypatch):
    """near_stream_fraction = 0.5: the near field is launch_near_hybrid's two kernels, never near_spmv_pipe_kernel alone."""
    v = _two_spheres(fb, 5)
    x = np.random.default_rng(51).standard_normal(len(v))
    o = _opts(fb, 64)
    o.near_stream_fraction = 0.5
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    pl = fb.FMM_plan(fb.LaplaceSphericalBEM(10, 3), v, o)
    assert pl.stats()["near_recomputed_pairs"] > 0
    before = _run(pl, x, 10)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "2")
    _refused(fb, pl, x, 10)
    monkeypatch.setenv("FMMBEM_NEAR_P2M", "1")
    assert _same(_run(pl, x, 10), before)

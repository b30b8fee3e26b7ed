"""The cases of tests/m2l_form_cases.py have the M2L lists that tests/test_gpu_m2l_forms.py needs them to have: held here on the
host, with the CPU oracle, so that a changed generator cannot quietly empty a case of the path it is there for."""
import numpy as np
import pytest

import m2l_form_cases as mfc


@pytest.fixture(scope="module")
def measured(oracle_mod):
    out = {}
    for name in mfc.CASES:
        o = mfc.make_oracle(oracle_mod, name, "velocity" if mfc.is_stokes(name) else "potential")
        out[name] = mfc.m2l_figures(o)
        o.close()
    return out


@pytest.mark.parametrize("name", list(mfc.CASES))
def test_the_lists_are_the_recorded_ones(measured, name):
    fig, st = measured[name]
    print(name, fig)
    assert fig == mfc.FIGURES[name]
    assert st["l2l_skipped"] == 0                      # the reference's L2L rule and the complete one coincide on these trees


def test_what_each_case_is_for(measured):
    fig = {name: f for name, (f, _) in measured.items()}
    # m2l_small_kernel's lane loop, pi = pb + lane; pi += 64: one, two and three rounds
    assert fig["two_r54"]["le64"] > 0 and fig["two_r54"]["le128"] > 0 and fig["two_r54"]["gt128"] > 0
    assert 128 < fig["two_r54"]["sources"][1] <= 192
    assert fig["soup2500"]["gt128"] > 0
    # the XCD remap of m2l_kernel deals targets in blocks of 512 workgroups
    assert fig["two_r54"]["targets"] < 512
    assert fig["soup2500"]["targets"] > 1024 and fig["soup2500"]["targets"] % 512 != 0
    assert fig["stokes_soup1500"]["targets"] > 512
    assert fig["tiny48"]["targets"] < 64 and fig["tiny48"]["sources"][0] == 1
    assert fig["stokes_r43"]["pairs"] > 0


@pytest.mark.parametrize("name", ["two_r54", "soup2500", "tiny48"])
def test_flag_sets_pick_the_slots(oracle_mod, name):
    n = len(mfc.vertices(oracle_mod, name))
    assert mfc.flags(name, "potential", n) is None
    assert mfc.flags(name, "normal_deriv", n).all()
    mixed = mfc.flags(name, "mixed", n)
    assert 0 < mixed.sum() < n
    assert np.array_equal(mixed, mfc.flags(name, "mixed", n))              # seeded


def test_the_far_part_is_a_visible_share_of_the_result(oracle_mod):
    """0.07 (tiny48) to 0.57 of |y| at p = 8: an M2L that went wrong moves the rows far above the gates"""
    for name in ("two_r54", "tiny48"):
        o = mfc.make_oracle(oracle_mod, name, "potential")
        x = mfc.density(name, o.n)
        far = o.matvec(x, 8) - o.near_only(x)
        share = float(np.linalg.norm(far) / np.linalg.norm(o.matvec(x, 8)))
        print(name, "far part %.3f of |y|" % share)
        assert 0.05 <= share <= 0.7, (name, share)
        o.close()

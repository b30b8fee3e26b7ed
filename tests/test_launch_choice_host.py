"""csrc/launch_choice.hpp without a device: which kernel a launch takes, its grid and its dynamic LDS, at the edges of every rule.
tests/cpp/launch_choice_cases.cpp fills DevicePlan fields by hand and prints the header's answers; the expectations below are
written out from the launchers as they stood before the header existed (kernels_near.hip, kernels_far.hip), not computed by it:
  near grid   min(items, 256 * workgroups per CU): 5 for the single-vector kernels; 4, 2, 1 for the pipelined kernel at 2, 4, 8
              vectors; 3, 2, 1 for the symmetric Stokes kernel at 2, 3, 4
  near LDS    Pipe 2 * nv * 1024 * 8 + 4 * 4 * max_runs;  Sym3 nv * 3 * 1024 * 8 + 2 * 4 * max_runs;  Plain 2048 * 8 + 2 * 4 * max_runs
  P2M grid    Stream min(ceil(leaves / 4), 2048);  Apply min(ceil(leaves / 4), 4096);  Recurrence min(ceil(leaves / 4), 2048)
  tree pass   the rule as it stood in plan.hip (PlanGeometry::shift_form): with FMMBEM_SHIFT_ROT on, the wavefront kernel up to
              lanes_max pair-slots (pairs x live slots) where it is switched on and instantiated -- L2L 16 384; M2M 16 384 at
              p = 10, 8 192 at p = 9, else 2 048; FMMBEM_SHIFT_LANES_MAX for all -- then the rotation kernel where instantiated
              and (wavefront kernel switched on, or the child level has shift_rot_min = 2 048 boxes), else the sparse operators"""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "launch_choice_cases.cpp")

NEAR = {
    "runs256": "Pipe grid=1280 lds=20480",              # 256 runs: one descriptor per thread of the workgroup, the last that fits
    "runs257": "Plain grid=1280 lds=18440",
    "stokes_sym": "Sym3 grid=1280 lds=24656",
    "stokes_full": "Plain grid=1280 lds=16464",
    "hybrid": "Hybrid",
    "hybrid_empty": "Hybrid",                           # launch_near_spmv refuses a hybrid plan before it looks at the items
    "empty": "Empty",
    "items1279": "Pipe grid=1279 lds=16544",
    "items1280": "Pipe grid=1280 lds=16544",
    "items1281": "Pipe grid=1280 lds=16544",
}
P2M = {
    "p7": "Apply grid=250",                             # 28 coefficients
    "p8": "Stream grid=250",                            # 36: more than half a wavefront
    "p0": "Invalid",
    "p16": "Stream grid=250",
    "p17": "Invalid",
    "two_slots": "Apply grid=250",
    "no_table": "Recurrence grid=250",
    "no_leaves": "Empty",
    "no_leaves_p0": "Empty",                            # an empty P2M succeeds before the order is looked at
    "leaves8188": "Stream grid=2047",
    "leaves8192": "Stream grid=2048",
    "leaves8196": "Stream grid=2048",
    "apply_cap": "Apply grid=4096",
    "recurrence_cap": "Recurrence grid=2048",
}
MULTI = {
    "Pipe nv=2": "grid=1024 lds=32928",
    "Pipe nv=4": "grid=512 lds=65696",
    "Pipe nv=8": "grid=256 lds=131232",
    "Sym3 nv=2": "grid=768 lds=49232",
    "Sym3 nv=3": "grid=512 lds=73808",
    "Sym3 nv=4": "grid=256 lds=98384",
}
SYM3_OK = {"width=1": 0, "width=2": 1, "width=4": 1, "width=5": 0,
           "runs7680": 1,                               # 4 * 24 576 + 8 * 7 680 = 159 744 = 156 KiB exactly
           "runs7681": 0, "laplace": 0, "no_items": 0}
# key: switches_pass_order_pairs x live slots_boxes of the child level
SHIFT_THRESHOLDS = {
    "M2M_p8_2048x1": "Lanes", "M2M_p8_2049x1": "Rot",
    "M2M_p8_512x4": "Lanes", "M2M_p8_513x4": "Rot",          # Stokes: four live slots
    "M2M_p9_8192x1": "Lanes", "M2M_p9_8193x1": "Rot",
    "M2M_p10_16384x1": "Lanes", "M2M_p10_16385x1": "Rot",
    "M2M_p11_2048x1": "Lanes", "M2M_p11_2049x1": "Rot",
    "L2L_p3_16384x1": "Lanes", "L2L_p3_16385x1": "Rot",
    "L2L_p10_4096x4": "Lanes", "L2L_p10_4097x4": "Rot",
}
SHIFT = {"dflt_%s_boxes0" % k: v for k, v in SHIFT_THRESHOLDS.items()}
SHIFT.update({"rot_off_%s_boxes0" % k: "Sparse" for k in SHIFT_THRESHOLDS})          # FMMBEM_SHIFT_ROT=0
SHIFT.update({"unsupported_%s_boxes0" % k: "Sparse" for k in SHIFT_THRESHOLDS})      # p > 12: neither kernel is instantiated
SHIFT.update({
    "dflt_M2M_p10_1073741824x4_boxes0": "Rot",              # 2^32 pair-slots: a 32-bit product would be 0 and say Lanes
    "dflt_L2L_p10_1073741824x4_boxes0": "Rot",
    "dflt_M2M_p10_1x1_boxes0": "Lanes",
    "lanes_off_M2M_p10_1x1_boxes2047": "Sparse",            # FMMBEM_SHIFT_LANES=0: the level's size in the whole tree decides
    "lanes_off_M2M_p10_1x1_boxes2048": "Rot",
    "lanes_unsupported_M2M_p10_1x1_boxes0": "Rot",
    "rot_off_M2M_p10_1x1_boxes2048": "Sparse",
    "unsupported_M2M_p10_1x1_boxes2048": "Sparse",
    "max100_M2M_p10_100x1_boxes0": "Lanes", "max100_M2M_p10_101x1_boxes0": "Rot",    # FMMBEM_SHIFT_LANES_MAX=100: both passes, all orders
    "max100_L2L_p3_100x1_boxes0": "Lanes", "max100_L2L_p3_101x1_boxes0": "Rot",
})


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_choice") / "launch_choice_cases")
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", out, SRC], check=True)
    return out


def _lines(exe, **env):
    e = {k: v for k, v in os.environ.items() if k != "FMMBEM_P2M_STREAM"}
    e.update(env)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, env=e).stdout
    got = {}
    for line in out.splitlines():
        kind, rest = line.split(" ", 1)
        got.setdefault(kind, []).append(rest)
    return got


def _table(rows, key_words=1):
    t = {}
    for r in rows:
        w = r.split(" ")
        t[" ".join(w[:key_words])] = " ".join(w[key_words:])
    return t


def test_near_forms_grids_and_lds(exe):
    assert _table(_lines(exe)["near"]) == NEAR


def test_p2m_forms_and_grids(exe):
    assert _table(_lines(exe)["p2m"]) == P2M


def test_p2m_stream_switch_in_the_environment(exe):
    off = _table(_lines(exe, FMMBEM_P2M_STREAM="0")["p2m"])
    assert off["p8"] == "Apply grid=250" and off["p16"] == "Apply grid=250"
    assert off["leaves8196"] == "Apply grid=2049"        # Apply's cap is 4 096 workgroups
    assert off["no_table"] == "Recurrence grid=250" and off["p7"] == "Apply grid=250"
    assert all(r.endswith(" 0") for r in _lines(exe, FMMBEM_P2M_STREAM="0")["fused"])
    assert _table(_lines(exe, FMMBEM_P2M_STREAM="1")["p2m"]) == P2M


def test_combined_launch_is_pipe_and_stream_exactly(exe):
    fused = _table(_lines(exe)["fused"])
    assert len(fused) == 25
    for pair, ok in fused.items():
        assert int(ok) == (pair == "Pipe+Stream"), pair


def test_multi_vector_grids_and_lds(exe):
    got = _lines(exe)
    assert _table(got["multi"], 2) == MULTI
    assert got["batch_near_ok"] == ["laplace=1 runs257=0 stokes=0 hybrid=0"]
    assert got["near_f32_ok"] == ["1010"]               # (1, 256), (1, 257), (3, symmetric), (3, full rows)


def test_stokes_batch_widths_and_the_lds_limit(exe):
    assert {k: int(v) for k, v in _table(_lines(exe)["sym3_ok"]).items()} == SYM3_OK


def test_tree_pass_rule(exe):
    got = _table(_lines(exe)["shift"])
    assert len(got) == len(SHIFT) == 3 * 14 + 12
    assert got == SHIFT

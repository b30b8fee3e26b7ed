"""csrc/plan_layout.hpp without a device: what the arrays of a plan hold before they are uploaded.

The cutters (tests/cpp/plan_layout_cases.cpp prints what they return for inputs written by hand).  The expectations below are
written out from the rules as they stood in plan.hip (to_device_near, to_device_far, build_side_lists), not computed by the header:
  row cut        per = item_bytes // row_bytes whole rows, rounded DOWN to a multiple of 8; fewer than 8 fit: min(4, rows).  Then
                 cnt = ceil(rows / per) ranges of ceil(rows / cnt) rows, which is rounded UP to a multiple of 8 if it is 8 or more.
                 So a leaf of 58 rows x 128 248 bytes (two fit in 256 KB) is cut into ranges of 4 rows, not 2: below 8 the rule
                 never looks at how many fit.  Item sizes: 256 KB for the double rows, 512 KB for the symmetric Stokes blocks
                 at 48 bytes per pair.
  recompute cut  cnt = ceil(rows / cap) ranges of ceil(rows / cnt) rows; cap 32 (Laplace) or what rcg_item_rows() says (60)
  L2P groups     consecutive leaves until the next one would pass 64 rows or the group holds max_leaves (8; Stokes 4); a leaf of
                 more than 64 rows is a group of its own; no leaves: {0, 0}, which far_layout counts as no group
  single pass    whole units until the next one would pass 64 pairs; positions from pair_base
  side items     runs of consecutive non-empty owned rows with at most 256 entries together and at most 256 rows; a row of more
                 than 256 entries is alone; (first entry : one past, first row : one past)

Real plans (tests/cpp/plan_layout_plans.cpp, compiled with csrc/host_plan.cpp): near_layout runs inside after_near_lists, where
plan.hip runs it, and far_layout after the build; the program checks structure against the host plan -- every owned row of a
leaf that keeps its matrix in exactly one item and a recomputed leaf in none, items largest first with equal ones in leaf / row
order, records that say what the leaf's offsets, strides and runs imply, runs that expand to the rows of near_src, contiguous block
offsets and matching totals, float records on the rows of their FP64 twins, the hybrid choice (1 - f of the pairs or nothing left,
most rows first, no leaf above 8 192 columns or 256 runs), L2P groups that partition the list within their limits, l2p_scatter
exactly when the groups' rows are all rows of a single-shard Laplace plan on its own panels, launches whose pairs, unit pointers
and items partition their level, M2P chains root first along the leaf's path -- and prints one FAIL line per broken property."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import near_form_cases as NFC

CSRC = os.path.join(ROOT, "fmm-bem-relaxed_amd", "csrc")
GXX = ["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]

ROWS = {
    "r1": "0+1", "r3": "0+3", "r4": "0+4", "r7": "0+7", "r8": "0+8", "r9": "0+9",       # 256 rows of 1 KB fit: one range
    "fits": "0+64",                                     # 64 rows x 4 KB = 256 KB exactly
    "one_over": "0+40 40+25",                           # 65 rows: two ranges of ceil(65 / 2) = 33 -> 40
    "redeal": "0+56 56+44",                             # 100 rows, 64 fit: two ranges of 50 -> 56
    "wide10": "0+4 4+4 8+2", "wide3": "0+3", "wide1": "0+1",      # a row wider than an item: per = 1 -> min(4, rows)
    "coarse58": " ".join("%d+4" % r for r in range(0, 56, 4)) + " 56+2",
    "sym512": "0+7 7+7 14+6",                           # 48 000 bytes a row: 10 fit -> 8; three ranges of ceil(20 / 3) = 7, below 8: kept
    "sym256": "0+4 4+4 8+4 12+4 16+4",                  # 5 fit -> min(4, rows)
    "sym512_fits": "0+64",                              # 170 pairs: 8 160 bytes a row, 64 fit
}
RECOMPUTE = {"cap32_r32": "0+32", "cap32_r33": "0+17 17+16", "cap32_r61": "0+31 31+30",
             "cap60_r60": "0+60", "cap60_r61": "0+31 31+30", "cap60_r1": "0+1"}
L2P = {"rows64": "0 2", "rows65": "0 1 2", "nine_max8": "0 8 9", "nine_max4": "0 4 8 9", "big_between": "0 1 2 3", "big_first": "0 1 2",
       "empty": "0 0"}
PASS = {"pairs64": "0 64", "pairs65": "0 64 65", "pairs65_base100": "100 164 165", "none": "5"}
SIDE = {"e256": "0:256,0:2", "e257": "0:128,0:1 128:257,1:2", "row300": "0:5,0:1 5:305,1:2 305:310,2:3", "empty_row": "0:3,0:1 3:7,2:3",
        "rows300": "0:256,0:256 256:300,256:300", "owned_1_3": "1:3,1:3", "nothing": ""}


def test_cutters_by_hand(tmp_path):
    exe = str(tmp_path / "plan_layout_cases")
    subprocess.run(GXX + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_layout_cases.cpp"), "-pthread"], check=True)
    got = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, name, *rest = line.split(" ")
        got.setdefault(kind, {})[name] = " ".join(rest)
    assert got == {"rows": ROWS, "recompute": RECOMPUTE, "l2p": L2P, "pass": PASS, "side": SIDE}


@pytest.fixture(scope="module")
def plans(tmp_path_factory, fb):
    """The driver, and the meshes as files: int64 n, n x 9 doubles, n flag bytes (targets: m, m x 3 doubles, m flag bytes)"""
    d = tmp_path_factory.mktemp("plan_layout")
    exe = str(d / "plan_layout_plans")
    subprocess.run(GXX + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_layout_plans.cpp"), os.path.join(CSRC, "host_plan.cpp"), "-pthread"],
                   check=True)

    def write(name, v, flags):
        path = str(d / name)
        with open(path, "wb") as f:
            f.write(np.int64(len(v)).tobytes())
            f.write(np.ascontiguousarray(v, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(flags, dtype=np.uint8).tobytes())
        return path

    s = np.asarray(fb.unit_sphere(5), dtype=np.float64).reshape(-1, 3, 3)
    assert len(s) == 2048
    two = np.concatenate([s, 0.5 * s + np.array([2.0, 0.3, 0.0])])
    rng = np.random.default_rng(31)
    soup, soup_bc, soup_ncrit = NFC.case_input(107, True)               # leaves of 1-59 rows
    ssoup, ssoup_bc, ssoup_ncrit = NFC.case_input(201, True)            # Stokes: leaves of 1-15 rows
    # targets: on the first sphere's centroids, close to the surfaces, and far away from both
    pts = np.concatenate([s[:300].mean(axis=1), 1.02 * s[300:600].mean(axis=1), rng.normal(size=(400, 3)) * 3 + np.array([1.0, 0, 0])])
    return dict(exe=exe, targets=write("targets.bin", pts, rng.random(len(pts)) < 0.5),
                meshes={"spheres": (write("spheres.bin", two, rng.random(len(two)) < 0.3), 64),
                        "soup": (write("soup.bin", soup, soup_bc), soup_ncrit),
                        "stokes_soup": (write("stokes_soup.bin", ssoup, ssoup_bc), ssoup_ncrit)})


def _run(plans, mesh, **keys):
    path, ncrit = plans["meshes"][mesh]
    r = subprocess.run([plans["exe"], path, str(ncrit)] + ["%s=%s" % kv for kv in keys.items()], capture_output=True, text=True, timeout=120)
    out = {}
    for line in r.stdout.splitlines():
        w = line.split(" ")
        out[w[0]] = dict(zip(w[0::2], w[1::2])) if w[0] == "hybrid" else dict(zip(w[1::2], w[2::2])) if w[0] == "summary" else line
    assert r.returncode == 0 and "FAIL" not in out and "summary" in out, r.stdout[-4000:] + r.stderr[-2000:]
    assert out["summary"]["failures"] == "0"
    return out


CONFIGS = {
    "laplace": dict(),
    "stokes_sym3": dict(kernel=1),
    "stokes_full_rows": dict(kernel=1, sym=0),
    "hybrid_laplace": dict(f=0.5),
    "hybrid_stokes": dict(kernel=1, f=0.5),
    "float_laplace": dict(f32=8),
    "float_stokes": dict(kernel=1, f32=6),
    "matrix_free": dict(sparse=0),
    "matrix_free_stokes": dict(kernel=1, sparse=0),
    "shard_1_of_2_gather": dict(rank=1, world=2, upward=1),
    "shard_1_of_2_selective": dict(rank=1, world=2, upward=2),
    "treecode": dict(tree=1),
}


@pytest.mark.parametrize("mesh", ["spheres", "soup"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_layouts_of_real_plans(plans, mesh, config):
    keys = CONFIGS[config]
    if mesh == "soup" and keys.get("kernel") == 1:
        mesh = "stokes_soup"                            # the Stokes soups of near_form_cases are their own inputs
    out = _run(plans, mesh, **keys)
    assert out["hybrid"]["hybrid"] == ("1" if "f" in keys else "0")
    assert (int(out["hybrid"]["recomputed"]) > 0) == ("f" in keys)
    assert out["summary"]["f32"] == ("1" if "f32" in keys else "0")
    assert out["summary"]["sym"] == ("1" if keys.get("kernel") == 1 and keys.get("sym", 1) and keys.get("sparse", 1) else "0")
    assert ("m2p" in out) == ("tree" in keys)
    if "f" in keys:
        assert int(out["summary"]["rc_items"]) > 0


@pytest.mark.parametrize("mesh", ["spheres", "soup"])
def test_dual_plan_layouts(plans, mesh):
    out = _run(plans, mesh, targets=plans["targets"])
    assert out["l2p"].endswith("scatter 0")             # a dual plan delivers through the scatter kernel


@pytest.mark.parametrize("kernel", [0, 1])
def test_hybrid_choice_is_the_same_on_every_shard(plans, kernel):
    whole = _run(plans, "spheres", kernel=kernel, f=0.5)["hybrid"]
    for rank in (0, 1):
        shard = _run(plans, "spheres", kernel=kernel, f=0.5, rank=rank, world=2, upward=1)["hybrid"]
        assert shard == whole and int(whole["recomputed"]) > 0

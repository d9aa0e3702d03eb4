"""CPU-only: which launches of the 2-D tiles run paired patch columns, and which physical workgroup hosts which two
virtual ones (ec3d_patch_pairs_ok and ec3d_patch_pair_virtual in csrc/ec3d_sweep_lists.hpp).

tests/support/patch_pairs_cases.cpp (a stand-alone program, built with the address and undefined-behaviour sanitizers)
prints the decision and the map for each layout below; both are compared with the rule restated here.

The rule.  A z-marching launch of nblk workgroups on a plane of tpp = sdx * sdy / 512 patches (npx = sdx / 128 per patch
row) deals its columns to eight XCD labels in runs of cpx = tpp / 8: workgroup v has label v % 8, column
(v % 8) * cpx + (v / 8) % cpx and z segment (v / 8) / cpx.  Two columns may share a workgroup when their patches are
y-neighbours (columns npx apart), lie in the same label's run and march the same planes.  So the launch pairs exactly when
tpp % 8 == 0 (no short run), cpx % (2 npx) == 0 (every run is an even number of whole patch rows), nblk is nseg * tpp with
nseg * pps == planes (segments of equal length), and the handle is neither a z-slab nor a rank of a distributed job.
What that says of the layouts the cases name:
  128 x 8  (tpp 2), 256 x 16 (tpp 8), 128 x 12 (tpp 3, odd patch rows): refused -- a label's run holds less than two patch rows
  128 x 64 (tpp 16, cpx 2), 256 x 64 (tpp 32, cpx 4), 512 x 512 (tpp 512, cpx 64): paired
  128 x 72 (tpp 18: not divisible across the eight runs), 128 x 96 (tpp 24, cpx 3: an odd number of patch rows per run): refused"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "patch_pairs_cases.cpp")

# name -> (sdx, sdy, planes, nblk, pps, slab, dist), and whether the rule pairs it
LAYOUTS = {
    "128x8_one_pair_of_columns": ((128, 8, 9, 8, 9, 0, 0), False),
    "256x16": ((256, 16, 9, 8, 9, 0, 0), False),
    "128x12_odd_y_blocks": ((128, 12, 9, 8, 9, 0, 0), False),
    "128x64": ((128, 64, 9, 48, 3, 0, 0), True),
    "128x64_one_segment": ((128, 64, 9, 16, 9, 0, 0), True),
    "128x64_three_segments_of_eight": ((128, 64, 24, 48, 8, 0, 0), True),
    "256x64": ((256, 64, 9, 96, 3, 0, 0), True),
    "512x512_cube": ((512, 512, 512, 1024, 256, 0, 0), True),
    "512x512_three_rounds": ((512, 512, 512, 4096, 64, 0, 0), True),
    "128x72_columns_not_divisible_by_8": ((128, 72, 9, 24, 9, 0, 0), False),
    "128x96_odd_rows_per_run": ((128, 96, 9, 24, 9, 0, 0), False),
    "128x64_unequal_segments": ((128, 64, 9, 64, 3, 0, 0), False),       # four segments of three planes: the last is empty
    "128x64_short_last_segment": ((128, 64, 10, 48, 4, 0, 0), False),    # 4 + 4 + 2 planes
    "128x64_slab": ((128, 64, 9, 48, 3, 1, 0), False),
    "128x64_dist": ((128, 64, 9, 48, 3, 0, 1), False),
}


def rule(sdx, sdy, planes, nblk, pps, slab, dist):
    tpp, npx = sdx * sdy // 512, sdx // 128
    if slab or dist or tpp % 8:
        return False
    cpx = tpp // 8
    return cpx % (2 * npx) == 0 and nblk % tpp == 0 and (nblk // tpp) * pps == planes


def place(v, tpp, npx):
    """(XCD label, z segment, patch column, patch row) of workgroup v of the unpaired launch."""
    cpx = tpp // 8
    col = (v % 8) * cpx + (v // 8) % cpx
    return v % 8, (v // 8) // cpx, col % npx, col // npx


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("patch_pairs") / "patch_pairs_cases")
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    args = [":".join(map(str, lay)) for lay, _ in LAYOUTS.values()]
    out = subprocess.run([exe, *args], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr   # a sanitizer report
    found, cur = {}, None
    for line in out.stdout.splitlines():
        key, *rest = line.split(" ")
        if key == "layout":
            given, got = line[len("layout "):].split(" | ")
            cur = found.setdefault(tuple(int(v) for v in given.split()), {"got": tuple(int(v) for v in got.split()), "wg": {}})
        else:
            phys, v0, v1 = (int(v) for v in rest)
            assert phys not in cur["wg"]
            cur["wg"][phys] = (v0, v1)
    return found


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_the_decision_follows_the_rule(cases, name):
    lay, stated = LAYOUTS[name]
    ok, tpp, npx = cases[lay]["got"]
    assert (tpp, npx) == (lay[0] * lay[1] // 512, lay[0] // 128)
    assert bool(ok) == rule(*lay) == stated
    assert (len(cases[lay]["wg"]) == lay[3] // 2) if stated else not cases[lay]["wg"]


@pytest.mark.parametrize("name", sorted(k for k, (_, paired) in LAYOUTS.items() if paired))
def test_every_virtual_workgroup_is_hosted_once_beside_its_y_neighbour(cases, name):
    lay, _ = LAYOUTS[name]
    sdx, sdy, planes, nblk, pps, _, _ = lay
    tpp, npx = sdx * sdy // 512, sdx // 128
    wg = cases[lay]["wg"]
    assert sorted(wg) == list(range(nblk // 2))
    hosted = [v for phys in sorted(wg) for v in wg[phys]]
    assert sorted(hosted) == list(range(nblk))                      # the launch's nblk workgroups, each exactly once
    for phys, (v0, v1) in wg.items():
        x0, s0, px0, py0 = place(v0, tpp, npx)
        x1, s1, px1, py1 = place(v1, tpp, npx)
        assert x0 == x1 == phys % 8                                 # the label the hardware gives the physical workgroup
        assert s0 == s1 and px0 == px1 and py1 == py0 + 1 and py0 % 2 == 0
    # dispatch order within a label: as the lower halves follow each other among the unpaired workgroups
    for x in range(8):
        lower = [wg[p][0] for p in sorted(wg) if p % 8 == x]
        assert lower == sorted(lower)

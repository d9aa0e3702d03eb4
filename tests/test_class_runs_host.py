"""CPU-only: the "same classes as the tile below" flags of the dictionary form (ec3d_class_runs and
ec3d_class_runs_shape in csrc/ec3d_sweep_lists.hpp).

tests/support/class_runs_cases.cpp (a stand-alone program, built with the address and undefined-behaviour sanitizers)
prints, for each case, the class array it gave the rule and the flags that came back.  Every flag array is compared
exactly with a numpy restatement of the rule as the kernels rely on it: flag[plane k][patch q] = 1 exactly when k > 0 and
all class bytes of the patch on plane k equal those one plane below, padded rows included; behind the flags a plane of
zeros and four more (the kernels read the flag of the tile above, by dwords)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "class_runs_cases.cpp")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("class_runs") / "class_runs_cases")
    subprocess.run([cc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr   # a sanitizer report
    found, cur = {}, None
    for line in out.stdout.splitlines():
        key, *rest = line.split(" ")
        if key == "case":
            cur = found.setdefault(rest[0], {}).setdefault(rest[1], {})
        else:
            assert key not in cur, line
            cur[key] = [int(v) for v in rest]
    return found


from class_runs_numpy import class_runs   # the rule: [plane][patch row][row in patch][patch column][cell in patch row]


def test_flags_equal_the_rule(cases):
    seen = set()
    for name, c in cases["runs"].items():
        sdx, sdy, pad, planes, px, py = c["in"]
        kdz = sdx * pad
        assert len(c["cls"]) == kdz * planes and pad > sdy and pad % py == 0 and sdx % px == 0, name
        want = class_runs(c["cls"], planes, kdz, sdx, px, py)
        assert np.array_equal(np.array(c["flag"], np.uint8), want), name
        tpp = kdz // (px * py)
        assert not any(c["flag"][:tpp]) and not any(c["flag"][planes * tpp:]), name   # plane 0 and the trailing zeros
        seen.add(name.rsplit("_", 1)[0])
    assert seen == {"all_equal", "all_different", "one_cell", "patch_corners", "padded_row", "last_plane", "single_plane",
                    "two_planes_equal", "two_planes_different"}


@pytest.mark.parametrize("shape", ["8x2", "128x4"])
def test_flags_of_the_stated_cases(cases, shape):
    """Independent of the restatement: where the flags of each case must be 0."""
    runs = cases["runs"]

    def zeros(name):
        c = runs[f"{name}_{shape}"]
        sdx, sdy, pad, planes, px, py = c["in"]
        tpp = sdx * pad // (px * py)
        return planes, tpp, sdx // px, {(t // tpp, t % tpp) for t in range(tpp, planes * tpp) if not c["flag"][t]}

    planes, tpp, npx, z = zeros("all_equal")
    assert planes == 5 and tpp >= 4 and z == set()                                  # every tile above plane 0 repeats
    planes, tpp, npx, z = zeros("all_different")
    assert z == {(k, q) for k in range(1, planes) for q in range(tpp)}
    planes, tpp, npx, z = zeros("one_cell")
    assert z == {(2, npx + 1), (3, npx + 1)}                                        # the change, and the change back
    planes, tpp, npx, z = zeros("patch_corners")
    assert z == {(1, 0), (2, 0), (4, npx + 1), (5, npx + 1)}
    planes, tpp, npx, z = zeros("padded_row")
    assert z == {(3, tpp - npx)} and planes == 4                                    # first patch of the last patch row
    planes, tpp, npx, z = zeros("last_plane")
    assert z == {(3, 0)} and planes == 4
    planes, tpp, npx, z = zeros("single_plane")
    assert planes == 1 and z == set() and len(runs[f"single_plane_{shape}"]["flag"]) == 2 * tpp + 4
    assert not any(runs[f"single_plane_{shape}"]["flag"])
    planes, tpp, npx, z = zeros("two_planes_equal")
    assert planes == 2 and z == set() and runs[f"two_planes_equal_{shape}"]["flag"][tpp:2 * tpp] == [1] * tpp
    planes, tpp, npx, z = zeros("two_planes_different")
    assert planes == 2 and z == {(1, q) for q in range(tpp)}


def test_shape_rule(cases):
    got = {name: c for name, c in cases["shape"].items()}
    for name, c in got.items():
        off, (n, px, py), (ok, planes, tpp) = c["off"], c["in"], c["out"]
        want = False
        if len(off) == 7:
            sdx, kdz = off[5], off[6]
            want = sdx > 0 and kdz > 0 and sdx % px == 0 and kdz % sdx == 0 and (kdz // sdx) % py == 0 and n > 0 and n % kdz == 0
        assert bool(ok) == want, name
        assert (planes, tpp) == ((n // off[6], off[6] // (px * py)) if want else (0, 0)), name
    assert {n for n, c in got.items() if c["out"][0]} == {"cube", "one_plane"}
    assert got["cube"]["out"] == [1, 9, 4] and got["one_plane"]["out"] == [1, 1, 1]


def test_generated_operators_change_classes_where_stated():
    """The operators tests/test_gpu_class_runs.py brings as CSR (tests/class_runs_numpy.py): their classes -- the distinct
    coefficient rows, as the dictionary form finds them -- change along z exactly at the stated tiles, and stay within the
    dictionary's 256 classes."""
    import class_runs_numpy as R
    sdx, sdy, sdz = R.DIMS
    kdz, tpp = sdx * sdy, sdx * sdy // 512
    want_planes = {"layers_1_2_3": {1, 2, 4, 7, 8}, "consecutive": {1, 3, 4, 8}, "inclusion": {1, 8},
                   "segment_edges": {1, 3, 5, 8}, "last_plane": {1, 8}}
    assert set(want_planes) == set(R.OPERATORS)
    for name in R.OPERATORS:
        valA, irow, jcol, c = R.operator(name)
        ids = R.classes_of_bands(c)
        assert ids.max() < 256, name
        flag = R.class_runs(ids, sdz, kdz, sdx)
        zeros = R.zero_tiles(flag, sdz, tpp)
        assert zeros == R.changed_tiles(name), name
        whole = {k for k in range(1, sdz) if all((k, q) in zeros for q in range(tpp))}
        assert whole == want_planes[name], name
        assert len(irow) == sdx * sdy * sdz + 1 and np.all(np.diff(irow) <= 7), name
    # the inclusion: exactly one tile of plane 4 (and of plane 5, where the classes change back) differs
    zeros = R.zero_tiles(R.class_runs(R.classes_of_bands(R.operator("inclusion")[3]), sdz, kdz, sdx), sdz, tpp)
    assert {t for t in zeros if t[0] in (4, 5)} == {(4, 3), (5, 3)}
    # layers of one, two and three planes between two changes
    ch = sorted(want_planes["layers_1_2_3"])
    assert {b - a for a, b in zip(ch, ch[1:])} == {1, 2, 3}

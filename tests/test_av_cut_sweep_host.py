"""The cut-sweep family (tests/av_cut_sweep.py) is what tests/test_gpu_av_cut_sweep.py needs it to be: every member
is a system the reference assembles (oracle.gen_sparse_matrix, src/EC3D.f90:465-1049) and the structured form holds,
and over the (member, world) pairs every situation of a z-slab cut against a conductor face occurs at least once with
the face below the cut and once with it above.  The situations are read off slab_bounds and the per-plane counts of
conducting cells (av_cut_sweep.situations): conditions on the inputs -- if one fails, the family is wrong."""
import numpy as np
import pytest

import av_cut_sweep as CS
import av_generate as AG
import multidomain_numpy as MD


def test_members_are_the_table():
    assert len(CS.THIN_PLATE) == 12 and len(CS.THICK_PLATE) == 8 and len(CS.THIN_SLABS) == 4 + 3
    assert sum(1 for k in CS.THIN_PLATE if k[3] == "z") == 6
    assert len(CS.PAIRS) == 3 * 20 + 7
    for (sdz, z0, t, hole), worlds in CS.MEMBERS.items():
        geo, geoC, valPHYS, BND, delta, dt = CS.member(sdz, z0, t, hole)
        assert geo.shape == (sdz, CS.SDY, CS.SDX)
        per = CS.per_plane(geoC)
        cells = 8 * 7 - (1 if hole else 0)
        assert np.array_equal(per, [cells if z0 <= k < z0 + t else 0 for k in range(sdz)])
        assert all(sdz // w >= 2 for w in worlds)
        if sdz == 8:
            assert all(CS.slab_bounds(sdz, r, 4)[1] - CS.slab_bounds(sdz, r, 4)[0] == 2 for r in range(4))


def test_slab_bounds_is_the_packages():
    from eddy_currents_3d_amd.dist import slab_bounds
    for sdz in (8, 14, 16, 17):
        for world in (1, 2, 3, 4, 5):
            assert all(CS.slab_bounds(sdz, r, world) == slab_bounds(sdz, r, world) for r in range(world))
    assert CS.cuts(16, 2) == [8] and CS.cuts(16, 3) == [6, 11] and CS.cuts(16, 4) == [4, 8, 12]


@pytest.mark.parametrize("key", list(CS.MEMBERS), ids=CS.key_id)
def test_oracle_accepts_every_member(oracle, key):
    args = CS.member(*key)
    m = oracle.gen_sparse_matrix(*args)
    assert m["n"] == 3 * args[0].size + int(CS.per_plane(args[1]).sum())
    assert MD.structured_applies(args[0], args[1])
    assert len(MD.conductors(args[0], args[1])) == 1


def test_the_hole_gives_every_u_row_branch():
    for key in CS.THIN_PLATE:
        assert AG.u_row_patterns(CS.member(*key)[1]) == set(range(27)), key     # (a plate of 8 x 7 x 3 has them already)


def test_world_two_meets_every_position_from_four_under_to_four_over():
    assert sorted(8 - z0 for _, z0, _, _ in CS.THIN_PLATE) == list(range(-4, 8))


def test_every_situation_occurs_from_below_and_from_above():
    seen = {}
    for key, world in CS.PAIRS:
        per = CS.per_plane(CS.member(*key)[1])
        for s in CS.situations(per, key[0], world):
            seen.setdefault(s, []).append((key, world))
    for s in CS.SITUATIONS:
        print(f"{s}: {len(seen.get(s, []))} pairs")
    assert len(CS.SITUATIONS) == 16
    assert [s for s in CS.SITUATIONS if s not in seen] == []
    assert set(seen) <= set(CS.SITUATIONS)
    # the members the GPU test solves against the twin hold the two "one plane inside" cuts themselves
    thin2 = set().union(*(CS.situations(CS.per_plane(CS.member(*k)[1]), 16, 2) for k in CS.THIN_PLATE))
    assert {"cut one plane inside a face below", "cut one plane inside a face above"} <= thin2
    thin4 = set().union(*(CS.situations(CS.per_plane(CS.member(*k)[1]), 8, 4) for k in CS.THIN_SLABS))
    assert {"two-plane rank, both planes travel below", "two-plane rank, both planes travel above",
            "rank owned entirely by conductor below", "rank owned entirely by conductor above"} <= thin4


@pytest.mark.parametrize("zi", CS.TWO_DOMAIN)
def test_oracle_accepts_the_two_domain_plate(oracle, zi):
    args = CS.two_domain(zi)
    oracle.gen_sparse_matrix(*args)
    assert MD.structured_applies(args[0], args[1])
    assert [len(c) for _, c in MD.conductors(args[0], args[1])] == [3 * 56, 3 * 56]
    assert sorted(zi - 8 for zi in CS.TWO_DOMAIN) == [-1, 0, 1]

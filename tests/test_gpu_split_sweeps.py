"""The launch pairs of a z-slab on real handles: the two launches of every split kernel visit what the whole kernel visits.

csrc/ec3d_split_sweeps.hpp derives, per slab, K1 / K3 (ec3d_get_visit_order 3 / 4), K2 / K5 (5 / 6) and the 2-D-tile
kernels of the three-launch iteration (7 / 8) as an interior and a boundary launch; tests/test_split_sweeps_host.py pins
the arithmetic on sweeps made by hand.  Here the sweeps are the library's own, on 2-rank jobs on one card: the
single-component operator on 2-D tiles with 12 owned planes per rank, and one structured A-V plate on pitched planes with 8.
EC3D_SLAB_PLAN=5 is the plan that asks a slab for the K2 / K5 split as well.  A pair that comes back unsplit fails."""
import numpy as np
import pytest

import av_cut_sweep as CS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import eddy_currents_3d_amd as E
    E.load_library()
    return E


def tiles_of(view, *which):
    return np.sort(np.concatenate([view.visit_order(w)[1] for w in which]))


def assert_split(view, pair, whole, what):
    a, b = (view.visit_order(w)[1] for w in pair)
    want = tiles_of(view, whole)
    assert len(a) > 0 and len(b) > 0 and len(a) + len(b) == len(want), (what, pair, "came back unsplit")
    assert np.array_equal(tiles_of(view, *pair), want), (what, pair)


@pytest.mark.parametrize("shape", [(128, 8, 24), (256, 16, 24)], ids=lambda s: "x".join(map(str, s)))
def test_poisson_slabs_on_2d_tiles_split_every_kernel(E, monkeypatch, shape):
    monkeypatch.setenv("EC3D_SLAB_PLAN", "5")
    with E.EC3DMulti(2, devices=[0, 0]) as m:
        m.assemble_poisson(*shape)
        for r in range(2):
            view, k0, k1 = m.slab(r)
            assert k1 - k0 == 12 and view.geometry(1).patch_x > 0 and view.can_overlap()
            assert len(np.unique(tiles_of(view, 1))) == len(tiles_of(view, 1))
            assert_split(view, (3, 4), 1, (shape, r))
            assert_split(view, (7, 8), 1, (shape, r))
            assert_split(view, (5, 6), 2, (shape, r))


def test_structured_plate_on_pitched_planes_splits_k13_and_k25(E, monkeypatch):
    monkeypatch.setenv("EC3D_SLAB_PLAN", "5")
    monkeypatch.setenv("EC3D_PITCH", "2")
    with E.EC3DMulti(2, devices=[0, 0], structured=True) as m:
        m.assemble(*CS.member(16, 6, 3))                  # the plate in planes 6 .. 8: the cut (plane 8) one plane inside its upper face
        assert m.plan()[0] == 5
        for r in range(2):
            view, k0, k1 = m.slab(r)
            assert k1 - k0 == 8 and view.can_overlap()
            assert len(np.unique(tiles_of(view, 1))) == len(tiles_of(view, 1))
            assert_split(view, (3, 4), 1, r)
            assert_split(view, (5, 6), 2, r)
            # no 2-D tiles, no three-launch iteration: 7 / 8 are both the unsplit SpMV launch
            for w in (7, 8):
                assert all(np.array_equal(x, y) for x, y in zip(view.visit_order(w), view.visit_order(1)))

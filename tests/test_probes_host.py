"""Probes without a GPU: the numpy twin of ec3d_probe_sample against the float32 field twin, the line and box helpers of
eddy_currents_3d_amd/probes.py, the CSV form and the command line's refusals."""
import numpy as np
import pytest

import fields_numpy as F
import probes_numpy as PN
from conftest import load_golden
from eddy_currents_3d_amd import probes as P
from eddy_currents_3d_amd import run

G2 = "g2_conducting_hole_16x15x14"


# ------------------------------------------------------------------------------------------------------------ the twin
def assert_rounds_to_the_fields(geoC, delta, x, b):
    got = PN.whole_box(geoC, delta, x, b)
    want = F.fields(geoC, delta, x, b)
    assert got.shape == (geoC.size, 13) and got.dtype == np.float64
    for key, at in (("A", 0), ("eddy", 3), ("source", 6), ("B", 9)):
        assert got[:, at:at + 3].astype(np.float32).tobytes() == want[key].tobytes(), key
    uid = np.asarray(geoC).reshape(-1)
    assert np.array_equal(got[uid != 0, 12], np.asarray(x)[uid[uid != 0] - 1]) and not got[uid == 0, 12].any()
    cells = np.array([5, 0, geoC.size - 1, 5, 1234])
    assert PN.sample(geoC, delta, x, b, cells).tobytes() == got[cells].tobytes()


def test_twin_rounded_to_float32_is_the_field_twin_on_the_captured_step():
    g = load_golden(G2)
    assert np.count_nonzero(g["geoPHYS_C"]) and g["xout0"].any()
    assert_rounds_to_the_fields(g["geoPHYS_C"], g["delta"], g["xout0"], g["b0"])


def test_twin_rounded_to_float32_is_the_field_twin_on_random_vectors():
    g = load_golden(G2)
    n = 3 * g["geoPHYS_C"].size + int(np.count_nonzero(g["geoPHYS_C"]))
    rng = np.random.Generator(np.random.PCG64(77))
    assert_rounds_to_the_fields(g["geoPHYS_C"], g["delta"], rng.standard_normal(n), rng.standard_normal(n))


# ---------------------------------------------------------------------------------------------------------- probe_line
def stated_rule(c0, c1, dims):
    d = [b - a for a, b in zip(c0, c1)]
    n = max(abs(v) for v in d)
    out = []
    for t in range(n + 1):
        i, j, k = (a + ((2 * t * v + n) // (2 * n) if n else 0) for a, v in zip(c0, d))
        out.append(i + j * dims[0] + k * dims[0] * dims[1])
    return out


def test_an_axis_aligned_line_is_consecutive_cells():
    dims = (9, 7, 5)
    assert P.probe_line((2, 3, 1), (7, 3, 1), dims).tolist() == [2 + 3 * 9 + 63 + t for t in range(6)]
    assert P.probe_line((4, 0, 2), (4, 6, 2), dims).tolist() == [4 + 9 * t + 126 for t in range(7)]
    assert P.probe_line((4, 5, 0), (4, 5, 4), dims).tolist() == [4 + 45 + 63 * t for t in range(5)]
    assert P.probe_line((3, 3, 3), (3, 3, 3), dims).tolist() == [3 + 27 + 189]
    assert P.probe_line((2, 3, 1), (7, 3, 1), dims).dtype == np.int64


def test_a_space_diagonal_equals_the_list_written_out():
    # n = 4: j = (2*t*3 + 4) // 8 -> 0 1 2 2 3, k = (2*t*2 + 4) // 8 -> 0 1 1 2 2
    ijk = [(0, 0, 0), (1, 1, 1), (2, 2, 1), (3, 2, 2), (4, 3, 2)]
    got = P.probe_line((0, 0, 0), (4, 3, 2), (5, 4, 3))
    assert got.tolist() == [i + 5 * j + 20 * k for i, j, k in ijk]
    assert P.cells_to_ijk(got, (5, 4, 3)).tolist() == [list(c) for c in ijk]


def test_a_line_running_backwards_follows_the_stated_rule():
    dims = (11, 9, 7)
    for c0, c1 in (((10, 8, 6), (0, 0, 0)), ((9, 2, 5), (1, 7, 4)), ((3, 8, 0), (5, 1, 6)), ((0, 4, 6), (10, 4, 0))):
        got = P.probe_line(c0, c1, dims).tolist()
        n = max(abs(a - b) for a, b in zip(c0, c1))
        assert got == stated_rule(c0, c1, dims)
        assert len(got) == n + 1 == len(set(got))
        ijk = P.cells_to_ijk(got, dims)
        assert tuple(ijk[0]) == c0 and tuple(ijk[-1]) == c1
    # floor division, not truncation: di = -3 over n = 4 gives 0 -1 -1 -2 -3 (halves upwards)
    assert P.cells_to_ijk(P.probe_line((3, 4, 0), (0, 0, 0), dims), dims)[:, 0].tolist() == [3, 2, 2, 1, 0]


@pytest.mark.parametrize("c0,c1", [((0, 0, 0), (5, 0, 0)), ((0, -1, 0), (1, 1, 1)), ((0, 0, 0), (0, 0, 3)), ((0, 4, 0), (0, 0, 0))])
def test_a_line_outside_the_box_raises(c0, c1):
    with pytest.raises(ValueError, match="outside"):
        P.probe_line(c0, c1, (5, 4, 3))


# ----------------------------------------------------------------------------------------------------------- probe_box
def test_a_box_is_in_scan_order():
    dims = (6, 5, 4)
    got = P.probe_box((1, 2, 1), (3, 3, 2), dims)
    want = [i + 6 * j + 30 * k for k in (1, 2) for j in (2, 3) for i in (1, 2, 3)]
    assert got.tolist() == want and got.dtype == np.int64
    assert P.probe_box((3, 3, 2), (1, 2, 1), dims).tolist() == want
    assert P.probe_box((0, 0, 0), (5, 4, 3), dims).tolist() == list(range(120))
    assert P.probe_box((0, 0, 2), (5, 4, 2), dims).tolist() == list(range(60, 90))      # a plane


def test_a_one_cell_box_and_a_box_outside():
    assert P.probe_box((5, 4, 3), (5, 4, 3), (6, 5, 4)).tolist() == [119]
    with pytest.raises(ValueError, match="outside"):
        P.probe_box((0, 0, 0), (6, 4, 3), (6, 5, 4))
    with pytest.raises(ValueError, match="outside"):
        P.cells_to_ijk([120], (6, 5, 4))


# ------------------------------------------------------------------------------------------------------------------ CSV
def test_csv_rows_round_trip_exactly(tmp_path):
    dims = (6, 5, 4)
    cells = np.array([7, 119, 7, 0])
    rng = np.random.Generator(np.random.PCG64(5))
    steps = [rng.standard_normal((4, 13)) * 10.0 ** rng.integers(-300, 300, (4, 13)) for _ in range(3)]
    steps[1][2, 5], steps[1][0, 0], steps[2][3, 12] = np.nan, -0.0, 5e-324
    T = [0.0, 0.1 + 0.2, 1e-3 * 7]
    path = tmp_path / "p.csv"
    with open(path, "w") as f:
        f.write(P.CSV_HEADER + "\n")
        for k, v in enumerate(steps):
            rows = P.csv_rows(k, T[k], cells, dims, v)
            assert len(rows) == 4 and all(len(r.split(",")) == 19 for r in rows)
            f.writelines(r + "\n" for r in rows)
    assert P.CSV_HEADER == "step,T,probe,i,j,k,ax,ay,az,eddy_x,eddy_y,eddy_z,source_x,source_y,source_z,bx,by,bz,u"
    back = P.read_csv(str(path))
    assert back["values"].tobytes() == np.concatenate(steps).tobytes()
    assert back["T"].tobytes() == np.repeat(np.array(T), 4).tobytes()
    assert back["step"].tolist() == [0] * 4 + [1] * 4 + [2] * 4 and back["probe"].tolist() == [0, 1, 2, 3] * 3
    assert back["ijk"][:4].tolist() == P.cells_to_ijk(cells, dims).tolist()


def test_stack_puts_the_arrays_in_component_order():
    v = np.arange(2 * 3 * 13, dtype=np.float64).reshape(2, 3, 13)
    d = dict(a=v[..., 0:3], eddy=v[..., 3:6], source=v[..., 6:9], b=v[..., 9:12], u=v[..., 12])
    assert np.array_equal(P.stack(d), v)
    assert np.array_equal(P.stack({k: a[0] for k, a in d.items()}), v[0])


# ------------------------------------------------------------------------------------------------------------ arguments
def test_the_parser_takes_repeated_probe_options():
    a = run.build_parser().parse_args(["m.vxc", "--probes", "p.csv", "--probe", "1,2,2", "--probe", "0,0,0", "--probe-line",
                                       "0,0,0:4,3,2", "--probe-line", "4,0,0:0,0,0", "--probe-box", "1,1,1:2,2,1"])
    assert a.probes == "p.csv" and a.probe == ["1,2,2", "0,0,0"] and len(a.probe_line) == 2 and len(a.probe_box) == 1
    cells = P.cells_from_options(a.probe, a.probe_line, a.probe_box, (5, 4, 3))
    want = [1 + 10 + 40, 0] + P.probe_line((0, 0, 0), (4, 3, 2), (5, 4, 3)).tolist() + [4, 3, 2, 1, 0] \
        + P.probe_box((1, 1, 1), (2, 2, 1), (5, 4, 3)).tolist()
    assert cells.tolist() == want
    run.check_probe_options(run.build_parser(), a, 1)             # accepted
    none = run.build_parser().parse_args(["m.vxc"])
    assert none.probes is None and none.probe == [] and none.probe_line == [] and none.probe_box == []
    run.check_probe_options(run.build_parser(), none, 4)          # nothing asked for: several ranks are fine
    for bad in ("1,2", "1,2,3,4", "a,b,c", "1,2,3:4,5,6"):
        with pytest.raises(ValueError):
            P.parse_point(bad)
    for bad in ("1,2,3", "1,2,3:4,5", "1,2,3:4,5,6:7,8,9"):
        with pytest.raises(ValueError):
            P.parse_span(bad)


@pytest.mark.parametrize("argv,world,text", [
    (["m.vxc", "--probes", "p.csv"], "1", "needs at least one"),
    (["m.vxc", "--probes", "p.csv", "--probe", "1,1,1"], "2", "one GPU only"),
    (["m.vxc", "--probe-line", "0,0,0:1,1,1"], "1", "need --probes"),
])
def test_main_refuses_before_reading_the_model(monkeypatch, capsys, argv, world, text):
    monkeypatch.setenv("WORLD_SIZE", world)
    with pytest.raises(SystemExit) as e:
        run.main(argv)                                            # m.vxc does not exist: refused before it is opened
    assert e.value.code == 2 and text in capsys.readouterr().err

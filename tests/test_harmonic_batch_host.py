"""host.run_harmonic_sweep and --harmonic F0 --sweep without a GPU: what the sweep asks of an
EC3DSolver, recorded by a stand-in -- the grouping of the frequencies into batches, one b^ built at the drive frequency
and uploaded to every system beside x^ = 0, select before every harmonic_load -- and everything it refuses before it
assembles; the parser's refusals of --sweep."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from eddy_currents_3d_amd import host, run, vxc


class Recorder:
    """Stands in for an EC3DSolver: records (name, arguments) of every call and answers what the sweep reads."""

    def __init__(self, n):
        self.calls, self.n, self.nsys, self.selected = [], n, 0, None

    def _note(self, name, *a):
        self.calls.append((name,) + a)

    def assemble(self, *a):
        self._note("assemble")

    def harmonic_batch_setup(self, omegas):
        self.nsys = len(omegas)
        self._note("batch_setup", tuple(float(w) for w in omegas))

    def harmonic_batch_upload(self, sys, which, z):
        assert 0 <= sys < self.nsys
        self._note("batch_upload", sys, which, np.array(z, np.complex128))

    def harmonic_batch_solve(self, tol, itmax):
        self._note("batch_solve", tol, itmax)
        return [(3 + s, 1e-4) for s in range(self.nsys)]

    def harmonic_batch_info(self, sys):
        return dict(ready=True, omega=0.0, iter=3 + sys, restarts=0, stop_kind=2, relres=1e-4, ms=1.0, device_bytes=0)

    def harmonic_batch_select(self, sys):
        assert 0 <= sys < self.nsys
        self.selected = sys
        self._note("select", sys)

    def harmonic_true_residual(self):
        assert self.selected is not None
        return 2e-4, 1.0

    def harmonic_download(self, which):
        return np.zeros(self.n, np.complex128)

    def harmonic_load(self, part):
        self._note("load", part, self.selected)

    def domain_integrals(self, delta):
        return [dict(domain=2, cells=10, sigma=1.0, joule_w=1.0 + self.selected, force_n=np.ones(3))]


@pytest.fixture(scope="module")
def elmer():
    model = vxc.read_vxc(os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc"))
    t = vxc.domain_tables(model)
    return model, t, 3 * model.vox.size + t["ncells0"]


def test_grouping_one_rhs_and_the_order_of_calls(elmer):
    model, t, n = elmer
    freqs = [10.0, 20.0, 40.0, 80.0, 160.0]
    rec = Recorder(n)
    rs = host.run_harmonic_sweep(model, rec, 50.0, freqs, batch=2, integrals=True)
    assert [r["freq"] for r in rs] == freqs and [r["omega"] for r in rs] == [2.0 * np.pi * f for f in freqs]
    names = [c[0] for c in rec.calls]
    assert names[0] == "assemble" and names.count("assemble") == 1
    setups = [c[1] for c in rec.calls if c[0] == "batch_setup" and c[1]]
    assert [len(w) for w in setups] == [2, 2, 1]
    assert [w for g in setups for w in g] == [2.0 * np.pi * f for f in freqs]
    assert [c[1:] for c in rec.calls if c[0] == "batch_solve"] == [(float(t["tol"]), int(t["itmax"]))] * 3
    # one b^: the phasors at the DRIVE frequency, the same bits in every system of every batch; x^ = 0 beside it
    b = host.harmonic_rhs(host.SourceProgram(model, t), 50.0, n)
    ups = [c for c in rec.calls if c[0] == "batch_upload"]
    assert [(c[1], c[2]) for c in ups] == [(s, w) for size in (2, 2, 1) for s in range(size) for w in ("B", "X")]
    for c in ups:
        want = b if c[2] == "B" else np.zeros(n)
        assert np.array_equal(c[3].view(np.float64).view(np.uint64), np.asarray(want, np.complex128).view(np.float64).view(np.uint64))
    assert all(r["b"] is rs[0]["b"] for r in rs) and np.array_equal(rs[0]["b"], b)
    # within a batch: uploads, the solve, then per system select before its two loads
    i = 0
    for size in (2, 2, 1):
        assert names[i + 1] == "batch_setup"
        body = names[i + 2:i + 2 + 2 * size + 1 + 3 * size]
        assert body == ["batch_upload"] * (2 * size) + ["batch_solve"] + ["select", "load", "load"] * size
        i += 1 + len(body)
    loads = [c for c in rec.calls if c[0] == "load"]
    assert [(c[1], c[2]) for c in loads] == [(p, s) for size in (2, 2, 1) for s in range(size) for p in (0, 1)]
    assert [r["iter"] for r in rs] == [3, 4, 3, 4, 3]
    assert [r["integrals"][0]["joule_w"] for r in rs] == [1.0, 2.0, 1.0, 2.0, 1.0]
    assert set(rs[0]) >= {"freq", "omega", "iter", "relres", "true_residual", "bnorm", "x", "b", "parts", "info", "integrals"}


def test_refusals_before_anything_is_assembled(elmer):
    model, t, n = elmer
    moving = vxc.read_vxc(os.path.join(GOLDEN, "g4_LIM.vxc"))
    rec = Recorder(3 * moving.vox.size + vxc.domain_tables(moving)["ncells0"])
    with pytest.raises(ValueError, match="move"):
        host.run_harmonic_sweep(moving, rec, 50.0, [25.0, 50.0])
    assert rec.calls == []
    rec = Recorder(n)
    for freqs in ([], [50.0, 0.0], [-1.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="frequency"):
            host.run_harmonic_sweep(model, rec, 50.0, freqs)
    for batch in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="batch"):
            host.run_harmonic_sweep(model, rec, 50.0, [50.0], batch=batch)
    with pytest.raises(ValueError, match="EC3DSolver"):
        host.run_harmonic_sweep(model, object(), 50.0, [50.0])
    assert rec.calls == []


@pytest.mark.parametrize("argv", [["--sweep", "25,50"],
                                  ["--harmonic", "50", "--sweep", "25,50", "--null-projection"],
                                  ["--harmonic", "50", "--sweep", ""],
                                  ["--harmonic", "50", "--sweep", ","],
                                  ["--harmonic", "50", "--sweep", "0"],
                                  ["--harmonic", "50", "--sweep", "25,-5"],
                                  ["--harmonic", "50", "--sweep", "25,x"],
                                  ["--harmonic", "50", "--sweep", "25", "--sweep-batch", "17"],
                                  ["--harmonic", "50", "--sweep", "25", "--sweep-batch", "0"]],
                         ids=["no-harmonic", "null-projection", "empty", "only-commas", "zero", "negative", "no-number",
                              "batch-17", "batch-0"])
def test_the_parsers_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        run.main([os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc")] + argv)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_sweep_options_accepted():
    ap = run.build_parser()
    a = ap.parse_args(["m.vxc", "--harmonic", "50", "--sweep", "10, 100,1e3", "--sweep-batch", "4"])
    assert run.check_sweep_options(ap, a) == [10.0, 100.0, 1000.0] and a.sweep_batch == 4
    assert run.check_sweep_options(ap, ap.parse_args(["m.vxc", "--harmonic", "50"])) is None

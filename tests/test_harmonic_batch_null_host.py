"""host.run_harmonic_sweep(..., null_projection=True) and --sweep-null-projection without a GPU:
what the sweep asks of an EC3DSolver with the option on, recorded by a stand-in -- the setting read once behind the
first batch set-up, switched on in every batch before its uploads, the projected residuals read behind the solve, the
report per system before its select -- that the setting is put back as it was found, also when a solve raises; and the
parser's new refusals and acceptances."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from eddy_currents_3d_amd import host, run, vxc
from test_harmonic_batch_host import Recorder


class NullRecorder(Recorder):
    """The Recorder of tests/test_harmonic_batch_host.py with the batch's null-projection setting."""

    def __init__(self, n, on=False, null_tol=1e-10, fail_at_solve=None, fail_at_set=None):
        super().__init__(n)
        self.on, self.null_tol, self.fail_at_solve, self.solves = on, null_tol, fail_at_solve, 0
        self.fail_at_set, self.sets = fail_at_set, 0

    def harmonic_batch_set_null_projection(self, on=True, null_tol=1e-10):
        self.sets += 1
        if self.fail_at_set == self.sets:
            self._note("set_null_refused", bool(on), float(null_tol))
            raise ValueError("call ec3d_harmonic_batch_setup first")
        assert self.nsys > 0 or not on, "switching on needs a batch"
        self.on, self.null_tol = bool(on), float(null_tol)
        self._note("set_null", bool(on), float(null_tol))

    def harmonic_batch_null_projection(self, sys):
        assert 0 <= sys < self.nsys
        self._note("get_null", sys)
        return dict(on=self.on, built=False, found=1, kept=1, dropped=0, null_tol=self.null_tol, removed=1e-4, setup_ms=1.0,
                    components=[dict(seed_row=7, iterations=100 + sys, residual=1e-9, kept=True, restarts=0)], shares_with=sys)

    def harmonic_batch_solve(self, tol, itmax):
        self.solves += 1
        if self.fail_at_solve == self.solves:
            self._note("batch_solve", tol, itmax)
            raise RuntimeError("the set-up missed null_tol")
        return super().harmonic_batch_solve(tol, itmax)

    def harmonic_batch_projected_residual(self):
        self._note("projected")
        return [(1e-7 * (s + 1), 2e-4) for s in range(self.nsys)]


@pytest.fixture(scope="module")
def elmer():
    model = vxc.read_vxc(os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc"))
    t = vxc.domain_tables(model)
    return model, t, 3 * model.vox.size + t["ncells0"]


def test_the_calls_with_the_option_on(elmer):
    model, t, n = elmer
    freqs = [10.0, 20.0, 40.0]
    rec = NullRecorder(n)
    rs = host.run_harmonic_sweep(model, rec, 50.0, freqs, batch=2, tol=1e-6, null_projection=True, null_tol=1e-9)
    names = [c[0] for c in rec.calls]
    want = ["assemble"]
    for k, size in enumerate((2, 1)):
        want += ["batch_setup"] + (["get_null"] if k == 0 else []) + ["set_null"] + ["batch_upload"] * (2 * size)
        want += ["batch_solve", "projected"] + ["get_null", "select", "load", "load"] * size
    want += ["set_null", "batch_setup"]
    assert names == want
    sets = [c[1:] for c in rec.calls if c[0] == "set_null"]
    assert sets == [(True, 1e-9), (True, 1e-9), (False, 1e-10)]            # on in both batches, then as it was found
    assert [c[1:] for c in rec.calls if c[0] == "batch_solve"] == [(1e-6, int(t["itmax"]))] * 2
    assert rec.calls[-1] == ("batch_setup", ()) and not rec.on
    assert [r["projected_residual"] for r in rs] == [1e-7, 2e-7, 1e-7] and all(r["removed"] == 2e-4 for r in rs)
    assert [r["null"]["components"][0]["iterations"] for r in rs] == [100, 101, 100]
    assert [r["iter"] for r in rs] == [3, 4, 3]


def test_the_default_null_tol_and_a_setting_that_was_on(elmer):
    model, t, n = elmer
    rec = NullRecorder(n, on=True, null_tol=1e-8)
    host.run_harmonic_sweep(model, rec, 50.0, [25.0, 50.0], null_projection=True)
    sets = [c[1:] for c in rec.calls if c[0] == "set_null"]
    assert sets == [(True, 1e-10), (True, 1e-8)]                           # the default, then back to what was found
    i = [c[0] for c in rec.calls].index
    assert i("set_null") < i("batch_upload")
    assert [c[0] for c in rec.calls][-2:] == ["set_null", "batch_setup"]    # restored while the batch exists
    assert rec.on and rec.null_tol == 1e-8


def test_the_default_leaves_the_setting_alone(elmer):
    model, t, n = elmer
    rec = NullRecorder(n, on=True, null_tol=1e-8)
    rs = host.run_harmonic_sweep(model, rec, 50.0, [25.0, 50.0])
    names = {c[0] for c in rec.calls}
    assert not names & {"set_null", "get_null", "projected"}
    assert "projected_residual" not in rs[0] and "null" not in rs[0] and "removed" not in rs[0]
    assert rec.on and rec.null_tol == 1e-8


@pytest.mark.parametrize("fail_at", [1, 2])
def test_the_setting_is_restored_when_a_solve_raises(elmer, fail_at):
    model, t, n = elmer
    rec = NullRecorder(n, on=False, null_tol=1e-7, fail_at_solve=fail_at)
    with pytest.raises(RuntimeError, match="missed null_tol"):
        host.run_harmonic_sweep(model, rec, 50.0, [10.0, 20.0, 40.0], batch=2, null_projection=True)
    assert rec.calls[-1] == ("set_null", False, 1e-7) and rec.calls[-2][0] == "batch_solve"
    assert not rec.on and rec.null_tol == 1e-7
    assert rec.nsys > 0                                                     # (the batch is left to the caller)


def test_a_refused_restore_does_not_hide_the_error_of_the_solve(elmer):
    model, t, n = elmer
    rec = NullRecorder(n, on=True, null_tol=1e-8, fail_at_solve=1, fail_at_set=2)      # (the second set is the restore)
    with pytest.raises(RuntimeError, match="missed null_tol"):
        host.run_harmonic_sweep(model, rec, 50.0, [10.0, 20.0], null_projection=True)
    assert rec.calls[-1] == ("set_null_refused", True, 1e-8)


@pytest.mark.parametrize("argv", [["--harmonic", "50", "--sweep-null-projection"],
                                  ["--sweep-null-projection"],
                                  ["--harmonic", "50", "--sweep", "25,50", "--sweep-null-tol", "1e-9"],
                                  ["--harmonic", "50", "--sweep-null-tol", "1e-9"],
                                  ["--sweep-null-tol", "1e-9"],
                                  ["--harmonic", "50", "--sweep", "25,50", "--sweep-null-projection", "--null-projection"],
                                  ["--sweep", "25,50", "--sweep-null-projection"],
                                  ["--harmonic", "50", "--sweep", "25,50", "--sweep-null-projection", "--sweep-null-tol", "x"]],
                         ids=["projection-no-sweep", "projection-alone", "tol-no-projection", "tol-no-sweep", "tol-alone",
                              "both-projections", "no-harmonic", "tol-no-number"])
def test_the_parsers_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        run.main([os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc")] + argv)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_the_refusal_of_null_projection_points_to_the_new_flag(capsys):
    with pytest.raises(SystemExit) as e:
        run.main([os.path.join(GOLDEN, "g4_compare_to_Elmer.vxc"), "--harmonic", "50", "--sweep", "25,50", "--null-projection"])
    assert e.value.code == 2
    assert "--sweep-null-projection" in capsys.readouterr().err


def test_the_new_options_accepted():
    ap = run.build_parser()
    a = ap.parse_args(["m.vxc", "--harmonic", "50", "--sweep", "10,100", "--sweep-null-projection", "--sweep-null-tol", "1e-8"])
    assert run.check_sweep_options(ap, a) == [10.0, 100.0] and a.sweep_null_projection and a.sweep_null_tol == 1e-8
    a = ap.parse_args(["m.vxc", "--harmonic", "50", "--sweep", "10,100", "--sweep-null-projection"])
    assert run.check_sweep_options(ap, a) == [10.0, 100.0] and a.sweep_null_tol is None
    a = ap.parse_args(["m.vxc", "--harmonic", "50", "--sweep", "10,100"])
    assert run.check_sweep_options(ap, a) == [10.0, 100.0] and not a.sweep_null_projection

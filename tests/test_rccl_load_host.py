"""CPU-only: ec3d_rccl_load (csrc/ec3d_rccl.cpp) answers a bad EC3D_RCCL_LIB with a message, not with a crash.

tests/support/rccl_load_cases.cpp (a stand-alone program, built together with csrc/ec3d_rccl.cpp under the address and
undefined-behaviour sanitizers) calls the loader as often as asked and prints what came back.  Every case ends with exit
status 0, the answer on stdout with the variable's value in it, and no sanitizer report on stderr.  Where no library was
opened stderr is empty; where one was -- the empty shared object, the loopback library -- the loader announces it there by
design ("a job never runs on a substitute silently", csrc/ec3d_rccl.cpp), and stderr is exactly that one line.  Each
failing case runs twice in one process, so that the second call takes the cached-error branch."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "eddy_currents_3d_amd", "csrc")
SRC = os.path.join(REPO, "tests", "support", "rccl_load_cases.cpp")


def _cc():
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    return cc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rccl_load") / "rccl_load_cases")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_cc()))), "include")
    subprocess.run([_cc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", rocm_inc,
                    SRC, os.path.join(CSRC, "ec3d_rccl.cpp"), "-ldl", "-o", out], check=True)
    return out


def run(exe, lib, calls):
    env = {k: v for k, v in os.environ.items() if k != "EC3D_RCCL_LIB"}      # everything else as this process has it
    if lib is not None:
        env["EC3D_RCCL_LIB"] = lib
    out = subprocess.run([exe, str(calls)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    lines = out.stdout.splitlines()
    assert len(lines) == calls, out.stdout
    shown = lib if lib is not None else "(unset)"
    answers = []
    for i, line in enumerate(lines):
        head = f"call {i} EC3D_RCCL_LIB={shown} "
        assert line.startswith(head), line
        answers.append(line[len(head):])
    return answers, out.stderr


def announced(lib):
    return f"ec3d: RCCL entry points taken from EC3D_RCCL_LIB={lib}\n"


def test_no_such_file(exe):
    lib = "/no/such/file"
    answers, err = run(exe, lib, 2)
    assert err == "", err                          # nothing was opened, so nothing is announced
    assert answers[0].startswith(f"error EC3D_RCCL_LIB={lib}: ") and lib in answers[0][len(f"error EC3D_RCCL_LIB={lib}: "):]
    assert "No such file" in answers[0] or "cannot open" in answers[0], answers[0]      # dlerror()'s text, not the stand-in
    assert answers[1] == answers[0]                # the cached error


def test_empty_shared_object(exe, tmp_path):
    src, lib = tmp_path / "empty.c", str(tmp_path / "libempty.so")
    src.write_text("")
    subprocess.run([_cc(), "-x", "c", "-shared", "-fPIC", str(src), "-o", lib], check=True)
    answers, err = run(exe, lib, 2)
    assert answers == ["error RCCL symbol missing: ncclGetUniqueId"] * 2
    assert err == announced(lib), err              # opened once, announced once; the second call is the cached error


def test_loopback_library_loads(exe):
    from eddy_currents_3d_amd.build import build_test_support
    lib = build_test_support()
    assert lib and os.path.exists(lib)
    answers, err = run(exe, lib, 2)
    assert err == announced(lib), err
    for a in answers:
        assert a.startswith("loaded path=") and len(a) > len("loaded path="), a
        assert os.path.samefile(a[len("loaded path="):], lib)


def test_unset_loads_librccl_or_says_not_found(exe):
    """Which of the two depends on the machine; a crash is neither."""
    answers, err = run(exe, None, 2)
    assert err == "", err
    assert answers[1] == answers[0]
    a = answers[0]
    if a.startswith("loaded path="):
        assert "rccl" in os.path.basename(a[len("loaded path="):]), a
    else:
        assert a.startswith("error RCCL not found (dlopen librccl.so.1): ") and len(a) > len("error RCCL not found (dlopen librccl.so.1): "), a

"""CPU-only: which instance of an SpMV-type kernel a launch picks (csrc/ec3d_form.hpp).

Every form of a kernel produces the same bits, so the GPU parity tests cannot tell a launcher that picks the plain
z-march where the 2-D-tile kernel belongs: it would only lose time.  Here the selector and the LDS size it hands the
launch are pinned on the host: tests/support/spmv_form_table.cpp (a stand-alone program, built with the address and
undefined-behaviour sanitizers) prints both for every combination of the fields the rule reads, and each line is
compared with the rule restated below."""
import itertools
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "support", "spmv_form_table.cpp")

GENERIC, DIA7, DICT7, SAV = 0, 7, 107, 207
STRIDE, NSTAGE, NSTAGE_RT, TILE = 16, 4, 2, 512

# sav, nb, ncls, has_tail, zm_tpp, bnd_last, patch_npx, rp_px, il_planes, nt, halo_store
AXES = [(0, 1), (3, 7), (0, 28), (0, 1), (0, 4), (-1, 5), (0, 2), (0, 64), (0, 8), (0, 1, 3), (0, 3)]


def form_rule(sav, nb, ncls, has_tail, zm_tpp, bnd_last, patch_npx, rp_px, il_planes, nt, halo_store):
    fmt = SAV if sav else DICT7 if nb == 7 and ncls > 0 else DIA7 if nb == 7 else GENERIC
    zm = zm_tpp > 0 and bnd_last < 0 and fmt != GENERIC
    tail = fmt != SAV and bool(has_tail)
    patch = zm and not tail and ((fmt == DICT7 and patch_npx > 0) or (fmt == SAV and rp_px > 0))
    il = zm and not patch and fmt == SAV and il_planes > 0
    hs = fmt == DICT7 and halo_store != 0
    return fmt, int(nt & 1), int(zm), int(tail), int(patch), int(il), int(hs)


def lds_rule(ncls, form):
    fmt, _, zm, _, patch, il, _ = form
    if il:
        return ncls * STRIDE * 8
    if patch and fmt == SAV:
        return ncls * STRIDE * 8 + (2 + NSTAGE_RT) * TILE * 8
    if patch:
        return ((ncls * 7 + 1 if fmt == DICT7 else 0) & ~1) * 8 + 2 * TILE * 8
    if fmt == DICT7:
        return ncls * 7 * 8
    if fmt == SAV:
        return ncls * STRIDE * 8 + (NSTAGE * TILE * 8 if zm else 0)
    return 0


# <FMT, NT, ZM, TAIL, PATCH> of k_spmv, k_residual, k1_spmv_dot, k3_spmv_dots: 15 for each cache policy.  On the
# structured form, which has no tail, TAIL = 1 is the interleaved z-march.
INSTANCES = {(fmt, nt, zm, tail, patch) for nt in (0, 1) for fmt, zm, tail, patch in
             [(GENERIC, 0, 0, 0), (GENERIC, 0, 1, 0),
              (DIA7, 0, 0, 0), (DIA7, 0, 1, 0), (DIA7, 1, 0, 0), (DIA7, 1, 1, 0),
              (DICT7, 0, 0, 0), (DICT7, 0, 1, 0), (DICT7, 1, 0, 0), (DICT7, 1, 1, 0), (DICT7, 1, 0, 1),
              (SAV, 0, 0, 0), (SAV, 1, 0, 0), (SAV, 1, 1, 0), (SAV, 1, 0, 1)]}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{inputs: (form, LDS bytes)} as the C++ selector gives them."""
    from eddy_currents_3d_amd.build import hipcc
    cc = shutil.which(hipcc())
    assert cc, "hipcc not found"
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(cc)))
    exe = str(tmp_path_factory.mktemp("spmv_form") / "spmv_form_table")
    subprocess.run([cc, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-std=c++17", "-O1", "-g",
                    "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr   # a sanitizer report
    rows = {}
    for line in out.stdout.splitlines():
        given, got = line.split("|")
        got = tuple(int(v) for v in got.split())
        rows[tuple(int(v) for v in given.split())] = (got[:7], got[7])
    return rows


def test_every_case_follows_the_rule(table):
    cases = list(itertools.product(*AXES))
    assert len(cases) == 3072 and set(table) == set(cases)
    for case in cases:
        form = form_rule(*case)
        assert table[case] == (form, lds_rule(case[2], form)), case


def test_the_forms_are_the_thirty_instances(table):
    picked = {(fmt, nt, zm, tail or il, patch) for (fmt, nt, zm, tail, patch, il, hs), _ in table.values()}
    assert picked == INSTANCES and len(INSTANCES) == 30


def test_keep_bits_do_not_change_the_instance(table):
    """Sweep::nt carries the keep hints above bit 0: nt = 3 is nt = 1 with hints, the same instance and LDS."""
    for case in table:
        if case[9] == 3:
            assert table[case] == table[case[:9] + (1,) + case[10:]], case

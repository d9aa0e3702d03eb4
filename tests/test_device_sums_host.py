"""CPU: tests/device_sums_numpy.py -- the one numpy statement of csrc/ec3d_stream.hpp's summation chain -- against the
chain written out as plain Python loops over lanes, waves, threads and workgroups, compared as uint64.

* block_sum, strided and stream_dot on 1, 2 and 3 workgroups' worth of random doubles, on all -0.0 (the result is +0.0:
  the sums start from 0.0, which is where the hot path's ((w0 + w1) + w2) + w3 would give -0.0) and with one NaN and one
  inf among the values;
* stream_dot at nchunk = 1, WGS and WGS + 1 with WGS = 4: the second trip of a workgroup's chunk loop;
* null_projection_numpy.project_device: plain-loop coefficients and subtraction, rows >= n left alone, and the r.r
  partials of a launch with more workgroups than chunks."""
import numpy as np
import pytest

import device_sums_numpy as DS
import null_projection_numpy as NP


def bits(v):
    return np.atleast_1d(np.asarray(v, np.float64)).view(np.uint64)


def loop_block_sum(v):
    """256 thread values -> thread 0's sum."""
    assert len(v) == 256
    waves = []
    for w in range(4):
        lane = [float(x) for x in v[64 * w:64 * w + 64]]
        for o in (32, 16, 8, 4, 2, 1):      # __shfl_down: lane l reads lane l + o, its own value past the wave's end
            lane = [lane[l] + (lane[l + o] if l + o < 64 else lane[l]) for l in range(64)]
        waves.append(lane[0])
    s = 0.0
    for w in waves:
        s = s + w
    return s


def loop_strided(part):
    acc = []
    for t in range(256):
        a = 0.0
        for i in range(t, len(part), 256):
            a = a + float(part[i])
        acc.append(a)
    return loop_block_sum(acc)


def loop_stream_dot(a, b, wgs):
    nchunk = len(a) // 512
    G = min(nchunk, wgs)
    part = []
    for wg in range(G):
        acc = []
        for t in range(256):
            s = 0.0
            for ch in range(wg, nchunk, G):
                r = ch * 512 + 2 * t
                s = s + float(a[r]) * float(b[r])
                s = s + float(a[r + 1]) * float(b[r + 1])
            acc.append(s)
        part.append(loop_block_sum(acc))
    return loop_strided(part)


def values(kind, n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    if kind == "minus_zero":
        v = np.full(n, -0.0)
    elif kind == "nan_inf":
        v[rng.integers(0, n)] = np.nan
        v[(n // 2 + 7) % n] = np.inf
    return v


KINDS = ["random", "minus_zero", "nan_inf"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", [1, 2, 3])
def test_block_sum(kind, G):
    acc = values(kind, G * 256, 10 + G).reshape(G, 256)
    want = [loop_block_sum(row) for row in acc]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits(DS.block_sum(acc)), bits(want))
        assert np.array_equal(bits(DS.block_sum(acc.reshape(-1))), bits(want))      # mg_numpy passes G * 256 flat
    if kind == "minus_zero":
        assert np.array_equal(bits(want), bits(np.zeros(G)))                        # +0.0, not -0.0
    if kind == "nan_inf":
        assert np.isnan(want).sum() >= 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("count", [1, 255, 256, 2 * 256, 3 * 256 - 5])
def test_strided(kind, count):
    part = values(kind, count, 20 + count)
    assert np.array_equal(bits(DS.strided(part)), bits(loop_strided(part)))
    if kind == "minus_zero":
        assert np.array_equal(bits(DS.strided(part)), bits(0.0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nchunk, wgs", [(1, DS.WGS), (2, DS.WGS), (3, DS.WGS), (1, 4), (4, 4), (5, 4)])
def test_stream_dot(kind, nchunk, wgs):
    a = values(kind, nchunk * 512, 30 + nchunk)
    b = values("random", nchunk * 512, 40 + nchunk)
    if kind == "minus_zero":
        b = np.abs(b)                       # every product -0.0
    got, want = DS.stream_dot(a, b, wgs), loop_stream_dot(a, b, wgs)
    assert np.array_equal(bits(got), bits(want))
    if kind == "minus_zero":
        assert np.array_equal(bits(got), bits(0.0))
    if kind == "random":                    # (and it is the dot product)
        assert abs(got - float(a @ b)) <= 1e-12 * float(np.abs(a * b).sum())


def test_names_kept_by_the_twins():
    import field_integrals_numpy as FI
    import guess_history_numpy as GH
    import mg_numpy as M
    assert GH.dot_device is DS.stream_dot and FI.strided is DS.strided and FI.block_sum is DS.block_sum
    assert M._block_sums is DS.block_sum and M.mg_scalar_sum is DS.strided


@pytest.mark.parametrize("n, launched", [(5 * 512 - 3, None), (5 * 512 - 3, 8), (2 * 512, 1)])
def test_project_device(n, launched):
    n_pad = -(-n // 512) * 512
    rng = np.random.default_rng(7)
    Q = [np.where(np.arange(n_pad) < n, rng.standard_normal(n_pad), 0.0) for _ in range(2)]
    r = rng.standard_normal(n_pad)          # rows >= n hold something: they must neither count nor change
    got, c, part = NP.project_device(Q, r, n, launched=launched)
    live = np.where(np.arange(n_pad) < n, r, 0.0)
    want_c = [loop_stream_dot(q, live, DS.WGS) for q in Q]
    assert np.array_equal(bits(c), bits(want_c))
    want = r.copy()
    for row in range(n):
        x = float(r[row])
        for ci, q in zip(want_c, Q):
            x = x - ci * float(q[row])
        want[row] = x
    assert np.array_equal(bits(got), bits(want))
    G = min(n_pad // 512, DS.WGS) if launched is None else launched
    assert len(part) == G
    x = np.where(np.arange(n_pad) < n, want, 0.0)
    if launched is None:
        assert np.array_equal(bits(DS.strided(part)), bits(loop_stream_dot(x, x, DS.WGS)))
    if launched == 8:                       # 5 chunks, 8 workgroups: the last three leave +0.0
        assert np.array_equal(bits(part[5:]), bits(np.zeros(3)))
        assert np.array_equal(bits(part[:5]), bits([loop_block_sum((x * x).reshape(-1, 256, 2)[w].sum(axis=1)) for w in range(5)]))
    if launched == 1:                       # one workgroup takes both chunks
        assert np.array_equal(bits(DS.strided(part)), bits(loop_stream_dot(x, x, 1)))

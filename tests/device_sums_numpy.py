"""numpy twin of csrc/ec3d_stream.hpp: the fixed-order sums of every kernel outside the iteration's hot path, bit for bit.

    block_sum(acc)              [G, 256] thread values -> [G]: stream_block_sum of every workgroup
    strided(part)               one workgroup over `part`: stream_strided_sum, then block_sum (the collapse kernels)
    stream_partials(terms)      [nchunk, 256, 2] per-row terms of a streaming launch -> its per-workgroup partials
    stream_dot(a, b)            a . b over vectors of n_pad doubles: stream_partials of the products, then strided

`wgs` is EC3D_STREAM_WGS; the tests pass a small one to reach a workgroup's second chunk with few values.
No test lives here (the name does not start with test_)."""
import numpy as np

TILE, THREADS, WGS = 512, 256, 1024     # EC3D_TILE, EC3D_THREADS, EC3D_STREAM_WGS


def block_sum(acc):
    """Six levels of the wave's shuffle tree (lane l takes lane l + 32, + 16, ... + 1), then the four waves in order from
    0.0.  Also takes a flat array of G * 256 values."""
    w = np.asarray(acc, np.float64).reshape(-1, 4, 64)
    with np.errstate(invalid="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            w = w[:, :, :o] + w[:, :, o:2 * o]
        w = w[:, :, 0]
        return (((0.0 + w[:, 0]) + w[:, 1]) + w[:, 2]) + w[:, 3]


def strided(part):
    """Thread t adds the entries t, t + 256, ... in order from 0.0, then the tree."""
    t = np.zeros(THREADS)
    with np.errstate(invalid="ignore"):
        for j in range(0, len(part), THREADS):
            seg = part[j:j + THREADS]
            t[:len(seg)] = t[:len(seg)] + seg
    return float(block_sum(t)[0])


def stream_partials(terms, wgs=WGS, launched=None):
    """Workgroup w of G = min(nchunk, wgs) takes the chunks w, w + G, ...; thread t adds term 2t, then term 2t + 1, chunk
    after chunk from 0.0.  launched: the launch's workgroups where it is not G (those past the last chunk leave +0.0)."""
    nchunk = len(terms)
    G = min(nchunk, wgs) if launched is None else launched
    acc = np.zeros((G, THREADS))
    with np.errstate(invalid="ignore"):
        for j in range(0, nchunk, G):
            blk = terms[j:j + G]
            acc[:len(blk)] = acc[:len(blk)] + blk[:, :, 0]
            acc[:len(blk)] = acc[:len(blk)] + blk[:, :, 1]
    return block_sum(acc)


def stream_dot(a, b, wgs=WGS):
    assert len(a) == len(b) and len(a) % TILE == 0
    with np.errstate(invalid="ignore"):
        prod = (a * b).reshape(len(a) // TILE, THREADS, 2)
    return strided(stream_partials(prod, wgs))

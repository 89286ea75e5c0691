"""The pair-run kernel's run deal on the host, at every grid size (CPU).

crc32c_pair_kernel takes its schedule from prismdb::dev::pair_deal
(crc32c_device.h): K runs of record pairs, the first Kst dealt statically
(wave w: w, w + nwaves, ...), the rest claimed on demand from nctr claim
counters, counter c dealing Kst + c + nctr * j.  The hooks
prismdb_crc32c_pair_deal / _pair_csets / _pair_runs call that very function
on the host (no HIP call), so the arithmetic the kernel compiles is checked
here for every grid of 1..320 groups: the device suite only ever runs the
grid of the device it is on (and a few reduced ones, test_gpu_small_grid.py).
A counter without a group -- (b / 8) % 8 at 56 or fewer groups, before the
counters were sized from the grid -- leaves its runs unfolded: results,
flags and trailers unwritten, and the call returns 0.
"""
import ctypes

import numpy as np
import pytest

WAVES_PER_GROUP = 16  # kWavesPerGroup
CLAIM_LINES = 8       # kClaimLines
GRIDS = range(1, 321)


def _sizes(G):
    """The issue's batch sizes for a grid of G groups, from kPairMinSpans (2^18) up."""
    cand = [1 << 18, (1 << 18) + 1, 300001, 6144 * G - 1, 6144 * G, 6144 * G + 1, 9600 * G, 36800 * G]
    return sorted({n for n in cand if n >= 1 << 18})


@pytest.fixture(scope="module")
def deal(native):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    native.prismdb_crc32c_pair_deal.restype = ctypes.c_int
    native.prismdb_crc32c_pair_deal.argtypes = [ctypes.c_uint64, ctypes.c_uint32, u32p]
    native.prismdb_crc32c_pair_csets.restype = ctypes.c_int
    native.prismdb_crc32c_pair_csets.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    native.prismdb_crc32c_pair_runs.restype = ctypes.c_int
    native.prismdb_crc32c_pair_runs.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.c_void_p, ctypes.c_void_p]

    def get(n, G):
        out = (ctypes.c_uint32 * 8)()
        assert native.prismdb_crc32c_pair_deal(n, G, out) == 0
        d = dict(zip(("m", "K", "rq", "rr", "ptail", "Kst", "nctr", "nwaves"), (int(x) for x in out)))
        csets = np.empty(G, dtype=np.uint32)
        assert native.prismdb_crc32c_pair_csets(n, G, csets.ctypes.data) == 0
        lo = np.empty(d["K"], dtype=np.uint32)
        hi = np.empty(d["K"], dtype=np.uint32)
        assert native.prismdb_crc32c_pair_runs(n, G, 0, d["K"], lo.ctypes.data, hi.ctypes.data) == 0
        return d, csets, lo, hi

    return get


def test_deal_hook_rejects_what_no_launch_has(deal, native):
    out = (ctypes.c_uint32 * 8)()
    assert native.prismdb_crc32c_pair_deal(0, 8, out) == -1
    assert native.prismdb_crc32c_pair_deal(1 << 18, 0, out) == -1
    assert native.prismdb_crc32c_pair_deal((1 << 30) + 1, 8, out) == -1


@pytest.mark.parametrize("G", GRIDS)
def test_pair_deal_covers_every_run_once(deal, G):
    nwaves = WAVES_PER_GROUP * G
    tails = 0
    for n in _sizes(G):
        d, csets, lo, hi = deal(n, G)
        K, Kst, nctr = d["K"], d["Kst"], d["nctr"]
        assert d["nwaves"] == nwaves and 1 <= K and Kst <= K, (n, d)
        # the runs' records partition [0, n): consecutive, none empty, <= 64
        # records (one result lane each)
        assert lo[0] == 0 and hi[-1] == n, (n, d)
        assert (lo[1:] == hi[:-1]).all(), (n, d)
        width = hi.astype(np.int64) - lo.astype(np.int64)
        assert width.min() >= 1 and width.max() <= 64, (n, d, int(width.min()), int(width.max()))
        # the tail is on exactly when the issue's arithmetic says so
        active = d["rq"] >= 3 and K > 16 * nwaves
        assert (Kst < K) == active and (not active or K - Kst == 16 * nwaves), (n, d)
        tails += active
        # every counter in use has a group, no group has a counter past them
        assert 1 <= nctr <= CLAIM_LINES, (n, d)
        assert csets.max() < nctr, (n, d, csets.max())
        assert set(np.unique(csets).tolist()) == set(range(nctr)), (n, d, np.unique(csets).tolist())
        # static runs w, w + nwaves, ... < Kst of every wave, then what each
        # counter deals until its index passes K: [0, K) exactly once
        rounds = (Kst + nwaves - 1) // nwaves
        ks = (np.arange(nwaves, dtype=np.int64)[None, :] + nwaves * np.arange(rounds, dtype=np.int64)[:, None]).ravel()
        cover = np.bincount(ks[ks < Kst], minlength=K)
        for c in np.unique(csets).tolist():
            cover += np.bincount(np.arange(Kst + c, K, nctr, dtype=np.int64), minlength=K)
        assert cover.shape == (K,) and (cover == 1).all(), (n, d, np.nonzero(cover != 1)[0][:8].tolist())
    # 6144 * G + 1 and up have a tail at every grid (rq >= 3 from 96 pairs a wave on)
    assert tails >= 3, (G, tails)


def test_deal_at_64_groups_and_up_is_the_eight_counter_deal(deal):
    """From 64 groups on the deal is the one the round-6 numbers were measured
    on: eight counters, group b on counter (b / 8) % 8."""
    for G in (64, 65, 71, 72, 128, 256, 304, 320):
        d, csets, _, _ = deal(36800 * G, G)
        assert d["nctr"] == 8
        assert (csets == (np.arange(G) >> 3) % 8).all()

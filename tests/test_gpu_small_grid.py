"""Every route at reduced grids (test hook prismdb_crc32c_grid).

Each kernel on the hot path sizes its schedule from the grid it was launched
with, and the host launches one workgroup per CU: the library behaves
differently on every device or partition size it meets (an MI355X partition
in CPX mode has 32 CUs, an MI300X one 38).  The hook shrinks the grid (never
above the device's CU count), so the schedule arithmetic is checked here at
grids of 1..64 groups on whatever device the suite runs on.  Bit-exact
against the oracle; every output the call should write is prefilled with a
poison value, so an unwritten result cannot pass on a previous call's bytes.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
POISON_MM = 0x7F


@pytest.fixture(scope="module")
def dev(native):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from prismdb_amd import crc32c

    crc32c.device_init(0)
    native.prismdb_crc32c_grid.restype = ctypes.c_int
    native.prismdb_crc32c_grid.argtypes = [ctypes.c_int]
    native.leveldb_crc32c_last_error.restype = ctypes.c_char_p
    return torch.device("cuda", 0)


@pytest.fixture
def grid(native, dev):
    """grid(G): run what follows on G workgroups; the device's own count again afterwards."""
    try:
        yield lambda g: native.prismdb_crc32c_grid(g)
    finally:
        native.prismdb_crc32c_grid(0)


@pytest.fixture
def pin(native):
    """pin(direct_max, lane_mode, windows): a route, as conftest.set_route pins it."""
    def set_(direct_max, lane, windows):
        native.prismdb_crc32c_direct_max(direct_max)
        native.prismdb_crc32c_lane_mode(lane)
        native.prismdb_crc32c_windows(windows)

    try:
        yield set_
    finally:
        set_(1 << 17, 0, 2)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev(arr, dev):
    import torch

    return torch.from_numpy(np.array(arr, copy=True)).to(dev)


def _poison_out(n, dev):
    import torch

    return torch.full((n,), POISON, dtype=torch.int32, device=dev)


def _poison_mm(n, dev):
    import torch

    return torch.full((n,), POISON_MM, dtype=torch.uint8, device=dev)


def _schedule(native):
    arr = (ctypes.c_uint64 * 3)()
    rc = native.prismdb_crc32c_last_schedule(arr)
    return rc, tuple(int(x) for x in arr)


def _claims(native):
    arr = (ctypes.c_uint64 * 2)()
    assert native.prismdb_crc32c_last_claims(arr) == 0
    return [int(x) for x in arr]


def _split_rc(native):
    arr = (ctypes.c_uint64 * 4)()
    return native.prismdb_crc32c_last_split(arr)


def _mask_np(raw):
    raw = raw.astype(np.uint32)
    return (((raw >> np.uint32(15)) | (raw << np.uint32(17))) + np.uint32(0xA282EAD8)).astype(np.uint32)


def _store_u32(img, at, vals):
    idx = at.astype(np.int64)[:, None] + np.arange(4)[None, :]
    img[idx] = vals.astype("<u4").view(np.uint8).reshape(-1, 4)


def _seal_abi(native, buf, d_off, d_len, d_init, n, out, flags):
    import torch

    rc = native.leveldb_crc32c_batch(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(d_off.data_ptr()),
                                     ctypes.c_void_p(d_len.data_ptr()),
                                     ctypes.c_void_p(d_init.data_ptr()) if d_init is not None else None,
                                     ctypes.c_size_t(n), ctypes.c_void_p(out.data_ptr()) if out is not None else None,
                                     None, ctypes.c_uint32(flags),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, native.leveldb_crc32c_last_error()


# ---------------------------------------------------------------- pair-run kernel


def _pair_n(G):
    n = max(1 << 18, 6200 * G)
    return n | 1


@functools.lru_cache(maxsize=2)
def _pair_plain(n, oracle):
    """The existing `pair` shape: 61-byte spans at stride 64, offset +3."""
    off = np.arange(n, dtype=np.uint64) * 64 + 3
    lens = np.full(n, 61, dtype=np.uint32)
    host = oracle.synth(n * 64 + 64, 0x5EED0090)
    want, _ = oracle.batch(host, off, lens, mask=True)
    return host, off, lens, want


@functools.lru_cache(maxsize=2)
def _pair_slots(n, oracle):
    """test_pair_run_schedule's shape at 64-byte slots: random lengths 0..56 at
    random offsets inside their slot, the trailer right after, per-span init,
    three long spans (the segment pass) behind the slots, every seventh
    trailer damaged."""
    rng = np.random.default_rng(0x5EED0091 + n)
    lens = rng.integers(0, 57, size=n).astype(np.int64)
    off = (8 + 64 * np.arange(n, dtype=np.int64) + (rng.random(n) * (61 - lens)).astype(np.int64))
    longs = [5, n // 2, n - 2]
    at = 8 + 64 * n + 64
    for i in longs:
        lens[i] = int(rng.integers(131073, 200000))
        off[i] = at + int(rng.integers(0, 4))
        at = int(off[i] + lens[i] + 4 + 8)
    host = oracle.synth(at + 64, 0x5EED0092)
    init = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    off = off.astype(np.uint64)
    masked, _ = oracle.batch(host, off, lens.astype(np.uint32), init, mask=True)
    damaged = np.zeros(n, dtype=bool)
    damaged[3::7] = True
    tr = off.astype(np.int64) + lens
    _store_u32(host, tr, masked ^ damaged.astype(np.uint32))
    return host, off, lens.astype(np.uint32), init, masked, damaged, tr


@pytest.mark.parametrize("G", [1, 8, 38, 56, 57, 64])
def test_pair_kernel_tail_at_reduced_grid(dev, oracle, native, grid, pin, G):
    """The pair-run kernel with its claimed tail on, at grids where (group / 8)
    % 8 left claim counters without a group (56 groups or fewer) and where it
    did not (57, 64): n = max(2^18, 6200 G) spans, plain + mask, VERIFY with
    every seventh trailer damaged, MASK | WRITE_TRAILER without and with out.
    Every crc, every flag, every byte of the sealed image.

    Before the counters were sized from the grid (nctr = min(8, max(1, G / 8))),
    measured once on a build with the hook alone: G = 1, 8, 38 and 56 failed
    every one of the four ways (13 439, 57 343, 21 887 and 10 751 results, as
    many verify flags and those spans' trailers -- the tail runs of the
    counters without a group -- left at their poison, return code 0), 57 and
    64 passed."""
    import torch
    from prismdb_amd import crc32c

    n = _pair_n(G)
    grid(G)
    pin(0, -1, 0)  # the planner path alone
    errs = []  # every way is run and reported; the test fails on any

    def check(what, ok, detail):
        print(f"G={G} n={n} {what}: {'ok' if ok else 'WRONG'} {detail}")
        if not ok:
            errs.append((what, detail))

    def engaged(what):
        rc, sched = _schedule(native)
        claims = _claims(native)
        check(what + " schedule", rc == 0 and sched == (n, 0, 1), (rc, sched))
        check(what + " tail claimed", claims[0] > 0, claims)

    def same(what, got, want):
        bad = np.nonzero(got != want)[0]
        check(what, len(bad) == 0, f"{len(bad)} of {len(want)} differ, first at {bad[:4].tolist()}")

    # plain + mask
    host, off, lens, want = _pair_plain(n, oracle)
    buf = torch.from_numpy(host).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    out = _poison_out(n, dev)
    crc32c.batch(buf, d_off, d_len, mask=True, out=out, check_bounds=False)
    engaged("plain")
    same("plain crcs", _u32(out), want)
    del buf, d_off, d_len, out

    # verify, every seventh trailer damaged
    host, off, lens, init, masked, damaged, tr = _pair_slots(n, oracle)
    buf = torch.from_numpy(host).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_init = torch.from_numpy(init.view(np.int32)).to(dev)
    out, mm = _poison_out(n, dev), _poison_mm(n, dev)
    crc32c.batch(buf, d_off, d_len, d_init, mask=True, verify=True, out=out, mismatch=mm)
    engaged("verify")
    same("verify crcs", _u32(out), masked)
    same("verify flags", mm.cpu().numpy(), damaged.astype(np.uint8))

    # seal over zeroed trailers: out = NULL, then out given
    zeroed = host.copy()
    _store_u32(zeroed, tr, np.zeros(n, dtype=np.uint32))
    want_img = host.copy()
    _store_u32(want_img, tr, masked)
    for with_out in (False, True):
        sbuf = torch.from_numpy(zeroed).to(dev)
        out = _poison_out(n, dev) if with_out else None
        _seal_abi(native, sbuf, d_off, d_len, d_init, n, out, 0x3)
        engaged(f"seal out={with_out}")
        if with_out:
            same("seal crcs", _u32(out), masked)
        same(f"seal out={with_out} image", sbuf.cpu().numpy(), want_img)
        del sbuf
    assert not errs, errs


def test_pair_kernel_without_tail_at_56_groups(dev, oracle, native, grid, pin):
    """56 groups, 2^18 spans: runs of two pairs, so no claimed tail (claims 0)."""
    import torch
    from prismdb_amd import crc32c

    n = 1 << 18
    host, off, lens, want = _pair_plain(n, oracle)
    buf = torch.from_numpy(host).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    grid(56)
    pin(0, -1, 0)
    out = _poison_out(n, dev)
    crc32c.batch(buf, d_off, d_len, mask=True, out=out, check_bounds=False)
    rc, sched = _schedule(native)
    assert rc == 0 and sched == (n, 0, 1), (rc, sched)
    assert _claims(native)[0] == 0
    np.testing.assert_array_equal(_u32(out), want)


# ---------------------------------------------------------------- every descriptor route

ROUTE_PINS = {"direct": (1 << 17, 0, 1), "windows": (1000, 0, 1), "lane_log": (0, 0, 0), "lane_all": (0, 1, 0),
              "span_only": (0, -1, 0)}


@functools.lru_cache(maxsize=1)
def _random_batch(oracle):
    """~3000 spans of 0..4096 bytes, one in 97 of 131 073..400 000, 6 bytes
    free before each (a log header) and 4 after (a block trailer)."""
    rng = np.random.default_rng(0x5EED0093)
    n = 3001
    lens = rng.integers(0, 4097, size=n).astype(np.int64)
    lens[11::97] = rng.integers(131073, 400001, size=len(lens[11::97]))
    off = np.concatenate([[19], 19 + np.cumsum(lens + 4 + 6 + rng.integers(0, 6, size=n))[:-1]]).astype(np.uint64)
    host = oracle.synth(int(off[-1] + lens[-1]) + 64, 0x5EED0094)
    init = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    lens = lens.astype(np.uint32)
    raw, _ = oracle.batch(host, off, lens, init)
    masked, _ = oracle.batch(host, off, lens, init, mask=True)
    damaged = rng.random(n) < 0.05
    return host, off, lens, init, raw, masked, damaged


@pytest.mark.parametrize("route", list(ROUTE_PINS))
@pytest.mark.parametrize("G", [1, 2, 7, 32])
def test_routes_at_reduced_grid(dev, oracle, golden, native, grid, pin, G, route):
    """The golden sweep and a random batch (plain, verify, seal; on the
    log-record route also with LOG_HEADER, the lane kernel's batches) through
    every descriptor route at 1, 2, 7 and 32 groups."""
    import torch
    from prismdb_amd import crc32c

    grid(G)
    pin(*ROUTE_PINS[route])
    # golden sweep: per-span init, mask
    buf = _dev(np.frombuffer(golden["input"], dtype=np.uint8), dev)
    rows = np.array(golden["vectors"]["rows"], dtype=np.uint64)
    g_off = _dev(rows[:, 0].astype(np.int64), dev)
    g_len = _dev(rows[:, 1].astype(np.uint32).view(np.int32), dev)
    g_init = _dev(rows[:, 2].astype(np.uint32).view(np.int32), dev)
    for mask, col in ((False, 3), (True, 4)):
        out = _poison_out(len(rows), dev)
        crc32c.batch(buf, g_off, g_len, g_init, mask=mask, out=out)
        np.testing.assert_array_equal(_u32(out), rows[:, col].astype(np.uint32))
    # random batch
    host, off, lens, init, raw, masked, damaged = _random_batch(oracle)
    n = len(off)
    d_off = _dev(off.astype(np.int64), dev)
    d_len = _dev(lens.view(np.int32), dev)
    d_init = _dev(init.view(np.int32), dev)
    out = _poison_out(n, dev)
    crc32c.batch(_dev(host, dev), d_off, d_len, d_init, out=out)
    np.testing.assert_array_equal(_u32(out), raw)
    for hdr in ((False, True) if route == "lane_log" else (False,)):
        at = off.astype(np.int64) - 6 if hdr else off.astype(np.int64) + lens.astype(np.int64)
        img = host.copy()
        _store_u32(img, at, masked ^ damaged.astype(np.uint32))
        out, mm = _poison_out(n, dev), _poison_mm(n, dev)
        crc32c.batch(_dev(img, dev), d_off, d_len, d_init, mask=True, verify=True, log_header=hdr, out=out, mismatch=mm)
        np.testing.assert_array_equal(_u32(out), masked, err_msg=f"verify hdr={hdr}")
        np.testing.assert_array_equal(mm.cpu().numpy(), damaged.astype(np.uint8), err_msg=f"verify hdr={hdr}")
        zeroed, want_img = host.copy(), host.copy()
        _store_u32(zeroed, at, np.zeros(n, dtype=np.uint32))
        _store_u32(want_img, at, masked)
        sbuf = _dev(zeroed, dev)
        out = _poison_out(n, dev)
        crc32c.batch(sbuf, d_off, d_len, d_init, mask=True, trailer=True, log_header=hdr, out=out)
        np.testing.assert_array_equal(_u32(out), masked, err_msg=f"seal hdr={hdr}")
        got = sbuf.cpu().numpy()
        assert (got == want_img).all(), (hdr, np.nonzero(got != want_img)[0][:8])


# ---------------------------------------------------------------- one-launch kernel


@functools.lru_cache(maxsize=1)
def _huge(oracle):
    """A 40 MiB span at an odd offset with twelve small spans in front of it."""
    rng = np.random.default_rng(0x5EED0095)
    size = (40 << 20) + (1 << 16)
    host = oracle.synth(size, 0x5EED0096)
    lens = np.concatenate([rng.integers(0, 4097, size=12), [40 << 20]]).astype(np.uint32)
    off = np.concatenate([np.arange(12) * 4100 + 5, [12 * 4100 + 7]]).astype(np.uint64)
    order = np.array([0, 1, 2, 3, 4, 12, 5, 6, 7, 8, 9, 10, 11])  # the huge span in the middle of the batch
    off, lens = off[order], lens[order]
    want, _ = oracle.batch(host, off, lens, mask=True)
    return host, off, lens, want


@functools.lru_cache(maxsize=1)
def _small(oracle):
    rng = np.random.default_rng(0x5EED0097)
    n = 3 * 768 * 3 + 1  # three windows of 3 groups' capacity and one span
    lens = rng.integers(0, 4097, size=n).astype(np.int64)
    lens[::50] = rng.integers(4097, 20000, size=len(lens[::50]))  # ring spans of several chunks
    off = np.concatenate([[3], 3 + np.cumsum(lens + rng.integers(0, 9, size=n))[:-1]]).astype(np.uint64)
    host = oracle.synth(int(off[-1] + lens[-1]) + 64, 0x5EED0098)
    init = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    want, _ = oracle.batch(host, off, lens.astype(np.uint32), init, mask=True)
    return host, off, lens.astype(np.uint32), init, want


@pytest.mark.parametrize("G", [1, 2, 3])
def test_one_launch_edges_at_reduced_grid(dev, oracle, native, grid, pin, G):
    """The one-launch kernel where its deal depends on the wave count: 12 G
    waves (no ticket workers below 3 groups), capacity 768 G spans.  Batches of
    one span, of a span less, as many and one more than waves, and around the
    capacity (one more falls through to the planner); a 40 MiB span alone (its
    tickets claimed by its pusher and by whoever the help flag calls) and
    inside a 13-span batch."""
    import torch
    from prismdb_amd import crc32c

    host, off, lens, init, want = _small(oracle)
    buf = _dev(host, dev)
    d_off, d_len, d_init = _dev(off.astype(np.int64), dev), _dev(lens.view(np.int32), dev), _dev(init.view(np.int32), dev)
    grid(G)
    pin(1 << 17, 0, 1)
    cap = 768 * G
    for n in sorted({1, 11, 12, 13, 767, 768, 769, 12 * G - 1, 12 * G, 12 * G + 1, cap - 1, cap, cap + 1}):
        out = _poison_out(n, dev)
        crc32c.batch(buf, d_off[:n], d_len[:n], d_init[:n], mask=True, out=out, check_bounds=False)
        assert _split_rc(native) == (-2 if n <= cap else 0), (n, cap)  # one launch, or the planner past the capacity
        np.testing.assert_array_equal(_u32(out), want[:n], err_msg=f"n={n}")
    # windows of the capacity: a batch of three windows and one span
    pin(cap, 0, 1)
    n = 3 * cap + 1 if 3 * cap + 1 <= len(off) else len(off)
    out = _poison_out(n, dev)
    crc32c.batch(buf, d_off[:n], d_len[:n], d_init[:n], mask=True, out=out, check_bounds=False)
    assert _split_rc(native) == -2
    np.testing.assert_array_equal(_u32(out), want[:n])
    pin(1 << 17, 0, 1)
    del buf
    host, off, lens, want = _huge(oracle)
    buf = _dev(host, dev)
    d_off, d_len = _dev(off.astype(np.int64), dev), _dev(lens.view(np.int32), dev)
    for sel in (slice(5, 6), slice(0, 13)):
        for dbg in ((0, 1, 3) if G == 2 else (0,)):
            prev = native.prismdb_crc32c_direct_debug(dbg)
            try:
                out = _poison_out(sel.stop - sel.start, dev)
                crc32c.batch(buf, d_off[sel], d_len[sel], mask=True, out=out, check_bounds=False)
                got = _u32(out)
            finally:
                native.prismdb_crc32c_direct_debug(prev)
            assert _split_rc(native) == -2
            np.testing.assert_array_equal(got, want[sel], err_msg=f"spans {sel} dbg {dbg}")


# ---------------------------------------------------------------- fixed-geometry kernel


@functools.lru_cache(maxsize=1)
def _fixed(oracle):
    nblk = 4097
    host = oracle.synth(nblk * 4096 + 8, 0x5EED0099)
    want = oracle.batch_fixed(host, 4096, 4096, nblk, init=0x12345678, mask=True)
    off = np.arange(nblk, dtype=np.uint64) * 4096
    raw, _ = oracle.batch(host, off, np.full(nblk, 4092, dtype=np.uint32))
    damaged = np.zeros(nblk, dtype=bool)
    damaged[[0, 999, 1000, 2048, 4096]] = True
    img = host.copy()
    _store_u32(img, off.astype(np.int64) + 4092, _mask_np(raw) ^ damaged.astype(np.uint32))
    return host, want, img, raw, damaged


@pytest.mark.parametrize("nblk", [1000, 4097])
@pytest.mark.parametrize("G", [1, 7, 32])
def test_fixed_kernel_at_reduced_grid(dev, oracle, native, grid, G, nblk):
    """The fixed-geometry kernel's run deal (runs shortened until every wave
    has a few) at 1, 7 and 32 groups: 4 KiB blocks, and 4092-byte blocks
    verified against their stored trailers."""
    import torch
    from prismdb_amd import crc32c

    host, want, img, raw, damaged = _fixed(oracle)
    grid(G)
    out = _poison_out(nblk, dev)
    crc32c.batch_fixed(_dev(host, dev), 4096, 4096, nblk, init=0x12345678, mask=True, out=out)
    np.testing.assert_array_equal(_u32(out), want[:nblk])
    out, mm = _poison_out(nblk, dev), _poison_mm(nblk, dev)
    crc32c.batch_fixed(_dev(img, dev), 4096, 4092, nblk, verify=True, out=out, mismatch=mm)
    np.testing.assert_array_equal(_u32(out), raw[:nblk])
    np.testing.assert_array_equal(mm.cpu().numpy(), damaged[:nblk].astype(np.uint8))


# ---------------------------------------------------------------- claimed tails of the lane and span kernels


def test_lane_kernel_tail_at_8_groups(dev, oracle, native, grid, pin):
    """A LOG_HEADER batch of ~1 KB records sized from the grid so that the lane
    kernel's claimed tail engages (more than kLaneTailRounds + 2 runs of 64
    records per wave, 8 waves a group), verified with 1 % damaged."""
    import torch
    from prismdb_amd import crc32c

    G = 8
    rng = np.random.default_rng(0x5EED009A)
    n = 64 * 11 * 8 * G
    lens = rng.integers(900, 1101, size=n).astype(np.uint64)
    lens[rng.integers(0, n, size=40)] = rng.integers(1281, 4000, size=40).astype(np.uint64)  # the generic path's
    off = np.cumsum(np.concatenate([[11], (lens + rng.integers(7, 20, size=n).astype(np.uint64))[:-1]])).astype(np.uint64)
    host = oracle.synth(int(off[-1] + lens[-1]) + 64, 0x5EED009B)
    want, _ = oracle.batch(host, off, lens.astype(np.uint32), mask=True)
    damaged = rng.random(n) < 0.01
    _store_u32(host, off.astype(np.int64) - 6, want ^ damaged.astype(np.uint32))
    buf = _dev(host, dev)
    d_off, d_len = _dev(off.astype(np.int64), dev), _dev(lens.astype(np.uint32).view(np.int32), dev)
    grid(G)
    pin(0, 0, 0)
    out, mm = _poison_out(n, dev), _poison_mm(n, dev)
    crc32c.batch(buf, d_off, d_len, mask=True, verify=True, log_header=True, out=out, mismatch=mm)
    claims = _claims(native)
    np.testing.assert_array_equal(_u32(out), want)
    np.testing.assert_array_equal(mm.cpu().numpy(), damaged.astype(np.uint8))
    assert claims[1] > 0, "the lane kernel's tail was never claimed"


def test_span_kernel_sliced_tail_at_2_groups(dev, oracle, native, grid, pin):
    """test_claimed_tails_engage's span leg sized for 2 groups (~19 000 spans of
    1-3 chunks, ~600 tasks per stream): task-balanced slices of >= 32 tasks,
    the last rounds claimed -- and, the batch being small here, every span
    against the oracle."""
    import torch
    from prismdb_amd import crc32c

    G = 2
    rng = np.random.default_rng(0x5EED009C)
    streams = 2 * 16 * G
    tasks = rng.integers(1, 4, size=600 * streams // 2).astype(np.uint64)
    lens = (tasks * 4096 - rng.integers(0, 300, size=len(tasks)).astype(np.uint64)).astype(np.uint32)
    n = len(lens)
    off = np.cumsum(np.concatenate([[5], lens[:-1].astype(np.uint64) + 7])).astype(np.uint64)
    host = oracle.synth(int(off[-1]) + int(lens[-1]) + 64, 0x5EED009D)
    want, _ = oracle.batch(host, off, lens, mask=True)
    buf = torch.from_numpy(host).to(dev)
    d_off, d_len = _dev(off.astype(np.int64), dev), _dev(lens.view(np.int32), dev)
    grid(G)
    pin(0, -1, 0)
    out = _poison_out(n, dev)
    crc32c.batch(buf, d_off, d_len, mask=True, out=out, check_bounds=False)
    rc, sched = _schedule(native)
    claims = _claims(native)
    assert rc == 0 and sched[1] > 0 and sched[0] // sched[1] >= 32 and sched[2] == 0, (rc, sched)
    np.testing.assert_array_equal(_u32(out), want)
    assert claims[0] > 0, f"the span kernel's tail was never claimed ({sched})"
    del buf
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- the hook itself


def test_grid_changes_on_one_stream(dev, oracle, native, grid, pin):
    """One stream's workspace through 1 group, the device's count and 1 group
    again: a sliced planner batch (more spans than the span kernel has
    streams at the device's grid; its slice starts are sized for the stream
    count, which grows with the grid) and a one-launch batch each time."""
    import torch
    from prismdb_amd import crc32c

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(0x5EED009E)
    n = 2 * 16 * cus + 1001
    lens = rng.integers(0, 5000, size=n).astype(np.int64)
    off = np.concatenate([[7], 7 + np.cumsum(lens + rng.integers(0, 9, size=n))[:-1]]).astype(np.uint64)
    host = oracle.synth(int(off[-1] + lens[-1]) + 64, 0x5EED009F)
    lens = lens.astype(np.uint32)
    want, _ = oracle.batch(host, off, lens, mask=True)
    buf = _dev(host, dev)
    d_off, d_len = _dev(off.astype(np.int64), dev), _dev(lens.view(np.int32), dev)
    stream = torch.cuda.Stream(device=dev)  # a fresh workspace
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for G in (1, 0, 1):
            grid(G)
            pin(0, -1, 0)
            out = _poison_out(n, dev)
            crc32c.batch(buf, d_off, d_len, mask=True, out=out, stream=stream, check_bounds=False)
            rc, sched = _schedule(native)
            assert rc == 0 and sched[1] > 0, (G, rc, sched)  # task-balanced slices
            np.testing.assert_array_equal(_u32(out), want, err_msg=f"planner at grid {G}")
            pin(1 << 17, 0, 1)
            out = _poison_out(500, dev)
            crc32c.batch(buf, d_off[:500], d_len[:500], mask=True, out=out, stream=stream, check_bounds=False)
            assert _split_rc(native) == -2
            np.testing.assert_array_equal(_u32(out), want[:500], err_msg=f"one launch at grid {G}")
    stream.synchronize()


def test_grid_hook_clamps_to_the_device(dev, oracle, native, grid, pin):
    """A grid above the device's CU count is the device's: same results, same
    schedule and claims as at the default.  The hook returns the previous
    value; negative values count as 0."""
    import torch
    from prismdb_amd import crc32c

    assert native.prismdb_crc32c_grid(5) == 0
    assert native.prismdb_crc32c_grid(-3) == 5
    assert native.prismdb_crc32c_grid(0) == 0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = _pair_n(1)
    host, off, lens, want = _pair_plain(n, oracle)
    buf = torch.from_numpy(host).to(dev)
    d_off, d_len = _dev(off.astype(np.int64), dev), _dev(lens.view(np.int32), dev)
    pin(0, -1, 0)
    seen = []
    for g in (0, 10**6):
        grid(g)
        out = _poison_out(n, dev)
        crc32c.batch(buf, d_off, d_len, mask=True, out=out, check_bounds=False)
        rc, sched = _schedule(native)
        assert rc == 0
        seen.append((sched, _claims(native)[0] > 0))
        np.testing.assert_array_equal(_u32(out), want)
    assert native.prismdb_crc32c_grid(0) == 10**6
    assert seen[0] == seen[1] and seen[0][0] == (n, 0, 1), seen
    # the tail's arithmetic at the device's own grid (test_pair_deal_model.py)
    np_, nwaves = (n + 1) // 2, 16 * cus
    m = max(-(-np_ // (31 * nwaves)), min(64, np_ // nwaves), 1)
    K = min(m * nwaves, np_)
    assert seen[0][1] == (np_ // K >= 3 and K > 16 * nwaves), (seen, K, nwaves)

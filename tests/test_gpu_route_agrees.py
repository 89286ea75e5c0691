"""The routing model agrees with what runs (and a released workspace is not read).

tests/test_route_model.py checks prismdb::route::route_of on the host; here
the same hook is asked for a batch's route, the batch is run, and the route
that ran is read back from the last-batch hooks: prismdb_crc32c_last_split
(-2 after a launch of the one-launch kernel -- a window is one -- 0 after a
planner batch), prismdb_crc32c_last_schedule (out[2]: the pair-run kernel was
launched) and prismdb_crc32c_last_fixed_claims (zero after a static fixed
batch, the claims after a claiming one).  Results bit-exact against the
oracle, outputs prefilled with a poison value.

The smallest shapes that cross each switch: a grid of 2 workgroups (one-launch
capacity 64 * 2 * 12 = 1536 spans; the fixed kernel claims from 64 * 4 * 32 =
8192 spans on), prismdb_crc32c_direct_max(1024), spans of 64 bytes.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASK, WRITE_TRAILER, LOG_HEADER = 1, 2, 4
FIXED, ONE_LAUNCH, WINDOWS, CUT, PLANNER = range(5)
FIELDS = ("kind", "claims", "window", "lane", "sliced", "pair", "trailer_pass")
POISON = 0x5A5A5A5A
POISON_MM = 0x7F
G = 2          # workgroups
SPAN = 64      # bytes
SLOT = 80      # 6 B of log-record header room, the span, its 4-byte trailer, padding
NMAX = 2049
FIXED_SWITCH = 64 * 4 * 16 * G


@pytest.fixture(scope="module")
def dev(native):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from prismdb_amd import crc32c

    crc32c.device_init(0)
    assert torch.cuda.get_device_properties(0).multi_processor_count >= G
    native.prismdb_crc32c_grid.restype = ctypes.c_int
    native.prismdb_crc32c_grid.argtypes = [ctypes.c_int]
    native.prismdb_crc32c_fixed_static.restype = None
    native.prismdb_crc32c_fixed_static.argtypes = [ctypes.c_int]
    native.prismdb_crc32c_last_fixed_claims.restype = ctypes.c_int
    native.prismdb_crc32c_last_fixed_claims.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    native.prismdb_crc32c_route.restype = ctypes.c_int
    native.prismdb_crc32c_route.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    return torch.device("cuda", 0)


@pytest.fixture
def small(native, dev):
    """The small grid and one-launch limit; every routing hook at its default afterwards."""
    try:
        native.prismdb_crc32c_grid(G)
        native.prismdb_crc32c_direct_max(1024)
        yield
    finally:
        native.prismdb_crc32c_grid(0)
        native.prismdb_crc32c_direct_max(1 << 17)
        native.prismdb_crc32c_windows(2)
        native.prismdb_crc32c_lane_mode(0)
        native.prismdb_crc32c_force_generic(0)
        native.prismdb_crc32c_fixed_static(0)


def _route(native, n, desc, verify, flags=0, length=0, stride=0):
    res = (ctypes.c_uint64 * 7)()
    assert native.prismdb_crc32c_route(int(desc), int(verify), 1, n, flags, length, stride, 0, G, 0, res) == 0
    return dict(zip(FIELDS, (int(x) for x in res)))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _split_rc(native):
    return native.prismdb_crc32c_last_split((ctypes.c_uint64 * 4)())


def _ran_as(native, r):
    """The route that ran, from the last-batch hooks, is the model's r."""
    if r["kind"] == FIXED:
        c = ctypes.c_uint64(0)
        assert native.prismdb_crc32c_last_fixed_claims(ctypes.byref(c)) == 0
        assert (c.value != 0) == bool(r["claims"]), (r, c.value)
    elif r["kind"] in (ONE_LAUNCH, WINDOWS):
        assert _split_rc(native) == -2, r
    else:
        assert r["kind"] == PLANNER, r
        assert _split_rc(native) == 0, r
        sched = (ctypes.c_uint64 * 3)()
        assert native.prismdb_crc32c_last_schedule(sched) == 0
        assert int(sched[2]) == r["pair"], (r, list(sched))


@pytest.fixture(scope="module")
def spans(oracle, dev):
    """NMAX 64-byte spans, one per 80-byte slot, each with its masked crc both
    behind it (a block trailer) and 6 bytes before it (a log-record header);
    every 97th span damaged after that.  A prefix serves every smaller batch."""
    import torch

    off = (8 + SLOT * np.arange(NMAX)).astype(np.uint64)
    lens = np.full(NMAX, SPAN, dtype=np.uint32)
    host = np.array(oracle.synth(NMAX * SLOT + 16, 0x5EED0801))
    masked, _ = oracle.batch(host, off, lens, mask=True)
    stored = masked.astype("<u4").view(np.uint8).reshape(NMAX, 4)
    for at in (off.astype(np.int64) + SPAN, off.astype(np.int64) - 6):
        host[at[:, None] + np.arange(4)[None, :]] = stored
    bad = np.zeros(NMAX, dtype=np.uint8)
    bad[5::97] = 1
    host[off.astype(np.int64)[bad == 1] + 17] ^= 0x20
    raw, mm = oracle.batch(host, off, lens, verify=True)
    assert (mm == bad).all()
    return {"raw": raw, "bad": bad, "buf": torch.from_numpy(host).to(dev),
            "off": torch.from_numpy(off.astype(np.int64)).to(dev),
            "len": torch.from_numpy(lens.view(np.int32)).to(dev)}


DESC_CASES = [  # (n, verify, log_header, the route)
    (1024, False, False, ONE_LAUNCH),  # n <= direct_max
    (1025, False, False, PLANNER),     # a plain batch above it
    (1025, True, False, ONE_LAUNCH),   # a verifying batch, up to the capacity
    (1536, True, False, ONE_LAUNCH),
    (1537, True, False, WINDOWS),      # up to two windows
    (2048, True, False, WINDOWS),
    (2049, True, False, PLANNER),
    (1100, True, True, PLANNER),       # log records: the planner, lane kernel first
]


@pytest.mark.parametrize("n,verify,log_header,kind", DESC_CASES)
def test_descriptor_batch_runs_the_modelled_route(dev, native, small, spans, n, verify, log_header, kind):
    import torch
    from prismdb_amd import crc32c

    r = _route(native, n, True, verify, LOG_HEADER if log_header else 0)
    assert r["kind"] == kind and r["lane"] == int(log_header) and r["pair"] == 0, r
    if kind == WINDOWS:
        assert r["window"] == 1024
    out = torch.full((n,), POISON, dtype=torch.int32, device=dev)
    mm = torch.full((n,), POISON_MM, dtype=torch.uint8, device=dev) if verify else None
    crc32c.batch(spans["buf"], spans["off"][:n], spans["len"][:n], verify=verify, log_header=log_header, out=out,
                 mismatch=mm)
    _ran_as(native, r)
    np.testing.assert_array_equal(_u32(out), spans["raw"][:n])
    if verify:
        np.testing.assert_array_equal(mm.cpu().numpy(), spans["bad"][:n])


@pytest.fixture(scope="module")
def blocks(oracle, dev):
    import torch

    host = np.array(oracle.synth(FIXED_SWITCH * SPAN + 16, 0x5EED0802))
    return {"want": oracle.batch_fixed(host, SPAN, SPAN, FIXED_SWITCH, init=7, mask=True),
            "buf": torch.from_numpy(host).to(dev)}


def _run_fixed(dev, blocks, n, stream=None):
    import torch
    from prismdb_amd import crc32c

    out = torch.full((n,), POISON, dtype=torch.int32, device=dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # (the poison fill)
    crc32c.batch_fixed(blocks["buf"], SPAN, SPAN, n, 7, mask=True, out=out, stream=stream)
    return out


@pytest.mark.parametrize("n,claims", [(FIXED_SWITCH - 1, 0), (FIXED_SWITCH, 1)])
def test_fixed_batch_runs_the_modelled_route(dev, native, small, blocks, n, claims):
    r = _route(native, n, False, False, MASK, SPAN, SPAN)
    assert (r["kind"], r["claims"]) == (FIXED, claims), r
    out = _run_fixed(dev, blocks, n)
    _ran_as(native, r)
    np.testing.assert_array_equal(_u32(out), blocks["want"][:n])
    assert _split_rc(native) == -1  # the last batch was no descriptor batch


def test_last_fixed_claims_after_its_workspace_is_released(dev, native, small, blocks, spans):
    """A claiming fixed batch on a stream of this thread, then batches on 8
    (kMaxWorkspaces) further streams: the first stream's workspace -- its
    counter blocks -- is evicted and freed.  The hook then answers -1 and
    reads nothing on the device (before the last-batch record was one record
    that a release clears, it copied from the freed block)."""
    import torch
    from prismdb_amd import crc32c

    first = torch.cuda.Stream()
    out = _run_fixed(dev, blocks, FIXED_SWITCH, stream=first)
    c = ctypes.c_uint64(0)
    assert native.prismdb_crc32c_last_fixed_claims(ctypes.byref(c)) == 0 and c.value > 0
    np.testing.assert_array_equal(_u32(out), blocks["want"])
    others = [torch.cuda.Stream() for _ in range(8)]
    outs = [crc32c.batch(spans["buf"], spans["off"][:100], spans["len"][:100], stream=s)[0] for s in others]
    c = ctypes.c_uint64(POISON)
    assert native.prismdb_crc32c_last_fixed_claims(ctypes.byref(c)) == -1
    assert c.value == 0
    torch.cuda.synchronize()
    for o in outs:
        np.testing.assert_array_equal(_u32(o), spans["raw"][:100])

"""The batch routing rule on the host (CPU).

Every device batch goes through RunBatch (crc32c_capi.hip), which switches on
prismdb::route::route_of (crc32c_route.h): the fixed-stride kernel (static or
claiming), the one-launch kernel, windows of it, the 2^30 cut, or the planner
(with its lane / sliced / pair / trailer_pass choices).  The hook
prismdb_crc32c_route calls that very function on the host (no HIP call) under
the current settings of the routing hooks, so the rule is checked here at any
grid; tests/test_gpu_route_agrees.py binds it to what runs.

Every expectation is read off the dispatcher this rule was lifted out of
(RunBatch in crc32c_capi.hip at 4564324, "L<n>" below: its line numbers there).
"""
import ctypes

import pytest

MASK, WRITE_TRAILER, LOG_HEADER = 1, 2, 4
FIXED, ONE_LAUNCH, WINDOWS, CUT, PLANNER = range(5)
AUTO, FORCE_DIRECT, FORCE_PLANNER = 0, 1, 2
FIELDS = ("kind", "claims", "window", "lane", "sliced", "pair", "trailer_pass")


@pytest.fixture
def route(native):
    """route(...): the Route of a batch, as a dict; the routing hooks at their
    defaults before and after."""
    native.prismdb_crc32c_route.restype = ctypes.c_int
    native.prismdb_crc32c_route.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    native.prismdb_crc32c_fixed_static.restype = None
    native.prismdb_crc32c_fixed_static.argtypes = [ctypes.c_int]
    assert native.prismdb_test_hooks_enabled() == 1

    def defaults():
        native.prismdb_crc32c_force_generic(0)
        native.prismdb_crc32c_fixed_static(0)
        native.prismdb_crc32c_lane_mode(0)
        native.prismdb_crc32c_direct_max(1 << 17)
        native.prismdb_crc32c_windows(2)

    def get(n, desc=True, verify=False, out=True, flags=0, length=0, stride=0, base=0, groups=256, forced=AUTO):
        res = (ctypes.c_uint64 * 7)()
        assert native.prismdb_crc32c_route(int(desc), int(verify), int(out), n, flags, length, stride, base, groups,
                                           forced, res) == 0
        return dict(zip(FIELDS, (int(x) for x in res)))

    defaults()
    try:
        yield get
    finally:
        defaults()


def fixed(route, n, length=4096, stride=4096, **kw):
    return route(n, desc=False, length=length, stride=stride, **kw)


def test_hook_rejects_what_no_batch_has(route, native):
    res = (ctypes.c_uint64 * 7)()
    assert native.prismdb_crc32c_route(1, 0, 1, 0, 0, 0, 0, 0, 256, 0, res) == -1   # n = 0: the entry points return first
    assert native.prismdb_crc32c_route(1, 0, 1, 10, 0, 0, 0, 0, 0, 0, res) == -1    # no grid
    assert native.prismdb_crc32c_route(1, 0, 1, 10, 0, 0, 0, 0, 256, 3, res) == -1  # no such imposed route


# ---- default knobs, 256 groups, fixed stride (L629-634: the fixed route's test; L641-642: its claims)


def test_fixed_bulk_batch_claims(route):
    assert fixed(route, 1 << 24) == dict(kind=FIXED, claims=1, window=0, lane=0, sliced=0, pair=0, trailer_pass=0)


def test_fixed_small_batch_is_static(route):
    r = fixed(route, 1000)  # L641: fixed_claims needs n >= 4096 * groups
    assert (r["kind"], r["claims"]) == (FIXED, 0)


def test_fixed_verify_limits(route):
    """L629-630: verify takes at most 4092 bytes, and no multiple of 256."""
    assert fixed(route, 1000, 3988, 3992, verify=True)["kind"] == FIXED
    assert fixed(route, 1000, 4092 - 4, 4096, verify=True)["kind"] == FIXED
    assert fixed(route, 1000, 4096, 4100, verify=True)["kind"] == PLANNER
    assert fixed(route, 1000, 3840, 3844, verify=True)["kind"] == PLANNER
    assert fixed(route, 1000, 3840, 3844)["kind"] == FIXED  # (the limit is verify's alone)


@pytest.mark.parametrize("kw", [dict(length=4098, stride=4100),    # L632: len <= 4096, a multiple of 4
                                dict(length=4096, stride=4097),    # L633: stride & 3
                                dict(base=2),                      # L633: base & 3
                                dict(out=False),                   # L630: verify || out
                                dict(length=0, stride=4096),       # L632: len >= 4
                                dict(flags=LOG_HEADER)])           # L631
def test_fixed_stride_batches_the_fixed_kernel_does_not_take(route, kw):
    r = fixed(route, 100000, **kw)
    assert (r["kind"], r["lane"], r["pair"], r["trailer_pass"]) == (PLANNER, 0, 0, 0), r
    assert r["sliced"] == 1  # L839: 100000 > 2 * 256 * 16 streams


def test_fixed_stride_seal_takes_the_trailer_pass(route):
    r = fixed(route, 100000, flags=MASK | WRITE_TRAILER)  # L631; L785: WRITE_TRAILER && !lane
    assert (r["kind"], r["trailer_pass"], r["lane"]) == (PLANNER, 1, 0)


def test_planner_small_batch_is_not_sliced(route):
    assert fixed(route, 1000, 4098, 4100)["sliced"] == 0  # L839, L755: n <= 2 * 256 * 16
    assert fixed(route, 8192, 4098, 4100)["sliced"] == 0
    assert fixed(route, 8193, 4098, 4100)["sliced"] == 1


# ---- default knobs, 256 groups, descriptors (L698-704 one launch; L724-727 windows; L729 cut; L749-750 lane;
# ---- L869-870 pair)


def test_plain_descriptor_batches(route):
    assert route(131072)["kind"] == ONE_LAUNCH  # L702: n <= g_direct_max
    r = route(131073)
    assert (r["kind"], r["sliced"], r["pair"]) == (PLANNER, 1, 0)  # L726: plain batches take no windows at wmode 2
    r = route(1 << 18)
    assert (r["kind"], r["pair"], r["lane"]) == (PLANNER, 1, 0)  # L869: n >= kPairMinSpans


def test_verify_descriptor_batches(route):
    assert route(196608, verify=True)["kind"] == ONE_LAUNCH  # L700: sst_batch, up to kDirectMaxSpans (L703)
    assert route(196608, out=False, flags=MASK | WRITE_TRAILER)["kind"] == ONE_LAUNCH
    r = route(196609, verify=True)
    assert (r["kind"], r["window"]) == (WINDOWS, 131072)  # L726: n <= 2 * wmax && block_trailers
    assert route(262144, verify=True)["kind"] == WINDOWS
    r = route(262145, verify=True)
    assert (r["kind"], r["pair"]) == (PLANNER, 1)


def test_log_record_batches(route):
    r = route(200000, verify=True, flags=LOG_HEADER)  # L700, L726: no LOG_HEADER batch by shape; L750 lane; L869 no pair
    assert (r["kind"], r["lane"], r["pair"], r["sliced"]) == (PLANNER, 1, 0, 1)
    r = route(300000, verify=True, flags=LOG_HEADER)
    assert (r["kind"], r["lane"], r["pair"]) == (PLANNER, 1, 0)
    r = route(200000, out=False, flags=LOG_HEADER | WRITE_TRAILER | MASK)
    assert (r["kind"], r["lane"], r["trailer_pass"]) == (PLANNER, 1, 0)  # L785: the lane kernel seals itself
    assert route(1000, flags=LOG_HEADER)["kind"] == ONE_LAUNCH  # L702: by size


def test_cut_above_2_30_spans(route):
    assert route((1 << 30) + 1)["kind"] == CUT  # L729
    assert route(1 << 30)["kind"] == PLANNER
    assert fixed(route, (1 << 30) + 1, 4098, 4100)["kind"] == CUT
    assert fixed(route, (1 << 30) + 1)["kind"] == FIXED  # (L630 comes first: the fixed kernel takes any n)
    r = route(1 << 30, forced=FORCE_PLANNER)  # L742: a piece of a cut batch
    assert (r["kind"], r["pair"]) == (PLANNER, 1)


# ---- a small grid: 8 groups, one-launch capacity 64 * 8 * 12 = 6144 (L704)


def test_one_launch_capacity_at_8_groups(route):
    assert route(6144, groups=8)["kind"] == ONE_LAUNCH
    assert route(6145, groups=8)["kind"] == PLANNER  # (not windows: n <= wmax, L725)
    assert route(6144, groups=8, verify=True)["kind"] == ONE_LAUNCH
    assert route(6145, groups=8, verify=True)["kind"] == PLANNER
    r = route(131073, groups=8, verify=True)
    assert (r["kind"], r["window"]) == (WINDOWS, 6144)  # L584-585: the window size, clamped to the capacity


def test_imposed_routes(route):
    """L701: an imposed route is no size question; above the capacity it falls
    to the planner (L703-704), never to windows (L725: kRouteAuto only)."""
    assert route(3, forced=FORCE_DIRECT)["kind"] == ONE_LAUNCH
    assert route(3, forced=FORCE_PLANNER)["kind"] == PLANNER
    assert route(150000, forced=FORCE_DIRECT)["kind"] == ONE_LAUNCH
    assert route(196609, forced=FORCE_DIRECT, verify=True)["kind"] == PLANNER
    assert route(6145, groups=8, forced=FORCE_DIRECT)["kind"] == PLANNER
    assert route(150000, forced=FORCE_PLANNER, verify=True)["kind"] == PLANNER
    assert fixed(route, 1000, forced=FORCE_PLANNER)["kind"] == FIXED  # (L630 does not look at the imposed route)
    assert fixed(route, 1000, 4098, 4100, forced=FORCE_DIRECT)["kind"] == PLANNER  # L701: desc &&


# ---- the knobs


def test_direct_max_0_needs_windows_0_to_pin_the_planner(route, native):
    native.prismdb_crc32c_direct_max(0)
    assert route(100, verify=True)["kind"] == ONE_LAUNCH  # L700-702: sst_batch does not ask g_direct_max
    assert route(100)["kind"] == PLANNER
    native.prismdb_crc32c_windows(0)
    assert route(100, verify=True)["kind"] == PLANNER
    assert route(300000, verify=True)["kind"] == PLANNER  # L725: wmax > 0


def test_windows_1_takes_plain_batches_at_any_size(route, native):
    native.prismdb_crc32c_windows(1)
    r = route(300000)
    assert (r["kind"], r["window"]) == (WINDOWS, 131072)  # L726: wmode == 1
    assert route(300000, flags=LOG_HEADER)["kind"] == PLANNER
    assert route(150000, verify=True)["kind"] == WINDOWS  # L700: sst_batch is wmode 2's alone
    native.prismdb_crc32c_direct_max(1000)
    assert route(150000)["window"] == 1000


def test_windows_0_sends_bulk_batches_to_the_planner(route, native):
    native.prismdb_crc32c_windows(0)
    assert route(196608, verify=True)["kind"] == PLANNER
    assert route(131072, verify=True)["kind"] == ONE_LAUNCH


def test_lane_mode(route, native):
    native.prismdb_crc32c_direct_max(0)
    native.prismdb_crc32c_windows(0)
    native.prismdb_crc32c_lane_mode(1)  # L750: every descriptor batch; not a fixed-stride one (desc &&)
    assert route(1 << 18)["lane"] == 1 and route(1 << 18)["pair"] == 0
    assert fixed(route, 1 << 18, 4098, 4100)["lane"] == 0
    assert route(1000, flags=WRITE_TRAILER)["trailer_pass"] == 0
    native.prismdb_crc32c_lane_mode(-1)
    r = route(1 << 18, flags=LOG_HEADER)
    assert (r["lane"], r["pair"]) == (0, 0)  # L870: no pair on log records
    assert route(1000, flags=LOG_HEADER | WRITE_TRAILER)["trailer_pass"] == 1


def test_force_generic_and_fixed_static(route, native):
    native.prismdb_crc32c_fixed_static(1)
    assert fixed(route, 1 << 24) == dict(kind=FIXED, claims=0, window=0, lane=0, sliced=0, pair=0, trailer_pass=0)
    native.prismdb_crc32c_fixed_static(0)
    native.prismdb_crc32c_force_generic(1)
    r = fixed(route, 1 << 24)  # L634
    assert (r["kind"], r["lane"], r["sliced"], r["pair"]) == (PLANNER, 0, 1, 1)


@pytest.mark.parametrize("G", range(1, 321))
def test_fixed_claims_at_every_grid(route, G):
    """L641: claims exactly when dev::fixed_claims says so -- four full runs of
    64 spans for each of the grid's 16 G waves -- and (n >> 37) == 0."""
    switch = 64 * 4 * 16 * G
    for n in (1, switch - 1, switch, switch + 1, 10 * switch + 63, (1 << 37) - 1, 1 << 37, (1 << 40) + 5):
        r = fixed(route, n, groups=G)
        want = (n >> 6) >= 4 * 16 * G and n < (1 << 37)
        assert (r["kind"], r["claims"]) == (FIXED, int(want)), (G, n, r)

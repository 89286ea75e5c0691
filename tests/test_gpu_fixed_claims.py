"""The fixed-stride kernel's claimed runs (crc32c_fixed_kernel, fixed_deal).

A bulk fixed batch -- at least four full runs of 64 spans for every wave,
n >= 4096 * groups -- claims its runs on demand from the stream workspace's
counters; smaller ones keep the static deal.  Checked here bit-exact against
the oracle at the grids where the counter count changes, at sizes around the
switch, with every output prefilled with a poison value (an unwritten or a
doubly claimed run shows), and against the static deal pinned by the hook
prismdb_crc32c_fixed_static.  With no static share (kFixedStaticEighths = 0)
a claiming batch claims every run, so "one claimed run" and "fewer claimed
runs than counters" cannot occur: the nearest cases are the sizes at the
switch, where each wave claims four runs and fails once.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
POISON_MM = 0x7F
WAVES = 16  # per workgroup


@pytest.fixture(scope="module")
def dev(native):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from prismdb_amd import crc32c

    crc32c.device_init(0)
    native.prismdb_crc32c_grid.restype = ctypes.c_int
    native.prismdb_crc32c_grid.argtypes = [ctypes.c_int]
    native.prismdb_crc32c_fixed_static.restype = None
    native.prismdb_crc32c_fixed_static.argtypes = [ctypes.c_int]
    native.prismdb_crc32c_last_fixed_claims.restype = ctypes.c_int
    native.prismdb_crc32c_last_fixed_claims.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    return torch.device("cuda", 0)


@pytest.fixture
def grid(native, dev):
    try:
        yield lambda g: native.prismdb_crc32c_grid(g)
    finally:
        native.prismdb_crc32c_grid(0)
        native.prismdb_crc32c_fixed_static(0)


def _groups(g):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus if g == 0 or g > cus else g


def _switch(g):
    """The smallest n that claims on a grid of g groups."""
    return 64 * 4 * WAVES * _groups(g)


def _claims(native):
    c = ctypes.c_uint64(0)
    assert native.prismdb_crc32c_last_fixed_claims(ctypes.byref(c)) == 0
    return int(c.value)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class Case:
    """One geometry's bytes on host and device, and the oracle's results for
    its largest batch (a prefix serves every smaller one)."""

    def __init__(self, oracle, dev, stride, length, nmax, seed, init=0, mask=False, trailers=False):
        import torch

        self.stride, self.length, self.init, self.mask = stride, length, init, mask
        self.host = np.array(oracle.synth(nmax * stride + 16, seed))
        self.want = oracle.batch_fixed(self.host, stride, length, nmax, init=init, mask=mask)
        if trailers:  # ReadBlock's stored (masked) crcs behind every block
            tr = oracle.batch_fixed(self.host, stride, length, nmax, mask=True).astype("<u4")
            img = self.host[:nmax * stride].reshape(nmax, stride)
            img[:, length:length + 4] = tr.view(np.uint8).reshape(nmax, 4)
        self.buf = torch.from_numpy(self.host).to(dev)
        self.dev = dev

    def run(self, n, verify=False, stream=None):
        import torch
        from prismdb_amd import crc32c

        out = torch.full((n,), POISON, dtype=torch.int32, device=self.dev)
        mm = torch.full((n,), POISON_MM, dtype=torch.uint8, device=self.dev) if verify else None
        crc32c.batch_fixed(self.buf, self.stride, self.length, n, self.init, mask=self.mask, verify=verify, out=out,
                           mismatch=mm, stream=stream)
        return out, mm

    def check(self, native, n, g, verify=False, bad=()):
        """n blocks on the claiming build and on the pinned static deal: both
        equal the oracle, and the claims are there exactly from the switch on."""
        native.prismdb_crc32c_fixed_static(0)
        out, mm = self.run(n, verify)
        claims = _claims(native)
        got = _u32(out)
        assert (got == self.want[:n]).all(), (n, g, np.flatnonzero(got != self.want[:n])[:8])
        nwaves = WAVES * _groups(g)
        if n >= _switch(g):
            assert claims == (n + 63) // 64 + nwaves, (n, g, claims)  # every run, and each wave's failed claim
        else:
            assert claims == 0, (n, g, claims)
        native.prismdb_crc32c_fixed_static(1)
        out_s, mm_s = self.run(n, verify)
        assert _claims(native) == 0
        native.prismdb_crc32c_fixed_static(0)
        assert (_u32(out_s) == got).all()
        if verify:
            flags = mm.cpu().numpy()
            assert (flags == mm_s.cpu().numpy()).all()
            want = np.zeros(n, dtype=np.uint8)
            want[list(bad)] = 1
            assert (flags == want).all(), (n, g, np.flatnonzero(flags != want)[:8])


def _sizes(g):
    t = _switch(g)
    # below, at and above the switch; a partial last run (odd n); one more full round and a bit
    return [t - 1, t, t + 1, t + 64 * 5 + 37, t + 64 * WAVES * _groups(g) + 129]


@pytest.mark.parametrize("g,stride,length", [(1, 4096, 4096), (7, 4096, 4096), (9, 4096, 4096), (32, 256, 256),
                                             (64, 256, 256), (0, 4, 4)])
def test_sizes_around_the_switch(dev, oracle, native, grid, g, stride, length):
    grid(g)
    sizes = _sizes(g)
    case = Case(oracle, dev, stride, length, max(sizes), 0x5EED0701 + g)
    for n in [1, 2, 129] + sizes:
        case.check(native, n, g)


def test_init_and_mask(dev, oracle, native, grid):
    grid(1)
    n = _switch(1) + 64 * 7 + 3
    Case(oracle, dev, 4096, 4096, n, 0x5EED0711, init=0x12345678).check(native, n, 1)
    Case(oracle, dev, 4096, 4096, n, 0x5EED0712, mask=True).check(native, n, 1)
    Case(oracle, dev, 4096, 4096, n, 0x5EED0713, init=0xFFFFFFFF, mask=True).check(native, n, 1)


def test_sst_blocks_plain_and_verified(dev, oracle, native, grid):
    """3988-B blocks at stride 3992 on 8 groups (one counter): plain, verified
    clean (the trailer rides in round 0), and with one stored trailer flipped
    in the first run and one in a late run -- exactly those two flags."""
    grid(8)
    sizes = _sizes(8)
    nmax = max(sizes)
    case = Case(oracle, dev, 3992, 3988, nmax, 0x5EED0721, trailers=True)
    for n in sizes:
        case.check(native, n, 8)
        case.check(native, n, 8, verify=True)
    bad = (5, _switch(8) + 64 * 3 + 9)
    for b in bad:
        case.buf[b * 3992 + 3988] ^= 0x40
    case.check(native, nmax, 8, verify=True, bad=bad)
    case.check(native, bad[1], 8, verify=True, bad=bad[:1])  # (a shorter claiming batch: the late one is outside it)


def test_back_to_back_calls(dev, oracle, native, grid):
    """The same batch 20 times on one stream with no synchronisation in
    between: each call's counters were zeroed by the call before it."""
    import torch

    grid(8)
    n = _switch(8) + 64 * 9 + 11
    case = Case(oracle, dev, 256, 256, n, 0x5EED0731)
    outs = [case.run(n)[0] for _ in range(20)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert (_u32(o) == case.want[:n]).all(), k


def test_two_streams_and_a_static_call_between(dev, oracle, native, grid):
    """Two streams alternate claiming calls of different sizes (each stream
    has its own counters), then claiming / small static / claiming on one."""
    import torch

    grid(9)
    t = _switch(9)
    na, nb = t + 64 * 3 + 1, t + 64 * 40 + 17
    case = Case(oracle, dev, 256, 256, nb, 0x5EED0741)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(4):
        outs.append((na, case.run(na, stream=sa)[0]))
        outs.append((nb, case.run(nb, stream=sb)[0]))
    torch.cuda.synchronize()
    for n, o in outs:
        assert (_u32(o) == case.want[:n]).all(), n
    seq = [nb, 1000, na, 2, nb]
    outs = [(n, case.run(n)[0]) for n in seq]
    torch.cuda.synchronize()
    for n, o in outs:
        assert (_u32(o) == case.want[:n]).all(), n

// crc32c_route.h -- which launch sequence a device batch takes: the whole
// routing rule as one pure function of the batch's shape, the grid and the
// test hooks' settings.  Host arithmetic only (no HIP call, no device): the
// dispatcher (crc32c_capi.hip, RunBatch) switches on its result, and the CPU
// suite checks it through the hook prismdb_crc32c_route.
#pragma once

#include <stdint.h>

#include "crc32c_device.h"

namespace prismdb {
namespace route {

// What the rule reads of a batch.
struct Shape {
  bool desc, verify, has_out;  // descriptor batch (else fixed stride); the caller passed a mismatch / an out array
  uint64_t n;        // spans
  uint32_t flags;    // PRISMDB_CRC32C_* (UNORDERED has no part in the rule)
  uint32_t len_c;    // fixed stride: every span's length
  uint64_t stride;   // fixed stride
  uint32_t base_lo;  // the low bits of the base address (its alignment)
};

// The test hooks' settings (crc32c_capi.hip's g_*), read once per batch.
struct Knobs {
  bool force_generic, fixed_static;  // prismdb_crc32c_force_generic, _fixed_static
  int lane_mode;                     // prismdb_crc32c_lane_mode: 0 log-record batches, 1 all, -1 none
  uint64_t direct_max;               // prismdb_crc32c_direct_max
  int windows;                       // prismdb_crc32c_windows: 0, 1 or 2
};

// A route the caller imposes: the self-test runs both descriptor paths, a
// window is one launch of the one-launch kernel, a piece of a cut batch is
// the planner's.
enum Forced { kRouteAuto = 0, kRouteDirect = 1, kRoutePlanner = 2 };

enum Kind { kFixed = 0, kOneLaunch = 1, kWindows = 2, kCut = 3, kPlanner = 4 };

struct Route {
  Kind kind;
  bool claims;      // kFixed: the runs are claimed on demand (the launch takes workspace counters)
  uint64_t window;  // kWindows: spans per window at most
  // kPlanner: the lane kernel runs first, the rest follows through its list;
  // task-balanced slices (the two slice kernels); the pair-run kernel is
  // launched next to the span kernel; WRITE_TRAILER by one pass after them
  bool lane, sliced, pair, trailer_pass;
};

// Spans one launch of the one-launch kernel takes on `groups` workgroups: one
// static run of <= 64 spans per wave (the kernel's own limit, kDirectMaxSpans, holds besides).
inline uint64_t one_launch_capacity(int groups) { return 64ull * (uint64_t)groups * (dev::kDirectThreads / 64); }

// The rule, in the order it is tried:
//
// kFixed.  Fixed stride, 4-byte aligned base and stride, 4..4096-byte
// multiple-of-4 spans with somewhere to put a result, no trailer or log-header
// flag: one kernel (crc32c_fixed_kernel).  Verifying: up to 4092 bytes and
// not a multiple of 256, so that the stored trailer word fits round 0's
// padding lanes.  Whatever route the caller imposes.  A bulk batch (full runs
// for every wave: dev::fixed_claims) claims its runs on demand from the
// stream workspace's counters; smaller ones (one SST file, a pipeline chunk)
// keep the static deal and take no workspace.
//
// kOneLaunch (crc32c_direct.hip).  Descriptor batches of <= direct_max spans
// (2^17), or, by default (windows 2), a batch that seals or verifies block
// trailers (not log records) whatever direct_max says -- the SST-file batches
// the windows below would otherwise cut in two -- up to the kernel's
// capacity.  An imposed one-launch route above the capacity falls to the
// planner, not to windows.
//
// kWindows.  Descriptor batches of more than direct_max spans, log-record
// batches aside: windows of the one-launch kernel (windows 1), the planner
// path (0), or (2, the default) windows up to two of them for batches that
// seal or verify block trailers, the planner path otherwise and beyond.  Two
// windows of SST files (twelve files, 201 744 spans) take 13.4 us per file,
// against 21.6 on the planner path, whose 5-7 launches and segment pass cost
// ~120 us per call; from there on the planner's balance wins, and on mixed
// span sizes it wins at any size (profiles/r04/r04h_bench.json,
// r04h_configs.json).  The one-launch kernel deals each wave a static run
// of consecutive spans, and a group leaves its CU only when its slowest wave
// is done: on spans of mixed sizes the windows lose to the planner's
// task-balanced slices (config-3 mix 65.7 against 74.8 % of the roofline,
// random spans 70.3 against 77.1 %), on uniform SST spans they win (72.8
// against 70.8 %; profiles/r04/r04e_configs.json).  The default's batches
// are TableBuilder / ReadBlock ones, whose spans are block_size-bounded data
// blocks plus one index block per file (uniform: the windows' static runs
// balance them).  A plain checksum batch has no such shape: 200 000 config-3
// spans (1-64 KiB) ran at 57.5 % of the roofline as windows against 70.5 %
// on the planner path (profiles/r06/r06s_configs.json, config3_band).
//
// kCut.  The span kernel indexes records with 32 bits: larger batches go to
// the planner in pieces of kMaxGenericSpans.
//
// kPlanner.  The rest: plan -> span pass -> segment pass -> combine.
//   lane: short spans first, one per lane (crc32c_lane_kernel), for
//     log-record batches (lane_mode 0) or every descriptor batch (1).
//   sliced: task-balanced slices need more records than span streams (two per
//     wave): with n <= the stream count every stream holds at most one record
//     either way, and the two slice kernels' launches are ~9 us of a
//     file-sized call.
//   pair: large sliced batches are offered to the pair-run kernel too (below
//     kPairMinSpans its extra launch costs more than it gains).
//   trailer_pass: sealing, the span kernels leave the trailers to one pass
//     after them (crc32c_trailer_kernel).  Not behind the lane kernel: it
//     stores each log record's header crc as the record finishes, and that
//     measured 5 % faster on ~1 KB WAL records than the pass (3931 against
//     3739 GB/s, profiles/r05/r05g_variants_lane_seal.json) -- a lane's
//     store is one of 64 records' in flight, not a wave-wide stall.
inline Route route_of(const Shape& b, int groups, const Knobs& k, Forced forced) {
  const bool log_header = (b.flags & dev::kFlagLogHeader) != 0;
  const bool seal = (b.flags & dev::kFlagWriteTrailer) != 0;
  const uint32_t max_len = 4u * dev::kChunkWords - (b.verify ? 4u : 0u);
  if (!b.desc && (b.verify || b.has_out) && (!b.verify || (b.len_c & 255u) != 0) && !seal && !log_header &&
      b.len_c >= 4 && b.len_c <= max_len && (b.len_c & 3u) == 0 && (b.stride & 3u) == 0 && (b.base_lo & 3u) == 0 &&
      !k.force_generic)
    return {kFixed, dev::fixed_claims(b.n, (uint32_t)groups) && (b.n >> 37) == 0 && !k.fixed_static};
  const bool block_trailers = b.verify || seal;
  const bool sst_batch = k.windows == 2 && block_trailers && !log_header;
  const bool direct =
      b.desc && (forced == kRouteDirect || (forced == kRouteAuto && (b.n <= k.direct_max || sst_batch)));
  const uint64_t cap = one_launch_capacity(groups);
  if (direct && b.n <= dev::kDirectMaxSpans && b.n <= cap) return {kOneLaunch};
  const uint64_t wmax = k.direct_max;
  if (b.desc && forced == kRouteAuto && wmax > 0 && b.n > wmax &&
      (k.windows == 1 || (k.windows == 2 && b.n <= 2 * wmax && block_trailers)) && !log_header)
    return {kWindows, false, wmax < cap ? wmax : cap};
  if (b.n > dev::kMaxGenericSpans) return {kCut};
  Route r{kPlanner};
  r.lane = b.desc && (k.lane_mode > 0 || (k.lane_mode == 0 && log_header));
  r.sliced = b.n > 2ull * (uint64_t)groups * dev::kWavesPerGroup;
  r.pair = r.sliced && b.n >= dev::kPairMinSpans && !r.lane && !log_header;
  r.trailer_pass = seal && !r.lane;
  return r;
}

}  // namespace route
}  // namespace prismdb

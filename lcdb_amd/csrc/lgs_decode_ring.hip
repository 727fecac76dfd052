// lgs_decode_ring.hip -- the lane-per-block ring decoder, decode_ring_kernel:
// the kernel of the large-batch route until decode_pair_kernel
// (lgs_decode.hip) split its trip between two waves.  PROBE LIBRARY ONLY
// (-DLGS_PROBE_DECODERS): exact, but it loses -- 268.4 against 247 us for C2
// (profiles/r9_*).  Selected with lgs_set_option("decoder",
// "ring32") or LGS_DECODE_KERNEL=ring32; it takes the "ring" route of
// launch_decode and of the split launch's smallest class.
//
// Semantics: lcdb src/util/snappy.c:386-412 and decode_blocks (:201-341).
// The rings' sizes, rrd_tag, out_put and RingJob are shared with the pair
// kernel (lgs_decode_common.h).
#ifndef LGS_PROBE_DECODERS
#error "lgs_decode_ring.hip is built into the probe library only (build.py build_probe)"
#endif
#include "lgs_device.h"
#include "lgs_decode_common.h"
#include "lgs_launch.h"
#include "lgs_probe_hooks.h"

// ---- measurement hooks of this kernel alone (lgs_probe_hooks.h has the ones
// it shares with decode_pair_kernel) -----------------------------------------
// LGS_PROBE_RING_PHASES: lane k < 8 writes phase k's sum, lane 8 the trip
// count, into its block's out_len entry (tools/ring_phases.py).
#ifdef LGS_PROBE_RING_PHASES
#define LGS_RING_PH_VALUE(lane, dflt) lgs_ring_ph_value_(ph_, ph_trips_, (lane), (dflt))
#define LGS_RING_PH_ACTIVE 1
#else
#define LGS_RING_PH_VALUE(lane, dflt) (dflt)
#define LGS_RING_PH_ACTIVE 0
#endif
// LGS_PROBE_TRIPCOUNT: every lane writes its wave's trip count to out_len
// (tools/ring_trips.py).
#ifdef LGS_PROBE_TRIPCOUNT
#define LGS_RING_TRIPS_DECL uint32_t trips_ = 0
#define LGS_RING_TRIP() (++trips_)
#define LGS_RING_OUT_LEN(v) (trips_)
#else
#define LGS_RING_TRIPS_DECL do {} while (0)
#define LGS_RING_TRIP() do {} while (0)
#define LGS_RING_OUT_LEN(v) (v)
#endif

namespace lgs {

// ---------------------------------------------------------------------------
// Ring decoder: lane-per-block with LDS staging (large batches).
//
// The lane kernel above moves every byte as a 16-byte access of its own
// lane, so each memory instruction touches 64 cache lines: on C2 the
// texture addresser is ~93 % busy and partially written lines are evicted
// and rewritten (3.4x the output bytes reach HBM).  Here each lane keeps
//   * an input window: a 128-byte ring of its compressed stream, refilled
//     64 bytes at a time by 4 cooperating lanes (one coalesced line), and
//   * an output ring of 256 bytes, flushed 128 bytes at a time by 8
//     cooperating lanes (whole lines, written once),
// both in LDS with a 64-byte mirror after the ring so that any read of up
// to 64 bytes from a ring offset is linear.  Literals and copies with
// dist <= kNear move LDS to LDS; farther copies read the already flushed
// output from memory, issued when the tag is parsed and used a trip later.
// A trip = one piece (<= 64 bytes) of one op per lane; every memory
// operation issued in a trip is waited for once, at the top of the next.
// TWO (the default): a trip has a second op slot after the flush -- the
// piece of the op just parsed, if its bytes are in LDS, and the tag after
// it -- so a literal and a near copy take one trip instead of two.  The
// ring bounds still hold: the flush leaves < 128 unflushed bytes, each slot
// adds <= 64, and the next trip's first piece starts below 192.  A far copy
// met in the second slot is taken only when its source is flushed already.
// BL: blocks per wave.  With BL = 32 (the default) lanes 32-63 only serve
// the refill and flush jobs; the rings then fit eight waves in a CU's LDS,
// two per SIMD, which overlap each other's once-per-trip memory waits.
// ---------------------------------------------------------------------------
template <bool TWO, uint32_t BL>
__global__ __launch_bounds__(64) void decode_ring_kernel(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
    const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
    const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ out_cap,
    uint32_t* __restrict__ out_len, uint8_t* __restrict__ status,
    const uint32_t* __restrict__ index, uint32_t n,
    const uint32_t* __restrict__ count) {
  using namespace ring;
  // BL lanes decode (BL blocks per wave); with BL < 64 the others only help
  // with refills and flushes.  At most BL lanes post a flush job and at most
  // min(BL, 32) a refill job per trip.
  constexpr uint32_t kJobs = BL > 32 ? BL : 32;
  __shared__ __attribute__((aligned(16))) uint8_t s_in[BL * kInStride];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[BL * kOutStride];
  __shared__ __attribute__((aligned(16))) RingJob s_job[kJobs];

  // Every lane stays to the end: lanes without a block still work for the
  // cooperative refills and flushes.
  const uint32_t lane = threadIdx.x;
  const uint32_t slot = blockIdx.x * BL + lane;
  if (count) n = *count;
  if (blockIdx.x * BL >= n) return;   // a whole wave without blocks
  const bool exists = lane < BL && slot < n;
  const uint32_t i = exists ? (index ? index[slot] : slot) : 0;
  const gptr<const uint8_t> src = to_global(in) + (exists ? in_off[i] : 0);
  const uint32_t slen = exists ? in_len[i] : 0;
  const gptr<uint8_t> dst = to_global(out) + (exists ? out_off[i] : 0);
  const uint32_t cap = exists ? out_cap[i] : 0;
  uint8_t* const ib = s_in + (lane < BL ? lane : 0) * kInStride;     // (helpers: unused)
  // The output ring is shifted by the destination's alignment (dst & 15), so
  // a flush job's 16-byte reads (which end on the destination's line
  // boundaries) are aligned in LDS whatever the slot's alignment: unaligned,
  // they cost 6 % of C2 decode with outputs 1 byte off (303 against 286 us).
  uint8_t* const ob = s_out + (lane < BL ? lane : 0) * kOutStride + 16 +
                      ((uint32_t)reinterpret_cast<uintptr_t>(dst) & 15u);

  // varint32 header, coding.h:169-204.  st: 1 decoding/ok, 0 corrupt,
  // 2 no space, 3 no block.
  uint32_t st = exists ? 1u : 3u, want = 0, hlen = 0;
  if (exists) {
    const uint64_t h = view8(src);
    for (uint32_t k = 0; k < 5 && k < slen; ++k) {
      const uint32_t b = (uint32_t)(h >> (8 * k)) & 0xffu;
      if ((b & 0x80u) == 0) {
        want |= b << (7 * k);
        hlen = k + 1;
        break;
      }
      want |= (b & 0x7fu) << (7 * k);
    }
    if (hlen == 0 || want > 0x7fffffffu) st = 0;                // snappy.c:405-409
    else if (want > cap) st = 2;
  }
  __builtin_amdgcn_s_waitcnt(0x0f70);

  uint32_t pos = hlen;               // next tag (stream offset)
  uint32_t made = 0, F = 0;          // output produced / flushed
  uint32_t in_req = 0, in_have = 0;  // input requested / landed (64-byte units)
  uint32_t orem = 0, okind = 0, odist = 0, olp = 0;   // current op: bytes left, ...
  bool ofar = false;
  u32x4 fa0 = {0, 0, 0, 0}, fa1 = fa0, fa2 = fa0, fa3 = fa0;   // far-copy bytes
  u32x4 rv0 = fa0, rv1 = fa0;                                  // refill bytes (worker)
  // A lane's sink for dropped refill writes: its own slack (helpers share a
  // decoding lane's).
  const uint32_t sink = (lane < BL ? lane : (lane - BL) % BL) * kInStride + kInSink;
  uint32_t ra0 = sink, rm0 = sink, ra1 = sink, rm1 = sink;

  // One piece (<= 64 bytes) of the current op (snappy.c:210-331) for every
  // lane whose bytes are in LDS (literal from the window, copy from the ring).
  auto piece = [&]() {
    const bool lit = okind == 0;
    const uint32_t piece = orem < 64 ? orem : 64;
    // (One condition, one exec-mask region.)
    if ((st == 1) & (orem > 0) & !ofar & (!lit | (in_have >= olp + piece))) {
      {
        const uint32_t dist = odist;
        const bool overlap = !lit & (dist < piece);
        const bool pat = overlap & (dist <= 8) & ((dist & (dist - 1)) == 0);
        if (overlap & !pat) {
          // Period not dividing 16: chunk by chunk, each reading bytes the
          // previous ones wrote (LDS program order); chunk 0 of a period
          // < 16 is built byte by byte, later chunks copy from qq back
          // (qq = a multiple of the period >= 16).
          const uint32_t qq = dist >= 16 ? dist : dist * ((16 + dist - 1) / dist);
          u32x4 p0;
          if (dist >= 16) {
            p0 = lrd16(ob + ((made - dist) & (kOutRing - 1)));
          } else {
            const u32x4 c0 = lrd16(ob + ((made - dist) & (kOutRing - 1)));
            uint32_t w[4] = {0, 0, 0, 0};
            uint32_t r = 0;
  #pragma clang loop unroll(disable)
            for (uint32_t j = 0; j < 16; ++j) {
              w[j >> 2] |= byte_of(c0, r) << (8 * (j & 3u));
              r = r + 1 == dist ? 0 : r + 1;
            }
            p0 = u32x4{w[0], w[1], w[2], w[3]};
          }
          out_put(ob, made, p0);
          order();
  #pragma clang loop unroll(disable)
          for (uint32_t k = 1; 16 * k < piece; ++k) {
            const u32x4 v = lrd16(ob + ((made + 16 * k - qq) & (kOutRing - 1)));
            out_put(ob, made + 16 * k, v);
            order();
          }
        } else {
          // A literal reads the input window, a copy the output ring.
          const uint8_t* sp = lit ? ib + (olp & (kInRing - 1))
                                  : ob + ((made - dist) & (kOutRing - 1));
          const u32x4 c0 = lrd16(sp);
          // Period 1/2/4/8: the dist bytes before d as a 16-byte pattern
          // (byte 0 four times, bytes 0-1 twice: one v_perm each, not a
          // quarter-rate v_mul_lo_u32).
          const uint32_t w1 = __builtin_amdgcn_perm(c0.x, c0.x, 0x00000000u);
          const uint32_t w2 = __builtin_amdgcn_perm(c0.x, c0.x, 0x01000100u);
          const uint32_t px = dist == 1 ? w1 : (dist == 2 ? w2 : c0.x);
          const uint32_t py = dist == 8 ? c0.y : px;
          const u32x4 pv = {px, py, px, py};
          out_put(ob, made, pat ? pv : c0);
          // Later chunks are read only when the piece has them (and not for
          // a pattern).  A source chunk can share ring slots only with a
          // later destination chunk (dist <= 240), so reading chunk k just
          // before writing chunk k keeps every read ahead of its clobber.
          // (All four reads issued before the first write -- legal here, no
          // source chunk holds a byte the piece writes -- is slower: 292-294
          // against 273-275 us on C2, profiles/r5b_ab.txt.  The LDS pipe, not
          // the round trips, is what a piece waits on.)
          if (piece > 16) out_put(ob, made + 16, pat ? pv : lrd16(sp + 16));
          if (piece > 32) out_put(ob, made + 32, pat ? pv : lrd16(sp + 32));
          if (piece > 48) out_put(ob, made + 48, pat ? pv : lrd16(sp + 48));
        }
        made += piece;
        orem -= piece;
        if (lit) olp += piece;
      }
    }
  };


  // Parse the next tag (its bytes are in the window); a far copy's bytes are
  // loaded from the flushed output for the next trip.
  auto parse = [&](bool second) {
    // Computed on every lane and committed with selects: one exec-mask
    // region (the far-copy loads) instead of three nested ones.  Lanes that
    // are not parsing read their own ring (in range) and discard the tag.
    const uint32_t need_to = slen - pos < 5 ? slen : pos + 5;
    const bool ready = (st == 1) & (orem == 0) & (pos < slen) & (in_have >= need_to);
    const Tag t = parse_tag(rrd_tag(ib + (pos & (kInRing - 1))), pos, slen, want, made);
    const bool far = (t.kind != 0) & (t.dist > kNear);
    if (ready & t.bad) st = 0;
    // (A far copy parsed in the second slot must find its source flushed
    // already; otherwise it waits for the next trip's first.)
    const bool take = ready & !t.bad & (!second | !far | (made - F + t.len <= t.dist));
    orem = take ? t.len : orem;
    okind = take ? (t.kind == 0 ? 0u : 1u) : okind;
    odist = take ? t.dist : odist;
    olp = take ? pos + t.hl : olp;
    pos = take ? t.next : pos;
    ofar = take ? far : ofar;
    if (take & far) {
      // The copy's own bytes are flushed already (first slot: they end <=
      // made - kNear + 64 < F; second slot: the take test above).  A granule
      // reads up to 15 bytes past the copy; they lie inside [0, made) of this
      // block (dist > kNear), may be bytes not yet flushed, and are never
      // used (the landing writes only orem bytes' worth that count).
      const gptr<const uint8_t> sp = (gptr<const uint8_t>)(dst + (made - odist));   // 32-bit offset
      fa0 = LGS_RING_FAR_LD16(sp);
      // Only the 16-byte granules the copy has: most far copies are 4-6
      // bytes (a key's shared prefix), and loading all 64 fetched 232 MB for
      // 70 MB used on C2.  Same time, less traffic
      // (profiles/r5b_ab.txt).
      if (t.len > 16) {
        fa1 = LGS_RING_FAR_LD16(sp + 16);
        if (t.len > 32) {
          fa2 = LGS_RING_FAR_LD16(sp + 32);
          if (t.len > 48) fa3 = LGS_RING_FAR_LD16(sp + 48);
        }
      }
    }
  };

  // Rotated: the loop's test is its last step (a test at the top became a
  // selector variable and a bool round trip through a VGPR).  A trip with no
  // active lane (every block's header corrupt) does nothing.
  LGS_RING_TRIPS_DECL;
  LGS_RING_PH_DECL;
  do {
    LGS_RING_TRIP();
    LGS_RING_PH_TRIP();
    LGS_RING_PH(7);                    // (the loop test, from the last trip)

    // ---- one piece of the current op for every lane whose bytes are in LDS;
    // this runs before the wait, so last trip's loads land meanwhile.
    piece();
    order();
    LGS_RING_PH(0);

    // ---- everything issued last trip has landed: far-copy pieces (never
    // overlapping, <= 64 bytes), then the input refills.
    __builtin_amdgcn_s_waitcnt(0x0f70);                         // vmcnt(0)
    LGS_RING_PH(1);
    if ((st == 1) & (orem > 0) & ofar) {
      out_put(ob, made, fa0);
      if (orem > 16) out_put(ob, made + 16, fa1);
      if (orem > 32) out_put(ob, made + 32, fa2);
      if (orem > 48) out_put(ob, made + 48, fa3);
      made += orem;
      orem = 0;
      ofar = false;
    }
    // (Lanes without a refill chunk, or a chunk without a mirror copy, hold
    // the sink: they skip the write.)
    if (ra0 != sink) lwr16(s_in + ra0, rv0);
    if (rm0 != sink) lwr16(s_in + rm0, rv0);
    if (ra1 != sink) lwr16(s_in + ra1, rv1);
    if (rm1 != sink) lwr16(s_in + rm1, rv1);
    order();
    in_have = in_req;
    LGS_RING_PH(2);

    // ---- flush finished bytes; the block's last ones once the stream is
    // consumed (snappy.c:337: it must end exactly at want).
    if ((st == 1) & (orem == 0) & (pos >= slen) & (made != want)) st = 0;
    const bool fin = (st == 1) & (orem == 0) & (pos >= slen);
    // Flush whole 128-byte lines of the destination: up to the last line
    // boundary at or below dst + made, so every interior line is written by
    // one job, once (a block's first and last lines are shared with its
    // neighbours), then the tail after the last boundary once the block is
    // finished.  A trip makes <= 128 bytes and F sits on a boundary (or at
    // the block's start, before its first one), so a job is <= 128 bytes
    // and D = made - F < 128 after the flush.
    const uint64_t dpa = reinterpret_cast<uint64_t>(dst);
    const uint64_t lb = (dpa + made) & ~(uint64_t)(kFlush - 1);
    const uint32_t lim = lb > dpa ? (uint32_t)(lb - dpa) : 0u;
    const uint32_t fcnt = lim > F ? lim - F : (fin ? made - F : 0u);
    {
      const bool need = (st == 1) & (fcnt > 0);
      const uint64_t m = ballot(need);
      const uint32_t j = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
      const uint32_t total = uni((uint32_t)__builtin_popcountll(m));
      if (need) {
        const uint64_t dp = reinterpret_cast<uint64_t>(dst);
        s_job[j] = RingJob(lane, F, fcnt, dp);
      }
      order();
      // 4 lanes a job, 32 bytes each (bytes 16w.. and 64 + 16w..): 16 jobs
      // per round, so a trip's flush is one round of two LDS round trips
      // (a job record, then the ring) whenever at most 16 blocks flush.
      // (8 lanes a job, 8 jobs a round: 274 against 268 us on C2,
      // profiles/r5e_ab.txt.)
#pragma clang loop unroll(disable)
      for (uint32_t base = 0; base < total; base += 16) {
        const uint32_t jj = base + (lane >> 2), w = lane & 3u;
        // jj < base + 16 <= kJobs: the record is in range (stale past total).
        const RingJob jb = s_job[jj];
        if ((jj < total) & (16 * w < jb.cnt)) {
          const uint8_t* rb = s_out + (jb.lane() & (BL - 1)) * kOutStride + 16 +
                              ((uint32_t)jb.ptr() & 15u);
          const u32x4 v0 = lrd16(rb + ((jb.off + 16 * w) & (kOutRing - 1)));
          const bool two = 64 + 16 * w < jb.cnt;
          u32x4 v1 = v0;
          if (two) v1 = lrd16(rb + ((jb.off + 64 + 16 * w) & (kOutRing - 1)));
          const gptr<uint8_t> g = (gptr<uint8_t>)jb.ptr() + jb.off + 16 * w;
          LGS_RING_FLUSH_ST(g, v0, jb.cnt - 16 * w);
          if (two) LGS_RING_FLUSH_ST(g + 64, v1, jb.cnt - 64 - 16 * w);
        }
      }
      order();
      if (need) F += fcnt;
    }
    LGS_RING_PH(3);

    // ---- parse the next tag.  TWO: then a second op slot -- its piece, if
    // its bytes are in LDS, and the tag after it.
    parse(false);
    LGS_RING_PH(4);
    if (TWO) {
      order();
      piece();
      order();
      parse(true);
    }
    LGS_RING_PH(5);

    // ---- refill requests: the next 64 input bytes, once the 64 they
    // overwrite in the ring are consumed.
    // 4 lanes per request, <= 32 a trip.  (Each lane loading its own
    // block's 64 bytes instead: the same time, profiles/r5f_ab.txt.)
    {
      const uint32_t cons = ((orem > 0) & (okind == 0)) ? olp : pos;
      const bool need = (st == 1) & (in_req < slen) & (in_req <= cons + 64);
      const uint64_t m = ballot(need);
      const uint32_t j = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
      const uint32_t total = uni((uint32_t)__builtin_popcountll(m));
      if (need & (j < 32)) {
        const uint64_t sp = reinterpret_cast<uint64_t>(src);
        s_job[j] = RingJob(lane, in_req, slen, sp);
      }
      order();
      ra0 = rm0 = ra1 = rm1 = sink;
      const uint32_t w = lane & 3u;
      if ((lane >> 2) < total) {
        const RingJob jb = s_job[lane >> 2];
        const uint32_t o = jb.off + 16 * w;
        const gptr<const uint8_t> g = (gptr<const uint8_t>)jb.ptr();
        // (A granule past the stream reloads its first: never consumed.)
        rv0 = ld16(g + (o < jb.cnt ? o : 0u));
        const uint32_t r = o & (kInRing - 1);
        ra0 = jb.lane() * kInStride + r;
        rm0 = r < 64 ? ra0 + kInRing : sink;
      }
      if (16 + (lane >> 2) < total) {
        const RingJob jb = s_job[16 + (lane >> 2)];
        const uint32_t o = jb.off + 16 * w;
        const gptr<const uint8_t> g = (gptr<const uint8_t>)jb.ptr();
        rv1 = ld16(g + (o < jb.cnt ? o : 0u));
        const uint32_t r = o & (kInRing - 1);
        ra1 = jb.lane() * kInStride + r;
        rm1 = r < 64 ? ra1 + kInRing : sink;
      }
      order();
      if (need & (j < 32)) in_req += 64;
    }
    LGS_RING_PH(6);
  } while (ballot(st == 1) & ~(ballot(orem == 0) & ballot(pos >= slen) & ballot(F >= made)));

  if (exists) {
    status[i] = (uint8_t)st;
    out_len[i] = LGS_RING_PH_VALUE(lane, LGS_RING_OUT_LEN(st == 1 ? want : 0));
  }
}

hipError_t launch_decode_ring32(const DecodeArgs& a, hipStream_t s) {
  // Two op slots per trip, 32 blocks per wave: the rings for 32 lanes take
  // 20 KB of LDS, so eight waves fit a CU, two per SIMD, and each hides the
  // other's memory waits.  (64 blocks per wave: 746 -> 709 GiB/s on C2; one
  // op slot: 632.  Those variants were removed in round 2.)
#ifndef LGS_RING_BL
#define LGS_RING_BL 32
#endif
  hipLaunchKernelGGL((decode_ring_kernel<true, LGS_RING_BL>), dim3((a.n + LGS_RING_BL - 1) / LGS_RING_BL), dim3(64), 0, s, a.in,
                     a.in_off, a.in_len, a.out, a.out_off, a.out_cap, a.out_len, a.status,
                     a.index, a.n, a.count);
  return hipGetLastError();
}

}  // namespace lgs

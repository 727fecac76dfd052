// lgs_probe_hooks.h -- measurement hooks of the codec kernels, one macro per
// site.  The product library defines no LGS_PROBE_* macro, so every hook
// below expands to nothing there; probe builds (tools/mk_variants.sh with
// -DLGS_PROBE_..., never loaded by lcdb or bench.py) turn one family on.
//
//   LGS_PROBE_RING_PHASES  decode_pair_kernel: shader-clock cycles per trip
//                          phase of each role, summed per wave
//                          (tools/ring_phases.py)
//   LGS_PROBE_NOFAR / NOFLUSH  decode_pair_kernel: drop the far-copy loads /
//                          the flush stores (same control flow; traffic
//                          calibration)
//   LGS_PROBE_DEC_TIMING   decode_kernel: staging, walk and flush cycles
//                          (tools/dec_phases.py)
//   LGS_PROBE_FORCE_REPLAY / ENC_TIMING  encode_kernel (tools/enc_phases.py)
//   LGS_PROBE_ENC_GENERAL_ROUND  encode_pass: the general batch after every
//                          copy, as before round 13
//
// decode_ring_kernel, the kernel decode_pair_kernel replaced, is in the probe
// library only (lgs_decode_ring.hip: a probe build needs -DLGS_PROBE_DECODERS
// and the probe sources of build.PROBE_SOURCES to run it, selected with
// "ring32").  It uses the RING_PH stamps and the traffic-calibration hooks
// below too; the hooks it alone uses (its out_len values under
// LGS_PROBE_RING_PHASES, and LGS_PROBE_TRIPCOUNT) are defined in its source.
#pragma once

#include <stdint.h>

// ---- trip phases: the stamps (decode_pair_kernel through the LGS_PAIR_PH
// aliases below, decode_ring_kernel directly) --------------------------------
// RING_PH_DECL at the kernel's start, RING_PH(k) at the end of phase k
// (adds the cycles since the previous stamp to phase k), RING_PH_TRIP() once
// a trip; lgs_ring_ph_value_ is what a lane writes at the end: lane k < 8
// phase k's sum, lane 8 the trip count.
#ifdef LGS_PROBE_RING_PHASES
#define LGS_RING_PH_DECL                                   \
  uint32_t ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0};               \
  uint32_t ph_trips_ = 0;                                   \
  uint64_t ph_t_ = __builtin_amdgcn_s_memtime()
#define LGS_RING_PH(k)                                     \
  do {                                                     \
    const uint64_t t_ = __builtin_amdgcn_s_memtime();      \
    ph_[k] += (uint32_t)(t_ - ph_t_);                      \
    ph_t_ = t_;                                            \
  } while (0)
#define LGS_RING_PH_TRIP() (++ph_trips_)
__device__ __forceinline__ uint32_t lgs_ring_ph_value_(const uint32_t* ph, uint32_t trips,
                                                       uint32_t lane, uint32_t dflt) {
  uint32_t v = lane == 8 ? trips : dflt;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) v = lane == k ? ph[k] : v;   // selects, no dynamic index
  return v;
}
#else
#define LGS_RING_PH_DECL do {} while (0)
#define LGS_RING_PH(k) do {} while (0)
#define LGS_RING_PH_TRIP() do {} while (0)
#endif

// ---- decode_pair_kernel trip phases (the same probe build) ----------------
// Both roles stamp their own phases 0-4 and 7 (the barrier and loop test).
// At the end the mover's lanes 0-8 write its sums and trip count into their
// blocks' out_len entries, the walker's lanes 16-24 its own, after a barrier
// behind the mover's drained stores (both waves execute PAIR_PH_END_*).
// Lane 9 of the mover and lane 25 of the walker write where their wave ran
// (lgs_hw_where_: HW_ID bits 15:0 -- wave slot 3:0, SIMD 5:4, pipe 7:6, CU
// 11:8, SH 12, SE 15:13 -- and the XCC id in bits 19:16), so
// tools/ring_phases.py can set a workgroup's life against what shared its
// mover's SIMD.
#ifdef LGS_PROBE_RING_PHASES
__device__ __forceinline__ uint32_t lgs_hw_where_() {
  // s_getreg_b32 immediates: register | offset << 6 | (size - 1) << 11;
  // HW_REG_HW_ID is register 4, HW_REG_XCC_ID register 20 (gfx942 / gfx950).
  const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11));
  const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));
  return hw | (xcc << 16);
}
#define LGS_PAIR_PH_DECL            \
  LGS_RING_PH_DECL;                 \
  const uint32_t ph_where_ = lgs_hw_where_()
#define LGS_PAIR_PH(k) LGS_RING_PH(k)
#define LGS_PAIR_PH_TRIP() LGS_RING_PH_TRIP()
#define LGS_PAIR_PH_END_MOVER(ok, lane, ptr)                              \
  do {                                                                    \
    if ((ok) && (lane) <= 9)                                              \
      *(ptr) = (lane) == 9 ? ph_where_ : lgs_ring_ph_value_(ph_, ph_trips_, (lane), 0u); \
    __builtin_amdgcn_s_waitcnt(0x0f70);                                   \
    pair_barrier();                                                       \
  } while (0)
#define LGS_PAIR_PH_END_WALKER(ok, lane, ptr)                             \
  do {                                                                    \
    pair_barrier();                                                       \
    if ((ok) && (lane) >= 16 && (lane) <= 25)                             \
      *(ptr) = (lane) == 25 ? ph_where_ : lgs_ring_ph_value_(ph_, ph_trips_, (lane) - 16, 0u); \
  } while (0)
#else
#define LGS_PAIR_PH_DECL do {} while (0)
#define LGS_PAIR_PH(k) do {} while (0)
#define LGS_PAIR_PH_TRIP() do {} while (0)
#define LGS_PAIR_PH_END_MOVER(ok, lane, ptr) do {} while (0)
#define LGS_PAIR_PH_END_WALKER(ok, lane, ptr) do {} while (0)
#endif

// ---- traffic calibration of the lane-per-block decoders ------
// LGS_RING_FAR_LD16(p): a far copy's 16-byte load; LGS_RING_FLUSH_ST(g, v, c):
// a flush job's store of c (<= 16) bytes.
#ifdef LGS_PROBE_NOFAR
#define LGS_RING_FAR_LD16(p) ((void)(p), u32x4{0, 0, 0, 0})
#else
#define LGS_RING_FAR_LD16(p) ld16(p)
#endif
#ifdef LGS_PROBE_NOFLUSH
// (never true: keeps v live, so the flush's LDS reads stay)
#define LGS_RING_FLUSH_ST(g, v, c) \
  do { if ((v).x == 0x12345678u && (c) == 77777u) st16((g), (v)); } while (0)
#else
#define LGS_RING_FLUSH_ST(g, v, c) \
  do { if ((c) >= 16) st16((g), (v)); else st_exact((g), (v), (c)); } while (0)
#endif

// ---- decode_kernel phases (tools/dec_phases.py) ---------------------------
// Shader-clock stamps of staging, the tag walk and the flush, and the 100 MHz
// real-time clock, stored by lane 0 at STORE_PTR (the tool gives every block
// 32 bytes of spare capacity).  The probe flushes inside the stamped region
// (FLUSH_STMT) and again after it; harmless.
#ifdef LGS_PROBE_DEC_TIMING
#define LGS_DEC_PH_DECL                                                   \
  const uint64_t dtp0_ = __builtin_amdgcn_s_memtime();                    \
  const uint64_t drt0_ = __builtin_amdgcn_s_memrealtime();                \
  uint64_t dtp1_ = dtp0_
#define LGS_DEC_PH_STAGED()                                               \
  do { __builtin_amdgcn_s_waitcnt(0); dtp1_ = __builtin_amdgcn_s_memtime(); } while (0)
#define LGS_DEC_PH_END(FLUSH_STMT, STORE_PTR)                             \
  do {                                                                    \
    __builtin_amdgcn_s_waitcnt(0);                                        \
    const uint64_t tp2_ = __builtin_amdgcn_s_memtime();                   \
    FLUSH_STMT;                                                           \
    __builtin_amdgcn_s_waitcnt(0);                                        \
    const uint64_t tp3_ = __builtin_amdgcn_s_memtime();                   \
    const uint64_t rt3_ = __builtin_amdgcn_s_memrealtime();               \
    if (lane_id() == 0) {                                                 \
      gptr<uint32_t> q_ = (STORE_PTR);                                    \
      q_[0] = (uint32_t)(dtp1_ - dtp0_);                                  \
      q_[1] = (uint32_t)(tp2_ - dtp1_);                                   \
      q_[2] = (uint32_t)(tp3_ - tp2_);                                    \
      q_[3] = (uint32_t)(rt3_ - drt0_);                                   \
    }                                                                     \
  } while (0)
#else
#define LGS_DEC_PH_DECL do {} while (0)
#define LGS_DEC_PH_STAGED() do {} while (0)
#define LGS_DEC_PH_END(FLUSH_STMT, STORE_PTR) do {} while (0)
#endif

// ---- encode_kernel ----------------------------------------------------------
// LGS_ENC_REPLAY(broke): whether encode_chunk runs its second pass (the
// chunk again from its start, every batch swapping lane by lane); `broke`
// is the product's condition, a lane that received a later position than
// its own.  LGS_PROBE_FORCE_REPLAY: every chunk takes the second pass.  The
// probe library (LGS_PROBE_DECODERS) takes it on request: a device word
// lgs_enc_second_pass, one per compilation of lgs_encode.hip, set through
// the library's lgs_probe_encode_second_pass() (tests/
// test_gpu_encode_round.py).  The product has neither, so its condition is
// `broke` alone.
// LGS_PROBE_ENC_TIMING: shader-clock cycles of staging and the parse, stored
// by lane 0 in the last 16 bytes of the block's output slot
// (tools/enc_phases.py).
#if defined(LGS_PROBE_FORCE_REPLAY)
#define LGS_ENC_REPLAY(broke) ((void)(broke), true)
#elif defined(LGS_PROBE_DECODERS)
#define LGS_ENC_REPLAY(broke) ((broke) | (__builtin_amdgcn_readfirstlane(lgs_enc_second_pass) != 0))
#else
#define LGS_ENC_REPLAY(broke) (broke)
#endif
// LGS_PROBE_ENC_GENERAL_ROUND: the batch after a copy is the general batch
// everywhere (validity per lane, lane B's 64-bit compare from a third probe
// dword), as before round 13; for A/Bs inside one library.
#ifdef LGS_PROBE_ENC_GENERAL_ROUND
#define LGS_ENC_POST_BATCH false
#else
#define LGS_ENC_POST_BATCH true
#endif
#ifdef LGS_PROBE_ENC_TIMING
#define LGS_ENC_PH_DECL                                                   \
  const uint64_t etp0_ = __builtin_amdgcn_s_memtime();                    \
  uint64_t etp1_ = etp0_
#define LGS_ENC_PH_STAGED()                                               \
  do { __builtin_amdgcn_s_waitcnt(0); etp1_ = __builtin_amdgcn_s_memtime(); } while (0)
#define LGS_ENC_PH_END(SLOT, LEN)                                         \
  do {                                                                    \
    __builtin_amdgcn_s_waitcnt(0);                                        \
    const uint64_t tp2_ = __builtin_amdgcn_s_memtime();                   \
    if (lane_id() == 0) {                                                 \
      const uint32_t b_ = 32 + (LEN) + (LEN) / 6 - 16;                    \
      (SLOT).put4(0, b_, (uint32_t)(etp1_ - etp0_));                      \
      (SLOT).put4(0, b_ + 4, (uint32_t)(tp2_ - etp1_));                   \
      (SLOT).put4(0, b_ + 8, 0x7e57u);                                    \
    }                                                                     \
  } while (0)
#else
#define LGS_ENC_PH_DECL do {} while (0)
#define LGS_ENC_PH_STAGED() do {} while (0)
#define LGS_ENC_PH_END(SLOT, LEN) do {} while (0)
#endif

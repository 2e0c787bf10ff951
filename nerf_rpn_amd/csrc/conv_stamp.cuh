// In-kernel phase stamps of the diagnostic conv instantiations (include/nerfrpn_stamps.h has the record's word order).
//
// Stamps<false> is what the product kernels are built with: an empty object whose members compile to nothing.  Stamps<true> reads the two
// device clocks in wave 0 of the workgroup (a wave-uniform branch; the other waves skip the reads) and lane 0 of that wave writes the
// record with plain per-lane stores into the caller's buffer, which nothing else in the kernel reads.  No output value is computed from a stamp.
//
// One stamp = ONE asm statement holding both clock reads and their lgkmcnt(0) wait (the reads return out of order with LDS reads; left to
// the compiler, the wait's place is not ours), fenced by sched_barrier(0) on both sides.  Stamps therefore stay out of stretches with
// hand-counted lgkmcnt(N) waits: every stamp below sits next to a wait or barrier the kernel already has.
#pragma once
#include "common.h"

typedef unsigned long long stamp_t;

__device__ __forceinline__ void stamp_read(stamp_t &rt, stamp_t &cy) {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=&s"(rt), "=&s"(cy) : : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <bool ON> struct Stamps;

template <> struct Stamps<false> {
  __device__ __forceinline__ Stamps(stamp_t *, unsigned, int) {}
  template <int P> __device__ __forceinline__ void mark() {}
  __device__ __forceinline__ void step_wait_begin() {}
  __device__ __forceinline__ void step_wait_end() {}
  __device__ __forceinline__ void finish(unsigned, unsigned, unsigned) {}
};

template <> struct Stamps<true> {
  static constexpr int NP = NRPN_SP_CONV_PHASES;
  stamp_t *rec;
  bool w0;               // wave 0 of the workgroup (wave-uniform)
  int kernel_id;
  stamp_t rt[NP], cy[NP], kst[8], wait_sum, wait_max, t_wait;
  unsigned steps;

  __device__ __forceinline__ Stamps(stamp_t *buf, unsigned record, int kid)
      : rec(buf + (size_t)record * NRPN_STAMP_WORDS), kernel_id(kid), wait_sum(0), wait_max(0), t_wait(0), steps(0) {
    w0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) rt[i] = cy[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) kst[i] = 0;
  }
  template <int P> __device__ __forceinline__ void mark() {
    if (w0) stamp_read(rt[P], cy[P]);
  }
  // around the K-step's own wait + barrier
  __device__ __forceinline__ void step_wait_begin() {
    if (w0) { stamp_t r; stamp_read(r, t_wait); }
  }
  __device__ __forceinline__ void step_wait_end() {
    if (w0) {
      stamp_t r, c;
      stamp_read(r, c);
      const stamp_t d = c - t_wait;
      wait_sum += d;
      wait_max = d > wait_max ? d : wait_max;
#pragma unroll
      for (int i = 0; i < 8; ++i) kst[i] = steps == (unsigned)i ? c : kst[i];
      ++steps;
    }
  }
  // behind the last store of the workgroup's result: stores issued -> vmcnt(0) -> stores complete -> exit, then the record
  __device__ __forceinline__ void finish(unsigned mtile, unsigned ntile, unsigned kslice) {
    mark<NRPN_SP_STORES_ISSUED>();
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    mark<NRPN_SP_STORES_DONE>();
    mark<NRPN_SP_EXIT>();
    if (w0) {
      unsigned xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
      if ((threadIdx.x & 63) == 0) {
        rec[NRPN_SW_VERSION] = NRPN_STAMP_VERSION;
        rec[NRPN_SW_KERNEL] = (stamp_t)kernel_id;
        rec[NRPN_SW_WG] = blockIdx.x;
        rec[NRPN_SW_MTILE] = mtile;
        rec[NRPN_SW_NTILE] = ntile;
        rec[NRPN_SW_KSLICE] = kslice;
        rec[NRPN_SW_XCD] = xcc;
        rec[NRPN_SW_KSTEPS] = steps;
#pragma unroll
        for (int i = 0; i < NP; ++i) { rec[NRPN_SW_PHASE0 + 2 * i] = rt[i]; rec[NRPN_SW_PHASE0 + 2 * i + 1] = cy[i]; }
        rec[NRPN_SW_WAIT_SUM] = wait_sum;
        rec[NRPN_SW_WAIT_MAX] = wait_max;
#pragma unroll
        for (int i = 0; i < 8; ++i) rec[NRPN_SW_KSTEP0 + i] = kst[i];
      }
    }
  }
};

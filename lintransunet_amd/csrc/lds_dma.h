// The primitives every LDS-DMA ring kernel is built from (gemm_ring, conv_halo's class ring, conv_ring, conv_fc_ring, conv_c16_ring,
// upconv_ring, sdgrad_ring, updgrad_ring, upconv_wgrad_ring, wgrad_halo_ring): operands travel global -> LDS without VGPR staging,
// completion is counted by hand, tap offsets are compile-time, out-of-volume rows come from a line of zeros.  One definition each.
#pragma once
#include "common.h"
#include <type_traits>

// 32-bit LDS byte address of a pointer into LDS (of the dynamic-LDS array: the base the LDS-DMA destinations are counted from)
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

// The LDS-DMA is issued from inline asm on purpose: hipcc then keeps no book on it and inserts no vmcnt(0) ahead of the
// fragment reads (it would, conservatively, for the builtin); completion is counted by hand below.  M0 = wave-uniform LDS
// byte address of the 1 KiB piece; lane l lands at M0 + 16 l.  M0 is reserved by the compiler, which keeps values of its own
// there and accepts no clobber for it: it is written in the statement that reads it and put back before the statement ends.
// The s_nop is the wait state between the scalar write of M0 and the vector-memory instruction that reads it.
__device__ __forceinline__ void glds16(const void* src, uint32_t lds_byte_addr) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr);
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
__device__ __forceinline__ void glds16(const void* src, const uint16_t* lds_wave_base) { glds16(src, lds_addr(lds_wave_base)); }
// 4-byte variant: lane l lands at M0 + 4 l (used for the bias row of the projection kernel)
__device__ __forceinline__ void glds4(const float* src, const float* lds_wave_base) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_addr(lds_wave_base));
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}

// retire all but the youngest N LDS-DMA of this wave, then meet the other waves: after it every wave's pieces of the
// oldest unit have landed and every wave has finished reading the unit before it
template <int N>
__device__ __forceinline__ void ring_sync() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// retire all but the youngest N LDS-DMA of this wave AND every LDS read it has issued, then meet the other waves
template <int N>
__device__ __forceinline__ void ring_sync_all() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// f(integral_constant<int, I>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant expression in the body
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// Source of out-of-volume halo rows, padding rows and absent bias entries: 2 KB of zeros, one line per translation unit (internal
// linkage: the library is not built with relocatable device code).  A lane reads 16 bytes at its 16-byte slot (< 64 B), to which
// upconv_ring (Ci <= 512) and sdgrad_ring (Co <= 512) alone add 64 B x channel chunk, chunk < 16 by their launchers' guards: the
// last byte read is 15 * 64 + 48 + 15 = 1023; every other kernel stays inside the first 64 bytes.
static __device__ __attribute__((aligned(64))) uint32_t ltu_zero_line[512];

// linear brick index -> (batch, brick h, brick w, brick d), d fastest; the caller multiplies by its own brick edges
struct Brick {
  int b, bh, bw, bd;
};
__device__ __forceinline__ Brick split_brick(int id, int nbh, int nbw, int nbd) {
  Brick q;
  q.bd = id % nbd; id /= nbd;
  q.bw = id % nbw; id /= nbw;
  q.bh = id % nbh;
  q.b = id / nbh;
  return q;
}

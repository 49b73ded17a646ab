// The LDS DMA (global_load_lds_*: global memory -> LDS with no staging registers and no ds_write).  This header is the only place of the library
// that issues one; the kernels call lds_dma16 / lds_dma4 below.
//
// Every DMA statement is  s_mov_b32 m0, <LDS address> ; s_nop 0 ; global_load_lds_* : M0 (the DMA's LDS base) is written in the statement that
// reads it (M0 is a reserved register: hipcc keeps nothing in it across statements, so writing it needs no clobber), and the SALU write of M0 ->
// LDS-DMA read takes one wait state, which nothing pads inside an asm string.  (Rounds 1-4 ran without the s_nop and bit-exact against the
// oracle; the pad costs one cycle per KiB moved and removes the question.)
//
// Inline asm, not __builtin_amdgcn_global_load_lds: the compiler's waitcnt pass treats the builtin as a store to LDS that any later ds_read may
// alias and drains vmcnt(0) in front of every fragment read, which serialises the pipeline.  The kernels count vmcnt for these instructions by
// hand (a constant number in flight, issued unconditionally).
//
// [r5] Two address forms: a 64-bit pointer per lane (`off`), or a wave-uniform 64-bit base in scalar registers + a 32-bit byte offset per lane
// (the instruction's s[base] form).  The second measured against the first on every kernel that was moved over: fp32 headline GEMM +1.6 %
// frames/s, weight-gradient GEMM's gathers -8 ... -13 %, decoder convolutions -4 %, attention -1 %.
#pragma once
#include <hip/hip_runtime.h>

// A value the whole wave agrees on, moved to scalar registers.  v_readfirstlane is a VALU write of an SGPR; a VMEM instruction that reads that SGPR as
// its base needs 5 wait states after it, and hipcc pads nothing for the operands of an asm statement (cdna_hip_programming.md 5.7, item 2): the s_nop
// sits between the two, bound to both through its operands.  (__builtin_amdgcn_readfirstlane returns int: the halves go through `unsigned` --
// a sign-extended low half ORed into the high one is an address 4 GB below the canonical hole.)
__device__ __forceinline__ unsigned long long lds_dma_base(unsigned long long v) {
    unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    asm volatile("s_nop 4" : "+s"(lo), "+s"(hi));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long lds_dma_base(const void* p) { return lds_dma_base((unsigned long long)(size_t)p); }

// LDS byte address of a __shared__ array (what M0 and the lds_addr arguments below count in)
__device__ __forceinline__ unsigned lds_addr_of(const void* smem) { return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)smem; }

// One wave instruction: 16 bytes (lds_dma16) or 4 bytes (lds_dma4) per lane, lane i landing at lds_addr + i * 16 (or 4); lds_addr is wave-uniform.
// Source: a pointer per lane, or lane byte offset voff from the wave-uniform sbase (an lds_dma_base value, plus scalar arithmetic).
__device__ __forceinline__ void lds_dma16(const void* g, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(__builtin_amdgcn_readfirstlane(lds_addr)) : "memory");
}
__device__ __forceinline__ void lds_dma16(unsigned voff, unsigned long long sbase, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(__builtin_amdgcn_readfirstlane(lds_addr)) : "memory");
}
__device__ __forceinline__ void lds_dma4(const void* g, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g), "s"(__builtin_amdgcn_readfirstlane(lds_addr)) : "memory");
}
__device__ __forceinline__ void lds_dma4(unsigned voff, unsigned long long sbase, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(__builtin_amdgcn_readfirstlane(lds_addr)) : "memory");
}

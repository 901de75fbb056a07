// What the bf16 GEMM kernels share: the fragment and LDS pointer types, and the one-piece global -> LDS DMA statement of
// the ring kernels (gemm_bf16.hip, gemm_nt.hip, gemm_ln.hip, wgrad.hip; gemm_small.hip takes the fragment type only).
#pragma once
#include "cwlt_common.h"

namespace cwlt {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;

// One LDS-DMA piece: 64 lanes x 16 bytes from the buffer `rsrc` describes (four SGPRs, built from wave-uniform values
// through readfirstlane) at byte offset voff (per lane) + soff (wave-uniform), written linearly (1 KiB) to the LDS byte
// address lds_addr.  Inline asm because through the builtin hipcc (ROCm 7.2) cannot tell which LDS bytes a DMA writes and
// drains ALL pieces in flight (s_waitcnt vmcnt(0)) before the next LDS read, which serialises a ring; issued like this
// the kernels count their waits by hand (`s_waitcnt vmcnt(n)`).  M0 carries the LDS address and is compiler-reserved:
// saved and restored inside the statement; s_nop: SGPR write -> M0 / VMEM-read hazards.  The kernels' multi-piece
// statements (GB_DMA2, GN_DMA, WG_DMA, GL_DMA_W) are the same sequence with one M0 save / restore around several pieces.
__device__ __forceinline__ void lds_dma_piece(uint32_t voff, u32x4_t rsrc, uint32_t lds_addr, uint32_t soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\t"
                 "buffer_load_dwordx4 %1, %2, %4 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff)
                 : "memory", "scc");
}

}  // namespace cwlt

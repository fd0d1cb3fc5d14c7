// kkt_wave_dma.h -- what the wavefront-per-problem kernels of kkt_wave.hip (float32) and kkt_wave64.hip (float64) share: blocks
// moved HBM -> LDS by LDS-DMA and the counted wait behind them.  Included inside each file's own anonymous namespace.
#pragma once

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;

// HBM -> LDS, 16 bytes per lane, `bytes` contiguous bytes (a multiple of 16) starting at g
__device__ __forceinline__ void dma_block(const void *g, char *lds, int bytes, int lane)
{
    for (int off = 0; off < bytes; off += 1024)
        if (off + 16 * lane < bytes)
            __builtin_amdgcn_global_load_lds((glb_void_t *)((const char *)g + off + 16 * lane),
                                             (lds_void_t *)(lds + off), 16, 0, 0);
}

// ... 4 bytes per lane, for blocks and rows at any (4-byte) alignment and of any length: the general-shape instantiations (round 6)
__device__ __forceinline__ void dma_block4(const void *g, char *lds, int bytes, int lane)
{
    for (int off = 0; off < bytes; off += 256)
        if (off + 4 * lane < bytes)
            __builtin_amdgcn_global_load_lds((glb_void_t *)((const char *)g + off + 4 * lane), (lds_void_t *)(lds + off), 4, 0, 0);
}

// s_waitcnt vmcnt(n) for a run-time n (the immediate has to be a constant): at most n of the newest vector-memory
// operations may still be in flight
__device__ __forceinline__ void wait_newer(int n)
{
#define MPC_W(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n) {
        MPC_W(0) MPC_W(1) MPC_W(2) MPC_W(3) MPC_W(4) MPC_W(5) MPC_W(6) MPC_W(7) MPC_W(8) MPC_W(9) MPC_W(10) MPC_W(11) MPC_W(12)
        MPC_W(13) MPC_W(14) MPC_W(15) MPC_W(16) MPC_W(17) MPC_W(18) MPC_W(19) MPC_W(20) MPC_W(21) MPC_W(22) MPC_W(23) MPC_W(24)
        MPC_W(25) MPC_W(26) MPC_W(27) MPC_W(28) MPC_W(29) MPC_W(30) MPC_W(31) MPC_W(32) MPC_W(33) MPC_W(34) MPC_W(35) MPC_W(36)
        MPC_W(37) MPC_W(38) MPC_W(39) MPC_W(40) MPC_W(41) MPC_W(42) MPC_W(43) MPC_W(44) MPC_W(45) MPC_W(46) MPC_W(47) MPC_W(48)
        MPC_W(49) MPC_W(50) MPC_W(51) MPC_W(52) MPC_W(53) MPC_W(54) MPC_W(55) MPC_W(56) MPC_W(57) MPC_W(58) MPC_W(59) MPC_W(60)
        MPC_W(61) MPC_W(62) MPC_W(63)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef MPC_W
}

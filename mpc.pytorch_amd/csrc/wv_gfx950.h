// wv_gfx950.h -- the shared part of the gfx950 binding of the `wv::` lane interface the fused kernel bodies are written against
// (lqr_dpp16_body.h, lqr_mfma40_body.h, lqr_mfma16_body.h, lqr_wave1_body.h; lqr_small_math.h inside the first and the third).  Every
// name whose gfx950 form is the same for more than one kernel is defined HERE and nowhere else; lqr_dpp16.hip, lqr_mfma40.hip,
// lqr_mfma16.hip and lqr_wave1_wv.h include this file and add what only their kernel uses.  The host emulator binds the same names once
// for all bodies (tests/emu/emu_mfma16.cpp).  tests/test_wv_binding.py holds the tree to "one definition per name".
//
// A wavefront is 64 lanes = four DPP rows of 16; one wavefront is one workgroup in every kernel that includes this.
//
// The file has three parts:
//   1  for every includer;
//   2  the forms that lean on "inline asm the compiler cannot see into" and "DS instructions of one wave run in order" -- left out where
//      the includer defines MPC_WV_ROW_PER_PROBLEM first (lqr_wave1_wv.h, which binds lds_sync and fmac_bcast for itself, see below);
//   3  the primitives that address THE staging array of a kernel, wv::g_stage, char[MPC_WV_STAGE_BYTES] of LDS -- only where the
//      includer defines MPC_WV_STAGE_BYTES first (lqr_dpp16.hip, lqr_mfma40.hip; each computes its own size).  lqr_mfma16.hip has two
//      typed arrays and a family of its own for them, lqr_wave1_wv.h a float array (`sm`): they take no part 3.
//
// ---- the shared names ------------------------------------------------------------------------------------------------------------
// (bodies: D = lqr_dpp16_body.h, M = lqr_mfma40_body.h, S = lqr_mfma16_body.h, W = lqr_wave1_body.h, m = lqr_small_math.h)
//
// | name                       | what it promises (and what the caller owes)                                               | called by |
// |----------------------------|-------------------------------------------------------------------------------------------|-----------|
// | f32x4, f64x4               | four floats / doubles in consecutive registers (element access v[i])                      | D M S     |
// | lane()                     | this lane's index in the wavefront, 0..63                                                 | D M S W   |
// | problem()                  | the workgroup's index: the problem (D: the group of four problems) of this wavefront      | D M S W   |
// | clock()                    | the shader clock, for the profiling builds (MPC_DPP16_PROF / MPC_MFMA40_PROF) only        | D M       |
// | any(c)                     | c holds in some lane; wave-uniform                                                        | D M W     |
// | ballot(c)                  | bit l = c of lane l; wave-uniform                                                         | D M S W   |
// | ctz64(m)                   | index of the lowest set bit; m != 0 is the caller's to ensure                              | S W       |
// | sched_fence()              | the compiler schedules nothing across this point (no instruction of its own)               | D M       |
// | pin(x)                     | an opaque identity on a register: the compiler may not reason through it                   | D M m     |
// | mfma(a, b, c)              | c + the 16x16x4 product on the matrix core, float or double (layouts: at the definition)   | M S       |
// | shfl_xor(x, m)             | the value of lane (l ^ m), through the LDS crossbar (ds_bpermute): any m < 64              | M S       |
// | bcast<N>(x)                | lane N of the caller's 16-lane row; compiler-visible DPP, its wait states are the compiler's | D M W   |
// | row_sum(x)                 | the sum over the 16 lanes of the row, in every lane of it; fixed order (bitwise repeatable) | D M       |
// | absmax3(acc, a, b)         | acc = max(acc, abs a, abs b) in one instruction; no NaN handling wanted; acc, a, b settled  | D M       |
// | load_uniform_u32(g)        | a dword at a WAVE-UNIFORM address through the scalar cache; the memory is read-only for    | D M       |
// |                            | the whole launch (the scalar cache is not coherent with this launch's stores)              |           |
// | store_f32x4(g, v)          | a cached 16-byte store; g is 16-byte aligned                                              | D M       |
// | store_f32_out(g, v)        | a cached dword store the emulator may hold back (parked gains, workspace records)          | D M       |
// | dma_wait<N>()              | at most N of this wave's vector-memory operations outstanding, and the ordering point      | D M S     |
// |                            | between an LDS-DMA and the LDS reads behind it; N < 64; the caller counts its own DMAs     |           |
// | fence_own_stores()         | this wave's global stores are visible to its own later loads and LDS-DMAs (same CU)        | D M S     |
// | lds_sync()            (2)  | LDS traffic between lanes of ONE wave is ordered across this point (a compiler barrier)    | D M S     |
// | fmac_bcast<N>(acc,s,m) (2) | acc += bcast<N>(s) * m right behind the instruction that wrote s (pays the wait states)     | M         |
// | fmac_bcast_settled<N>  (2) | the same without wait states: s written >= 3 instructions earlier, or just read through DPP | D M       |
// | dma16_if(on, g, off)   (3) | LDS-DMA: 16 bytes per lane from the lane's own address g to g_stage[off + 16 * lane];      | D M       |
// |                            | off wave-uniform; done only behind dma_wait; a lane with !on moves nothing                 |           |
// | dma4_if(on, g, off)    (3) | the same with 4 bytes per lane, to g_stage[off + 4 * lane]                                 | D M       |
// | dma16_at<IMM, KIND>    (3) | dma16 whose immediate IMM moves source AND destination: g is the source biased by -IMM,    | D M       |
// |                            | `mid` the LDS anchor; -4096 <= IMM < 4096; KIND picks the cache policy (DMA_C: read once)  |           |
// | dma16_at_if<IMM>       (3) | dma16_at<IMM> of the lanes with `on`                                                       | M         |
// | dma_buf<G>(on,b,n,vo,off) (3) | G = 4 | 16 bytes per lane from the raw buffer (b, n bytes; b wave-uniform) at per-lane    | M         |
// |                            | offset vo to g_stage[off + G * lane]; a lane whose vo lies beyond n gets ZERO              |           |
// | lds_f32(off), lds_f32x4(off) (3) | g_stage[off] as a float / four floats (16-byte aligned); per-lane off              | D M       |
// | lds_store_f32(off, v), lds_store_f32x4(off, v) (3) | the stores to match; visible to other lanes behind lds_sync()       | D M       |
//
// ---- the names a kernel binds for itself ---------------------------------------------------------------------------------------------
// These carry ONE name in the bodies and the emulator and DIFFERENT gfx950 forms per kernel, on purpose.  Moving lines of a body from one
// kernel to another changes what they compute or cost; tests/test_wv_binding.py (PER_KERNEL) lists the same names with the same reasons.
//
//   rcp(x), rcp_fast(x)   lqr_dpp16.hip: rcp is v_rcp_f32 as it comes, 1 ulp -- the 12/4 step is bound by its instruction count and two more
//                         links per pivot were not bought.  lqr_mfma40.hip, lqr_mfma16.hip: rcp is v_rcp_f32 plus one Newton step (<= 1 ulp,
//                         1/2 typically; double: 1.0 / x), and lqr_mfma40.hip has the raw form beside it as rcp_fast (lqr_mfma40_body.h says
//                         at each use which one it took and what was measured).  lqr_small_math.h (ldl4, pnqp4) calls wv::rcp and so has
//                         the precision of whichever binding it is compiled under: raw in the 12/4 kernel, refined in lqr_mfma16.hip.
//   uniform(c)            "every lane holds this value": the emulator CHECKS it and aborts on a lane that differs.  lqr_mfma40.hip and
//                         lqr_mfma16.hip: v_readfirstlane, so the branch on it is a scalar one.  lqr_dpp16.hip: the identity, a no-op -- a row
//                         of that wavefront is a problem of its own, so what is uniform there is uniform per ROW; its body has a row-wise
//                         box QP of its own (pnqp4_rows) and never reaches lqr_small_math.h's pnqp4, the one caller: the binding is
//                         there for that header to compile.
//   readlane(x, l)        lane l's value, l wave-uniform.  lqr_mfma40.hip, lqr_mfma16.hip: v_readlane with l as the compiler has it (a
//                         constant or a loop counter at every use).  lqr_dpp16.hip: l goes through v_readfirstlane first (its callers
//                         compute l at run time: 16 * the row of a line-search trial).  lqr_wave1_wv.h: __shfl (ds_bpermute), which also
//                         takes a per-lane l.
//   readlane_f64(x, l)    the same for a double, two halves: lqr_dpp16.hip through readfirstlane + v_readlane, lqr_wave1_wv.h through __shfl.
//   lds_sync()            part 2 here: a compiler barrier, since DS instructions of one wave execute in program order.  lqr_wave1_wv.h: a
//                         workgroup fence and a wave barrier, deliberately -- its body exchanges through a plain float array (`sm`) the
//                         compiler schedules freely around, and the phases have to be kept apart for it, too.
//   fmac_bcast<N>         part 2 here: `s_nop 1; v_fmac_f32_dpp` in an asm block.  lqr_wave1_wv.h: fmaf(bcast<N>(src), mul, acc), which
//                         the compiler schedules among the neighbouring chains, placing the DPP wait states itself: measured 4 %
//                         faster THERE (57.8 against 60.5 us per cart-pole step).
//   row_sum_f64(x)        lqr_dpp16.hip: four DPP steps on each half of the double, row_sum's order.  lqr_wave1_wv.h: four __shfl_xor
//                         steps (8, 4, 2, 1) -- another order of additions, so the two are not bitwise interchangeable.
#pragma once
#include "lqr_common.h"

#define MPC_DEV __device__ __forceinline__

namespace mpclqr {
namespace wv {
// ---- part 1 ----------------------------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;
MPC_DEV int lane() { return (int)threadIdx.x; }
MPC_DEV int problem() { return (int)blockIdx.x; }
MPC_DEV unsigned long long clock() { return (unsigned long long)clock64(); }
MPC_DEV bool any(bool c) { return __ballot(c) != 0ull; }
MPC_DEV unsigned long long ballot(bool c) { return __ballot(c); }
MPC_DEV int ctz64(unsigned long long m) { return __builtin_ctzll(m); }
// nothing is scheduled across this point
MPC_DEV void sched_fence() { __builtin_amdgcn_sched_barrier(0); }
// an opaque register-to-register identity: keeps hipcc from folding a chain of selects back into scalar mask logic (see mfma40::pick)
MPC_DEV void pin(float &x) { asm volatile("" : "+v"(x)); }
MPC_DEV void pin(double &x) { asm volatile("" : "+v"(x)); }
MPC_DEV f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// (round 5) v_mfma_f64_16x16x4_f64: lane 16 g + j holds A[i=j][k=g], B[k=g][j] like the float32 instruction, but D[4r+g][j] in element r
// (float32: D[4g+r][j]; measured, tools/ubench/mfma_f64_probe.hip) -- lqr_mfma16_body.h's SLOT_T
MPC_DEV f64x4 mfma(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
MPC_DEV float shfl_xor(float x, int m) { return __shfl_xor(x, m, 64); }
MPC_DEV double shfl_xor(double x, int m) { return __shfl_xor(x, m, 64); }
// DPP row broadcast (row_newbcast): lane N of the caller's 16-lane row
template <int N> MPC_DEV float bcast(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + N, 0xf, 0xf, true));
}
// sum over the 16 lanes of the row, result in every lane (compiler-visible DPP: hazards handled)
MPC_DEV float row_sum(float x)
{
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xf, 0xf, true));   // row_half_mirror
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xf, 0xf, true));   // row_mirror
    return x;
}
// acc = max(acc, |a|, |b|): one v_max3_f32 with source modifiers (fmaxf() costs a canonicalising v_max per operand)
MPC_DEV void absmax3(float &acc, float a, float b)
{
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(acc) : "v"(a), "v"(b));
}
// a dword at a wave-uniform address, through the scalar cache (s_load_dword: lgkmcnt, not vmcnt); the memory is
// read-only for the lifetime of the launch
MPC_DEV unsigned load_uniform_u32(const unsigned *g)
{
    typedef const __attribute__((address_space(4))) unsigned const_u32_t;
    return *(const_u32_t *)(unsigned long)g;
}
MPC_DEV void store_f32x4(float *g, f32x4 v) { *(f32x4 *)g = v; }
// (the gains the sweep parks for its rollout, the workspace records: a plain store here, a store the emulator can hold back --
// tests/emu/emu_mfma16.cpp)
MPC_DEV void store_f32_out(float *g, float v) { *g = v; }
// Wait until at most N of this wave's vector-memory operations are outstanding.  hipcc does not
// order LDS reads behind an LDS-DMA by itself; this is the ordering point (and a compiler barrier).
template <int N> MPC_DEV void dma_wait()
{
    static_assert(N >= 0 && N < 64, "vmcnt is 6 bits on gfx9");
    // (the trailing comment marks the wait as written by hand: tools/isa_lint.py looks for the UNMARKED vmcnt(0) the
    // compiler puts in front of a vector load it cannot count across a loop)
    asm volatile("s_waitcnt vmcnt(%0) ; counted" ::"n"(N) : "memory");
}
MPC_DEV void fence_own_stores()
{
    // same-CU visibility of this wave's own global stores (the gains) to its later loads and LDS-DMA reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#ifndef MPC_WV_ROW_PER_PROBLEM
// ---- part 2 ----------------------------------------------------------------------------------------------------------------------------
// LDS traffic between lanes of ONE wave: DS instructions execute in program order, so a compiler
// barrier is all the ordering there is to ask for.
MPC_DEV void lds_sync() { asm volatile("" ::: "memory"); }
// acc += bcast_N(src) * mul right behind the instruction that wrote src.  Inline asm, because hipcc does not fold a DPP mov into
// v_fmac; the s_nop 1, because the assembler's hazard padding does not look inside asm (VALU write of a VGPR -> DPP read of it
// needs 2 wait states).
template <int N> MPC_DEV void fmac_bcast(float &acc, float src, float mul)
{
    asm("s_nop 1\n"
        "v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf\n"
        : "+v"(acc) : "v"(src), "v"(mul), "n"(N));
}
// the same where src was written at least three instructions earlier (or has just been read through DPP by the instruction in
// front): no read-after-write wait states -- each s_nop is an issue slot on a chain that has nothing to fill it with (round 4)
template <int N> MPC_DEV void fmac_bcast_settled(float &acc, float src, float mul)
{
    asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf\n"
        : "+v"(acc) : "v"(src), "v"(mul), "n"(N));
}
#endif

#ifdef MPC_WV_STAGE_BYTES
// ---- part 3: HBM -> LDS staging ----------------------------------------------------------------------------------------------------------
__shared__ __attribute__((aligned(16))) char g_stage[MPC_WV_STAGE_BYTES];
// 16 (4) bytes per lane from the lane's own global address to LDS[off + 16 (4) * lane], of the lanes with `active`
MPC_DEV void dma16_if(bool active, const void *g, unsigned off)
{
    if (active) __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(g_stage + off), 16, 0, 0);
}
MPC_DEV void dma4_if(bool active, const void *g, unsigned off)
{
    if (active) __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(g_stage + off), 4, 0, 0);
}
// cache policy bits of the stage DMAs (aux bit 1 = non-temporal).  C is read exactly once per launch: nt (12/4 step, measured
// 129-132 -> 123-124 us).  F in the rollout is its second and last read -- yet nt there is 6 % SLOWER: the first
// part of the rollout finds the blocks the sweep touched last still in the Infinity Cache.
constexpr int C_AUX = 2, FR_AUX = 0;
enum { DMA_PLAIN = 0, DMA_C = 1, DMA_LAST = 2 };
// The immediate offset of an LDS-DMA moves the LDS destination together with the global source
// (tools/ubench/dma_offset_probe.hip).  With the source pointer biased by -IMM once, at set-up, every DMA of a
// stage names the same LDS anchor `mid` and differs only in IMM: one M0 write per stage instead of one per
// instruction (instructions of one block share pointer and M0).  `g` is the biased pointer (true source - IMM), -4096 <= IMM < 4096.
template <int IMM, int KIND = DMA_PLAIN> MPC_DEV void dma16_at(const void *g, unsigned mid)
{
    static_assert(IMM >= -4096 && IMM < 4096, "13-bit signed immediate");
    __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(g_stage + mid), 16, IMM,
                                     KIND == DMA_C ? C_AUX : (KIND == DMA_LAST ? FR_AUX : 0));
}
template <int IMM> MPC_DEV void dma16_at_if(bool active, const void *g, unsigned mid)
{
    if (active) __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(g_stage + mid), 16, IMM, 0);
}
// ---- the padded instantiations' staging (lqr_dpp16_body.h, lqr_mfma40_body.h: PADK) ----------------------------------------------------
// G bytes per lane from `base + voff` (base wave-uniform: a raw buffer of `nbytes`, voff per lane) to LDS offset `off` + G * lane.
// A lane whose voff lies beyond the buffer writes ZERO (the hardware's range check; measured, tools/ubench/buffer_lds_probe.hip):
// that is the zero padding of the kernels' 16 x 16 / 40 x 40 / 32 x 40 blocks, at no instruction.
template <int G> MPC_DEV void dma_buf(bool active, const void *base, unsigned nbytes, unsigned voff, unsigned off)
{
    static_assert(G == 4 || G == 16, "dword or dwordx4");
    if (active) {
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)nbytes, 0x00020000);
        if constexpr (G == 4) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t *)(g_stage + off), 4, (int)voff, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t *)(g_stage + off), 16, (int)voff, 0, 0, 0);
    }
}
MPC_DEV void lds_store_f32x4(unsigned off, f32x4 v) { *(f32x4 *)(g_stage + off) = v; }
MPC_DEV void lds_store_f32(unsigned off, float v) { *(float *)(g_stage + off) = v; }
MPC_DEV float lds_f32(unsigned off) { return *(const float *)(g_stage + off); }
MPC_DEV f32x4 lds_f32x4(unsigned off) { return *(const f32x4 *)(g_stage + off); }
#endif
}  // namespace wv
}  // namespace mpclqr

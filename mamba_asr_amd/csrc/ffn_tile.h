// ffn_tile.h — what the 64-token feed-forward tile kernels share: cm_ffn_fused at d_model 256 (ffn_fused.hip) and the d_model-144
// siblings (fused_d144.hip).  One copy, so that the fencing of the DPP row sum cannot drift between them.
#pragma once
#include "cm_common.h"

namespace {

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ uint32_t pack2(float a, float b) {         // one v_cvt_pk_bf16_f32
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
    typedef __attribute__((ext_vector_type(2))) float f32x2_;
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_{a, b}, bf16x2_));
}

// Sum over a row of 16 lanes with every DPP step fenced on BOTH sides: 5 wait states in front of it and behind it, inside one asm block,
// so that no packed-FP32 instruction can be scheduled next to it.  cm_group_sum settles each DPP's source only; in the RACC phase 0 the
// compiler then paired the last steps of two sums -- v_mov_b32_dpp into a register pair that a v_pk_fma_f32 had written two slots
// earlier, v_pk_add_f32 right behind -- and lanes 48-63 of the last token round kept the packed result: rows 15 mod 16 of a tile
// changed from run to run at 32000 rows (tests/test_bench_shapes.py), the packed-FP32 / DPP hazard of cm_common.h from the other side.
#define FFN_DPP_ADD(CTRL)                                                                                                             \
    asm volatile("s_nop 4\n\tv_add_f32_dpp %0, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 4" : "=v"(r) : "v"(v)); \
    v = r
__device__ __forceinline__ float group_sum16_fenced(float v) {
    float r;
    FFN_DPP_ADD("quad_perm:[1,0,3,2]");
    FFN_DPP_ADD("quad_perm:[2,3,0,1]");
    FFN_DPP_ADD("row_half_mirror");
    FFN_DPP_ADD("row_mirror");
    return v;
}
#undef FFN_DPP_ADD

}  // namespace

// lg_dpp_kat.h -- the table of the on-chip DPP operand known-answer test (lg_host.hip: dpp_kat_table_kernel / lg_dpp_kat_run;
// tests/test_gpu_dpp_operands.py runs it, tests/test_dpp_hazard_pass.py reads this file's text: the single copy of the table).
//
// One case = X(role, writer, distance, text).  `text` is the instruction sequence under test: a WRITE of register %[r] (by a plain VALU, or by
// a DPP multiply / multiply-add as lg_quad.h's blocks write), `distance` issue slots of other work (0, 1: an unrelated v_mov, 2: `s_nop 1`,
// the waited reference), and the DPP instruction that READS %[r] in `role`:
//   dpp_src  src0, the operand routed across lanes by the DPP control
//   src1     the plain second source
//   acc      the destination of v_fmac_f32, read as the addend
//   old      the destination of a DPP instruction whose row / bank mask leaves lanes unwritten (they keep what %[r] held)
// Around every case the kernel loads %[r] with a lane-distinct sentinel and %[d] with a lane-distinct old value, five wait states before the
// write, and stores %[d] and %[r] after it.  Operands: %[x] %[y] %[z] inputs (small nonzero integers: every result is exact in f32),
// %[t] scratch.  The DPP controls are spelled as the compiler prints the kernels' (the coverage test matches them textually).
// A kernel edit that makes the built kernels forward a new (mnemonic, role, writer, distance, control) needs a case here.
#pragma once

#define LG_DPP_KAT_CASES(X) \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mov_b32_dpp %[d], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_sub_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_subrev_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_subrev_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mul_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 2, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_ror:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("acc", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("acc", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("acc", "dpp", 0, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("acc", "dpp", 1, "v_fmac_f32_dpp %[r], %[x], %[y] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[r], %[z], %[x] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_add_f32_dpp %[d], %[z], %[r] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("dpp_src", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("dpp_src", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("dpp_src", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_add_f32_dpp %[d], %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("old", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_dpp %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("old", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mov_b32_dpp %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("old", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_mov_b32_dpp %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("old", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_dpp %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("old", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mov_b32_dpp %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("old", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mov_b32_dpp %[r], %[z] row_shl:4 row_mask:0xf bank_mask:0x5\n\t") \
    X("old", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_dpp %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("old", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mov_b32_dpp %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("old", "valu", 2, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "s_nop 1\n\t" "v_mov_b32_dpp %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("old", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_dpp %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("old", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mov_b32_dpp %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("old", "dpp", 2, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "s_nop 1\n\t" "v_mov_b32_dpp %[r], %[z] row_shr:4 row_mask:0xf bank_mask:0xa\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_fmac_f32_dpp %[d], %[z], %[r] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 0, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "valu", 1, "v_mul_f32_e32 %[r], %[x], %[y]\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_mul_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 0, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_sub_f32_dpp %[d], %[z], %[r] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t") \
    X("src1", "dpp", 1, "v_mul_f32_dpp %[r], %[x], %[y] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t" "v_mov_b32_e32 %[t], %[x]\n\t" "v_add_f32_dpp %[d], %[z], %[r] quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t")

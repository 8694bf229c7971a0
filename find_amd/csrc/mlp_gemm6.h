// bf16x3: fp32-FAITHFUL arithmetic on the bf16 matrix pipe, and the split helpers its kernels share (mlp_gemm7.h, mlp_fused6.h, mlp_dw6.h, mlp_dwpe6.h).
//
// gfx950's fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16 rate.  An fp32 number is, exactly, the sum of three bf16
// numbers: a = a1 + a2 + a3 with a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2) (round to nearest; both differences are exact
// in fp32, the last one has at most 8 significant bits, and bf16 has fp32's exponent range, so nothing overflows, underflows or is
// lost: |a2| <= 2^-9 |a|, |a3| <= 2^-18 |a|).  A product then is nine bf16 x bf16 products, each exact in the matrix pipe's fp32
// accumulator; the six of relative size >= 2^-18
//        a1 b1   +   a1 b2 + a2 b1   +   a1 b3 + a2 b2 + a3 b1
// leave out a2 b3 + a3 b2 + a3 b3 <= 2^-26 |a b| -- a quarter of the rounding error of ONE fp32 multiplication (2^-24) -- so the
// layer's results carry the error of fp32 accumulation and nothing else: they are as close to the float64 product as the exact-fp32
// MFMA kernel's (tests/test_gpu_mlp_bf16x3.py measures both), at 6/16 of its matrix-pipe time.  This is not a reduced-precision
// mode (that is gemm5's fp16: operands rounded to 11 bits); tensors stay fp32 in HBM, operands are split on their way into the pipe.
//
// (The header is named after gemm6, the first bf16x3 Linear kernel -- weight planes in LDS; gemm7 replaced it in round 4.)
#pragma once
#include "mlp_gemm5.h"

namespace find {
namespace mlp {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Two floats -> their three bf16 pieces, packed (element 0 in the low half): a = p1 + p2 + p3 exactly.  Written pair by pair so that
// the compiler emits the 9-instruction form (v_cvt_pk_bf16_f32; v_lshlrev_b32 + v_and_b32 to widen the pair back; v_pk_add_f32 with
// negated second operand; twice; v_cvt_pk_bf16_f32): over 8-wide vectors it converts and subtracts element by element (60 for 36).
struct Split2 { unsigned p1, p2, p3; };
__device__ __forceinline__ Split2 split_pair(const f32x2 a) {
	Split2 o;
	o.p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2));
	const f32x2 r1 = a - f32x2{__uint_as_float(o.p1 << 16), __uint_as_float(o.p1 & 0xffff0000u)};
	o.p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
	const f32x2 r2 = r1 - f32x2{__uint_as_float(o.p2 << 16), __uint_as_float(o.p2 & 0xffff0000u)};
	o.p3 = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
	return o;
}

// 8 floats -> the three 8 x bf16 MFMA operands
__device__ __forceinline__ void split3(const float4& lo, const float4& hi, bf16x8& p1, bf16x8& p2, bf16x8& p3) {
	const Split2 q0 = split_pair(f32x2{lo.x, lo.y}), q1 = split_pair(f32x2{lo.z, lo.w}), q2 = split_pair(f32x2{hi.x, hi.y}), q3 = split_pair(f32x2{hi.z, hi.w});
	p1 = __builtin_bit_cast(bf16x8, u32x4{q0.p1, q1.p1, q2.p1, q3.p1});
	p2 = __builtin_bit_cast(bf16x8, u32x4{q0.p2, q1.p2, q2.p2, q3.p2});
	p3 = __builtin_bit_cast(bf16x8, u32x4{q0.p3, q1.p3, q2.p3, q3.p3});
}

}  // namespace mlp
}  // namespace find

// gpboost_amd/csrc/dev_common.h -- device-side helpers shared by the gfx950 kernels.
//
// Everything here is written for CDNA4 (gfx950) only: 64-lane wavefronts, DPP
// row_newbcast on the fp64 pipe, v_rsq_f64 / v_ldexp_f64.  No other target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace gpb {

// ---- compile-time loop: f(integral_constant<int, I>) for I in [B, E) ------
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}
// descending: I = E-1 ... B
template <int B, int E, class F>
__device__ __forceinline__ void static_for_down(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, E - 1>{});
    static_for_down<B, E - 1>(f);
  }
}

// ---- fp64 DPP within a row of 16 lanes ------------------------------------
// gfx90a+ allows DPP on the DP ALU only with row_newbcast:N (lane N of each 16-lane row is broadcast to
// the row).  There is no clang builtin for the 64-bit form, hence inline asm.  Measured on MI355X
// (scripts/ubench/fp64_rates.hip): v_fmac_f64_dpp issues at the plain v_fmac_f64 rate (4 cycles per wave).
//
// Hazard: "VALU writes VGPR -> DPP reads that VGPR" needs 2 wait states, and the compiler neither sees the
// DPP inside an asm statement nor pads for it.  row_bcast() therefore opens with s_nop 1.  row_fnma() -- issued
// ~600 times per point, where the nops cost ~12 % of the kernel -- carries NO padding: the statements are
// `volatile` (program order is kept) and the elimination is written so that a DPP source register is always
// produced several instructions earlier; scripts/check_dpp_hazards.py verifies that property on the generated
// ISA of every translation unit at build time and fails the build otherwise.
// All 64 lanes must be active (a disabled source lane would read as 0): the kernels never early-exit a lane.
template <int LANE>
__device__ __forceinline__ double row_bcast(double x) {
  static_assert(LANE >= 0 && LANE < 16, "row_newbcast lane");
  double r;
  asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf"
               : "=v"(r)
               : "v"(x), "n"(LANE));
  return r;
}
// The same without the wait states, for a source that was written several instructions earlier (the hazard check covers it like the fmacs).
template <int LANE>
__device__ __forceinline__ double row_bcast_nopad(double x) {
  static_assert(LANE >= 0 && LANE < 16, "row_newbcast lane");
#ifdef GPB_DPP_PAD_EVERY_FMAC
  return row_bcast<LANE>(x);
#else
  double r;
  asm volatile("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf"
               : "=v"(r)
               : "v"(x), "n"(LANE));
  return r;
#endif
}
// acc -= bcast<LANE>(b) * own      (one v_fmac_f64 with the broadcast folded in)
template <int LANE>
__device__ __forceinline__ void row_fnma(double& acc, double b, double own) {
  static_assert(LANE >= 0 && LANE < 16, "row_newbcast lane");
#ifdef GPB_DPP_PAD_EVERY_FMAC
  asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
               : "+v"(acc)
               : "v"(b), "v"(own), "n"(LANE));
#else
  asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
               : "+v"(acc)
               : "v"(b), "v"(own), "n"(LANE));
#endif
}
// Explicit hazard fence: makes the listed values opaque (they must exist before this point) and supplies the two
// wait states, so that DPP reads of them further down are safe whatever the compiler scheduled just before.
__device__ __forceinline__ void dpp_fence(double& a) { asm volatile("s_nop 1" : "+v"(a)); }
__device__ __forceinline__ void dpp_fence(double& a, double& b) { asm volatile("s_nop 1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void dpp_fence(double& a, double& b, double& c) { asm volatile("s_nop 1" : "+v"(a), "+v"(b), "+v"(c)); }
__device__ __forceinline__ void dpp_fence(double& a, double& b, double& c, double& d) { asm volatile("s_nop 1" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
// sum over the 16 lanes of a DPP row, result in every lane (fp64 DPP only knows row_newbcast, so the halves travel as two 32-bit DPP movs
// the compiler schedules and pads itself): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
template <int CTRL>
__device__ __forceinline__ double dpp_move_f64(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned int)lo);
}
__device__ __forceinline__ double row_sum16(double v) {
  v += dpp_move_f64<0xB1>(v);
  v += dpp_move_f64<0x4E>(v);
  v += dpp_move_f64<0x141>(v);
  v += dpp_move_f64<0x140>(v);
  return v;
}
// ---- LDS by address -------------------------------------------------------------------------------------------------
// A 32-bit LDS address as a pointer the compiler reads with ds_read and no base register (the low 32 bits of a generic pointer into LDS are that address).
using LdsDouble = __attribute__((address_space(3))) double;
__device__ __forceinline__ const LdsDouble* lds_doubles_at(unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (const LdsDouble*)addr;
#else
  (void)addr;
  return nullptr;
#endif
}
// ---- compile-time lane sets ------------------------------------------------------------------------------------------
// A workgroup's thread t is lane t % 64 of its wavefront and lane l = t % 16 of its point's DPP row, so "l in S" for a compile-time set
// S is a compile-time 64-bit mask (S replicated in the four rows).  Selecting with it needs no v_cmp: the mask goes to an SGPR pair.
__host__ __device__ constexpr unsigned long long row_lanes_le(int j) {   // lanes l <= j of every row
  return j < 0 ? 0ull : (j >= 15 ? ~0ull : ((1ull << (j + 1)) - 1ull) * 0x0001000100010001ull);
}
__host__ __device__ constexpr unsigned long long row_lane_eq(int j) { return (1ull << j) * 0x0001000100010001ull; }
// lanes in MASK get a, the others b
// The mask travels as two 32-bit literals INSIDE the asm (-> vcc / exec), not as an "s" operand: as an operand every distinct mask is
// a loop-invariant SGPR pair, and inside the persistent point kernel's loop the compiler materialises all ~60 of them (and the VGPR copies
// of the constants they select between) ahead of the loop and keeps them live: 102 -> 170 VGPRs for MT = 30, i.e. two wavefronts per
// SIMD instead of four.  The two s_mov issue on the scalar port, beside the VALU-bound instruction stream.
// `tok`: any wave-uniform value that changes with every trip of the enclosing loop (the kernel passes its group index): an INPUT the
// instruction does not read, so that a select between loop-invariant registers stays inside the loop as well.
template <unsigned long long MASK>
__device__ __forceinline__ int sel_lanes(int a, int b, int tok) {      // lanes in MASK get a, the others b
  int r;
  asm("s_mov_b32 vcc_lo, %3\n\ts_mov_b32 vcc_hi, %4\n\tv_cndmask_b32_e32 %0, %1, %2, vcc ; %5"
      : "=v"(r) : "v"(b), "v"(a), "n"((int)(unsigned)(MASK & 0xffffffffull)), "n"((int)(unsigned)(MASK >> 32)), "s"(tok) : "vcc");
  return r;
}
// the same between two compile-time constants in 0..64 (inline constants of the VOP3 encoding: no registers at all)
template <unsigned long long MASK, int A, int B>
__device__ __forceinline__ int sel_lanes_const(int tok) {
  static_assert(A >= 0 && A <= 64 && B >= 0 && B <= 64, "inline constants only");
  int r;
  asm("s_mov_b32 vcc_lo, %3\n\ts_mov_b32 vcc_hi, %4\n\tv_cndmask_b32_e64 %0, %1, %2, vcc ; %5"
      : "=v"(r) : "n"(B), "n"(A), "n"((int)(unsigned)(MASK & 0xffffffffull)), "n"((int)(unsigned)(MASK >> 32)), "s"(tok) : "vcc");
  return r;
}
// lanes in MASK := v (one v_mov_b64 under a constant exec mask).  Only for code every lane of the wavefront executes (exec = all ones).
template <unsigned long long MASK>
__device__ __forceinline__ void set_lanes(double& dst, double v) {
  asm volatile("s_mov_b32 exec_lo, %2\n\ts_mov_b32 exec_hi, %3\n\tv_mov_b64 %0, %1\n\ts_mov_b64 exec, -1"
               : "+v"(dst) : "v"(v), "n"((int)(unsigned)(MASK & 0xffffffffull)), "n"((int)(unsigned)(MASK >> 32)));
}
// Portable-in-HIP variant of the same two primitives (two 32-bit DPP movs that the
// compiler schedules and pads itself).  Used by the self-test kernel to validate the
// asm forms on the device, and selectable with -DGPB_DPP_VIA_BUILTIN for debugging.
template <int LANE>
__device__ __forceinline__ double row_bcast_builtin(double x) {
  const long long v = __builtin_bit_cast(long long, x);
  int lo = (int)(v & 0xffffffffll), hi = (int)(v >> 32);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x150 + LANE, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x150 + LANE, 0xf, 0xf, false);
  const long long r = ((long long)hi << 32) | (unsigned long long)(unsigned int)lo;
  return __builtin_bit_cast(double, r);
}
#ifdef GPB_DPP_VIA_BUILTIN
#define GPB_ROW_BCAST(L, x) ::gpb::row_bcast_builtin<L>(x)
#define GPB_ROW_BCAST_NOPAD(L, x) ::gpb::row_bcast_builtin<L>(x)
#define GPB_ROW_FNMA(L, acc, b, own) (acc) = __builtin_fma(-::gpb::row_bcast_builtin<L>(b), (own), (acc))
#else
#define GPB_ROW_BCAST(L, x) ::gpb::row_bcast<L>(x)
#define GPB_ROW_BCAST_NOPAD(L, x) ::gpb::row_bcast_nopad<L>(x)
#define GPB_ROW_FNMA(L, acc, b, own) ::gpb::row_fnma<L>((acc), (b), (own))
#endif

// ---- fast fp64 elementary functions (relative error ~1e-15, far inside the 1e-8 parity budget) ----

// 1/x: v_rcp_f64 + one Newton step.
__device__ __forceinline__ double fast_rcp(double x) {
  const double y0 = __builtin_amdgcn_rcp(x);
  const double e = __builtin_fma(-x, y0, 1.0);
  return __builtin_fma(y0, e, y0);
}

#ifndef GPB_EXP_TAB_SIZE
#define GPB_EXP_TAB_SIZE 256   // 2^(j/256), j = 0..255 (filled on the host, pre-multiplied by the variance in the kernels)
#endif
static_assert(GPB_EXP_TAB_SIZE == 256, "exp_of_scaled is written for a 256-entry table");

// ---- isotropic Matern kernels on the transformed scale --------------------
// reference: include/GPBoost/cov_fcts.h:2100-2118 (CovarianceMaternShape0_5/1_5/2_5)
enum CovType : int { kMatern05 = 0, kMatern15 = 1, kMatern25 = 2 };

// ---- scaled-distance form used by the hot kernels -------------------------------------------
// exp(-a d) = 2^(-rho/256) with rho = a d 256/ln2: no multiply by the range, no Cody-Waite reduction, the polynomial absorbs ln2/256,
// the table absorbs the variance.  Coordinates are pre-multiplied by HALF of that (a * kCoordScale), so the squared distance the
// kernels form is d2q = rho^2 / 4: with h = rsq(d2q) = 2/rho the square root needs 3 fp64 ops instead of 4 (below).
constexpr double kLn2OverT = 0.0027076061740622863;   // ln2 / 256
constexpr double kCoordScale = 184.6649652337873;     // (256 / ln2) / 2

// Everything a kernel evaluation needs, from d2q = (rho / 2)^2:
//   ev = var * exp(-a d)   (tabv already carries var),   rp = rho = a d 256/ln2
struct KernEval { double ev, rp; };
__device__ __forceinline__ KernEval exp_of_scaled(double d2q, const double* __restrict__ tabv) {
  const double h = __builtin_amdgcn_rsq(d2q);               // 2/rho (1 + delta)
  const double g = d2q * h;                                 // rho/2 (1 + delta)
  const double e = __builtin_fma(-h, g, 3.0);               // 3 - (1 + delta)^2 = 2 - 2 delta - delta^2
  const double rp = g * e;                                  // rho (1 - 1.5 delta^2): one Newton step on v_rsq_f64, folded
  const double kf = __builtin_rint(-rp);
  const double rr = -rp - kf;                               // exact; |rr| <= 1/2, in units of ln2/256
  const int k = (int)kf;                                    // saturates for the dummy rows
  // exp(rr ln2/256) = sum_j (ln2/256)^j rr^j / j!, j <= 4  (remainder < 4e-17)
  double p = __builtin_fma(rr, 2.239395190875157e-12, 3.3083026805413713e-09);
  p = __builtin_fma(p, rr, 3.6655655969101062e-06);
  p = __builtin_fma(p, rr, kLn2OverT);
  p = __builtin_fma(p, rr, 1.0);
  KernEval o;
  o.ev = __builtin_ldexp(tabv[k & (GPB_EXP_TAB_SIZE - 1)] * p, k >> 8);
  o.rp = rp;
  return o;
}
// include/GPBoost/cov_fcts.h:2100-2118 (CovarianceMaternShape0_5/1_5/2_5), transformed scale
template <int COV>
__device__ __forceinline__ double matern_cov_s(double d2s, const double* __restrict__ tabv) {
  const KernEval k = exp_of_scaled(d2s, tabv);
  if constexpr (COV == kMatern05) return k.ev;
  else if constexpr (COV == kMatern15) return k.ev * __builtin_fma(k.rp, kLn2OverT, 1.0);
  else { const double r = k.rp * kLn2OverT; return k.ev * __builtin_fma(r, __builtin_fma(r, 1.0 / 3.0, 1.0), 1.0); }
}
// kernel value and d/d log(a) from ONE exp evaluation (MODE_GRAD keeps the derivative in LDS)
template <int COV>
__device__ __forceinline__ double matern_cov_dlog_s(double d2s, const double* __restrict__ tabv, double& dk) {
  const KernEval k = exp_of_scaled(d2s, tabv);
  const double r = k.rp * kLn2OverT;
  if constexpr (COV == kMatern05) { dk = -r * k.ev; return k.ev; }
  else if constexpr (COV == kMatern15) { dk = -(r * r) * k.ev; return k.ev * (1.0 + r); }
  else { dk = -(1.0 / 3.0) * (r * r) * (1.0 + r) * k.ev; return k.ev * __builtin_fma(r, __builtin_fma(r, 1.0 / 3.0, 1.0), 1.0); }
}
// d/d log(a) of the kernel (transf_scale == true): include/GPBoost/cov_fcts.h:2182-2193 (cm), :2535-2554
template <int COV>
__device__ __forceinline__ double matern_dlog_range_s(double d2s, const double* __restrict__ tabv) {
  const KernEval k = exp_of_scaled(d2s, tabv);
  const double r = k.rp * kLn2OverT;
  if constexpr (COV == kMatern05) return -r * k.ev;                                 // cm d sigma, cm = -a
  else if constexpr (COV == kMatern15) return -(r * r) * k.ev;                      // cm d^2 e^{-ad}, cm = -var a^2
  else return -(1.0 / 3.0) * (r * r) * __builtin_fma(1.0, r, 1.0) * k.ev;           // cm/3 d^2 (1+ad) e^{-ad}
}

}  // namespace gpb

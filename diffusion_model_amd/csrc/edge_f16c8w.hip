// Per-edge kernels of precision 'f16c8' (gfx950): fp32-grade accuracy for TWO bf16-equivalents of matrix work per product.
//
// north_star asks for eps within 1e-4 of the reference's fp32 path (EquivariantGraphNeuralNetwork.py:55-65 is fp32
// throughout).  Precision 'bf16x3' meets it with three full-rate products per operand pair (edge_bf16x3.hip).  Here both
// operands of the two per-edge second-layer products (:15-16 mlp_m.2, :21-22 mlp_x.2) are split into an fp16 head (11
// significant bits) and a remainder,          a = a_hi + a_lo,      W = W_hi + W_lo,
//     a . W  ~=  a_hi . W_hi                          v_mfma_f32_32x32x16_f16           (exact products, fp32 accumulate)
//              + a_lo . W_hi  +  a_hi . W_lo          v_mfma_scale_f32_32x32x64_f8f6f4  on e4m3 operands (TWICE the f16 rate)
// and the two remainder products run on OCP e4m3 (4 significant bits): a remainder is 2^-12 of its operand, so the e4m3
// rounding of the correction's operands is 2^-16 of the product -- what bf16x3's dropped term and remainder rounding
// cost (2^-17).  Both corrections share ONE block-scaled instruction per 32 x 32 tile and 32 hidden units: its K = 64 is
// two blocks of 32 with a scale each, [a_lo8 | a_hi8] against [W_hi8 ; W_lo8], and the e8m0 block scales carry the FIXED
// powers of two the operands were multiplied by before rounding (2^12 for a_lo, 2 for a_hi8; per-matrix exponents for the
// weights, c8_exp), so the instruction adds straight into the main product's accumulators.  No dynamic (per-block) scale is
// needed: e4m3 spans 2^-9 ... 448, and whatever underflows is 2^-21 of the largest activation the scale admits.
// Measured (tools/micro/mfma_scale_probe.hip, profiles/r05a_mfma_scale_probe.txt, on the 16x16 shapes of the first build): the
// mix {2 f16 + 1 scaled e4m3} takes 64 SIMD-cycles per tile and chunk against 96.5 for bf16x3's six bf16 MFMAs.
// CPU emulation of every rounding (tools/rounding_budget.py, profiles/r05_rounding_budget.txt): 6e-6 / 1e-5 on h' / eps_x
// of the full-width goldens (bar 1e-4).
//
// Everything else is the fp32 path's arithmetic: fp32 first-layer table (exact f32 MFMA in node_pre), fp32 geometry, SiLU /
// sigmoid, heads and segment sums; split-operand node MLP (node_bf16.hip).
//
// Instruction shapes: an MFMA holds its SIMD's vector issue for 8 cycles whatever its shape (MI355X_MICROARCH.md, cycle
// constants): 48 16x16 MFMAs per wave and chunk take 384 issue cycles out of the partner wave's activation build, 24 of the 32x32
// shapes take 192 -- and there are half as many operand waits.  The first build on 16x16 tiles was stall-bound (held clock
// 2.38 GHz, MFMA pipe ~50 % busy: DESIGN.md section 4); on 32x32 tiles the coordinate kernel went 4.13 -> 3.54 ms, its matrix
// pipe 50 % -> 71 % busy and the held clock 2.38 -> 1.92-2.0 GHz: on these shapes the kernel reaches the power limit (where
// edge_x_m16.hip's bf16 loop already is), and is faster there (HISTORY.md).
// Workgroup tile: 128 edges, 8 waves, 64-deep chunks, phase-opposed SIMD partners; generated matrix-phase bodies
// (tools/gen/gen_c8_mphase.py w {2|k}); the epilogues are the shared 32x32-accumulator ones of edge_tile.h.  Two kernels:
//   edge_c8w_kernel<false, 2>  coordinate branch: 512 columns per workgroup, 2 column blocks of 32 per wave (128 accumulator
//                              registers), three-slot operand requests, one column share per XCD;
//   edge_c8wk_kernel           message branch: 256 columns, the K loop split inside SIMD pairs (below).
//   fp16 image of a chunk: [8 k-groups][129 rows][16 B] (row padding instead of an XOR swizzle: a lane's pieces of all four k-steps
//   and row blocks are ONE base + immediates; the 8 lanes that store a row's pieces hit 8 different slots);
//   e4m3 image: four K blocks [128 rows][32 B] at q * 4096 + 64 (q >> 1) (a store instruction's two blocks on the two halves of
//   the store bank row), the two 16-byte halves of a row swapped in rows with bit 4 set (an operand read of 16 lanes covers rows
//   0-3, 12-15 and 20-27 of one block: they then hit 16 different slots);
//   weight streams: fp16 [N/32][K/16][64][8] (pack_frags_bf16<_Float16>), e4m3 [N/32][K/32][2][64][16 B] (pack_frags_c8w).
#include <type_traits>

#include "diag.h"
#include "edge_tile.h"

namespace egnn {

namespace {

using namespace tile128;
constexpr int kT = 512;
constexpr int kKC = 64;
constexpr int kRPADW = kR + 1;
constexpr size_t kA1W = (size_t)8 * kRPADW * 16;   // fp16 image of a chunk
constexpr size_t kC8W = 4 * 4096 + 128;            // e4m3 image of a chunk
__host__ __device__ constexpr size_t c8w_block(int q) { return (size_t)q * 4096 + 64 * (q >> 1); }
__host__ __device__ inline size_t c8w_smem_bytes(int KP) { return kOffLoop + 2 * kA1W + 2 * kC8W + (size_t)KP * 4; }

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// SiLU + the three operand forms of one build unit (8 hidden units of one row): table, wd pre-scaled by -log2(e).  slot16: 16 B of
// the fp16 image; slot_lo / slot_hi: 8 B each of the e4m3 image (remainder x 2^12, value x 2).  The build's vector instructions
// are K-loop time (a SIMD's matrix and vector work overlap little in these kernels: chunk time ~ matrix cycles + vector cycles
// of both waves, profiles/r05H_c8w_stamps.txt), so the remainder a - fp16(a) is ONE
// v_fma_mix_f32 (fp16 operand x -1 + a, exact) instead of a conversion and a subtraction: message kernel -5 %.  (Packed fp32 adds /
// fmas / multiplies -- half the instructions -- made both kernels 5 % SLOWER: profiles/r05J_c8w_ab.txt; MI355X_MICROARCH.md prices
// v_pk_*_f32 beside MFMAs as an anti-lever.)
template <int HALF>
__device__ __forceinline__ float minus_f16(const float a, const unsigned hw) {   // a - float(half HALF of hw)
  float r;
  if constexpr (HALF == 0) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hw), "v"(a));
  else asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hw), "v"(a));
  return r;
}
__device__ __forceinline__ void unit_finish_c8w(const Unit& u, const float* wd, float d2, char* slot16, char* slot_lo, char* slot_hi) {
  const f32x4 w0 = *reinterpret_cast<const f32x4*>(wd), w1 = *reinterpret_cast<const f32x4*>(wd + 4);
  float a[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = silu_s(fmaf(w0[j], d2, u.p0[j] + u.q0[j]));   // table, wd pre-scaled by -log2(e)
    a[j + 4] = silu_s(fmaf(w1[j], d2, u.p1[j] + u.q1[j]));
  }
  const f16x8 h = pack8<f16x8>(a);   // RNE; MODE.FP16_OVFL: saturates instead of inf
  if constexpr (diag::kC8NoCvt8) { *reinterpret_cast<f16x8*>(slot16) = h; return; }
  const u32x4 hw = __builtin_bit_cast(u32x4, h);
  const float lo[8] = {minus_f16<0>(a[0], hw.x), minus_f16<1>(a[1], hw.x), minus_f16<0>(a[2], hw.y), minus_f16<1>(a[3], hw.y),
                       minus_f16<0>(a[4], hw.z), minus_f16<1>(a[5], hw.z), minus_f16<0>(a[6], hw.w), minus_f16<1>(a[7], hw.w)};
  // v_cvt_scalef32_pk_fp8_f32: e4m3(src / scale), RNE, saturating at +-448 under MODE.FP16_OVFL
  i16x2 l0 = {0, 0}, l1 = {0, 0}, h0 = {0, 0}, h1 = {0, 0};
  l0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(l0, lo[0], lo[1], 0x1p-12f, false);
  l0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(l0, lo[2], lo[3], 0x1p-12f, true);
  l1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(l1, lo[4], lo[5], 0x1p-12f, false);
  l1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(l1, lo[6], lo[7], 0x1p-12f, true);
  h0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(h0, a[0], a[1], 0.5f, false);
  h0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(h0, a[2], a[3], 0.5f, true);
  h1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(h1, a[4], a[5], 0.5f, false);
  h1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(h1, a[6], a[7], 0.5f, true);
  *reinterpret_cast<f16x8*>(slot16) = h;
  *reinterpret_cast<u32x2*>(slot_lo) = u32x2{__builtin_bit_cast(unsigned, l0), __builtin_bit_cast(unsigned, l1)};
  *reinterpret_cast<u32x2*>(slot_hi) = u32x2{__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)};
}

// Coordinate branch, CB = 2 32-column blocks per wave (512 columns per workgroup).  (The template arguments name the kernel in
// profiles and records; the message branch is edge_c8wk_kernel.)
template <bool IS_M, int CB>
__global__ __launch_bounds__(kT, 2) void edge_c8w_kernel(const EdgeParams p) {
  static_assert(!IS_M && CB == 2, "coordinate branch: 2 column blocks per wave");
  f16_saturate_mode();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L(smem);
  char* s_a1 = smem + kOffLoop;             // [2 buffers] fp16 image
  char* s_c8 = s_a1 + 2 * kA1W;             // [2 buffers] e4m3 image
  float* s_wd = reinterpret_cast<float*>(s_c8 + 2 * kC8W);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int KP = p.WxP;
  // workgroup -> (tile, column share).  1024-wide coordinate branch: an XCD works on ONE column share (XCD x: share x & 1, tiles of
  // quarter x >> 1 of the edge list) -- its L2 (4 MB) then holds that share's fragments (fp16 + e4m3: 2 MB) instead of thrashing on
  // both (4 MB + the table rows streaming through); the table rows of a graph are read by the two XCDs of its quarter.  -2.3 %.
  int tile, half = 0;
  if (p.WxP == 1024) {
    const int ntiles = (p.E + kR - 1) / kR, per = (ntiles + 3) >> 2;
    const int xcd = blockIdx.x & 7, g = xcd >> 1;
    half = xcd & 1;
    tile = g * per + (int)(blockIdx.x >> 3);
    if (tile >= min((g + 1) * per, ntiles)) return;   // (grid: 8 x per workgroups)
  } else {
    tile = xcd_tile(blockIdx.x, gridDim.x);
  }
  const int e0 = tile * kR;
  const int nvalid = min(kR, p.E - e0);
  DIAG_STAMP_SETUP(p.stamps + (size_t)wave * 32 * 4);
  DIAG_STAMP(30, 0);

  // ---- weight streams ----
  const int NC = KP / kKC, KS16 = KP / 16, KS32 = KP / 32;
  const int brow = tid >> 3, kg = tid & 7;   // this thread builds rows brow and brow + 64, hidden units 8 kg .. 8 kg + 7 of a chunk
  const unsigned wbytes = diag::drop_weight_loads(p.dbg) ? 0u : (unsigned)((size_t)p.WxP * KP * 2);
  const rsrc_t rs_w = make_rsrc(p.w2x, wbytes);        // fp16 fragments [N/32][K/16][64][8]
  const rsrc_t rs_w8 = make_rsrc(p.w2x_c8, wbytes);   // e4m3 fragments [N/32][K/32][2][64][16 B]
  const unsigned lane16 = lane * 16u;
  const int cb0 = half * 16 + wave * 2;            // first 32-column block of this wave
  const unsigned w0 = (unsigned)cb0 * KS16 * 1024u;              // fp16 stream: 1 KiB per (column block, k-step of 16)
  const unsigned w80 = (unsigned)cb0 * KS32 * 2048u;             // e4m3 stream: 2 KiB per (column block, 32 hidden units)
  const bool hotw = diag::hot_weight_loads(p.dbg);
  auto ld16 = [&](const int cq, const int ks, const int cb) {     // fp16 fragment of (chunk c, k-step ks of 16, column block cb)
    const int c = hotw ? 0 : cq;
    return ldbuf_v8<f16x8>(rs_w, lane16, w0 + ((unsigned)cb * KS16 + (unsigned)(4 * c + ks)) * 1024u);
  };
  auto ld8 = [&](const int cq, const int t, const int cb) {       // e4m3 fragment (32 bytes per lane) of (chunk c, hidden half t, column block cb)
    const int c = hotw ? 0 : cq;
    const unsigned o = w80 + ((unsigned)cb * KS32 + (unsigned)(2 * c + t)) * 2048u;
    const u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rs_w8, lane16, __builtin_amdgcn_readfirstlane(o), 0);
    const u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(rs_w8, lane16, __builtin_amdgcn_readfirstlane(o + 1024u), 0);
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };
  f16x8 bq[4][CB];   // [k-step of 16][column block]
  i32x8 b8[2][CB];   // [hidden half][column block]

  prologue_rows(p, L, e0, nvalid, p.wdx, KP, s_wd, tid);
  DIAG_STAMP(30, 1);

  // ---- K loop ----
  const rsrc_t rs_tab = make_rsrc(p.table, diag::drop_table_loads(p.dbg) ? 0u : (unsigned)min((size_t)p.N * p.TC * 4, (size_t)0xFFFFFFFFu));
  const unsigned vdst0 = (unsigned)L.dst[brow] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned vsrc0 = (unsigned)L.src[brow] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned vdst1 = (unsigned)L.dst[brow + 64] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned vsrc1 = (unsigned)L.src[brow + 64] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned offP = 0u, offQ = (unsigned)p.WxP * 4u;   // fp32 table {Px|Qx|Pm|Qm}
  // store slots of this thread (rows brow, brow + 64).  e4m3: hidden units 8 kg .. + 7 sit in block 2 (kg >> 2) (remainder) / + 1
  // (value), bytes 8 (kg & 3) .. + 7 of the row's 32, the 16-byte halves swapped in rows with bit 4 set (same for brow + 64)
  char* slot0 = s_a1 + ((size_t)kg * kRPADW + brow) * 16;
  const unsigned sw = ((unsigned)brow >> 4) & 1u;
  char* slo0 = s_c8 + (size_t)(kg >> 2) * (c8w_block(2) - c8w_block(0)) + (size_t)brow * 32 + ((((unsigned)kg >> 1) & 1u) ^ sw) * 16u + (unsigned)(kg & 1) * 8u;
  constexpr int shi_delta = (int)(c8w_block(1) - c8w_block(0));
  // operand reads of this lane: fp16 pieces (row r of a row block, k-group 2 ks + hh) = ONE base + immediates; e4m3 operands
  // (row r, block 2 t + hh): the half that holds hidden units 0-15 of the block first, then the other
  const unsigned abase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(s_a1 + ((size_t)hh * kRPADW + r) * 16);
  const unsigned lds8 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)s_c8;
  const unsigned rsw = ((unsigned)r >> 4) & 1u;
  const unsigned cbaseA = lds8 + (unsigned)hh * 4096u + (unsigned)r * 32u + rsw * 16u;
  const unsigned cbaseB = cbaseA ^ 16u;
  constexpr int kScaleA = 127 - 12;   // block scales: see the top of this file (both kinds of block need the same product of scales)
  const int scale_b = __builtin_amdgcn_readfirstlane(p.c8_exp[0]);

  f32x16 acc[4][CB];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[rb][cb][i] = 0.f;

  Unit ua0, ua1;
  auto vload0 = [&](const int cq) {
    const int c = cq < NC ? cq : NC - 1;   // past the end: a harmless repeat
    unit_load(ua0, rs_tab, vdst0, vsrc0, offP + (unsigned)c * kKC * 4u, offQ + (unsigned)c * kKC * 4u);
  };
  auto vload1 = [&](const int cq) {
    const int c = cq < NC ? cq : NC - 1;
    unit_load(ua1, rs_tab, vdst1, vsrc1, offP + (unsigned)c * kKC * 4u, offQ + (unsigned)c * kKC * 4u);
  };
  auto vrow = [&](auto par_c, auto row_c, const int c) {
    constexpr int PAR = decltype(par_c)::value, ROW = decltype(row_c)::value;
    unit_finish_c8w(ROW ? ua1 : ua0, s_wd + c * kKC + kg * 8, L.d2[brow + 64 * ROW], slot0 + PAR * kA1W + ROW * 64 * 16,
                    slo0 + PAR * kC8W + ROW * 64 * 32, slo0 + PAR * kC8W + ROW * 64 * 32 + shi_delta);
  };
  const std::integral_constant<int, 0> P0;
  const std::integral_constant<int, 1> P1;
  int S = 0;

#define LDS_RD(dst, base, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(base), "n"(off))
#define LDS_WAIT(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory")
#define MAIN_STEP(A, KSTEP, RB)                                                                                          \
  do {                                                                                                                   \
    asm volatile("" : "+v"(A));                                                                                          \
    if constexpr (!diag::kC8NoMain) {                                                                                    \
      _Pragma("unroll") for (int cb = 0; cb < CB; ++cb)                                                                  \
          acc[RB][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, BQ(KSTEP)[cb], acc[RB][cb], 0, 0, 0);                  \
    } else {                                                                                                             \
      asm volatile("" ::"v"(BQ(KSTEP)[0]), "v"(BQ(KSTEP)[CB - 1]));                                                      \
    }                                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
  } while (0)
#define CORR_STEP(C0, C1, T, RB)                                                                                         \
  do {                                                                                                                   \
    if constexpr (!diag::kC8NoCorr) {                                                                                    \
      asm volatile("" : "+v"(C0), "+v"(C1));                                                                             \
      const u32x4 x0_ = C0, x1_ = C1;                                                                                    \
      const i32x8 a8_ = {(int)x0_.x, (int)x0_.y, (int)x0_.z, (int)x0_.w, (int)x1_.x, (int)x1_.y, (int)x1_.z, (int)x1_.w}; \
      _Pragma("unroll") for (int cb = 0; cb < CB; ++cb)                                                                  \
          acc[RB][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8_, B8(T)[cb], acc[RB][cb], 0, 0, 0, kScaleA, 0, scale_b); \
    } else {                                                                                                             \
      asm volatile("" ::"v"(B8(T)[0]), "v"(B8(T)[CB - 1]));                                                              \
    }                                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
  } while (0)

  // ---- 128 accumulator registers.  The operands of a chunk are six groups of 16 registers,
  // each consumed by 512 cycles of matrix instructions (or one row of the build): fp16 fragments of k-steps 0-1 (G1) and 2-3 (G2),
  // e4m3 fragments of hidden units 0-31 (G3) and 32-63 (G4), table rows of the next build's two rows (U0, U1).  Three groups
  // are live at any time -- one being consumed, two in flight (48 registers; hipcc spills beyond that):
  //   G3 at the start of the matrix phase | G4 behind G1 | U0 behind G2 | U1 behind G3 | G1 of the next matrix phase at the
  //   start of the build in front of it, G2 between its two rows
  auto wload16 = [&](const int cq, const int s) {   // k-steps 2 s, 2 s + 1 of chunk cq
    const int c = cq < NC ? cq : NC - 1;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) bq[2 * s + k2][cb] = ld16(c, 2 * s + k2, cb);
  };
  auto wload8 = [&](const int c, const int t) {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) b8[t][cb] = ld8(c, t, cb);
  };
  auto vfinish = [&](auto par_c, const int c, const int mchunk) {
    __builtin_amdgcn_s_setprio(3);
    wload16(mchunk, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (!(diag::kC8NoBuild && c > 1)) vrow(par_c, P0, c);
    else asm volatile("" :: "v"(ua0.p0), "v"(ua0.p1), "v"(ua0.q0), "v"(ua0.q1));
    __builtin_amdgcn_sched_barrier(0);
    DIAG_STAMP2(c + 15, 3, c >= 1 && c < 15);
    wload16(mchunk, 1);
    __builtin_amdgcn_sched_barrier(0);
    if (!(diag::kC8NoBuild && c > 1)) vrow(par_c, P1, c);
    else asm volatile("" :: "v"(ua1.p0), "v"(ua1.p1), "v"(ua1.q0), "v"(ua1.q1));
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
  };
  vload0(0);
  vload1(0);
  S = prologue_segments<false>(p, L, e0, nvalid, tid, lane, wave);
  vfinish(P0, 0, 0);
  if (wave >= 4) { vload0(1); vload1(1); }
  __syncthreads();
  DIAG_STAMP(30, 2);
  DIAG_RSTAMP(31, 1);
  auto mphase = [&](auto par_c, const int c, const int tab_chunk) {
    constexpr int PAR = decltype(par_c)::value;
    constexpr int kO16 = PAR * (int)kA1W, kO8 = PAR * (int)kC8W;
    f16x8 a[3];
    u32x4 c0[2], c1[2];
#define BQ(ks) bq[ks]
#define B8(t) b8[t]
#define MPHASE_AFTER_FIRST_READS do { __builtin_amdgcn_sched_barrier(0); wload8(c, 0); __builtin_amdgcn_sched_barrier(0); } while (0)
#define MPHASE_AFTER_KSTEP0 do { DIAG_STAMP2(c + 16, 0, c < 14); wload8(c, 1); __builtin_amdgcn_sched_barrier(0); } while (0)
#define MPHASE_AFTER_KSTEP1 do { DIAG_STAMP2(c + 16, 1, c < 14); if (tab_chunk >= 0) vload0(tab_chunk); __builtin_amdgcn_sched_barrier(0); } while (0)
#define MPHASE_AFTER_CORR0 do { if (tab_chunk >= 0) vload1(tab_chunk); __builtin_amdgcn_sched_barrier(0); } while (0)
#include "edge_f16c8w_mphase2.inc"
    DIAG_STAMP2(c + 16, 2, c < 14);
#undef MPHASE_AFTER_CORR0
#undef MPHASE_AFTER_KSTEP1
#undef MPHASE_AFTER_KSTEP0
#undef MPHASE_AFTER_FIRST_READS
#undef B8
#undef BQ
  };
  if (wave < 4) {
    const int my_mode = tid < S ? segment_mode(p, L, e0, tid) : 0;
    DIAG_STAMP(0, 0);
    mphase(P0, 0, 1);
    DIAG_STAMP(0, 1);
    if (tid < S) L.seg_mode[tid] = my_mode;
    vfinish(P1, 1, 1);
    DIAG_STAMP(0, 2);
    __syncthreads();
    DIAG_STAMP(0, 3);
    for (int i = 1; i + 1 < NC - 1; i += 2) {
      DIAG_STAMP(i, 0); mphase(P1, i, i + 1); DIAG_STAMP(i, 1); vfinish(P0, i + 1, i + 1); DIAG_STAMP(i, 2); __syncthreads(); DIAG_STAMP(i, 3);
      DIAG_STAMP(i + 1, 0); mphase(P0, i + 1, i + 2); DIAG_STAMP(i + 1, 1); vfinish(P1, i + 2, i + 2); DIAG_STAMP(i + 1, 2); __syncthreads(); DIAG_STAMP(i + 1, 3);
    }
  } else {
    DIAG_STAMP(0, 0);
    vfinish(P1, 1, 0);
    DIAG_STAMP(0, 1);
    __builtin_amdgcn_sched_barrier(0);
    mphase(P0, 0, 2);
    DIAG_STAMP(0, 2);
    __syncthreads();
    DIAG_STAMP(0, 3);
    for (int i = 1; i + 1 < NC - 1; i += 2) {
      DIAG_STAMP(i, 0); vfinish(P0, i + 1, i); DIAG_STAMP(i, 1); __builtin_amdgcn_sched_barrier(0); mphase(P1, i, i + 2); DIAG_STAMP(i, 2); __syncthreads(); DIAG_STAMP(i, 3);
      DIAG_STAMP(i + 1, 0); vfinish(P1, i + 2, i + 1); DIAG_STAMP(i + 1, 1); __builtin_amdgcn_sched_barrier(0); mphase(P0, i + 1, i + 3); DIAG_STAMP(i + 1, 2); __syncthreads(); DIAG_STAMP(i + 1, 3);
    }
    wload16(NC - 1, 0);
    wload16(NC - 1, 1);
  }
  DIAG_STAMP(NC - 1, 0);
  mphase(P1, NC - 1, -1);
  DIAG_STAMP(NC - 1, 1);
#undef CORR_STEP
#undef MAIN_STEP
#undef LDS_WAIT
#undef LDS_RD
  __syncthreads();
  DIAG_STAMP(NC - 1, 3);
  DIAG_STAMP(30, 3);
  DIAG_RSTAMP(31, 2);

  // ---- epilogue: the shared 32x32-accumulator forms (edge_tile.h); the weight fragments carry 2^8 ----
  constexpr float kAcc = kNegLog2e / kF16WScale;
  if constexpr (diag::kC8NoEpi) {
    float v = 0.f;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) v += acc[rb][cb][i];
    if (v == 123.456f) p.agg_x[0] = v;
    return;
  }
  x_head<CB>(p, L, acc, cb0, half, tid, lane, wave, kAcc);
  coordinate_segment_sums(p, L, S, tile, half, tid, lane, wave);
  DIAG_STAMP(31, 0);
}

// Message branch with the K loop SPLIT between the two waves of a SIMD pair.  With one 32-column block per wave (the first message kernel)
// every operand read from LDS feeds ONE matrix instruction: 16 bytes per lane and 32 MFMA cycles, x 4 SIMDs = the 128 bytes per
// clock the LDS delivers -- the message kernel's K loop ran against the LDS (49 % MFMA-busy, profiles/r05F_c8w_stamps.txt).  Here
// wave w owns column blocks 2 (w & 3), 2 (w & 3) + 1 (64 columns: a read feeds two instructions) and HALF of every chunk: k-steps
// 2 (w >> 2), + 1 of the fp16 product and e4m3 instruction (w >> 2).  Same matrix work and weight bytes per wave, half the LDS reads;
// the build is unchanged (512 threads, 2 rows each).  After the K loop the pair exchanges half of its partial sums through LDS (the
// loop buffers are dead): wave w keeps column block 2 (w & 3) + (w >> 2) -- one block per wave, the layout of message_epilogue.
// Operand requests: four groups of 16 registers per chunk and wave -- fp16 fragments (G1), e4m3 fragments (G3), table rows of the
// build's two rows (U0, U1) -- consumed in a fixed cycle; each is requested when the consumption of the group two places ahead of
// it starts (three live groups beside the 128 accumulators).
constexpr size_t kXchg = (size_t)8 * 16384;   // exchange buffer: 64 accumulator registers per wave
__host__ __device__ inline size_t c8wk_smem_bytes(int KP) {
  const size_t loop = c8w_smem_bytes(KP), x = kOffLoop + kXchg;
  return loop > x ? loop : x;
}
__global__ __launch_bounds__(kT, 2) void edge_c8wk_kernel(const EdgeParams p) {
  constexpr int CB = 2;
  f16_saturate_mode();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L(smem);
  char* s_a1 = smem + kOffLoop;
  char* s_c8 = s_a1 + 2 * kA1W;
  float* s_wd = reinterpret_cast<float*>(s_c8 + 2 * kC8W);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int kh = wave >> 2, cb0 = 2 * (wave & 3);
  const int KP = p.WmP;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int e0 = tile * kR;
  const int nvalid = min(kR, p.E - e0);
  DIAG_STAMP_SETUP(p.stamps + ((size_t)8 + wave) * 32 * 4);
  DIAG_STAMP(30, 0);

  const int NC = KP / kKC, KS16 = KP / 16, KS32 = KP / 32;
  const int brow = tid >> 3, kg = tid & 7;
  const unsigned wbytes = diag::drop_weight_loads(p.dbg) ? 0u : (unsigned)((size_t)p.MP * KP * 2);
  const rsrc_t rs_w = make_rsrc(p.w2m, wbytes);
  const rsrc_t rs_w8 = make_rsrc(p.w2m_c8, wbytes);
  const unsigned lane16 = lane * 16u;
  const unsigned w0 = ((unsigned)cb0 * KS16 + 2u * kh) * 1024u;
  const unsigned w80 = ((unsigned)cb0 * KS32 + (unsigned)kh) * 2048u;
  auto ld16 = [&](const int c, const int ksl, const int cb) {   // fp16 fragment of (chunk c, this wave's k-step ksl, column block cb)
    return ldbuf_v8<f16x8>(rs_w, lane16, w0 + ((unsigned)cb * KS16 + (unsigned)(4 * c + ksl)) * 1024u);
  };
  auto ld8 = [&](const int c, const int cb) {                   // e4m3 fragment of (chunk c, this wave's instruction, column block cb)
    const unsigned o = w80 + ((unsigned)cb * KS32 + (unsigned)(2 * c)) * 2048u;
    const u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rs_w8, lane16, __builtin_amdgcn_readfirstlane(o), 0);
    const u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(rs_w8, lane16, __builtin_amdgcn_readfirstlane(o + 1024u), 0);
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };
  f16x8 bq[1][2][CB];
  i32x8 b8[1][1][CB];

  prologue_rows(p, L, e0, nvalid, p.wdm, KP, s_wd, tid);
  DIAG_STAMP(30, 1);

  const rsrc_t rs_tab = make_rsrc(p.table, diag::drop_table_loads(p.dbg) ? 0u : (unsigned)min((size_t)p.N * p.TC * 4, (size_t)0xFFFFFFFFu));
  const unsigned vdst0 = (unsigned)L.dst[brow] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned vsrc0 = (unsigned)L.src[brow] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned vdst1 = (unsigned)L.dst[brow + 64] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned vsrc1 = (unsigned)L.src[brow + 64] * (unsigned)p.TC * 4u + (unsigned)kg * 32u;
  const unsigned offP = 2u * p.WxP * 4u, offQ = (2u * p.WxP + p.WmP) * 4u;   // fp32 table {Px|Qx|Pm|Qm}
  char* slot0 = s_a1 + ((size_t)kg * kRPADW + brow) * 16;
  const unsigned sw = ((unsigned)brow >> 4) & 1u;
  char* slo0 = s_c8 + (size_t)(kg >> 2) * (c8w_block(2) - c8w_block(0)) + (size_t)brow * 32 + ((((unsigned)kg >> 1) & 1u) ^ sw) * 16u + (unsigned)(kg & 1) * 8u;
  constexpr int shi_delta = (int)(c8w_block(1) - c8w_block(0));
  // operand reads: this wave's half of the chunk rides in the base registers (k-groups 4 kh .., e4m3 blocks 2 kh ..)
  const unsigned abase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(s_a1 + ((size_t)(4 * kh + hh) * kRPADW + r) * 16);
  const unsigned lds8 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)s_c8;
  const unsigned rsw = ((unsigned)r >> 4) & 1u;
  const unsigned cbaseA = lds8 + (unsigned)c8w_block(2) * (unsigned)kh + (unsigned)hh * 4096u + (unsigned)r * 32u + rsw * 16u;
  const unsigned cbaseB = cbaseA ^ 16u;
  constexpr int kScaleA = 127 - 12;
  const int scale_b = __builtin_amdgcn_readfirstlane(p.c8_exp[2]);

  f32x16 acc[4][CB];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[rb][cb][i] = 0.f;

  Unit ua0, ua1;
  auto vload0 = [&](const int cq) {
    const int c = cq < NC ? cq : NC - 1;
    unit_load(ua0, rs_tab, vdst0, vsrc0, offP + (unsigned)c * kKC * 4u, offQ + (unsigned)c * kKC * 4u);
  };
  auto vload1 = [&](const int cq) {
    const int c = cq < NC ? cq : NC - 1;
    unit_load(ua1, rs_tab, vdst1, vsrc1, offP + (unsigned)c * kKC * 4u, offQ + (unsigned)c * kKC * 4u);
  };
  auto vrow = [&](auto par_c, auto row_c, const int c) {
    constexpr int PAR = decltype(par_c)::value, ROW = decltype(row_c)::value;
    unit_finish_c8w(ROW ? ua1 : ua0, s_wd + c * kKC + kg * 8, L.d2[brow + 64 * ROW], slot0 + PAR * kA1W + ROW * 64 * 16,
                    slo0 + PAR * kC8W + ROW * 64 * 32, slo0 + PAR * kC8W + ROW * 64 * 32 + shi_delta);
  };
  const std::integral_constant<int, 0> P0;
  const std::integral_constant<int, 1> P1;
  auto wload16 = [&](const int cq) {
    const int c = cq < NC ? cq : NC - 1;
#pragma unroll
    for (int ksl = 0; ksl < 2; ++ksl)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) bq[0][ksl][cb] = ld16(c, ksl, cb);
  };
  auto wload8 = [&](const int cq) {
    const int c = cq < NC ? cq : NC - 1;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) b8[0][0][cb] = ld8(c, cb);
  };
  auto vfinish = [&](auto par_c, const int c, const int mchunk) {   // build of chunk c; requests the weights of matrix phase mchunk
    __builtin_amdgcn_s_setprio(3);
    wload16(mchunk);
    __builtin_amdgcn_sched_barrier(0);
    if (!(diag::kC8NoBuild && c > 1)) vrow(par_c, P0, c);
    else asm volatile("" :: "v"(ua0.p0), "v"(ua0.p1), "v"(ua0.q0), "v"(ua0.q1));
    __builtin_amdgcn_sched_barrier(0);
    wload8(mchunk);
    __builtin_amdgcn_sched_barrier(0);
    if (!(diag::kC8NoBuild && c > 1)) vrow(par_c, P1, c);
    else asm volatile("" :: "v"(ua1.p0), "v"(ua1.p1), "v"(ua1.q0), "v"(ua1.q1));
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
  };
  vload0(0);
  vload1(0);
  const int S = prologue_segments<false>(p, L, e0, nvalid, tid, lane, wave);
  vfinish(P0, 0, 0);
  if (wave >= 4) { vload0(1); vload1(1); }
  __syncthreads();
  DIAG_STAMP(30, 2);
  DIAG_RSTAMP(31, 1);

#define LDS_RD(dst, base, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(base), "n"(off))
#define LDS_WAIT(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory")
#define MAIN_STEP(A, KSTEP, RB)                                                                                          \
  do {                                                                                                                   \
    asm volatile("" : "+v"(A));                                                                                          \
    if constexpr (!diag::kC8NoMain) {                                                                                    \
      _Pragma("unroll") for (int cb = 0; cb < CB; ++cb)                                                                  \
          acc[RB][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, bq[0][KSTEP][cb], acc[RB][cb], 0, 0, 0);               \
    } else {                                                                                                             \
      asm volatile("" ::"v"(bq[0][KSTEP][0]), "v"(bq[0][KSTEP][CB - 1]));                                                \
    }                                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
  } while (0)
#define CORR_STEP(C0, C1, T, RB)                                                                                         \
  do {                                                                                                                   \
    if constexpr (!diag::kC8NoCorr) {                                                                                    \
      asm volatile("" : "+v"(C0), "+v"(C1));                                                                             \
      const u32x4 x0_ = C0, x1_ = C1;                                                                                    \
      const i32x8 a8_ = {(int)x0_.x, (int)x0_.y, (int)x0_.z, (int)x0_.w, (int)x1_.x, (int)x1_.y, (int)x1_.z, (int)x1_.w}; \
      _Pragma("unroll") for (int cb = 0; cb < CB; ++cb)                                                                  \
          acc[RB][cb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8_, b8[0][T][cb], acc[RB][cb], 0, 0, 0, kScaleA, 0, scale_b); \
    } else {                                                                                                             \
      asm volatile("" ::"v"(b8[0][T][0]), "v"(b8[0][T][CB - 1]));                                                        \
    }                                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
  } while (0)
  auto mphase = [&](auto par_c, const int c, const int tab_chunk) {   // this wave's half of chunk c; requests the table rows of build tab_chunk
    constexpr int PAR = decltype(par_c)::value;
    constexpr int kO16 = PAR * (int)kA1W, kO8 = PAR * (int)kC8W;
    f16x8 a[3];
    u32x4 c0[2], c1[2];
#define MPHASE_AFTER_FIRST_READS do { __builtin_amdgcn_sched_barrier(0); if (tab_chunk >= 0) vload0(tab_chunk); __builtin_amdgcn_sched_barrier(0); } while (0)
#define MPHASE_AFTER_KSTEP1 do { if (tab_chunk >= 0) vload1(tab_chunk); __builtin_amdgcn_sched_barrier(0); } while (0)
#include "edge_f16c8w_mphasek.inc"
#undef MPHASE_AFTER_KSTEP1
#undef MPHASE_AFTER_FIRST_READS
  };
  if (wave < 4) {
    const int my_mode = tid < S ? segment_mode(p, L, e0, tid) : 0;
    DIAG_STAMP(0, 0);
    mphase(P0, 0, 1);
    DIAG_STAMP(0, 1);
    if (tid < S) L.seg_mode[tid] = my_mode;
    vfinish(P1, 1, 1);
    DIAG_STAMP(0, 2);
    __syncthreads();
    DIAG_STAMP(0, 3);
    for (int i = 1; i + 1 < NC - 1; i += 2) {
      DIAG_STAMP(i, 0); mphase(P1, i, i + 1); DIAG_STAMP(i, 1); vfinish(P0, i + 1, i + 1); DIAG_STAMP(i, 2); __syncthreads(); DIAG_STAMP(i, 3);
      DIAG_STAMP(i + 1, 0); mphase(P0, i + 1, i + 2); DIAG_STAMP(i + 1, 1); vfinish(P1, i + 2, i + 2); DIAG_STAMP(i + 1, 2); __syncthreads(); DIAG_STAMP(i + 1, 3);
    }
  } else {
    DIAG_STAMP(0, 0);
    vfinish(P1, 1, 0);
    DIAG_STAMP(0, 1);
    __builtin_amdgcn_sched_barrier(0);
    mphase(P0, 0, 2);
    DIAG_STAMP(0, 2);
    __syncthreads();
    DIAG_STAMP(0, 3);
    for (int i = 1; i + 1 < NC - 1; i += 2) {
      DIAG_STAMP(i, 0); vfinish(P0, i + 1, i); DIAG_STAMP(i, 1); __builtin_amdgcn_sched_barrier(0); mphase(P1, i, i + 2); DIAG_STAMP(i, 2); __syncthreads(); DIAG_STAMP(i, 3);
      DIAG_STAMP(i + 1, 0); vfinish(P1, i + 2, i + 1); DIAG_STAMP(i + 1, 1); __builtin_amdgcn_sched_barrier(0); mphase(P0, i + 1, i + 3); DIAG_STAMP(i + 1, 2); __syncthreads(); DIAG_STAMP(i + 1, 3);
    }
    wload16(NC - 1);
    wload8(NC - 1);
  }
  DIAG_STAMP(NC - 1, 0);
  mphase(P1, NC - 1, -1);
  DIAG_STAMP(NC - 1, 1);
#undef CORR_STEP
#undef MAIN_STEP
#undef LDS_WAIT
#undef LDS_RD
  __syncthreads();   // the loop buffers are dead
  DIAG_STAMP(NC - 1, 3);
  DIAG_STAMP(30, 3);
  DIAG_RSTAMP(31, 2);

  constexpr float kAcc = kNegLog2e / kF16WScale;
  if constexpr (diag::kC8NoEpi) {
    float v = 0.f;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) v += acc[rb][cb][i];
    if (v == 123.456f) p.agg_m[0] = v;
    return;
  }
  // the pair (w, w ^ 4) holds the two K halves of column blocks cb0, cb0 + 1: wave w keeps block cb0 + kh and hands the other to its
  // partner; [receiving wave][16 pieces][64 lanes] x 16 bytes (a + b = b + a: both waves of a pair round alike)
  f32x16 keep[4][1];
  {
    f32x4* xb = reinterpret_cast<f32x4*>(smem + kOffLoop);
    f32x4* mine = xb + (size_t)wave * 1024 + lane;
    f32x4* theirs = xb + (size_t)(wave ^ 4) * 1024 + lane;
    auto give = [&](auto kc) {   // (compile-time register indices in both arms: kh is uniform over the wave)
      constexpr int G = 1 - decltype(kc)::value;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          theirs[(rb * 4 + q) * 64] = f32x4{acc[rb][G][4 * q], acc[rb][G][4 * q + 1], acc[rb][G][4 * q + 2], acc[rb][G][4 * q + 3]};
    };
    auto take = [&](auto kc) {
      constexpr int K = decltype(kc)::value;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 o = mine[(rb * 4 + q) * 64];
#pragma unroll
          for (int i = 0; i < 4; ++i) keep[rb][0][4 * q + i] = acc[rb][K][4 * q + i] + o[i];
        }
    };
    if (kh) give(P1); else give(P0);
    __syncthreads();
    if (kh) take(P1); else take(P0);
  }
  message_epilogue(p, L, keep, S, tile, tid, lane, wave, kAcc, cb0 + kh);
  DIAG_STAMP(31, 0);
}

// Scale exponents of a weight matrix from its largest |v| (c8_absmax_kernel, v = W * scale = what the fp16 stream holds):
// 2^s_hi max in [112, 224] (e4m3 tops out at 448), s_lo = s_hi + 11 (a remainder is at most 2^-11 of its head).
__device__ __forceinline__ int c8_shift(unsigned maxbits) {
  const float mx = fminf(__builtin_bit_cast(float, maxbits), 65504.f);
  int s_hi = 0;
  if (mx > 0.f) s_hi = (int)floorf(log2f(224.0f / mx));
  return s_hi > 40 ? 40 : (s_hi < -40 ? -40 : s_hi);
}
// e4m3 B fragments of the correction product for v_mfma_scale_f32_32x32x64_f8f6f4, one instruction per 32 hidden units:
//   out[((nb * KS32 + t) * 2 + piece) * 1024 + lane * 16 + j],  lane l: column 32 nb + (l & 31), K block h = l >> 5
//   block 0 holds e4m3(2^s_hi W_hi), block 1 e4m3(2^s_lo W_lo) of hidden units 32 t + [0, 32), W_hi = fp16(v), W_lo = v - W_hi;
//   register piece `piece` holds hidden units 16 piece .. + 15 of the block.
// Every thread derives s_hi from *maxbits itself; block 0 writes exps[0..1] = {127 - s_hi, 127 - s_lo}, the e8m0 bytes of the block
// scales the edge kernels read.
__global__ void pack_frags_c8w(const float* __restrict__ W, int Nout, int K, int ldw, int NP, int KP, unsigned char* __restrict__ out,
                               float scale, const unsigned* __restrict__ maxbits, int* __restrict__ exps) {
  __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1);   // MODE.FP16_OVFL: the conversions saturate
  const int KS32 = KP / 32;
  const int s_hi = c8_shift(*maxbits);
  if (blockIdx.x == 0 && threadIdx.x == 0) { exps[0] = 127 - s_hi; exps[1] = 127 - s_hi - 11; }
  const float inv_hi = __builtin_ldexpf(1.0f, -s_hi), inv_lo = __builtin_ldexpf(1.0f, -s_hi - 11);   // 2^-s: the cvt divides
  const size_t total = (size_t)(NP / 32) * KS32 * 2 * 64 * 8;   // byte PAIRS
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int jp = i & 7, lane = (i >> 3) & 63, piece = (i >> 9) & 1;
    const size_t f = i >> 10;
    const int t = f % KS32, nb = f / KS32;
    const int h = lane >> 5, n = 32 * nb + (lane & 31);
    const int k = 32 * t + 16 * piece + 2 * jp;
    float v[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float w = (n < Nout && k + q < K) ? W[(size_t)n * ldw + k + q] * scale : 0.f;
      w = fminf(fmaxf(w, -65504.f), 65504.f);
      const float hi = (float)(_Float16)w;
      v[q] = h ? w - hi : hi;
    }
    typedef __attribute__((ext_vector_type(2))) short i16x2_;
    i16x2_ rr = {0, 0};
    rr = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(rr, v[0], v[1], h ? inv_lo : inv_hi, false);
    reinterpret_cast<unsigned short*>(out)[i] = (unsigned short)rr.x;
  }
}

// largest |W scale| of the matrix as float bits (non-negative floats order like unsigned integers): grid-stride maximum, one
// atomicMax per workgroup into *maxbits (zeroed by the caller).  (The first build reduced in ONE workgroup: 0.87 ms per matrix,
// 7 ms of every TRAINING step, which repacks all layers -- profiles/r05u_train_f16c8_summary.txt.)
__global__ void c8_absmax_kernel(const float* __restrict__ W, int Nout, int K, int ldw, float scale, unsigned* __restrict__ maxbits) {
  __shared__ float red[256];
  float m = 0.f;
  const size_t total = (size_t)Nout * K;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float v = fabsf(W[(i / K) * ldw + (i % K)] * scale);
    m = v > m ? v : m;   // (a NaN weight never becomes the maximum: the scale stays finite)
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(maxbits, __builtin_bit_cast(unsigned, red[0]));
}

}  // namespace

int init_edge_f16c8w_attributes() {
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_c8w_kernel<false, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_c8wk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return EGNN_OK;
}

// shapes: hidden width 512 / 1024 (512-column workgroups), 256 message columns; p.w2x / p.w2m = the fp16 32-column streams,
// p.w2x_c8 / p.w2m_c8 = the e4m3 streams of pack_c8w_stream
bool edge_f16c8w_supported(const EdgeParams& p) {
  return (p.WxP == 512 || p.WxP == 1024) && p.MP == 256 && p.WmP % 128 == 0 && p.WmP >= 128 && p.w2x && p.w2m && p.w2x_c8 && p.w2m_c8 && p.c8_exp &&
         c8w_smem_bytes(p.WxP) <= 160 * 1024 && c8wk_smem_bytes(p.WmP) <= 160 * 1024 && (size_t)p.N * p.TC * 4 < ((size_t)1 << 32);
}

int launch_edge_f16c8w_x(const EdgeParams& p, hipStream_t st) {
  const int tiles = (p.E + kR - 1) / kR;
  const int grid = p.WxP == 1024 ? 8 * ((tiles + 3) / 4) : tiles;   // (1024: see the kernel's workgroup map)
  hipLaunchKernelGGL((edge_c8w_kernel<false, 2>), dim3(grid), dim3(kT), c8w_smem_bytes(p.WxP), st, p);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}
int launch_edge_f16c8w_m(const EdgeParams& p, hipStream_t st) {
  const int tiles = (p.E + kR - 1) / kR;
  hipLaunchKernelGGL(edge_c8wk_kernel, dim3(tiles), dim3(kT), c8wk_smem_bytes(p.WmP), st, p);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

// out: e4m3 fragment stream of NP x KP bytes x 2; exps: int[2] (e8m0 bytes of the block scales); maxbits: one scratch word
int pack_c8w_stream(const float* W, int Nout, int K, int ldw, int NP, int KP, void* out, float scale, int* exps, unsigned* maxbits,
                    hipStream_t st) {
  EGNN_HIP(hipMemsetAsync(maxbits, 0, sizeof(unsigned), st));
  hipLaunchKernelGGL(c8_absmax_kernel, dim3(128), dim3(256), 0, st, W, Nout, K, ldw, scale, maxbits);
  hipLaunchKernelGGL(pack_frags_c8w, dim3(256), dim3(256), 0, st, W, Nout, K, ldw, NP, KP, static_cast<unsigned char*>(out), scale,
                     maxbits, exps);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // namespace egnn

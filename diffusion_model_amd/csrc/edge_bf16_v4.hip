// Message-branch edge kernels on v_mfma_f32_32x32x16 (bf16 or fp16 operands), 128-edge tiles (gfx950): mlp_m and the
// attention gate (EquivariantGraphNeuralNetwork.py:13-18, :31-34, :55-61), one workgroup per tile holding all 256 message
// columns (8 wave64, one 32-column block per wave).  Forward, training forward and the backward's recompute pass.
//
// Same tile and prologue as the coordinate kernels of edge_bf16_v3.hip (edge_tile.h; why a 128-edge tile: see there); the
// K loop differs:
//   * v3 runs the two waves of a SIMD in opposite phase (multiply chunk c | build chunk c+1): the partner's vector work
//     hides under this wave's matrix work, but every wave still executes its OWN matrix phase and vector phase one after
//     the other, so a chunk costs (matrix 1.3 k + vector 1.0 k cycles) per wave however well the partners overlap.
//   * v4 interleaves inside each wave: between two groups of MFMAs (which only occupy the issue port for 8 of their 32
//     cycles) the wave finishes ONE activation of the chunk two ahead (SiLU(P[dst] + Q[src] + wd*d2) -> bf16), so its
//     vector work rides in its own MFMA shadow.  The activation chunks live in a 3-deep LDS ring: chunk c is multiplied
//     while chunk c+2 is written, and chunk c+1 (complete since the previous barrier) can already be read for the first
//     k-step of the next iteration BEFORE this iteration's barrier -- no LDS-latency bubble after the barrier.
//   * table rows are re-requested the moment their registers are free (row 0 mid-chunk, row 1 at the end) and have a
//     whole chunk to arrive.
//
// Per 16-deep k-step: 4 A fragments from the LDS ring, one B fragment straight from the packed weights, 4 MFMAs.
#include <type_traits>

#include "diag.h"
#include "edge_tile.h"

namespace egnn {

namespace {

#ifdef EGNN_EXP_WGSTAMP   // diagnostic build (diag.h, tools/fwd_stamps.py)
__device__ unsigned long long g_mwg_stamps[20000][6];
#define WG_STAMP(k) DIAG_WG_STAMP(g_mwg_stamps, 20000, k)
#define WG_STAMP_HW() DIAG_WG_STAMP_HW(g_mwg_stamps, 20000, 5)
#else
#define WG_STAMP(k)
#define WG_STAMP_HW()
#endif

using namespace tile128;
constexpr size_t kOffA1 = kOffLoop;      // ring of 3 activation chunks, then wd[KP] (the per-tile arrays: edge_tile.h)
constexpr int kRing = 3;
__host__ __device__ constexpr size_t v4_smem_bytes(int KP) { return kOffA1 + kRing * kChunkBytes + (size_t)KP * 4; }
static_assert(v4_smem_bytes(256) == 64960 && v4_smem_bytes(512) == 65984 && v4_smem_bytes(1024) == 68032,
              "LDS allocation of the message kernels");
static_assert(kStageBytes <= kRing * kChunkBytes, "store staging must fit the K-loop buffers");

#ifndef EGNN_V4_M_WAVES
#define EGNN_V4_M_WAVES 4   // waves per SIMD the message kernel is compiled for (4 = two workgroups per CU)
#endif
// BWD = true (message kernel): the training backward's recompute pass over a chunk of edges: the activation chunks are
// also written to HBM (s1_out) and the epilogue produces dL/d(a2m) through the gate instead of the segment sums.
// SAVE = true (message kernel): the training forward: also leaves the activation chunks (s1_out) and the scaled
// second-layer pre-activations (g_a2_out) in HBM (see edge_bf16_v3.hip).
// V8 = the MFMA operand type: bf16x8 (precision bf16) or f16x8 (precision fp16, plain forward only; kernels.h).
// CB and IS_M are kept in the argument list for the kernel's name only: one 32-column block per wave, message branch.
template <int CB, bool IS_M, bool BWD = false, bool SAVE = false, typename V8 = bf16x8>
__global__ __launch_bounds__(kTileThreads, (!BWD ? EGNN_V4_M_WAVES : 2)) void edge_kernel_bf16_v4(const EdgeParams p) {
  static_assert(CB == 1 && IS_M, "edge_bf16_v4.hip keeps the message kernels only, one 32-column block per wave "
                                 "(coordinate kernels: edge_x_m16.hip, edge_bf16_v3.hip)");
  static_assert(!((BWD || SAVE) && OpTraits<V8>::f16), "the training kernels keep bf16 activations");
  typedef typename OpTraits<V8>::elem elem;
  if constexpr (OpTraits<V8>::f16) f16_saturate_mode();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L(smem);
  char* s_a1 = smem + kOffA1;
  float* s_wd = reinterpret_cast<float*>(s_a1 + kRing * kChunkBytes);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int KP = p.WmP;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int e0 = tile * kR;
  const int nvalid = min(kR, p.E - e0);

  DIAG_STAMP_SETUP(p.stamps + ((size_t)8 + wave) * 32 * 4);
  DIAG_STAMP(30, 0);   // kernel entry
  WG_STAMP(0);
  prologue_rows(p, L, e0, nvalid, p.wdm, KP, s_wd, tid);

  DIAG_STAMP(30, 1);   // tile structure ready
  WG_STAMP(1);

  // ---- K-loop ----
  const int NC = KP / kChunkK;
  const BuildRows<2> b(p, L, tid, true, diag::drop_table_loads(p.dbg) ? 0u : (unsigned)((size_t)p.N * p.TC * 2));   // fp16 table
  const rsrc_t rs_w = make_rsrc(p.w2m, diag::drop_weight_loads(p.dbg) ? 0u : (unsigned)((size_t)p.MP * KP * 2));
  char* slot0 = s_a1 + ((size_t)b.kg * kRowPad + b.brow) * 16;
  char* slot1 = slot0 + 64 * 16;
  const unsigned lane16 = lane * 16u;
  // 32-bit LDS byte address of this lane's A-fragment slot in ring buffer 0
  const unsigned lds_a1_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(s_a1 + ((size_t)hh * kRowPad + r) * 16);
  const unsigned w0off = (unsigned)wave * (KP / 16) * 1024u;   // the wave's 32-column block of the packed weights

  f32x16 acc[4][1];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[rb][0][i] = 0.f;

  UnitH u0, u1;   // table rows of rows brow / brow + 64 for the chunk that is built next
  auto uload = [&](UnitH& u, const unsigned vd, const unsigned vs, const int cq) {
    const int c = cq < NC ? cq : NC - 1;                    // past the end: a harmless repeat of the last chunk
    const unsigned kb = (unsigned)c * kChunkK * 2u;
    unith_load(u, b.tab, vd, vs, b.offP + kb, b.offQ + kb);
  };
  // chunks 0 and 1 are built up front (ring slots 0 and 1)
  // backward: the activation chunk also goes to HBM, 16 bytes per thread, 128 contiguous bytes per row and chunk
  auto s1_store = [&](const V8 ov, const int row, const int c) {
    if (row < nvalid)
      *reinterpret_cast<V8*>(static_cast<__bf16*>(p.s1_out) + (size_t)(e0 + row) * KP + c * kChunkK + b.kg * 8) = ov;
  };
  // chunks 0 and 1: all four table pieces and the first weight fragments are requested, THEN the segment structure of the tile
  // is worked out (two barriers, waves 0 and 1 only) while they are in flight, then the activations are finished (as in
  // edge_x_m16.hip; the segment modes' row_ptr loads ride under the first chunk of the K loop)
  UnitH u2, u3;
  uload(u0, b.vdst0, b.vsrc0, 0); uload(u1, b.vdst1, b.vsrc1, 0);
  uload(u2, b.vdst0, b.vsrc0, 1); uload(u3, b.vdst1, b.vsrc1, 1);
  // weight fragments, requested BQD k-steps ahead of their use (a whole chunk for the recompute kernel; the forward
  // kernels, compiled for <= 128 VGPRs so that two workgroups share a CU, keep 2 -- the other workgroup covers the rest)
  constexpr int BQD = (!BWD && EGNN_V4_M_WAVES >= 4) ? 2 : 4;
  V8 bq[BQD];
#pragma unroll
  for (int s = 0; s < BQD; ++s) bq[s] = ldbuf_v8<V8>(rs_w, lane16, w0off + (unsigned)s * 1024u);
  const int S = prologue_segments<false>(p, L, e0, nvalid, tid, lane, wave);
  {
    const V8 o0 = unith_finish<V8>(u0, s_wd + b.kg * 8, b.d2r0, slot0);
    const V8 o1 = unith_finish<V8>(u1, s_wd + b.kg * 8, b.d2r1, slot1);
    if constexpr (BWD || SAVE) { s1_store(o0, b.brow, 0); s1_store(o1, b.brow + 64, 0); }
  }
  {
    const V8 o0 = unith_finish<V8>(u2, s_wd + kChunkK + b.kg * 8, b.d2r0, slot0 + kChunkBytes);
    const V8 o1 = unith_finish<V8>(u3, s_wd + kChunkK + b.kg * 8, b.d2r1, slot1 + kChunkBytes);
    if constexpr (BWD || SAVE) { s1_store(o0, b.brow, 1); s1_store(o1, b.brow + 64, 1); }
  }
  uload(u0, b.vdst0, b.vsrc0, 2); uload(u1, b.vdst1, b.vsrc1, 2);
  const int my_mode = tid < S ? segment_mode(p, L, e0, tid) : 0;   // stored after the first chunk
  __syncthreads();

  // ring offsets (bytes): chunk c is read at off_cur, chunk c+1 at off_nxt, chunk c+2 is written at off_wr
  unsigned off_cur = 0u, off_nxt = (unsigned)kChunkBytes, off_wr = 2u * (unsigned)kChunkBytes;
  V8 a[4];
  TILE_LDS_RD(a[0], lds_a1_base, 0); TILE_LDS_RD(a[1], lds_a1_base, 512); TILE_LDS_RD(a[2], lds_a1_base, 1024); TILE_LDS_RD(a[3], lds_a1_base, 1536);

  // One chunk.  16 groups (k-step s, row block rb): wait for a[rb] (LDS returns in order: the 3 younger refills may
  // still fly), the MFMA, refill a[rb] in place for the next k-step (from the NEXT chunk's buffer after the last
  // k-step), and ONE activation of chunk c+2 in two halves of ~16 issue cycles, each behind an MFMA: an in-order wave can
  // only use the 24 free issue cycles of an MFMA's 32 if the fillers sit BETWEEN two MFMAs in program order.
  // sched_barrier(0) pins this order; inside a half the compiler schedules freely.
  auto chunk = [&](const int c, const bool build, const bool last) {
    DIAG_STAMP(c, 0);
    const unsigned abase = lds_a1_base + off_cur, nbase = lds_a1_base + off_nxt;
    f16x8 t;
    V8 o;
    const float* wdc = s_wd + (c + 2) * kChunkK + b.kg * 8;   // d^2 column of the first layer for this thread's 8 hidden units
    // The 16 activations a thread owes to chunk c+2 are finished 4 per k-step, as a software pipeline over the 8 MFMA
    // gaps of the k-step: every gap issues ~16 cycles of INDEPENDENT vector instructions whose operands were produced at
    // least one gap earlier (an in-order wave stalls on a dependent transcendental otherwise), between two MFMAs in
    // program order (that is where an in-order wave can use the 24 issue cycles an MFMA leaves free of its 32):
    //   gap 0: 4 x fma_mix (pre-activation)   1-2: 2 x exp2 each   3: 4 x add 1   4-5: 2 x rcp each   6: 4 x mul
    //   gap 7: bf16 pack; every second k-step completes a 16-byte LDS slot and re-requests the consumed table row.
    float pu[4], pe[4];
#define STAGE(S, Q)                                                                                           \
    if (build) {                                                                                              \
      constexpr int e0_ = 4 * ((S) & 1);   /* first element of this k-step inside its unit */                 \
      if ((Q) == 0) {                                                                                         \
        if ((S) == 0) t = u0.p + u0.q;                                                                        \
        if ((S) == 2) t = u1.p + u1.q;                                                                        \
        const f32x4 wv_ = *reinterpret_cast<const f32x4*>(wdc + e0_);                                         \
        _Pragma("unroll") for (int k = 0; k < 4; ++k)                                                         \
          pu[k] = fmaf(wv_[k], (S) < 2 ? b.d2r0 : b.d2r1, (float)t[e0_ + k]);                                     \
      }                                                                                                       \
      if ((Q) == 1) { pe[0] = __builtin_amdgcn_exp2f(pu[0]); pe[1] = __builtin_amdgcn_exp2f(pu[1]); }         \
      if ((Q) == 2) { pe[2] = __builtin_amdgcn_exp2f(pu[2]); pe[3] = __builtin_amdgcn_exp2f(pu[3]); }         \
      if ((Q) == 3) { _Pragma("unroll") for (int k = 0; k < 4; ++k) pe[k] = 1.0f + pe[k]; }                   \
      if ((Q) == 4) { pe[0] = __builtin_amdgcn_rcpf(pe[0]); pe[1] = __builtin_amdgcn_rcpf(pe[1]); }           \
      if ((Q) == 5) { pe[2] = __builtin_amdgcn_rcpf(pe[2]); pe[3] = __builtin_amdgcn_rcpf(pe[3]); }           \
      if ((Q) == 6) { _Pragma("unroll") for (int k = 0; k < 4; ++k) pu[k] = pu[k] * pe[k]; }                  \
      if ((Q) == 7) {                                                                                         \
        _Pragma("unroll") for (int k = 0; k < 4; ++k) o[e0_ + k] = (elem)pu[k];                             \
        if ((S) == 1) { *reinterpret_cast<V8*>(slot0 + off_wr) = o; uload(u0, b.vdst0, b.vsrc0, c + 3);       \
                        if constexpr (BWD || SAVE) s1_store(o, b.brow, c + 2); }                                        \
        if ((S) == 3) { *reinterpret_cast<V8*>(slot1 + off_wr) = o; uload(u1, b.vdst1, b.vsrc1, c + 3);       \
                        if constexpr (BWD || SAVE) s1_store(o, b.brow + 64, c + 2); }                                   \
      }                                                                                                       \
    }
#define GROUP(S, RB)                                                                                          \
    {                                                                                                         \
      if (!last || (S) < 3 || (RB) == 0) TILE_LDS_WAIT(3);                                                    \
      else if ((RB) == 1) TILE_LDS_WAIT(2);                                                                   \
      else if ((RB) == 2) TILE_LDS_WAIT(1);                                                                   \
      else TILE_LDS_WAIT(0);                                                                                  \
      asm volatile("" : "+v"(a[RB]));                                                                         \
      acc[RB][0] = mfma32(a[RB], bq[(S) % BQD], acc[RB][0]);                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
      STAGE(S, 2 * (RB))                                                                                      \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
      if ((S) < 3) TILE_LDS_RD(a[RB], abase, ((S) + 1) * 4128 + (RB) * 512);                                  \
      else if (!last) TILE_LDS_RD(a[RB], nbase, (RB) * 512);                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
      STAGE(S, 2 * (RB) + 1)                                                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
    }
#ifdef EGNN_V4_PRIO_FLIP   /* alternate which of the two waves of a SIMD wins arbitration, per k-step */
#define KPRIO(S) if (((((S) & 1) ^ (wave >> 2)) & 1) != 0) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
#else
#define KPRIO(S)
#endif
#define KSTEP(S)                                                                                              \
    KPRIO(S)                                                                                                  \
    GROUP(S, 0) GROUP(S, 1) GROUP(S, 2) GROUP(S, 3)                                                           \
    if (!last || (S) + BQD < 4)   /* k-step c*4 + S + BQD: this chunk's or the next one's */                  \
      bq[(S) % BQD] = ldbuf_v8<V8>(rs_w, lane16, w0off + (unsigned)(c * 4 + (S) + BQD) * 1024u);
    KSTEP(0) KSTEP(1)
    DIAG_STAMP(c, 1);
    KSTEP(2) KSTEP(3)
    DIAG_STAMP(c, 2);
#undef KSTEP
#undef GROUP
#undef STAGE
    const unsigned tmp = off_cur; off_cur = off_nxt; off_nxt = off_wr; off_wr = tmp;
  };
  // (the steady-state loop body is branch-free so that hipcc's waitcnt insertion keeps counted vmcnt waits across
  // the back edge instead of draining the queue at every control-flow join)
  DIAG_STAMP(30, 2);   // chunks 0 and 1 built, first weights requested
  WG_STAMP(2);
  DIAG_RSTAMP(31, 1);
  for (int c = 0; c < NC - 2; ++c) {
    chunk(c, true, false);
    if (c == 0 && tid < S) L.seg_mode[tid] = my_mode;
    __syncthreads(); DIAG_STAMP(c, 3);
  }
  chunk(NC - 2, false, false);
  __syncthreads();
  DIAG_STAMP(NC - 2, 3);
  chunk(NC - 1, false, true);
  __syncthreads();
  DIAG_STAMP(NC - 1, 3);
  DIAG_RSTAMP(31, 2);
  DIAG_STAMP(30, 3);   // K loop done
  WG_STAMP(3);

  __bf16* const a2_out = static_cast<__bf16*>(p.g_a2_out) + (size_t)e0 * p.MP + 32 * wave;   // BWD: dL/da2, SAVE: t2
  if constexpr (BWD) {
    // ---- backward of the message head (:57-60): m = SiLU(a2), z = wa . m + ba, gate = sigmoid(z), out = m * gate;
    //      with g = dL/d(sum_m[i]):  dL/dm = g * gate + (g . m) gate (1 - gate) wa,  dL/da2 = dL/dm * SiLU'(a2) ----
    const int ncol = 32 * wave + r;
    const float bb = p.b2m[ncol], wan = p.wa[ncol] * kNegLog2e;   // packed vectors carry the -log2(e) / -1/log2(e) scales
    const rsrc_t rs_gm = make_rsrc(p.g_sum_m, (unsigned)((size_t)p.N * p.MP * 4));
    const unsigned gcol = 4u * (unsigned)ncol, gld = 4u * (unsigned)p.MP;
    auto gm_at = [&](const int row) {   // dL/d(sum_m)[dst(row)][ncol]
      return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_gm, (unsigned)L.dst[row] * gld + gcol, 0, 0));
    };
    // pass 1: row sums z = wa . m and d = g . m (two halves of 64 rows to bound the live registers)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      float vz[32], vd[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const int rb = 2 * hf + (q >> 4), i = q & 15, row = 32 * rb + acc_row(i, lane);
        float m, ds;
        silu_grad_s(fmaf(acc[rb][0][i], kNegLog2e, bb), m, ds);
        vz[q] = wan * m;
        vd[q] = gm_at(row) * m;
      }
      const float tz = butterfly32(vz, lane), td = butterfly32(vd, lane);
      const int row = 64 * hf + 32 * (r >> 4) + acc_row(r & 15, lane);   // row of value index q = lane & 31 of this half
      L.part[wave * kR + row] = tz;
      L.gseg[wave * kR + row] = td;
    }
    __syncthreads();
    if (tid < kR) {
      float z = p.scal[1], d = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) { z += L.part[w * kR + tid]; d += L.gseg[w * kR + tid]; }
      const float gate = sigmoid_f(z);
      const bool valid = tid < nvalid;
      L.val[tid] = gate;
      L.d2[tid] = valid ? d * gate * (1.0f - gate) : 0.f;   // coef (the geometry is no longer needed)
    }
    __syncthreads();
    if (wave == 2) {   // g_ba = sum over edges of coef
      float v = L.d2[lane] + L.d2[lane + 64];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if (lane == 0) atomicAdd(p.g_scalar, v);
    }
    // pass 2: dL/da2, column sums, store
    float cs_b = 0.f, cs_w = 0.f;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = 32 * rb + acc_row(i, lane);
        float m, ds;
        silu_grad_s(fmaf(acc[rb][0][i], kNegLog2e, bb), m, ds);
        const float coef = L.d2[row];
        const float g = row < nvalid ? fmaf(gm_at(row), L.val[row], coef * wan) * ds : 0.f;
        cs_b += g;
        cs_w = fmaf(coef, m, cs_w);
        acc[rb][0][i] = g;
      }
    cs_b += __shfl_xor(cs_b, 32);
    cs_w += __shfl_xor(cs_w, 32);
    if (hh == 0) { atomicAdd(p.g_col_a + ncol, cs_b); atomicAdd(p.g_col_b + ncol, cs_w); }   // g_b2m, g_wa
    stage_store_rows(acc, s_a1, a2_out, (size_t)p.MP, nvalid, lane, wave);   // dL/da2 as row-major bf16
  } else {
    // ---- mlp_m epilogue: m = SiLU(acc + b2), gate = sigmoid(wa . m + ba) (:31-34, :59-60) ----
    if constexpr (SAVE) {   // scaled pre-activations to HBM first (the ring is free behind the last chunk's barrier)
      const float bb = p.b2m[32 * wave + r];
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[rb][0][i] = fmaf(acc[rb][0][i], kNegLog2e, bb);
      // stage_store_rows of edge_tile.h written out: behind any call boundary here, hipcc spills a register of this
      // 128-VGPR kernel around the K loop
      __bf16* stg = reinterpret_cast<__bf16*>(s_a1) + (size_t)wave * 32 * 72;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const f32x16 blk[2] = {acc[rb][0], acc[rb][0]};
        store_block_bf16(blk, 1, stg, a2_out + (size_t)(32 * rb) * p.MP, (size_t)p.MP, nvalid - 32 * rb, lane);
      }
    }
    message_epilogue<SAVE>(p, L, acc, S, tile, tid, lane, wave, kNegLog2e / OpTraits<V8>::wscale);
  }
  DIAG_STAMP(31, 0);   // epilogue done
  WG_STAMP(4);
  WG_STAMP_HW();
}

template <bool BWD = false, bool SAVE = false, typename V8 = bf16x8>
int launch_v4(const EdgeParams& p, int blocks, size_t smem, hipStream_t st) {
  hipLaunchKernelGGL((edge_kernel_bf16_v4<1, true, BWD, SAVE, V8>), dim3(blocks), dim3(kTileThreads), smem, st, p);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // namespace

int init_edge_bf16_v4_attributes() {
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v4<1, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v4<1, true, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v4<1, true, false, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v4<1, true, false, false, f16x8>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return EGNN_OK;
}

// the message kernels' own conditions: 256 message columns, whole chunks and at least 3 of them (the K loop has a
// steady-state iteration: the segment modes are stored there), the packed mlp_m.2 stream, the LDS of the ring, and a
// first-layer table the 32-bit row offsets reach
bool edge_bf16_v4_supported(const EdgeParams& p) {
  return p.MP == 256 && p.WmP % 64 == 0 && p.WmP >= 192 && p.w2m && v4_smem_bytes(p.WmP) <= 160 * 1024 &&
         (size_t)p.N * p.TC * 4 < ((size_t)1 << 32);
}

// backward recompute of the message branch over the chunk of edges described by p
int launch_edge_bf16_v4_m_bwd(const EdgeParams& p, hipStream_t st) {
  const int tiles = (p.E + kR - 1) / kR;
  return launch_v4<true>(p, tiles, v4_smem_bytes(p.WmP), st);
}

// message kernel only; f16: p.w2m = the fp16 fragment stream (scaled by -2^8 / log2(e)); save (bf16 only): the training forward,
// p.s1_out / p.g_a2_out receive the activations and the scaled pre-activations
int launch_edge_v4_m(const EdgeParams& p, hipStream_t st, bool f16, bool save) {
  const int tiles = (p.E + kR - 1) / kR;
  const size_t sm = v4_smem_bytes(p.WmP);
  if (save && f16) { set_error("edge_bf16_v4: the training forward runs on bf16 operands"); return EGNN_EINVAL; }
  if (save) return launch_v4<false, true>(p, tiles, sm, st);
  if (f16) return launch_v4<false, false, f16x8>(p, tiles, sm, st);
  return launch_v4<>(p, tiles, sm, st);
}

}  // namespace egnn

#ifdef EGNN_EXP_WGSTAMP
extern "C" int egnn_debug_mwg_stamps(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(egnn::g_mwg_stamps), sizeof(unsigned long long) * 20000 * 6) == hipSuccess ? 0 : -1;
}
#endif

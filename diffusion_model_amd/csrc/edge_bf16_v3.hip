// Coordinate-branch edge kernels on v_mfma_f32_32x32x16_bf16, 128-edge tiles with the output columns split over
// workgroups (gfx950).
//
// Why the tile: at a 64-edge tile every CU must stream 40 KiB of weight fragments per 640 MFMA-cycles = 64 B/clk, the
// per-CU L2 fill rate, and the tile cannot grow because the fp32 accumulators of all output columns already fill the
// register file.  Here a workgroup holds 128 edges x 256 CB columns of mlp_x.2 (EquivariantGraphNeuralNetwork.py:19-25,
// :62-65), a tile is processed by WxP / (256 CB) workgroups (column shares), and every weight fragment feeds 4 row blocks.
// Each share rebuilds the SiLU(P[dst] + Q[src] + wd*d2) activations it needs -- the price of not exchanging them between
// workgroups; s_ij is linear in the column shares, so the shares write separate coordinate sums that node_post adds: no
// inter-workgroup communication, bitwise deterministic.  (The message branch of the same tile: edge_bf16_v4.hip.)
//
// What this file still holds: the forward and training-forward kernels for WxP = 256 (wider coordinate MLPs run on
// edge_x_m16.hip) and the backward's recompute kernels for every width.
//
// Workgroup = 8 wave64 (2 per SIMD), wave w owns 32 CB columns; per 16-deep k-step: 4 A fragments from the double-buffered
// LDS activation chunk, CB B fragments straight from the packed weights, 4 CB MFMAs.  Tile prologue, build-thread setup,
// the phase-opposed chunk loop, the head and the segment sums are the shared ones of edge_tile.h.
#include <type_traits>

#include "diag.h"
#include "edge_tile.h"

namespace egnn {

namespace {

using namespace tile128;
constexpr size_t kOffA1 = kOffLoop;      // 2 activation chunks, then wd[KP] (the per-tile arrays: edge_tile.h)
// The BWD / SAVE epilogues stage their row-major bf16 stores in the K-loop region: the allocation of a kernel that stages is
// max(K-loop buffers, staging) -- the K-loop buffers alone cover the staging only at KP = 1024.
__host__ __device__ constexpr size_t v3_smem_bytes(int KP, bool staged = true) {
  const size_t loop = 2 * kChunkBytes + (size_t)KP * 4;
  return kOffA1 + (staged && kStageBytes > loop ? kStageBytes : loop);
}
static_assert(v3_smem_bytes(256) == 51264 && v3_smem_bytes(512) == 51264 && v3_smem_bytes(1024) == 51520 &&
              v3_smem_bytes(256, false) == 48448, "LDS allocation of the coordinate kernels");

// BWD = true: the training backward's recompute pass over a chunk of edges (egcl_backward_edge_recompute).  Same
// prologue and K loop; the activation chunks are also written to HBM (s1_out: the wgrad of mlp_x.2 needs them as a GEMM
// operand over ALL edges), and the epilogue turns the accumulators into dL/d(a2) instead of segment sums.
// SAVE = true: the training FORWARD (egcl_forward_save): the forward kernel as it is, which also leaves the activation
// chunks (s1_out) and the scaled second-layer pre-activations -log2(e) * (a2 + b2) (g_a2_out) in HBM, so that the backward
// needs no recompute pass (egcl_backward_heads_saved turns the pre-activations into dL/da2 in place).
// IS_M is kept in the argument list for the kernel's name only: this is the coordinate kernel.
template <int CB, bool IS_M, bool BWD = false, bool SAVE = false>
__global__ __launch_bounds__(kTileThreads, 2) void edge_kernel_bf16_v3(const EdgeParams p) {
  static_assert(!IS_M, "edge_bf16_v3.hip keeps the coordinate kernels only (message kernels: edge_bf16_v4.hip)");
  static_assert(CB == 1 || CB == 2, "one or two 32-column blocks per wave");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L(smem);
  char* s_a1 = smem + kOffA1;
  float* s_wd = reinterpret_cast<float*>(s_a1 + 2 * kChunkBytes);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int KP = p.WxP;
  const int nsplit = p.WxP / (256 * CB);
  const int j = xcd_tile(blockIdx.x, gridDim.x);
  const int tile = j / nsplit, half = j - tile * nsplit;
  const int e0 = tile * kR;
  const int nvalid = min(kR, p.E - e0);

  DIAG_STAMP_SETUP(p.stamps + (size_t)wave * 32 * 4);
  DIAG_STAMP(30, 0);   // kernel entry
  const int S = prologue(p, L, e0, nvalid, p.wdx, KP, s_wd, tid, lane, wave);
  if constexpr (BWD) {   // dL/ds_e = dL/d(sum_x[i]) . (x_i - x_j)   (:64, xm = (x_i - x_j) * s); read behind the K loop's barriers
    if (tid < kR) {
      const int d = L.dst[tid];
      L.gseg[tid] = tid < nvalid ? (p.g_sum_x[3 * d] * L.diff[tid] + p.g_sum_x[3 * d + 1] * L.diff[kR + tid] +
                                    p.g_sum_x[3 * d + 2] * L.diff[2 * kR + tid]) : 0.f;
    }
  }

  DIAG_STAMP(30, 1);   // tile structure ready

  // ---- K-loop ----
  const int NC = KP / kChunkK, KS = KP / 16;
  const BuildRows<2> b(p, L, tid, false, diag::drop_table_loads(p.dbg) ? 0u : (unsigned)((size_t)p.N * p.TC * 2));   // fp16 table
  const rsrc_t rs_w = make_rsrc(p.w2x, diag::drop_weight_loads(p.dbg) ? 0u : (unsigned)((size_t)p.WxP * KP * 2));
  char* slot0 = s_a1 + ((size_t)b.kg * kRowPad + b.brow) * 16;
  char* slot1 = slot0 + 64 * 16;
  const unsigned lane16 = lane * 16u;
  // 32-bit LDS byte address of this lane's A-fragment slot in activation buffer 0
  const unsigned lds_a1_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(s_a1 + ((size_t)hh * kRowPad + r) * 16);
  const int colblk0 = half * 8 * CB + wave * CB;   // first 32-column block of this wave
  const unsigned w0 = (unsigned)colblk0 * KS * 1024u;

  f32x16 acc[4][CB];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[rb][cb][i] = 0.f;

  // backward: the activation chunk also goes to HBM, 16 bytes per thread, 128 contiguous bytes per row and chunk
  // (the column-split coordinate workgroups build the same activations: only share 0 stores them)
  auto s1_store = [&](const bf16x8 o0, const bf16x8 o1, const int c) {
    if (half != 0) return;
    __bf16* base = static_cast<__bf16*>(p.s1_out) + (size_t)e0 * KP + c * kChunkK + b.kg * 8;
    if (b.brow < nvalid) *reinterpret_cast<bf16x8*>(base + (size_t)b.brow * KP) = o0;
    if (b.brow + 64 < nvalid) *reinterpret_cast<bf16x8*>(base + (size_t)(b.brow + 64) * KP) = o1;
  };
  {  // chunk 0
    UnitH u;
    unith_load(u, b.tab, b.vdst0, b.vsrc0, b.offP, b.offQ);
    const bf16x8 o0 = unith_finish(u, s_wd + b.kg * 8, b.d2r0, slot0);
    unith_load(u, b.tab, b.vdst1, b.vsrc1, b.offP, b.offQ);
    const bf16x8 o1 = unith_finish(u, s_wd + b.kg * 8, b.d2r1, slot1);
    if constexpr (BWD || SAVE) s1_store(o0, o1, 0);
  }
  bf16x8 bq[4][CB];   // weight fragments of the 4 k-steps of the current chunk
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) bq[s][cb] = ldbuf_bf16x8(rs_w, lane16, w0 + ((unsigned)cb * KS + s) * 1024u);
  __syncthreads();

  // matrix phase of chunk c: 4 k-steps x (4 row blocks x CB column blocks)
  // Operand pipeline of the matrix phase: the weight fragments of k-step s of chunk c+1 are requested right
  // after the MFMAs of k-step s of chunk c were issued (a whole chunk = 4 k-steps of distance, enough to cover
  // an L2 round trip under load), the LDS A fragments one k-step ahead.
  auto mphase = [&](const int c, const bool last) {
    // a[rb] is refilled in place for k-step s+1 right after the MFMAs of (s, rb) were issued and flies under the next 3
    // row blocks' MFMAs (a scalar load in flight only makes the counted wait conservative).
    const unsigned abase = lds_a1_base + (unsigned)(c & 1) * (unsigned)kChunkBytes;
    bf16x8 a[4];
    TILE_LDS_RD(a[0], abase, 0); TILE_LDS_RD(a[1], abase, 512); TILE_LDS_RD(a[2], abase, 1024); TILE_LDS_RD(a[3], abase, 1536);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        // LDS returns in order: at most 3 younger reads may still be in flight when a[rb] is consumed
        if (s < 3 || rb == 0) TILE_LDS_WAIT(3);
        else if (rb == 1) TILE_LDS_WAIT(2);
        else if (rb == 2) TILE_LDS_WAIT(1);
        else TILE_LDS_WAIT(0);
        asm volatile("" : "+v"(a[rb]));   // uses of a[rb] stay below the wait
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rb], bq[s][cb], acc[rb][cb], 0, 0, 0);
        // refill a[rb] in place for the next k-step (the MFMAs above have read it at issue)
        if (s == 0) { if (rb == 0) TILE_LDS_RD(a[0], abase, 4128); if (rb == 1) TILE_LDS_RD(a[1], abase, 4128 + 512); if (rb == 2) TILE_LDS_RD(a[2], abase, 4128 + 1024); if (rb == 3) TILE_LDS_RD(a[3], abase, 4128 + 1536); }
        if (s == 1) { if (rb == 0) TILE_LDS_RD(a[0], abase, 8256); if (rb == 1) TILE_LDS_RD(a[1], abase, 8256 + 512); if (rb == 2) TILE_LDS_RD(a[2], abase, 8256 + 1024); if (rb == 3) TILE_LDS_RD(a[3], abase, 8256 + 1536); }
        if (s == 2) { if (rb == 0) TILE_LDS_RD(a[0], abase, 12384); if (rb == 1) TILE_LDS_RD(a[1], abase, 12384 + 512); if (rb == 2) TILE_LDS_RD(a[2], abase, 12384 + 1024); if (rb == 3) TILE_LDS_RD(a[3], abase, 12384 + 1536); }
      }
      if (!last) {
        const unsigned ksn = (unsigned)((c + 1) * 4 + s) * 1024u;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) bq[s][cb] = ldbuf_bf16x8(rs_w, lane16, w0 + (unsigned)cb * KS * 1024u + ksn);
      }
      if (s == 0) DIAG_STAMP2(c, 2, wave < 4);
    }
  };
  // Table-row units: set A serves every chunk (depth 1) or the odd chunks (depth 2), set B the even chunks of
  // the depth-2 pipeline.  Depth 2 = rows requested two chunks ahead; one 32-column block per wave leaves the registers
  // for it (and has a chunk period shorter than an L2 round trip under load), two blocks per wave do not.
  constexpr bool DEPTH2 = (CB == 1);
  UnitH ua0, ua1, ub0, ub1;
  auto vload = [&](UnitH& x0, UnitH& x1, const int cq) {   // table rows for the activations of chunk cq (clamped)
    const int c = cq < NC ? cq : NC - 1;                    // past the end: a harmless repeat of the last chunk
    const unsigned kb = (unsigned)c * kChunkK * 2u;
    unith_load(x0, b.tab, b.vdst0, b.vsrc0, b.offP + kb, b.offQ + kb);
    unith_load(x1, b.tab, b.vdst1, b.vsrc1, b.offP + kb, b.offQ + kb);
  };
  auto vfinish = [&](const UnitH& x0, const UnitH& x1, const int c) {  // SiLU + bf16 pack of chunk c into its LDS buffer
    const size_t nbuf = (size_t)(c & 1) * kChunkBytes;
    // vector work wins issue arbitration over the partner wave's MFMAs (which only need 1 slot in 4)
    __builtin_amdgcn_s_setprio(3);
    const bf16x8 o0 = unith_finish(x0, s_wd + c * kChunkK + b.kg * 8, b.d2r0, slot0 + nbuf);
    DIAG_STAMP2(c - 1, 1, wave >= 4);
    const bf16x8 o1 = unith_finish(x1, s_wd + c * kChunkK + b.kg * 8, b.d2r1, slot1 + nbuf);
    DIAG_STAMP2(c - 1, 2, wave >= 4);
    __builtin_amdgcn_s_setprio(0);
    if constexpr (BWD || SAVE) s1_store(o0, o1, c);
  };
  DIAG_STAMP(30, 2);   // chunk 0 built, first weights requested
  DIAG_RSTAMP(31, 1);
  if constexpr (!DEPTH2) {
    phase_opposed_k_loop(NC, wave, mphase, [&](const int c) { vfinish(ua0, ua1, c); }, [&](const int c) { vload(ua0, ua1, c); });
  } else {
    // phase_opposed_k_loop of edge_tile.h unrolled by two for the two unit sets: a set is reloaded for the chunk three
    // ahead as soon as it has been consumed
    auto run = [&](auto step) {
      vload(ua0, ua1, 1);
      vload(ub0, ub1, 2);
      int i = 0;
      for (; i + 1 <= NC - 2; i += 2) { step(ua0, ua1, i); step(ub0, ub1, i + 1); }
      if (i <= NC - 2) step(ua0, ua1, i);
      mphase(NC - 1, true);
      __syncthreads();
    };
    if (wave < 4) {
      run([&](UnitH& x0, UnitH& x1, const int i) {   // chunk i: multiply, build i+1, request the set's next chunk
        DIAG_STAMP(i, 0);
        DIAG_STAMP2(i, 1, true);
        mphase(i, false);
        DIAG_STAMP1(i, 1);
        DIAG_STAMP2(i, 3, true);
        vfinish(x0, x1, i + 1);
        vload(x0, x1, i + 3);
        DIAG_STAMP1(i, 2);
        __syncthreads();
        DIAG_STAMP1(i, 3);
      });
    } else {
      run([&](UnitH& x0, UnitH& x1, const int i) {   // build i+1, request the set's next chunk, multiply chunk i
        DIAG_STAMP(i, 0);
        vfinish(x0, x1, i + 1);
        vload(x0, x1, i + 3);
        __builtin_amdgcn_sched_barrier(0);
        DIAG_STAMP1(i, 1);
        DIAG_STAMP2(i, 3, true);
        mphase(i, false);
        DIAG_STAMP1(i, 2);
        __syncthreads();
        DIAG_STAMP1(i, 3);
      });
    }
  }
  DIAG_STAMP(30, 3);   // K loop done
  DIAG_RSTAMP(31, 2);

  if constexpr (BWD) {
    // ---- backward of the mlp_x head (:62-65): s = w3 . SiLU(a2) + b3, dL/da2[e][n] = dL/ds_e * w3[n] * SiLU'(a2[e][n]) ----
    const float* s_gsc = L.gseg;
    float part[64];
#pragma unroll
    for (int q = 0; q < 64; ++q) part[q] = 0.f;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int n = 32 * (colblk0 + cb) + r;
      const float bb = p.b2x[n], w3n = p.w3x[n] * kNegLog2e;   // packed vectors carry the -log2(e) / -1/log2(e) scales
      float cs_b = 0.f, cs_w = 0.f;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float sv, ds;
          silu_grad_s(fmaf(acc[rb][cb][i], kNegLog2e, bb), sv, ds);
          part[rb * 16 + i] = fmaf(w3n, sv, part[rb * 16 + i]);
          const float gsc = s_gsc[32 * rb + acc_row(i, lane)];
          const float g = gsc * w3n * ds;
          cs_b += g;
          cs_w = fmaf(gsc, sv, cs_w);
          acc[rb][cb][i] = g;
        }
      cs_b += __shfl_xor(cs_b, 32);
      cs_w += __shfl_xor(cs_w, 32);
      if (hh == 0) { atomicAdd(p.g_col_a + n, cs_b); atomicAdd(p.g_col_b + n, cs_w); }   // g_b2x, g_w3
    }
    {
      float lo[32], hi[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) { lo[q] = part[q]; hi[q] = part[32 + q]; }
      const float t0 = butterfly32(lo, lane), t1 = butterfly32(hi, lane);
      const int row = 32 * (r >> 4) + acc_row(r & 15, lane);   // row of value index q = lane & 31
      L.part[wave * kR + row] = t0;
      L.part[wave * kR + 64 + row] = t1;
    }
    __syncthreads();   // also: every wave is done with the K-loop buffers (reused as store staging below)
    if (tid < kR) {
      float v = half == 0 ? p.scal[0] : 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) v += L.part[w * kR + tid];
      if (tid < nvalid) p.s_half_out[(size_t)half * p.E + e0 + tid] = v;
    }
    if (half == 0 && wave == 2) {   // g_b3 = sum over edges of dL/ds
      float v = s_gsc[lane] + s_gsc[lane + 64];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if (lane == 0) atomicAdd(p.g_scalar, v);
    }
    stage_store_rows(acc, s_a1, static_cast<__bf16*>(p.g_a2_out) + (size_t)e0 * p.WxP + 32 * colblk0, (size_t)p.WxP, nvalid, lane, wave);   // dL/da2 as row-major bf16
  } else {
    // ---- mlp_x epilogue: s[row] = [b3] + sum_n w3[n] * SiLU(acc + b2[n]) over this workgroup's columns ----
    if constexpr (SAVE) {   // the scaled pre-activations go to HBM first (the K-loop buffers are free: every wave passed
                            // the barrier behind the last matrix phase), the accumulators then hold them for the SiLU
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const float bb = p.b2x[32 * (colblk0 + cb) + r];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[rb][cb][i] = fmaf(acc[rb][cb][i], kNegLog2e, bb);
      }
      stage_store_rows(acc, s_a1, static_cast<__bf16*>(p.g_a2_out) + (size_t)e0 * p.WxP + 32 * colblk0, (size_t)p.WxP, nvalid, lane, wave);
    }
    x_head<CB, SAVE, SAVE>(p, L, acc, colblk0, half, tid, lane, wave, kNegLog2e, e0, nvalid);   // (SAVE: + this share of s_e)
    coordinate_segment_sums(p, L, S, tile, half, tid, lane, wave);
  }
  DIAG_STAMP(31, 0);   // epilogue done
}

template <int CB, bool BWD = false, bool SAVE = false>
int launch_v3(const EdgeParams& p, int blocks, size_t smem, hipStream_t st) {
  hipLaunchKernelGGL((edge_kernel_bf16_v3<CB, false, BWD, SAVE>), dim3(blocks), dim3(kTileThreads), smem, st, p);
  EGNN_HIP(hipGetLastError());
  return EGNN_OK;
}

}  // namespace

int init_edge_bf16_v3_attributes() {
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v3<1, false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v3<2, false, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v3<1, false, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  EGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edge_kernel_bf16_v3<1, false, false, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return EGNN_OK;
}

// the coordinate kernels' own conditions: a width they are instantiated for, the packed mlp_x.2 stream, the LDS of a staging
// kernel, and a first-layer table the 32-bit row offsets reach
bool edge_bf16_v3_supported(const EdgeParams& p) {
  return (p.WxP == 256 || p.WxP == 512 || p.WxP == 1024) && p.w2x && v3_smem_bytes(p.WxP) <= 160 * 1024 &&
         (size_t)p.N * p.TC * 4 < ((size_t)1 << 32);
}

// forward coordinate kernel for hidden width 256 (one 256-column workgroup per tile); wider coordinate MLPs run on
// edge_x_m16.hip (v_mfma_f32_16x16x32_bf16: 5-6 % faster by wall at the same workgroup tile, profiles/r03c_ab_xm16.log --
// the 512-column forward / training-forward instantiations of this 32x32x16 kernel were retired for it)
// save: the training forward (p.s1_out / p.g_a2_out / p.s_half_out receive what the backward needs)
int launch_edge_v3_x(const EdgeParams& p, hipStream_t st, bool save) {
  const int tiles = (p.E + kR - 1) / kR;
  if (p.WxP != 256) { set_error("edge_bf16_v3: forward kernels kept for WxP = 256 only"); return EGNN_EINVAL; }
  if (save) return launch_v3<1, false, true>(p, tiles, v3_smem_bytes(p.WxP), st);
  return launch_v3<1>(p, tiles, v3_smem_bytes(p.WxP, false), st);   // (the plain forward stages nothing)
}

// backward recompute of the coordinate branch over the chunk of edges described by p (p.E edges, p.edge_dst / p.edge_src
// already offset to the chunk)
int launch_edge_bf16_v3_x_bwd(const EdgeParams& p, hipStream_t st) {
  const int tiles = (p.E + kR - 1) / kR;
  if (p.WxP >= 512) return launch_v3<2, true>(p, tiles * (p.WxP / 512), v3_smem_bytes(p.WxP), st);
  return launch_v3<1, true>(p, tiles, v3_smem_bytes(p.WxP), st);
}

}  // namespace egnn

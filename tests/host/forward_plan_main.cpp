// Stand-alone test of plan_forward (csrc/host_logic.cpp), the one place that decides how a layer's forward runs, built with
// -fsanitize=address,undefined by tests/test_forward_plan_host.py.  Every case states the expected plan as one line:
//   <path> pre=<node_pre>[+fin] edge=<form> x=<coordinate kernel> R=<rows> ns=<nsplit_x> [fork] [save] sq=<d^2 sums> post=<node_post>
// (path generic/bf16 | generic/fp32: the generic kernel's fragment precision; +fin: node_pre can absorb a pending hidden-split
// finish).  The lines were written by hand from the launch ladder this planner replaced and DESIGN.md section 4, not by
// running plan_forward.  The predicate answers are restated from the width rules of the kernels' *_supported functions (every
// shape below is inside their LDS and 4 GiB limits); packed = false is a layer whose streams are missing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../diffusion_model_amd/csrc/host_logic.h"

using namespace egnn;

namespace {

int g_cases = 0, g_failed = 0;

struct Ask {
  int H = 36, M = 256, Wm = 1024, Wx = 1024, Wh = 1024;   // the reference widths
  int N = 128, E = 8064, B = 2;                           // two fully connected 64-atom graphs
  int prec = EGNN_PREC_BF16, scope = EGNN_NORM_GRAPH;
  bool save = false, need = false, side = true, prof = false, packed = true;
  int ncu = 256;
  ForwardSwitches sw;
};

KernelSupport support(const ModelDims& d, int H, bool packed) {
  KernelSupport s;
  if (!packed) return s;
  const bool w3 = d.WxP == 256 || d.WxP == 512 || d.WxP == 1024, w2 = d.WxP == 512 || d.WxP == 1024, m = d.MP == 256;
  s.v3 = w3;                                                       // edge_bf16_v3.hip: the coordinate kernels' own widths
  s.v4 = m && d.WmP % 64 == 0 && d.WmP >= 192;                     // edge_bf16_v4.hip: the message kernels' own widths
  s.bf16x3 = w3 && m && d.WmP % 64 == 0;                           // edge_bf16x3.hip: both branches
  s.x_m16 = w2;                                                    // edge_x_m16.hip
  s.small = w2 && m && d.WmP % 128 == 0 && d.WmP >= 256;           // edge_small.hip
  s.f16c8w = w2 && m && d.WmP % 128 == 0 && d.WmP >= 128;          // edge_f16c8w.hip
  s.post_split = d.HP <= 64 && H + d.MP > 160 && H + d.MP <= 320 && d.WhP % 128 == 0;   // node_bf16.hip: kSplitK = 320
  s.post_bf16 = d.WhP % 128 == 0 && d.HP / 32 <= 8 && d.K1Q / 16 <= 20;                 // node_bf16.hip: kMaxKS1 = 20
  return s;
}

std::string describe(const ForwardPlan& p) {
  static const char* const paths[] = {"generic", "bf16", "bf16x3", "fp16", "f16c8"};
  static const char* const pres[] = {"hilo8", "hilo2", "mfma", "valu"};
  static const char* const forms[] = {"none", "generic64", "small", "bf16x3", "f16c8", "tile128"};
  static const char* const sqs[] = {"node_d2", "memset", "launch", "node_post"};
  static const char* const posts[] = {"split", "bf16", "f32"};
  std::string s = paths[(int)p.path];
  if (p.path == EdgePath::kGeneric) s += p.frag_bf16 ? "/bf16" : "/fp32";
  s += std::string(" pre=") + pres[(int)p.node_pre] + (p.absorbs_finish ? "+fin" : "");
  s += std::string(" edge=") + forms[(int)p.form];
  if (p.form == EdgeForm::kSmall) s += std::to_string(p.R);
  s += " x=";
  switch (p.coord) {
    case CoordKernel::kOwn: s += "own"; break;
    case CoordKernel::kV3: s += "v3"; break;
    case CoordKernel::kXm16: s += "xm16"; break;
    case CoordKernel::kXm16Persistent: s += "persist:" + std::to_string(p.persist_grid); break;
  }
  s += " R=" + std::to_string(p.R) + " ns=" + std::to_string(p.nsplit_x);
  if (p.fork) s += " fork";
  if (p.save) s += " save";
  s += std::string(" sq=") + sqs[(int)p.sq] + " post=" + posts[(int)p.node_post];
  return s;
}

void check(const char* name, const Ask& k, const char* expect) {
  ++g_cases;
  ForwardAsk a;
  if (model_dims(2, k.H, k.M, k.Wm, k.Wx, k.Wh, &a.md) != EGNN_OK) { printf("FAILED %s: model_dims\n", name); ++g_failed; return; }
  a.N = k.N; a.E = k.E; a.B = k.B; a.H = k.H;
  a.small_ok = k.E <= (1 << 16);   // reserve(): the partial slots are sized for 32-edge tiles up to 65,536 edges
  a.prec = k.prec; a.norm_scope = k.scope; a.save = k.save; a.need_gscale = k.need; a.side_ok = k.side; a.prof = k.prof;
  a.ncu = k.ncu; a.sw = k.sw; a.sup = support(a.md, k.H, k.packed);
  ForwardPlan p;
  p.R = -7;   // a refused ask leaves *out alone
  const int rc = plan_forward(a, &p);
  std::string got;
  if (rc == EGNN_EINVAL && p.R == -7) got = std::string("EINVAL ") + egnn_last_error();
  else if (rc != EGNN_OK) got = "rc " + std::to_string(rc);
  else {
    got = describe(p);
    // what the one-line form leaves implicit
    const bool half = p.path == EdgePath::kBf16 || p.path == EdgePath::kF16;
    if (p.half_table != half || ((p.form == EdgeForm::kSmall || p.form == EdgeForm::kTile128) && p.f16 != (p.path == EdgePath::kF16)) ||
        (p.coord != CoordKernel::kXm16Persistent && p.persist_grid != 0) || (p.coord != CoordKernel::kOwn) != (p.form == EdgeForm::kTile128))
      got += " [inconsistent table / operand / coordinate fields]";
  }
  if (got != expect) { printf("FAILED %s\n  expected: %s\n  got:      %s\n", name, expect, got.c_str()); ++g_failed; }
}

Ask wide(int N, int E, int B, int prec = EGNN_PREC_BF16) { Ask k; k.N = N; k.E = E; k.B = B; k.prec = prec; return k; }
Ask narrow(int N, int E, int B, int prec = EGNN_PREC_BF16) {   // hidden width 256
  Ask k = wide(N, E, B, prec);
  k.Wm = k.Wx = k.Wh = 256;
  return k;
}
template <class F> Ask with(Ask k, F f) { f(k); return k; }

const int F32 = EGNN_PREC_F32, BF16 = EGNN_PREC_BF16, X3 = EGNN_PREC_BF16X3, F16 = EGNN_PREC_F16, C8 = EGNN_PREC_F16C8;
const char* const kRefused = "EINVAL egcl_forward_save needs the 128-edge-tile bf16 kernels";
const char* const kGenericF32 = "generic/fp32 pre=mfma edge=generic64 x=own R=64 ns=1 sq=node_d2 post=f32";

void reference_widths() {
  // E = 56, one 8-atom graph: 32-row small tiles on bf16 and fp16 operands, the side stream whenever there is one
  check("E56 bf16", wide(8, 56, 1), "bf16 pre=hilo2+fin edge=small32 x=own R=32 ns=2 fork sq=node_post post=bf16");
  check("E56 fp16", wide(8, 56, 1, F16), "fp16 pre=hilo2+fin edge=small32 x=own R=32 ns=2 fork sq=node_post post=split");
  check("E56 bf16 no side stream", with(wide(8, 56, 1), [](Ask& k) { k.side = false; }),
        "bf16 pre=hilo2+fin edge=small32 x=own R=32 ns=2 sq=node_post post=bf16");
  check("E56 bf16x3", wide(8, 56, 1, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=node_post post=split");
  check("E56 f16c8", wide(8, 56, 1, C8), "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 fork sq=node_post post=split");
  check("E56 fp32", wide(8, 56, 1, F32), kGenericF32);
  // E = 4,032, one 64-atom graph: 64-row small tiles; the limit itself
  check("E4032 bf16", wide(64, 4032, 1), "bf16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=bf16");
  check("E4032 fp16", wide(64, 4032, 1, F16), "fp16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=split");
  check("E2048 bf16", wide(46, 2048, 1), "bf16 pre=hilo2+fin edge=small32 x=own R=32 ns=2 fork sq=node_post post=bf16");
  check("E2049 bf16", wide(46, 2049, 1), "bf16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=bf16");
  check("E6144 bf16", wide(79, 6144, 1), "bf16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=bf16");
  check("E6144 fp16", wide(79, 6144, 1, F16), "fp16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=split");
  check("E6145 bf16", wide(79, 6145, 1), "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  check("E6145 fp16", wide(79, 6145, 1, F16), "fp16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=split");
  // E = 8,064: 128-row tiles, 126 units: per-unit x_m16; the message kernel fits the shadow of the coordinate kernel's round
  check("E8064 bf16", wide(128, 8064, 2), "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  check("E8064 fp16", wide(128, 8064, 2, F16), "fp16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=split");
  check("E8064 bf16x3", wide(128, 8064, 2, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=node_post post=split");
  check("E8064 f16c8", wide(128, 8064, 2, C8), "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 fork sq=node_post post=split");
  check("E8064 fp32", wide(128, 8064, 2, F32), kGenericF32);
  // E = 36,288: 284 tiles x 2 = 568 units > 2 x 256 CUs: persistent, one workgroup per CU; 200 idle CUs in the last round >= 142
  check("E36288 bf16", wide(576, 36288, 9), "bf16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 fork sq=node_post post=bf16");
  check("E36288 fp16", wide(576, 36288, 9, F16), "fp16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 fork sq=node_post post=split");
  check("E36288 bf16 EGNN_X_PERSIST=0", with(wide(576, 36288, 9), [](Ask& k) { k.sw.x_persist = false; }),
        "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  check("E36288 bf16 304 CUs", with(wide(576, 36288, 9), [](Ask& k) { k.ncu = 304; }),
        "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  check("E36288 fp16 EGNN_X_PERSIST=0", with(wide(576, 36288, 9, F16), [](Ask& k) { k.sw.x_persist = false; }),
        "fp16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=split");
  check("E36288 fp16 304 CUs", with(wide(576, 36288, 9, F16), [](Ask& k) { k.ncu = 304; }),
        "fp16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=split");
  check("E36288 bf16x3", wide(576, 36288, 9, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=node_post post=split");
  check("E36288 f16c8", wide(576, 36288, 9, C8), "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 fork sq=node_post post=split");
  // E = 64,512, sixteen graphs: 1,008 units leave 16 CUs idle in the fourth round: one stream
  check("E64512 bf16", wide(1024, 64512, 16), "bf16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 sq=node_post post=bf16");
  check("E64512 fp16", wide(1024, 64512, 16, F16), "fp16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 sq=node_post post=split");
  check("E64512 bf16x3", wide(1024, 64512, 16, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=node_post post=split");
  check("E64512 f16c8", wide(1024, 64512, 16, C8), "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 sq=node_post post=split");
  // small_ok: with the small-tile limit raised past it, 65,536 edges still run 64-row tiles, 65,537 cannot
  check("E65536 bf16 EGNN_SMALL64_EDGES=100000", with(wide(1100, 65536, 17), [](Ask& k) { k.sw.small64_edges = 100000; }),
        "bf16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=bf16");
  check("E65537 bf16 EGNN_SMALL64_EDGES=100000", with(wide(1100, 65537, 17), [](Ask& k) { k.sw.small64_edges = 100000; }),
        "bf16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 sq=node_post post=bf16");
  check("E65537 bf16", wide(1100, 65537, 17), "bf16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 sq=node_post post=bf16");
  check("E65537 fp16", wide(1100, 65537, 17, F16), "fp16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 sq=node_post post=split");
  check("E65537 fp16 EGNN_SMALL64_EDGES=100000", with(wide(1100, 65537, 17, F16), [](Ask& k) { k.sw.small64_edges = 100000; }),
        "fp16 pre=hilo2+fin edge=tile128 x=persist:256 R=128 ns=2 sq=node_post post=split");
  check("E65536 fp16 EGNN_SMALL64_EDGES=100000", with(wide(1100, 65536, 17, F16), [](Ask& k) { k.sw.small64_edges = 100000; }),
        "fp16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=split");
  check("E65537 bf16x3", wide(1100, 65537, 17, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=node_post post=split");
  check("E65537 f16c8", wide(1100, 65537, 17, C8), "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 sq=node_post post=split");
  check("E56 bf16 EGNN_SMALL_EDGES=0", with(wide(8, 56, 1), [](Ask& k) { k.sw.small_edges = 0; }),
        "bf16 pre=hilo2+fin edge=small64 x=own R=64 ns=2 fork sq=node_post post=bf16");
  // E = 0: no edge launch, node_post reads 64-row tiles of nothing; the tiled paths clear the sums
  check("E0 bf16", wide(3, 0, 3), "bf16 pre=hilo2+fin edge=none x=own R=64 ns=1 sq=memset post=bf16");
  check("E0 fp16", wide(3, 0, 3, F16), "fp16 pre=hilo2+fin edge=none x=own R=64 ns=1 sq=memset post=split");
  check("E0 bf16x3", wide(3, 0, 3, X3), "bf16x3 pre=mfma edge=none x=own R=64 ns=1 sq=memset post=split");
  check("E0 f16c8", wide(3, 0, 3, C8), "f16c8 pre=mfma edge=none x=own R=64 ns=1 sq=memset post=split");
  check("E0 fp32", wide(3, 0, 3, F32), "generic/fp32 pre=mfma edge=none x=own R=64 ns=1 sq=node_d2 post=f32");
  // N = 2,052: 65 node tiles x 4 thousand-column blocks >= 256 workgroups: the 1024-column node_pre
  check("N2052 bf16", wide(2052, 71820, 57), "bf16 pre=hilo8+fin edge=tile128 x=persist:256 R=128 ns=2 sq=node_post post=bf16");
  // profiling on: one stream
  check("E8064 bf16 profiling", with(wide(128, 8064, 2), [](Ask& k) { k.prof = true; }),
        "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 sq=node_post post=bf16");
  check("E56 fp16 profiling", with(wide(8, 56, 1, F16), [](Ask& k) { k.prof = true; }),
        "fp16 pre=hilo2+fin edge=small32 x=own R=32 ns=2 sq=node_post post=split");
  // EGNN_EDGE=1 and a layer whose streams are not packed: the generic kernel (bf16 keeps its node kernel where that one is packed)
  check("E8064 bf16 EGNN_EDGE=1", with(wide(128, 8064, 2), [](Ask& k) { k.sw.edge = 1; }),
        "generic/bf16 pre=mfma edge=generic64 x=own R=64 ns=1 sq=node_d2 post=bf16");
  check("E8064 fp16 EGNN_EDGE=1", with(wide(128, 8064, 2, F16), [](Ask& k) { k.sw.edge = 1; }), kGenericF32);
  check("E8064 bf16 not packed", with(wide(128, 8064, 2), [](Ask& k) { k.packed = false; }),
        "generic/bf16 pre=mfma edge=generic64 x=own R=64 ns=1 sq=node_d2 post=f32");
  check("E8064 f16c8 not packed", with(wide(128, 8064, 2, C8), [](Ask& k) { k.packed = false; }), kGenericF32);
}

void other_widths() {
  // hidden width 256: the v3 coordinate kernel, one share; fp16 and f16c8 have no kernels there and run as fp32
  check("Wx256 E56 bf16", narrow(8, 56, 1), "bf16 pre=hilo2+fin edge=tile128 x=v3 R=128 ns=1 fork sq=node_post post=bf16");
  check("Wx256 E8064 bf16", narrow(128, 8064, 2), "bf16 pre=hilo2+fin edge=tile128 x=v3 R=128 ns=1 fork sq=node_post post=bf16");
  check("Wx256 E64512 bf16", narrow(1024, 64512, 16), "bf16 pre=hilo2+fin edge=tile128 x=v3 R=128 ns=1 sq=node_post post=bf16");
  check("Wx256 E8064 bf16x3", narrow(128, 8064, 2, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=1 sq=node_post post=split");
  check("Wx256 E8064 fp16", narrow(128, 8064, 2, F16), kGenericF32);
  check("Wx256 E8064 f16c8", narrow(128, 8064, 2, C8), kGenericF32);
  // hidden width 512: one 512-column share
  check("Wx512 E8064 bf16", with(wide(128, 8064, 2), [](Ask& k) { k.Wx = 512; }),
        "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=1 fork sq=node_post post=bf16");
  check("Wx512 E8064 bf16x3", with(wide(128, 8064, 2, X3), [](Ask& k) { k.Wx = 512; }),
        "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=2 sq=node_post post=split");
  // M = 300 (MP = 512) at the reference widths, where every tiled kernel takes the hidden widths: outside every tiling because of
  // MP alone; bf16 keeps bf16 fragments, the others become fp32; K1Q = 560: fp32 node_post.  The same at hidden width 256.
  const int precs[] = {F32, BF16, X3, F16, C8};
  for (int prec : precs) {
    const char* want = prec == BF16 ? "generic/bf16 pre=mfma edge=generic64 x=own R=64 ns=1 sq=node_d2 post=f32" : kGenericF32;
    check("M300", with(wide(128, 8064, 2, prec), [](Ask& k) { k.M = 300; }), want);
    check("M300 E56", with(wide(8, 56, 1, prec), [](Ask& k) { k.M = 300; }), want);
    check("M300 Wx256", with(narrow(128, 8064, 2, prec), [](Ask& k) { k.M = 300; }), want);
  }
}

void training_forward() {
  const auto save = [](Ask& k) { k.save = k.need = true; };   // egcl_forward_save keeps the d^2 sums readable
  check("save E8064", with(wide(128, 8064, 2), save), "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 save sq=launch post=bf16");
  check("save E56: no small tiles", with(wide(8, 56, 1), save), "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 save sq=launch post=bf16");
  check("save E36288: per unit", with(wide(576, 36288, 9), save), "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 save sq=launch post=bf16");
  check("save Wx256", with(narrow(128, 8064, 2), save), "bf16 pre=hilo2+fin edge=tile128 x=v3 R=128 ns=1 save sq=launch post=bf16");
  check("save fp16", with(wide(128, 8064, 2, F16), save), kRefused);
  check("save f16c8", with(wide(128, 8064, 2, C8), save), kRefused);
  check("save bf16x3", with(wide(128, 8064, 2, X3), save), kRefused);
  check("save fp32", with(wide(128, 8064, 2, F32), save), kRefused);
  check("save M300", with(narrow(128, 8064, 2), [](Ask& k) { k.M = 300; k.save = k.need = true; }), kRefused);
}

void node_kernels() {
  const auto H = [](int h) { return [h](Ask& k) { k.H = h; }; };
  // node_pre of the half-precision table: hi/lo MFMA up to H = 48, exact f32 MFMA up to 64, VALU above; of the fp32 table: MFMA, VALU
  check("H40 bf16", with(wide(128, 8064, 2), H(40)), "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  check("H48 bf16", with(wide(128, 8064, 2), H(48)), "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  check("H56 bf16", with(wide(128, 8064, 2), H(56)), "bf16 pre=mfma edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  // H = 100: K1Q = 368 > 320: the fp32 node_post, which cannot add the per-graph sums up itself: it needs the launch
  check("H100 bf16", with(wide(128, 8064, 2), H(100)), "bf16 pre=valu edge=tile128 x=xm16 R=128 ns=2 fork sq=launch post=f32");
  check("H40 bf16x3", with(wide(128, 8064, 2, X3), H(40)), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=node_post post=split");
  check("H56 bf16x3", with(wide(128, 8064, 2, X3), H(56)), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=node_post post=split");
  check("H100 bf16x3", with(wide(128, 8064, 2, X3), H(100)), "bf16x3 pre=valu edge=bf16x3 x=own R=128 ns=4 sq=launch post=f32");
  check("H100 fp32", with(wide(128, 8064, 2, F32), H(100)), "generic/fp32 pre=valu edge=generic64 x=own R=64 ns=1 sq=node_d2 post=f32");
  // node_post: split-operand for H + MP in (160, 320] and HP <= 64 (MP >= 256, so only the upper end can be crossed), bf16 for
  // K1Q <= 320, else fp32
  check("H64 fp16", with(wide(128, 8064, 2, F16), H(64)), "fp16 pre=mfma edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=split");
  check("H65 fp16", with(wide(128, 8064, 2, F16), H(65)), "fp16 pre=valu edge=tile128 x=xm16 R=128 ns=2 fork sq=launch post=f32");
  check("H64 bf16", with(wide(128, 8064, 2), H(64)), "bf16 pre=mfma edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16");
  check("H65 bf16", with(wide(128, 8064, 2), H(65)), "bf16 pre=valu edge=tile128 x=xm16 R=128 ns=2 fork sq=launch post=f32");
  check("H64 f16c8", with(wide(128, 8064, 2, C8), H(64)), "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 fork sq=node_post post=split");
  check("H65 f16c8", with(wide(128, 8064, 2, C8), H(65)), "f16c8 pre=valu edge=f16c8 x=own R=128 ns=2 fork sq=launch post=f32");
  // the split-operand streams are packed for these shapes only: a precision that fell back to the generic kernel does not take them
  check("Wx256 H36 fp16: generic, fp32 node_post", narrow(128, 8064, 2, F16), kGenericF32);
}

void sq_sources() {
  // norm scope x need_gscale on a tiled path: only 'graph' scope with nobody else reading the sums leaves them to node_post
  const int scopes[] = {EGNN_NORM_CALL, EGNN_NORM_GRAPH};
  for (int scope : scopes)
    for (int need = 0; need < 2; ++need) {
      const auto set = [=](Ask& k) { k.scope = scope; k.need = need != 0; };
      const bool np = scope == EGNN_NORM_GRAPH && !need;
      check("sq bf16", with(wide(128, 8064, 2), set), np ? "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=node_post post=bf16"
                                                         : "bf16 pre=hilo2+fin edge=tile128 x=xm16 R=128 ns=2 fork sq=launch post=bf16");
      check("sq f16c8", with(wide(128, 8064, 2, C8), set), np ? "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 fork sq=node_post post=split"
                                                             : "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 fork sq=launch post=split");
      check("sq small", with(wide(8, 56, 1), set), np ? "bf16 pre=hilo2+fin edge=small32 x=own R=32 ns=2 fork sq=node_post post=bf16"
                                                      : "bf16 pre=hilo2+fin edge=small32 x=own R=32 ns=2 fork sq=launch post=bf16");
      check("sq fp32 node_post", with(wide(128, 8064, 2), [=](Ask& k) { set(k); k.H = 100; }),
            "bf16 pre=valu edge=tile128 x=xm16 R=128 ns=2 fork sq=launch post=f32");
      check("sq generic", with(wide(128, 8064, 2, F32), set), kGenericF32);
      check("sq E0", with(wide(3, 0, 3), set), "bf16 pre=hilo2+fin edge=none x=own R=64 ns=1 sq=memset post=bf16");
    }
}

// The ten shapes of tests/golden/egnn_golden.npz (fully connected graphs, 'call' scope), by their dimensions: which of them reach
// which kernels.  Only the three full-width ones reach the fp16 / f16c8 kernels; the other seven run those precisions as fp32.
void golden_shapes() {
  struct G { const char* tag; int H, M, Wm, Wx, Wh, N, E, B; const char* bf16_edge; };
  const G full[] = {{"full_g16x3", 36, 256, 1024, 1024, 1024, 48, 720, 3, "small32 x=own R=32"},
                    {"full_g64", 36, 256, 1024, 1024, 1024, 64, 4032, 1, "small64 x=own R=64"},
                    {"full_toy2x4_H3", 3, 256, 1024, 1024, 1024, 8, 8, 4, "small32 x=own R=32"}};
  const G small[] = {{"g16x3_H36", 36, 128, 256, 256, 256, 48, 720, 3, nullptr}, {"g64_H36", 36, 128, 256, 256, 256, 64, 4032, 1, nullptr},
                     {"g8_H36", 36, 128, 256, 256, 256, 8, 56, 1, nullptr},      {"odd_dims", 5, 40, 72, 96, 56, 11, 54, 2, nullptr},
                     {"ragged_H36", 36, 128, 256, 256, 256, 18, 98, 4, nullptr}, {"toy2x4_H3", 3, 128, 256, 256, 256, 8, 8, 4, nullptr},
                     {"toy2x4_H36", 36, 128, 256, 256, 256, 8, 8, 4, nullptr}};
  const auto ask = [](const G& g, int prec) {
    Ask k;
    k.H = g.H; k.M = g.M; k.Wm = g.Wm; k.Wx = g.Wx; k.Wh = g.Wh; k.N = g.N; k.E = g.E; k.B = g.B; k.prec = prec; k.scope = EGNN_NORM_CALL;
    return k;
  };
  for (const G& g : full) {
    const std::string e = g.bf16_edge;
    check(g.tag, ask(g, BF16), ("bf16 pre=hilo2+fin edge=" + e + " ns=2 fork sq=launch post=bf16").c_str());
    check(g.tag, ask(g, F16), ("fp16 pre=hilo2+fin edge=" + e + " ns=2 fork sq=launch post=split").c_str());
    check(g.tag, ask(g, C8), "f16c8 pre=mfma edge=f16c8 x=own R=128 ns=2 fork sq=launch post=split");
    check(g.tag, ask(g, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=4 sq=launch post=split");
    check(g.tag, ask(g, F32), kGenericF32);
  }
  for (const G& g : small) {
    check(g.tag, ask(g, BF16), "bf16 pre=hilo2+fin edge=tile128 x=v3 R=128 ns=1 fork sq=launch post=bf16");
    check(g.tag, ask(g, X3), "bf16x3 pre=mfma edge=bf16x3 x=own R=128 ns=1 sq=launch post=split");
    check(g.tag, ask(g, F16), kGenericF32);
    check(g.tag, ask(g, C8), kGenericF32);
    check(g.tag, ask(g, F32), kGenericF32);
  }
}

// edge_bf16_v3_supported / edge_bf16_v4_supported used to test each other's widths and LDS sizes; each now states the
// conditions of its own kernel.  Nothing reads one without the other (plan_forward: v4 && v3, v4 && x_m16;
// backward_recompute_supported: v4 && v3), so what must hold is that those conjunctions answer as before on every shape.
// Both forms restated here with the kernels' LDS formulas (edge_tile.h: 14,400 bytes of per-tile arrays, 16,512-byte
// activation chunks, 36,864 bytes of store staging); the formulas themselves are pinned by static_asserts next to them.
void predicate_conjunctions() {
  struct P { int WxP, WmP, MP; bool w2x, w2m, w2x16; size_t N, TC; };
  const size_t kLoop = 14400, kChunk = 16512, kStage = 36864, kLds = 160 * 1024;
  const auto v3_smem = [=](int KP) { const size_t loop = 2 * kChunk + (size_t)KP * 4; return kLoop + (kStage > loop ? kStage : loop); };
  const auto v4_smem = [=](int KP) { return kLoop + 3 * kChunk + (size_t)KP * 4; };
  const auto x16_smem = [=](int KP) { return kLoop + 2 * (size_t)16384 + (size_t)KP * 4; };
  const auto w3 = [](int WxP) { return WxP == 256 || WxP == 512 || WxP == 1024; };
  const auto table_ok = [](const P& p) { return p.N * p.TC * 4 < ((size_t)1 << 32); };
  const auto old_v3 = [&](const P& p) {
    return w3(p.WxP) && p.MP == 256 && p.WmP % 64 == 0 && p.w2x && v3_smem(p.WmP) <= kLds && v3_smem(p.WxP) <= kLds && table_ok(p);
  };
  const auto old_v4 = [&](const P& p) {
    return w3(p.WxP) && p.MP == 256 && p.WmP % 64 == 0 && p.WmP >= 192 && p.w2m && v4_smem(p.WmP) <= kLds && v4_smem(p.WxP) <= kLds &&
           table_ok(p);
  };
  const auto new_v3 = [&](const P& p) { return w3(p.WxP) && p.w2x && v3_smem(p.WxP) <= kLds && table_ok(p); };
  const auto new_v4 = [&](const P& p) {
    return p.MP == 256 && p.WmP % 64 == 0 && p.WmP >= 192 && p.w2m && v4_smem(p.WmP) <= kLds && table_ok(p);
  };
  const auto x_m16 = [&](const P& p) { return (p.WxP == 512 || p.WxP == 1024) && p.w2x16 && x16_smem(p.WxP) <= kLds && p.N * p.TC * 2 < ((size_t)1 << 32); };
  // the allocations the launchers ask for, as on the parent (staged coordinate kernels; the plain forward at 256: 48,448)
  const int kps[] = {256, 512, 1024};
  const size_t want_v3[] = {51264, 51264, 51520}, want_v4[] = {64960, 65984, 68032};
  for (int i = 0; i < 3; ++i) {
    ++g_cases;
    if (v3_smem(kps[i]) != want_v3[i] || v4_smem(kps[i]) != want_v4[i]) { printf("FAILED smem bytes at KP = %d\n", kps[i]); ++g_failed; }
  }
  const int wx[] = {64, 128, 256, 512, 1024}, wm[] = {64, 128, 192, 256, 320}, mp[] = {128, 256};
  for (int WxP : wx)
    for (int WmP : wm)
      for (int MP : mp)
        for (int streams = 0; streams < 8; ++streams)      // every combination of present / null weight streams
          for (int big = 0; big < 2; ++big) {              // a first-layer table inside / past the 4 GiB the row offsets reach
            ++g_cases;
            P p{WxP, WmP, MP, (streams & 1) != 0, (streams & 2) != 0, (streams & 4) != 0, big ? (size_t)1 << 20 : (size_t)128,
                (size_t)(2 * WxP + 2 * WmP)};
            const bool o3 = old_v3(p), o4 = old_v4(p), n3 = new_v3(p), n4 = new_v4(p), xm = x_m16(p);
            if ((o3 && o4) != (n3 && n4) || (o4 && xm) != (n4 && xm)) {
              printf("FAILED predicates WxP %d WmP %d MP %d streams %d big %d: v4 && v3 %d -> %d, v4 && x_m16 %d -> %d\n", WxP, WmP, MP,
                     streams, big, o3 && o4, n3 && n4, o4 && xm, n4 && xm);
              ++g_failed;
            }
          }
}

}  // namespace

int main() {
  reference_widths();
  other_widths();
  training_forward();
  node_kernels();
  sq_sources();
  golden_shapes();
  predicate_conjunctions();
  // the helpers the launcher shares with the planner
  if (path_of_precision(EGNN_PREC_F16C8) != EdgePath::kF16c8 || path_of_precision(EGNN_PREC_F32) != EdgePath::kGeneric ||
      node_pre_form(true, 2016, 36, 4096) != NodePre::kHilo2 || node_pre_form(true, 2017, 36, 4096) != NodePre::kHilo8 ||
      node_pre_form(false, 2017, 36, 4096) != NodePre::kMfma) { printf("FAILED helpers\n"); ++g_failed; }
  printf("%d cases, %d failed\n", g_cases, g_failed);
  if (g_failed) return 1;
  printf("FORWARD-PLAN-OK\n");
  return 0;
}

# Build libegnn_amd.so (gfx950 only).  `python -c "import __graft_entry__ as g; g.build()"` runs this.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
CSRC  := diffusion_model_amd/csrc
OUT   := diffusion_model_amd/libegnn_amd.so
SRCS  := $(CSRC)/egnn_forward.hip $(CSRC)/pack.hip $(CSRC)/edge_bf16_v3.hip $(CSRC)/edge_bf16_v4.hip $(CSRC)/edge_x_m16.hip $(CSRC)/edge_small.hip $(CSRC)/edge_bf16x3.hip $(CSRC)/edge_f16c8w.hip $(CSRC)/edge_bwd_dgrad.hip $(CSRC)/edge_bwd_dgrad_graph.hip $(CSRC)/edge_bwd_heads.hip $(CSRC)/edge_bwd_first.hip $(CSRC)/gemm_tn.hip $(CSRC)/gemm_rows.hip $(CSRC)/sampler.hip $(CSRC)/graph_stats.hip $(CSRC)/aux_mlp.hip $(CSRC)/node_bf16.hip $(CSRC)/backward.hip $(CSRC)/optim/optim_step.hip $(CSRC)/eval/kabsch.hip $(CSRC)/eval/assign.hip $(CSRC)/eval/structure.hip $(CSRC)/eval/topo.hip $(CSRC)/eval/rings.hip $(CSRC)/eval/soap.hip $(CSRC)/eval/sq.hip $(CSRC)/cells/cell_env.hip $(CSRC)/cells/cell_stats.hip $(CSRC)/cells/cell_grid.hip $(CSRC)/cells/cell_soap.hip $(CSRC)/cells/cell_boo.hip $(CSRC)/cells/cell_ewald.hip $(CSRC)/cells/cell_relax.hip
HDRS  := $(CSRC)/eval/eval_math.h $(CSRC)/eval/eval_device.h $(CSRC)/eval/lds_limit.h $(CSRC)/eval/eval_host.h $(CSRC)/edge_f16c8w_mphase2.inc $(CSRC)/edge_f16c8w_mphasek.inc $(CSRC)/common.h $(CSRC)/layer_pack.h $(CSRC)/kernels.h $(CSRC)/x_walk.h $(CSRC)/edge_tile.h $(CSRC)/host_logic.h $(CSRC)/diag.h $(CSRC)/bwd_graph.h $(CSRC)/optim/optim_step.h $(CSRC)/eval/kabsch.h $(CSRC)/eval/kabsch_math.h $(CSRC)/eval/assign.h $(CSRC)/eval/assign_host.h $(CSRC)/eval/structure_math.h $(CSRC)/eval/structure_host.h $(CSRC)/eval/topo_math.h $(CSRC)/eval/topo_host.h $(CSRC)/eval/rings_math.h $(CSRC)/eval/rings_host.h $(CSRC)/eval/soap_math.h $(CSRC)/eval/soap_device.h $(CSRC)/eval/soap_host.h $(CSRC)/eval/sq_math.h $(CSRC)/eval/sq_device.h $(CSRC)/eval/sq_host.h $(CSRC)/cells/cell_math.h $(CSRC)/cells/cell_device.h $(CSRC)/cells/cell_host.h $(CSRC)/cells/cell_stats_math.h $(CSRC)/cells/cell_stats_host.h $(CSRC)/cells/cell_grid_math.h $(CSRC)/cells/cell_grid_host.h $(CSRC)/cells/cell_soap_math.h $(CSRC)/cells/cell_soap_host.h $(CSRC)/cells/cell_boo_math.h $(CSRC)/cells/cell_boo_host.h $(CSRC)/cells/cell_ewald_math.h $(CSRC)/cells/cell_stress_math.h $(CSRC)/cells/cell_ewald_host.h $(CSRC)/cells/cell_relax_math.h $(CSRC)/cells/cell_relax_host.h include/egnn_amd.h
# -fvisibility=hidden: the library exports exactly the functions include/egnn_amd.h declares (the header wraps its
# declarations in a visibility push(default)); tests/test_cabi_and_host.py compares the two sets
FLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=off -fno-slp-vectorize -fvisibility=hidden
# host_logic.cpp, eval/assign_host.cpp, eval/kabsch_host.cpp, eval/structure_host.cpp, eval/topo_host.cpp, eval/rings_host.cpp, eval/soap_host.cpp, eval/sq_host.cpp, cells/cell_host.cpp, cells/cell_stats_host.cpp, cells/cell_grid_host.cpp, cells/cell_soap_host.cpp, cells/cell_boo_host.cpp, cells/cell_ewald_host.cpp, cells/cell_stress_host.cpp, cells/cell_relax_host.cpp: the HIP-free part of the host side (validation,
# schedule builder, plans, the host statements of the Kabsch gradient, of the structure statistics, of the topological fingerprint, of the ring statistics, of the SOAP descriptors, of the structure factors, of the periodic-cell environments, of the periodic-cell statistics, of the linked-cell search, of the periodic-cell SOAP descriptors, of the bond-orientational order, of the lattice energy, of its strain derivative and of the relaxation); plain C++ for both builds
HOSTSRC := $(CSRC)/host_logic.cpp $(CSRC)/eval/assign_host.cpp $(CSRC)/eval/kabsch_host.cpp $(CSRC)/eval/structure_host.cpp $(CSRC)/eval/topo_host.cpp $(CSRC)/eval/rings_host.cpp $(CSRC)/eval/soap_host.cpp $(CSRC)/eval/sq_host.cpp $(CSRC)/cells/cell_host.cpp $(CSRC)/cells/cell_stats_host.cpp $(CSRC)/cells/cell_grid_host.cpp $(CSRC)/cells/cell_soap_host.cpp $(CSRC)/cells/cell_boo_host.cpp $(CSRC)/cells/cell_ewald_host.cpp $(CSRC)/cells/cell_stress_host.cpp $(CSRC)/cells/cell_relax_host.cpp
HOSTHDR := $(CSRC)/host_logic.h $(CSRC)/layer_pack.h $(CSRC)/eval/eval_math.h $(CSRC)/eval/eval_host.h $(CSRC)/eval/assign_host.h $(CSRC)/eval/kabsch_math.h $(CSRC)/eval/structure_math.h $(CSRC)/eval/structure_host.h $(CSRC)/eval/topo_math.h $(CSRC)/eval/topo_host.h $(CSRC)/eval/rings_math.h $(CSRC)/eval/rings_host.h $(CSRC)/eval/soap_math.h $(CSRC)/eval/soap_host.h $(CSRC)/eval/sq_math.h $(CSRC)/eval/sq_host.h $(CSRC)/cells/cell_math.h $(CSRC)/cells/cell_host.h $(CSRC)/cells/cell_stats_math.h $(CSRC)/cells/cell_stats_host.h $(CSRC)/cells/cell_grid_math.h $(CSRC)/cells/cell_grid_host.h $(CSRC)/cells/cell_soap_math.h $(CSRC)/cells/cell_soap_host.h $(CSRC)/cells/cell_boo_math.h $(CSRC)/cells/cell_boo_host.h $(CSRC)/cells/cell_ewald_math.h $(CSRC)/cells/cell_stress_math.h $(CSRC)/cells/cell_ewald_host.h $(CSRC)/cells/cell_relax_math.h $(CSRC)/cells/cell_relax_host.h include/egnn_amd.h
HOSTOBJ := $(HOSTSRC:.cpp=.o)
ASAN_OUT := build/libegnn_host_asan.so

OBJS := $(SRCS:.hip=.o)

all: $(OUT)

%.o: %.hip $(HDRS)
	$(HIPCC) $(FLAGS) -c $< -o $@

%.o: %.cpp $(HOSTHDR)
	$(HIPCC) -O2 -std=c++17 -fPIC -Wall -fvisibility=hidden -c $< -o $@

$(OUT): $(OBJS) $(HOSTOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) $(HOSTOBJ) -o $@

# CPU-only sanitizer build of the host logic (no GPU, no HIP): what tests/test_host_asan.py loads in the build container
asan: $(ASAN_OUT)
$(ASAN_OUT): $(HOSTSRC) $(HOSTHDR)
	mkdir -p build
	g++ -O1 -g -std=c++17 -fPIC -shared -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DEGNN_HOST_TEST_API $(HOSTSRC) -o $@

clean:
	rm -f $(OBJS) $(HOSTOBJ) $(OUT) $(ASAN_OUT)

.PHONY: all clean asan

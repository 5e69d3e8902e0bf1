"""ctypes binding of libegnn_amd.so (C ABI: include/egnn_amd.h).  No fallback: if the library
is missing or a call fails, an exception is raised."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EGNN_LIB", os.path.join(_HERE, "libegnn_amd.so"))   # EGNN_LIB: timing-experiment builds

PREC_F32, PREC_BF16, PREC_BF16X3, PREC_F16, PREC_F16C8 = 0, 1, 2, 3, 4
NORM_CALL, NORM_GRAPH = 0, 1
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "float32": PREC_F32, "bf16": PREC_BF16, "bfloat16": PREC_BF16,
              "bf16x3": PREC_BF16X3, "f16c8": PREC_F16C8, "fp16": PREC_F16, "f16": PREC_F16, "float16": PREC_F16}
NORM_SCOPES = {"call": NORM_CALL, "graph": NORM_GRAPH}
OPTIM_ADAM, OPTIM_ADAMW_AMSGRAD, OPTIM_RADAM_SF = 0, 1, 2
KABSCH_CENTERS = {"centroid": 0, "first": 1}
KABSCH_FLIPS = {"row": 0, "column": 1}
ASSIGN_MAX_ATOMS = 1024   # EGNN_ASSIGN_MAX_ATOMS of include/egnn_amd.h (kAssignMaxAtoms)
STRUCT_MAX_TYPES, STRUCT_MAX_ATOMS = 4, 32768   # kStructMaxTypes, kStructMaxAtoms of csrc/eval/structure_math.h
STRUCT_CENTRE_BLOCK, STRUCT_CHUNK, STRUCT_BOND_CENTRES = 64, 1024, 8   # the tiles of egnn_struct_pair_counts / egnn_struct_bonds
CELL_MAX_TYPES, CELL_MAX_SHELLS, CELL_MAX_ENV_ATOMS, CELL_SHIFT_CODES = 4, 4, 1024, 729   # kCell* of csrc/cells/cell_math.h
TOPO_MAX_ATOMS, TOPO_MAX_DEGREE, TOPO_BRANCH_MODULUS, TOPO_MAX_LENGTH = 1024, 32, 7, 64   # csrc/eval/topo_math.h
RING_MAX_SITES, RING_MAX_SIZE = 4096, 32   # RING_MAX_SITES, kRingMaxSize of csrc/eval/rings_math.h
SOAP_MAX_TYPES, SOAP_MAX_N, SOAP_MAX_L, SOAP_MAX_K = 4, 16, 10, 8   # kSoap* of csrc/eval/soap_math.h
SQ_MAX_TYPES, SQ_MAX_Q, SQ_MAX_BINS, SQ_MAX_ATOMS, SQ_MAX_VECTORS = 4, 4096, 4096, 32768, 1 << 24   # kSq* of csrc/eval/sq_math.h
SQ_ROW_BLOCK, SQ_CHUNK, SQ_VECTOR_BLOCK = 64, 256, 256   # the tiles of egnn_sq_debye and egnn_sq_cell_rho
SQ_WINDOWS = {None: 0, "none": 0, "lorch": 1}
CELL_CENTRE_BLOCK = 64    # kCellCentreBlock: the centres of one tile of egnn_cell_bonds_count / _fill
# kCellStat* of csrc/cells/cell_stats_math.h: the tiles of egnn_cell_pair_counts / egnn_cell_bond_stats and their limits
CELL_STAT_CENTRE_BLOCK, CELL_STAT_CHUNK, CELL_STAT_BOND_CENTRES, CELL_STAT_MAX_IMAGES, CELL_STAT_MAX_HIST = 64, 1024, 8, 16, 16384
# kCellGrid* of csrc/cells/cell_grid_math.h: bins per axis, the reach, and the keys of a bond row staged per wavefront
CELL_GRID_MAX_BINS, CELL_GRID_MAX_REACH, CELL_GRID_ROW_KEYS = 256, 3, 128
CELL_SOAP_MAX_BOX = 4     # kCellSoapMaxBox of csrc/cells/cell_soap_math.h: the image box the shift code holds
EWALD_ATOM_CHUNK, EWALD_MAX_POWER = 1024, 64   # kEwaldAtomChunk, kEwaldMaxPower of csrc/cells/cell_ewald_math.h
# kRelax* of csrc/cells/cell_relax_math.h: the status codes and the columns of the scalars and counters of a relaxation
RELAX_CONVERGED, RELAX_COINCIDENT, RELAX_NOT_FINITE, RELAX_STUCK = 1, 3, 4, 5
RELAX_SCALARS, RELAX_COUNTERS = 5, 4
PREALIGN_MIN_ATOMS = 5    # kPrealignMinAtoms of csrc/eval/assign_host.h: atom 0 and its four nearest neighbours


_FLAGS_FALLBACK = b"FLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -fvisibility=hidden"


def _flags_line() -> bytes:
    """the compiler flags of the library build: the Makefile's FLAGS line where the Makefile travels with the package, else the
    flags this package's Makefile is known to use (a fingerprint must not fail, or change meaning, because a build file is absent)"""
    try:
        with open(os.path.join(os.path.dirname(_HERE), "Makefile"), "rb") as f:
            flags = [l for l in f.read().splitlines() if l.startswith(b"FLAGS")]
        return b"\n".join(flags)
    except OSError:
        return _FLAGS_FALLBACK


def _sources_sha256(names) -> str:
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    for name in names:
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    h.update(_flags_line())
    return h.hexdigest()


def edge_kernel_sources_sha256() -> str:
    """Fingerprint of the sources the dominant (edge) kernels are compiled from (every header they include, diag.h among them),
    of the packing that writes the streams they read (pack.hip), and the compiler flags: what a PMC measurement of those kernels
    (profiles/traffic.json) is valid for.  A hash of the .so itself would not survive a rebuild in another directory (hipcc
    derives its per-TU symbol ids from the path)."""
    return _sources_sha256(("edge_x_m16.hip", "edge_bf16_v4.hip", "pack.hip", "edge_tile.h", "kernels.h", "x_walk.h", "common.h", "layer_pack.h",
                            "diag.h"))


def forward_sources_sha256() -> str:
    """Fingerprint of every source an inference forward of any precision runs through (edge kernels of all precisions, node
    kernels, packing, and the dispatch: plan_forward in host_logic.cpp): what a measured error table (tools/prec_errors.py) is
    valid for."""
    return _sources_sha256(("egnn_forward.hip", "host_logic.h", "host_logic.cpp", "pack.hip", "edge_x_m16.hip", "edge_bf16_v4.hip", "edge_bf16_v3.hip", "edge_small.hip",
                            "edge_bf16x3.hip", "edge_f16c8w.hip", "edge_f16c8w_mphase2.inc", "edge_f16c8w_mphasek.inc", "node_bf16.hip",
                            "edge_tile.h", "kernels.h", "x_walk.h", "common.h", "layer_pack.h", "diag.h"))


def training_sources_sha256() -> str:
    """Fingerprint of everything the HBM traffic of ONE training step depends on: every kernel source and header of the
    library, the compiler flags and the launch sequence (autograd.py, gemm.py): what profiles/traffic_train.json is valid for."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    names = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.cpp")) +
                   glob.glob(os.path.join(csrc, "*.inc")))
    names += [os.path.join(_HERE, "autograd.py"), os.path.join(_HERE, "gemm.py")]
    for path in names:
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read())
    h.update(_flags_line())
    return h.hexdigest()


_vp, _i, _f, _u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
_fp = C.POINTER(C.c_float)


class OptimConsts(C.Structure):
    """egnn_optim_consts of include/egnn_amd.h: the per-step scalars of one optimizer step, computed by the caller in double
    (optim.py: adam_scalars / radam_schedule_free_scalars) and rounded to fp32 on assignment"""
    _fields_ = [(name, C.c_float) for name in ("beta2", "one_minus_beta2", "eps", "weight_decay", "one_minus_beta1",
                                               "bias_correction2_sqrt", "step_size", "decay_mul", "bias_correction2", "ckp1",
                                               "adaptive_y_lr", "lr")] + [("rectified", C.c_int32)]


_pp, _i64p, _dp = C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_double)

# name -> (restype, argtypes); kept in one table so tests can check every header symbol is exported
SIGNATURES = {
    "egnn_last_error": (C.c_char_p, []),
    "egnn_version": (_i, []),
    "egnn_create": (_i, [C.POINTER(_vp), _i]),
    "egnn_destroy": (_i, [_vp]),
    "egnn_set_model": (_i, [_vp] + [_i] * 6),
    "egnn_pack_layer": (_i, [_vp, _vp, _i] + [_vp] * 16),
    "egnn_set_graph": (_i, [_vp, _i, _i, _i] + [_vp] * 5),
    "egnn_set_side_stream": (_i, [_vp, _vp]),
    "egcl_forward": (_i, [_vp, _vp, _i, _i, _i] + [_vp] * 4),
    "egcl_forward_begin": (_i, [_vp, _vp, _i, _i, _i] + [_vp] * 3),
    "egcl_forward_end": (_i, [_vp, _vp, _i, _i, _i] + [_vp] * 5),
    "egnn_forward": (_i, [_vp, _vp, _i, _i] + [_vp] * 4),
    "egcl_read_aggregates": (_i, [_vp, _vp, _i] + [_vp] * 3),
    "egcl_backward_l1_act": (_i, [_vp, _i, _i, _i] + [_vp] * 7),
    "egcl_backward_heads": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 20),
    "egcl_backward_l1_grad": (_i, [_vp, _i, _i, _i] + [_vp] * 7),
    "egcl_backward_gather_in": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 6),
    "egcl_backward_scatter": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 9),
    "egcl_backward_first_reduce": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i] + [_vp] * 9),
    "egcl_backward_node_act": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "egcl_backward_scatter_geom": (_i, [_vp, _i, _i] + [_vp] * 8),
    "egcl_backward_fused_supported": (_i, [_vp]),
    "egcl_backward_table": (_i, [_vp, _vp, _i, _vp]),
    "egcl_backward_edge_recompute": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 11),
    "egcl_backward_dgrad": (_i, [_vp, _vp, _i, _vp, _i, _i] + [_vp] * 4),
    "egcl_backward_dgrad_reduce": (_i, [_vp, _vp, _i, _vp, _i, _i] + [_vp] * 6),
    "egcl_forward_save": (_i, [_vp, _vp, _i, _i] + [_vp] * 9),
    "egcl_backward_heads_saved": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 10),
    "egnn_gemm_tn_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "egnn_gemm_tn_bf16": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _vp, C.c_size_t]),
    "egnn_gemm_rows_pack": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "egnn_gemm_rows_bf16": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i]),
    "egnn_gamma_tilde": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "egnn_dense_rows": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "egnn_eps": (_i, [_vp, _i, _i, _i, _vp, _i] + [_vp] * 5),
    "egnn_remove_mean": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    "schedule_table_build": (_i, [_i, C.c_double, C.c_double, _fp, _fp, _fp]),
    "schedule_table_from_alpha": (_i, [_i, _fp, _fp, _fp]),
    "ddpm_reverse_step": (_i, [_vp, _i, _i, _i, _vp, _i, _f, _f, _f, _vp, _i, _vp, _vp, _vp, _i]),
    "egnn_sampler_prepare": (_i, [_vp, _i, _i, _f, _vp, _vp, _u64]),
    "egnn_sampler_set_mode": (_i, [_vp, _i]),
    "egnn_sampler_init": (_i, [_vp, _vp, _vp, _vp]),
    "egnn_sampler_run": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "egnn_sampler_final": (_i, [_vp, _vp, _i, _i] + [_vp] * 5),
    "egnn_sampler_state": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "ddpm_sampler_init": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _u64] + [_vp] * 6),
    "ddpm_sampler_step": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _f, _u64] + [_vp] * 7),
    "ddpm_sampler_final": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _u64] + [_vp] * 10),
    "egnn_fc_graph_build": (_i, [_vp, _i, _i] + [_vp] * 6),
    "egnn_radius_graph_count": (_i, [_vp, _i, _vp, _vp, _vp, _f, _vp]),
    "egnn_radius_graph_fill": (_i, [_vp, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    "egnn_rdf": (_i, [_vp, _i, _vp, _vp, C.c_double, C.c_double, _f, _i, _i, _vp]),
    "egnn_si_o_si": (_i, [_vp, _i, _i, _vp, _vp, _vp, _f, _vp]),
    "egnn_kabsch": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "egnn_kabsch_ordered": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "egnn_kabsch_backward": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "egnn_kabsch_grad_host": (_i, [_i, _dp, _dp, _i, _i, _dp, _dp, C.c_double, _dp, _dp]),
    "egnn_kabsch_perm_workspace_bytes": (C.c_size_t, [_i, _i]),
    "egnn_kabsch_perm": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.c_size_t]),
    "egnn_assign": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "egnn_assign_prealign": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "egnn_struct_pair_counts": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, C.c_double, _i, _vp]),
    "egnn_struct_bonds": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _f, C.c_double, _i, _vp, _vp, _vp]),
    "egnn_struct_rdf_finish": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, _i, _vp]),
    "egnn_struct_counts_host": (_i, [_i, _i, _vp, _vp, _vp, C.c_double, _i, _f, C.c_double, _i, _vp, _vp, _vp, _vp]),
    "egnn_topo_bonds": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "egnn_topo_paths": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "egnn_topo_tanimoto": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "egnn_topo_host": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i] + [_vp] * 8 + [_i] + [_vp] * 4),
    "egnn_rings": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i] + [_vp] * 8),
    "egnn_rings_host": (_i, [_i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i] + [_vp] * 4),
    "egnn_soap_features": (_i, [_i, _i, _i]),
    "egnn_soap_table_doubles": (_i, [_i, _i]),
    "egnn_soap_descriptor": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, C.c_double, _vp, _i, _vp, _vp, _vp, _vp]),
    "egnn_soap_cosine": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "egnn_soap_gram": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "egnn_spectrum_nearest": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 6),
    "egnn_soap_host": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _i, C.c_double, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp,
                            _i, _i, _i, _i] + [_vp] * 6),
    "egnn_cell_bonds_count": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _i, _vp]),
    "egnn_cell_bonds_fill": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _i, _vp, _i, _vp, _vp]),
    "egnn_cell_env_count": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp]),
    "egnn_cell_env_fill": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i] + [_vp] * 4),
    "egnn_cell_env_host": (_i, [_i, _i, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _i, _i, _vp, C.c_int64, _vp, _vp, _vp, C.c_int64] + [_vp] * 4),
    "egnn_cell_pair_counts": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, _i, _vp]),
    "egnn_cell_bond_stats": (_i, [_vp, _i, _i, _i] + [_vp] * 7 + [_i, _vp, _vp, C.c_double, _i, _i, _i, _vp, _i] + [_vp] * 6),
    "egnn_cell_stats_host": (_i, [_i, _i, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, C.c_double, C.c_double, _i, _i, _i] + [_vp] * 6),
    "egnn_cell_grid_dims": (_i, [_i, _vp, C.c_double, _i, C.c_double, _vp]),
    "egnn_cell_grid_count": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "egnn_cell_grid_fill": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_double, _i] + [_vp] * 5 + [_i] + [_vp] * 6),
    "egnn_cell_bonds_grid_count": (_i, [_vp, _i, _i] + [_vp] * 8 + [_i, _vp, _vp, _vp, C.c_double, _i, _vp, _i, _vp]),
    "egnn_cell_bonds_grid_fill": (_i, [_vp, _i, _i] + [_vp] * 8 + [_i, _vp, _vp, _vp, C.c_double, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "egnn_cell_pair_counts_grid": (_i, [_vp, _i, _i, _i] + [_vp] * 8 + [_i, _vp, _vp, _vp, C.c_double, _i, _i, _vp, _i, _vp]),
    "egnn_cell_grid_host": (_i, [_i, _i, _vp, _vp, _vp, _vp, C.c_double, _i, C.c_double, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int64,
                                 _vp, _vp, C.c_double, _i, _vp]),
    "egnn_cell_sites_count": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, _vp]),
    "egnn_cell_sites_fill": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _i, _vp, _vp]),
    "egnn_cell_soap_descriptor": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _i] + [_vp] * 4),
    "egnn_cell_soap_mean": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "egnn_cell_sites_host": (_i, [_i, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, C.c_int64, _vp, _vp]),
    "egnn_cell_soap_host": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _i, C.c_double, _vp, _i, _vp, _vp, _vp]),
    "egnn_cell_soap_mean_host": (_i, [_i, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "egnn_cell_boo_qlm": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [C.c_double, C.c_uint, _i, _vp, _i, _vp, _i, _vp, _vp, _i] + [_vp] * 4),
    "egnn_cell_boo_invariants": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [C.c_uint, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, C.c_double, _i, _i, _vp, _i, _vp,
                                      _vp, _i] + [_vp] * 5),
    "egnn_cell_boo_host": (_i, [_i, _i, _vp, _vp, _vp, _vp, C.c_double, C.c_uint, _i, _vp, _i, _vp, _vp, _vp, _i, C.c_double, _i, _i] + [_vp] * 5),
    "egnn_cell_ewald_real": (_i, [_vp, _i, _i, _i] + [_vp] * 8 + [_i, _i] + [C.c_double] * 5 + [_i, _i, _vp, _i, _vp, _vp, _i] + [_vp] * 4),
    "egnn_cell_ewald_amplitudes": (_i, [_vp, _i, _i, _i] + [_vp] * 11 + [C.c_double] * 4 + [_i, _vp, _i, _vp, _i, _vp, _vp]),
    "egnn_cell_ewald_recip": (_i, [_vp, _i, _i, _i] + [_vp] * 9 + [C.c_double] * 4 + [_i, _i] + [_vp] * 3),
    "egnn_cell_ewald_finish": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [C.c_double] * 4 + [_vp] * 8),
    "egnn_cell_ewald_host": (_i, [_i, _i] + [_vp] * 6 + [_i, _i] + [C.c_double] * 5 + [_i] + [_vp] * 8),
    "egnn_cell_ewald_virial_real": (_i, [_vp, _i, _i, _i] + [_vp] * 8 + [_i, _i] + [C.c_double] * 5 + [_i, _vp, _i, _vp, _vp, _i] + [_vp] * 4),
    "egnn_cell_ewald_virial_recip": (_i, [_vp, _i, _i, _i] + [_vp] * 9 + [C.c_double] * 4 + [_i] + [_vp] * 3),
    "egnn_cell_ewald_virial_finish": (_i, [_vp, _i, _i, _i] + [_vp] * 6 + [C.c_double] * 4 + [_vp] * 9),
    "egnn_cell_ewald_virial_host": (_i, [_i, _i] + [_vp] * 6 + [_i, _i] + [C.c_double] * 5 + [_vp] * 8),
    "egnn_cell_relax_real": (_i, [_vp, _i, _i, _i] + [_vp] * 8 + [_i, _i] + [C.c_double] * 6 + [_i, _vp, _i, _vp, _vp, _i] + [_vp] * 4),
    "egnn_cell_relax_step": (_i, [_vp, _i, _i] + [_vp] * 7 + [C.c_double, _i] + [C.c_double] * 6 + [_i, C.c_double] + [_vp] * 10),
    "egnn_cell_relax_step_host": (_i, [_i, _i] + [_vp] * 5 + [C.c_double, _i] + [C.c_double] * 6 + [_i, C.c_double] + [_vp] * 10),
    "egnn_cell_relax_host": (_i, [_i, _i] + [_vp] * 6 + [_i, _i] + [C.c_double] * 7 + [_i] + [C.c_double] * 6 + [_i, C.c_double] + [_vp] * 12),
    "egnn_sq_debye": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, C.c_double, _i, _vp, _i, _vp, _vp, _vp]),
    "egnn_sq_cell_plan": (_i, [_i, _vp, C.c_double, _vp, _vp]),
    "egnn_sq_cell_count": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.c_double, _i, _vp]),
    "egnn_sq_cell_rho": (_i, [_vp, _i, _i, _i] + [_vp] * 10 + [C.c_double, C.c_double, _i, _i, _vp, _i, _vp, _i] + [_vp] * 4),
    "egnn_sq_cell_shells": (_i, [_vp, _i, _i, _i, _vp, _vp, _i] + [_vp] * 6),
    "egnn_sq_host": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp, C.c_double, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i,
                          C.c_int64] + [_vp] * 8),
    "egnn_optim_step": (_i, [_vp, _i, _i, _pp, _pp, _pp, _pp, _pp, _i64p, C.POINTER(OptimConsts)]),
    "egnn_optim_interp": (_i, [_vp, _i, _pp, _pp, _i64p, _f]),
    "egnn_optim_tensors_per_launch": (_i, []),
    "egnn_debug_stamps": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "egnn_profile_enable": (_i, [_vp, _i]),
    "egnn_profile_read": (_i, [_vp, _fp, C.POINTER(_i), _fp]),
}

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP extension first (`make` at the repo root or "
                "`python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


class EgnnError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        msg = lib().egnn_last_error()
        raise EgnnError(f"libegnn_amd error {rc}: {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def host_ptr(a):
    """Pointer of a contiguous numpy array, for the entries that read a host copy."""
    return C.c_void_p(a.ctypes.data)


def stream_ptr(stream=None):
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s.cuda_stream)

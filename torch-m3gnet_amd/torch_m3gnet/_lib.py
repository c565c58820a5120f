"""ctypes binding of libm3gnet_hip.so (C ABI: include/m3gnet_hip.h)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

_PKG_ROOT = Path(__file__).resolve().parent.parent  # .../torch-m3gnet_amd
LIB_PATH = _PKG_ROOT / "lib" / "libm3gnet_hip.so"

M3G_OK, M3G_ERR_VALUE, M3G_ERR_STATE, M3G_ERR_SIZE, M3G_ERR_HIP, M3G_ERR_UNSUPPORTED = range(6)
ABI_VERSION = 11
VERLET_FILL_LISTS_MAX_ROW = 1024   # M3G_VERLET_FILL_LISTS_MAX_ROW (include/m3gnet_hip.h)
VERLET_ONE_LAUNCH_MAX_ATOMS = 512   # M3G_VERLET_ONE_LAUNCH_MAX_ATOMS: m3g_verlet_update is one launch up to here, three above


class M3GConfig(C.Structure):
    _fields_ = [
        ("cutoff", C.c_double), ("threebody_cutoff", C.c_double), ("energy_scale", C.c_double),
        ("length_scale", C.c_double), ("l_max", C.c_int32), ("n_max", C.c_int32), ("num_types", C.c_int32),
        ("embedding_dim", C.c_int32), ("num_blocks", C.c_int32), ("reserved", C.c_int32),
    ]


class M3GInfo(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device_count", C.c_int32), ("arch", C.c_char * 32)]


class M3GIO(C.Structure):
    _fields_ = [
        ("n_atoms", C.c_int64), ("n_edges", C.c_int64), ("n_triplets", C.c_int64), ("n_structs", C.c_int64),
        ("pos", C.c_void_p), ("atom_types", C.c_void_p), ("edge_cell_shift", C.c_void_p), ("lattice", C.c_void_p),
        ("topo", C.c_void_p), ("triplet_edge_index", C.c_void_p),
        ("total_energy", C.c_void_p), ("forces", C.c_void_p),
        ("stresses", C.c_void_p), ("scaled_total_energy", C.c_void_p), ("scaled_atomic_energies", C.c_void_p),
        ("node_features", C.c_void_p), ("edge_attr", C.c_void_p), ("edge_distances", C.c_void_p),
        ("edge_weights", C.c_void_p), ("triplet_angles", C.c_void_p), ("mid_edge_features", C.c_void_p),
        ("topo_hints", C.c_int32), ("reserved", C.c_int32),
    ]


class M3GMdLists(C.Structure):   # m3g_md_lists
    _fields_ = [
        ("n_atoms", C.c_int64), ("n_structs", C.c_int64), ("n_cand", C.c_int64), ("cap_edges", C.c_int64), ("cap_triplets", C.c_int64),
        ("cutoff", C.c_double), ("threebody_cutoff", C.c_double), ("skin", C.c_double),
        ("pos_ref", C.c_void_p), ("lattice", C.c_void_p), ("lattice32", C.c_void_p), ("batch", C.c_void_p), ("atom_types", C.c_void_p),
        ("cand_edge_index", C.c_void_p), ("cand_shift", C.c_void_p), ("cand_row_ptr", C.c_void_p), ("cand_state", C.c_void_p),
        ("verlet_scratch", C.c_void_p), ("verlet_scratch_bytes", C.c_size_t),
        ("edge_index", C.c_void_p), ("edge_cell_shift", C.c_void_p), ("triplet_edge_index", C.c_void_p), ("num_triplet_i", C.c_void_p),
        ("num_triplet_ij", C.c_void_p), ("pos32", C.c_void_p),
        ("topo", C.c_void_p), ("topo_bytes", C.c_size_t), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class M3GMdResult(C.Structure):   # m3g_md_result
    _fields_ = [("path", C.c_int32), ("topo_hints", C.c_int32), ("n_edges", C.c_int64), ("n_triplets", C.c_int64),
                ("max_displacement", C.c_double)]


MD_REUSE, MD_REFILL, MD_NEED_SEARCH, MD_UNSUPPORTED = range(4)


class M3GFireParams(C.Structure):   # m3g_fire_params
    _fields_ = [("dt", C.c_double), ("maxstep", C.c_double), ("dtmax", C.c_double), ("finc", C.c_double), ("fdec", C.c_double),
                ("astart", C.c_double), ("fa", C.c_double), ("fmax", C.c_double), ("nmin", C.c_int32), ("relax_cell", C.c_int32)]


FIRE_STARTED, FIRE_CONVERGED, FIRE_ERROR = 1, 2, 4   # M3G_FIRE_* flag bits


class M3GLbfgsParams(C.Structure):   # m3g_lbfgs_params
    _fields_ = [("maxstep", C.c_double), ("damping", C.c_double), ("alpha", C.c_double), ("fmax", C.c_double), ("memory", C.c_int32),
                ("relax_cell", C.c_int32)]


LBFGS_STARTED, LBFGS_CONVERGED, LBFGS_ERROR = FIRE_STARTED, FIRE_CONVERGED, FIRE_ERROR   # M3G_LBFGS_*: the bits of M3G_FIRE_*
LBFGS_MAX_MEMORY = 2047   # M3G_LBFGS_MAX_MEMORY


class M3GDynParams(C.Structure):   # m3g_dyn_params
    _fields_ = [("ensemble", C.c_int32), ("fix_com", C.c_int32), ("dt", C.c_double), ("taut", C.c_double), ("friction", C.c_double),
                ("pressure", C.c_double), ("taup", C.c_double), ("compressibility", C.c_double)]


class M3GNhcParams(C.Structure):   # m3g_nhc_params
    _fields_ = [("ensemble", C.c_int32), ("fix_com", C.c_int32), ("chain_length", C.c_int32), ("chain_substeps", C.c_int32),
                ("dt", C.c_double), ("taut", C.c_double), ("pressure", C.c_double), ("taup", C.c_double)]


class M3GMtkParams(C.Structure):   # m3g_mtk_params
    _fields_ = [("cell_mask", C.c_int32), ("fix_com", C.c_int32), ("chain_length", C.c_int32), ("chain_substeps", C.c_int32),
                ("dt", C.c_double), ("taut", C.c_double), ("pressure", C.c_double), ("taup", C.c_double)]


class M3GPimdParams(C.Structure):   # m3g_pimd_params
    _fields_ = [("thermostat", C.c_int32), ("n_beads", C.c_int32), ("dt", C.c_double), ("centroid_friction", C.c_double),
                ("pile_lambda", C.c_double)]


class M3GTiParams(C.Structure):   # m3g_ti_params
    _fields_ = [("schedule", C.c_int32), ("reserved", C.c_int32), ("dt", C.c_double), ("friction", C.c_double)]


class M3GRnemdParams(C.Structure):   # m3g_rnemd_params
    _fields_ = [("kind", C.c_int32), ("axis", C.c_int32), ("flow_axis", C.c_int32), ("n_slabs", C.c_int32), ("n_swaps", C.c_int32),
                ("reserved", C.c_int32)]


class M3GMetaParams(C.Structure):   # m3g_meta_params
    _fields_ = [("n_cv", C.c_int32), ("reserved", C.c_int32), ("max_hills", C.c_int64), ("kind", C.c_int32 * 2), ("power", C.c_int32 * 2),
                ("r0", C.c_double * 2), ("r_cut", C.c_double * 2), ("direction", (C.c_double * 3) * 2)]


DYN_NVE, DYN_NVT_BERENDSEN, DYN_NVT_LANGEVIN, DYN_NPT_BERENDSEN = range(4)   # M3G_DYN_* ensembles
NHC_NVT, NHC_NPT_MTK, NHC_MAX_CHAIN, NHC_OBS = 0, 1, 8, 6                   # M3G_NHC_* ensembles, M3G_NHC_MAX_CHAIN, M3G_NHC_OBS
MTK_CELL_FULL, MTK_CELL_ORTHORHOMBIC, MTK_OBS = 0, 1, 12                    # M3G_MTK_CELL_* masks, M3G_MTK_OBS
PIMD_NONE, PIMD_PILE_L, PIMD_MAX_BEADS, PIMD_OBS = 0, 1, 64, 8               # M3G_PIMD_* thermostats, M3G_PIMD_MAX_BEADS, M3G_PIMD_OBS
TI_LINEAR, TI_SMOOTH, TI_OBS = 0, 1, 8                                      # M3G_TI_* schedules, M3G_TI_OBS
DYN_STARTED, DYN_ERROR = 1, 2                                               # M3G_DYN_* flag bits
MC_NO_PAIR, MC_PENDING, MC_ERR_ORDER = 1, 2, 4                              # M3G_MC_* flag bits
RNEMD_HEAT, RNEMD_MOMENTUM, RNEMD_MAX_SWAPS, RNEMD_MAX_SLABS = 0, 1, 8, 64   # M3G_RNEMD_* kinds, M3G_RNEMD_MAX_SWAPS, M3G_RNEMD_MAX_SLABS
META_MAX_CV, META_OBS, META_ERROR, META_FULL = 2, 8, 1, 2                    # M3G_META_MAX_CV, M3G_META_OBS, M3G_META_* flag bits
CV_DISTANCE, CV_PROJECTION, CV_COORDINATION = range(3)                       # M3G_CV_* kinds
NEB_ROWS = 5                                                              # M3G_NEB_ROWS
PH_MAX_MULTIPLICITY = 27                                                     # M3G_PH_MAX_MULTIPLICITY
EIGH_MAX_N, EIGH_MAX_SWEEPS = 64, 30                                         # M3G_EIGH_MAX_N, M3G_EIGH_MAX_SWEEPS
EIGH_SWEEPS_MASK, EIGH_NONFINITE, EIGH_NOT_CONVERGED = 0xff, 0x100, 0x200    # M3G_EIGH_* info bits
PH_THZ, PH_GV_MAX_N, PH_GV_MAX_SET = 15.63330423985619, 256, 16              # M3G_PH_THZ, M3G_PH_GV_MAX_N, M3G_PH_GV_MAX_SET


class M3GTrajSizes(C.Structure):   # m3g_traj_sizes
    _fields_ = [("n_atoms", C.c_int64), ("n_structs", C.c_int64), ("max_species", C.c_int32), ("rdf_bins", C.c_int32),
                ("n_lags", C.c_int32)]


class M3GTrajParams(C.Structure):   # m3g_traj_params
    _fields_ = [("r_max", C.c_double), ("remove_com", C.c_int32)]


TRAJ_RDF_RANGE, TRAJ_MAX_SPECIES, TRAJ_MAX_BINS, TRAJ_MAX_LAGS = 1, 8, 4096, 4096   # M3G_TRAJ_RDF_RANGE and the limits of m3g_traj_sizes


class M3GSqSizes(C.Structure):   # m3g_sq_sizes
    _fields_ = [("n_atoms", C.c_int64), ("n_structs", C.c_int64), ("n_q", C.c_int64), ("max_species", C.c_int32), ("n_lags", C.c_int32)]


class M3GSqParams(C.Structure):   # m3g_sq_params
    _fields_ = [("remove_com", C.c_int32), ("reserved", C.c_int32)]


SQ_MAX_INDEX, SQ_MAX_Q, SQ_MAX_SPECIES, SQ_MAX_LAGS, SQ_CELL = 128, 4096, 4, 4096, 1   # M3G_SQ_MAX_*, M3G_SQ_CELL

LO_MAX_DEGREE, LO_MAX_DEGREES, LO_MAX_NEIGHBORS, LO_MAX_SPECIES, LO_MAX_BINS, LO_MAX_SERIES = 12, 3, 32, 4, 1024, 65536   # M3G_LO_MAX_*
LO_CELL, LO_RANGE, LO_NEIGHBORS, LO_NONFINITE = 1, 2, 4, 8   # M3G_LO_* flags


class M3GLoSizes(C.Structure):   # m3g_lo_sizes
    _fields_ = [("n_atoms", C.c_int64), ("n_structs", C.c_int64), ("max_species", C.c_int32), ("n_degrees", C.c_int32),
                ("hist_bins", C.c_int32), ("series_cap", C.c_int32)]


class M3GLoParams(C.Structure):   # m3g_lo_params
    _fields_ = [("degrees", C.c_int32 * LO_MAX_DEGREES), ("solid_degree", C.c_int32), ("solid_bonds", C.c_int32),
                ("solid_threshold", C.c_double)]


THERMO_ROW, THERMO_COMOMENTS, THERMO_TENSOR, THERMO_MAX_LAGS, THERMO_NONFINITE = 11, 66, 7, 4096, 1   # M3G_THERMO_*


class M3GThermoSizes(C.Structure):   # m3g_thermo_sizes
    _fields_ = [("n_atoms", C.c_int64), ("n_structs", C.c_int64), ("n_lags", C.c_int32)]


class M3GThermoParams(C.Structure):   # m3g_thermo_params
    _fields_ = [("remove_com", C.c_int32)]


class M3GNmaSizes(C.Structure):   # m3g_nma_sizes
    _fields_ = [("n_atoms", C.c_int64), ("n_structs", C.c_int64), ("n_unit_atoms", C.c_int64), ("n_qpoints", C.c_int64),
                ("n_modes", C.c_int64), ("n_eig", C.c_int64), ("n_phase", C.c_int64), ("max_n", C.c_int32), ("n_lags", C.c_int32)]


class M3GNmaParams(C.Structure):   # m3g_nma_params
    _fields_ = [("remove_com", C.c_int32), ("reserved", C.c_int32)]


NMA_MAX_N, NMA_MAX_LAGS, NMA_NONFINITE = 64, 4096, 1                          # M3G_NMA_MAX_N, M3G_NMA_MAX_LAGS, M3G_NMA_NONFINITE


class M3GPhSizes(C.Structure):   # m3g_ph_sizes
    _fields_ = [("n_structs", C.c_int64), ("n_unit_atoms", C.c_int64), ("n_super_atoms", C.c_int64), ("n_pairs", C.c_int64)]


class M3GElSizes(C.Structure):   # m3g_el_sizes
    _fields_ = [("n_structs", C.c_int64), ("n_atoms", C.c_int64), ("n_deform", C.c_int32), ("mode", C.c_int32)]


EL_VOLUMETRIC, EL_MODE_ELASTIC, EL_MODE_EOS, EL_MAX_DEFORM, EL_MAX_STRAIN = 6, 0, 1, 64, 0.2   # M3G_EL_*
EL_ROW, EL_EOS_ROW = 132, 8                                                  # M3G_EL_ROW, M3G_EL_EOS_ROW
EL_EOS_NONFINITE, EL_EOS_NO_MINIMUM = 1, 2                                   # M3G_EL_EOS_* error bits

# name -> (restype, argtypes); every symbol include/m3gnet_hip.h declares
SYMBOLS = {
    "m3g_get_info": (C.c_int, [C.POINTER(M3GInfo)]),
    "m3g_last_error": (C.c_char_p, []),
    "m3g_plan_create": (C.c_int, [C.POINTER(M3GConfig), C.POINTER(C.c_void_p)]),
    "m3g_plan_destroy": (None, [C.c_void_p]),
    "m3g_plan_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "m3g_plan_set_const": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "m3g_plan_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "m3g_plan_commit": (C.c_int, [C.c_void_p]),
    "m3g_topology_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_topology_build": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.c_void_p]),
    "m3g_topology_build_hints": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "m3g_topology_build_canonical": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "m3g_topology_build_canonical_begin": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "m3g_topology_build_canonical_end": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "m3g_topology_hints": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "m3g_topology_status": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "m3g_topology_active_edges": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "m3g_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_energy_forces": (C.c_int, [C.c_void_p, C.POINTER(M3GIO), C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_distance_angle": (C.c_int, [C.c_double, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_edge_featurizer": (C.c_int, [C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "m3g_atom_featurizer": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_atom_ref": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_linear": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_multiply": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_bessel_basis": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_three_body": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_conv_block_scratch_bytes": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_conv_block": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_readout": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_verlet_scratch_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_verlet_rows": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_verlet_update": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_double, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]),
    "m3g_verlet_update_async": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_double, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "m3g_verlet_fill": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_verlet_fill_lists": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_neighbor_scratch_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_neighbor_count": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                     C.c_size_t, C.POINTER(C.c_int64), C.c_void_p]),
    "m3g_neighbor_count_triplets": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_float,
                                              C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]),
    "m3g_threebody_build": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_neighbor_fill": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_threebody_scratch_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_threebody_count": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_int64), C.c_void_p]),
    "m3g_threebody_fill": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "m3g_debug_read_stamps": (C.c_int, [C.c_void_p, C.c_void_p]),
    "m3g_debug_live_handles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "m3g_md_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "m3g_md_destroy": (None, [C.c_void_p]),
    "m3g_md_set_lists": (C.c_int, [C.c_void_p, C.POINTER(M3GMdLists)]),
    "m3g_md_invalidate": (C.c_int, [C.c_void_p]),
    "m3g_md_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(M3GMdResult),
                              C.c_void_p]),
    "m3g_topology_data_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_topology_debug_last_path": (C.c_int, [C.POINTER(C.c_int32)]),
    "m3g_debug_exclusive_scan": (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_debug_radix_sort": (C.c_int, [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "m3g_debug_topology_layout": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "m3g_count_launches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "m3g_fire_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_fire_init": (C.c_int, [C.POINTER(M3GFireParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p]),
    "m3g_fire_step": (C.c_int, [C.POINTER(M3GFireParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_fire_read": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_lbfgs_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
    "m3g_lbfgs_init": (C.c_int, [C.POINTER(M3GLbfgsParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "m3g_lbfgs_step": (C.c_int, [C.POINTER(M3GLbfgsParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_lbfgs_read": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "m3g_dyn_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_dyn_init": (C.c_int, [C.POINTER(M3GDynParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_dyn_step": (C.c_int, [C.POINTER(M3GDynParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_dyn_read": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_dyn_state_view": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "m3g_nhc_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
    "m3g_nhc_state_view": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "m3g_nhc_init": (C.c_int, [C.POINTER(M3GNhcParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_void_p]),
    "m3g_nhc_step": (C.c_int, [C.POINTER(M3GNhcParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_nhc_read": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "m3g_mtk_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
    "m3g_mtk_state_view": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "m3g_mtk_init": (C.c_int, [C.POINTER(M3GMtkParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_void_p]),
    "m3g_mtk_step": (C.c_int, [C.POINTER(M3GMtkParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_mtk_read": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "m3g_pimd_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
    "m3g_pimd_state_view": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "m3g_pimd_init": (C.c_int, [C.POINTER(M3GPimdParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_pimd_step": (C.c_int, [C.POINTER(M3GPimdParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p]),
    "m3g_pimd_read": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "m3g_ti_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_ti_state_view": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "m3g_ti_init": (C.c_int, [C.POINTER(M3GTiParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_ti_path": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "m3g_ti_step": (C.c_int, [C.POINTER(M3GTiParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_ti_read": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_remd_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_remd_init": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_remd_exchange": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                    C.c_int64, C.c_void_p]),
    "m3g_remd_read": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_remd_target_view": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_mc_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_mc_init": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_mc_propose": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "m3g_mc_decide": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "m3g_mc_read": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_rnemd_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
    "m3g_rnemd_init": (C.c_int, [C.POINTER(M3GRnemdParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "m3g_rnemd_exchange": (C.c_int, [C.POINTER(M3GRnemdParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "m3g_rnemd_read": (C.c_int, [C.POINTER(M3GRnemdParams), C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_meta_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_meta_state_view": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_meta_init": (C.c_int, [C.POINTER(M3GMetaParams), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_size_t, C.c_void_p]),
    "m3g_meta_bias": (C.c_int, [C.POINTER(M3GMetaParams), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_meta_set_hills": (C.c_int, [C.POINTER(M3GMetaParams), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_meta_read": (C.c_int, [C.POINTER(M3GMetaParams), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_traj_state_bytes": (C.c_int, [C.POINTER(M3GTrajSizes), C.POINTER(C.c_size_t)]),
    "m3g_traj_init": (C.c_int, [C.POINTER(M3GTrajSizes), C.POINTER(M3GTrajParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_size_t, C.c_void_p]),
    "m3g_traj_sample": (C.c_int, [C.POINTER(M3GTrajSizes), C.POINTER(M3GTrajParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "m3g_traj_read": (C.c_int, [C.POINTER(M3GTrajSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_traj_frame": (C.c_int, [C.POINTER(M3GTrajSizes), C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_sq_state_bytes": (C.c_int, [C.POINTER(M3GSqSizes), C.POINTER(C.c_size_t)]),
    "m3g_sq_init": (C.c_int, [C.POINTER(M3GSqSizes), C.POINTER(M3GSqParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_sq_sample": (C.c_int, [C.POINTER(M3GSqSizes), C.POINTER(M3GSqParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_double, C.c_void_p]),
    "m3g_sq_read": (C.c_int, [C.POINTER(M3GSqSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]),
    "m3g_sq_frame": (C.c_int, [C.POINTER(M3GSqSizes), C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_lo_state_bytes": (C.c_int, [C.POINTER(M3GLoSizes), C.POINTER(C.c_size_t)]),
    "m3g_lo_init": (C.c_int, [C.POINTER(M3GLoSizes), C.POINTER(M3GLoParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                              C.c_void_p]),
    "m3g_lo_sample": (C.c_int, [C.POINTER(M3GLoSizes), C.POINTER(M3GLoParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_lo_read": (C.c_int, [C.POINTER(M3GLoSizes), C.c_void_p, C.c_size_t] + [C.c_void_p] * 10),
    "m3g_lo_frame": (C.c_int, [C.POINTER(M3GLoSizes), C.c_void_p, C.c_size_t] + [C.c_void_p] * 8),
    "m3g_thermo_state_bytes": (C.c_int, [C.POINTER(M3GThermoSizes), C.POINTER(C.c_size_t)]),
    "m3g_thermo_init": (C.c_int, [C.POINTER(M3GThermoSizes), C.POINTER(M3GThermoParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_thermo_sample": (C.c_int, [C.POINTER(M3GThermoSizes), C.POINTER(M3GThermoParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p]),
    "m3g_thermo_read": (C.c_int, [C.POINTER(M3GThermoSizes), C.c_void_p, C.c_size_t] + [C.c_void_p] * 10),
    "m3g_thermo_frame": (C.c_int, [C.POINTER(M3GThermoSizes), C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_nma_state_bytes": (C.c_int, [C.POINTER(M3GNmaSizes), C.POINTER(C.c_size_t)]),
    "m3g_nma_init": (C.c_int, [C.POINTER(M3GNmaSizes), C.POINTER(M3GNmaParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_nma_sample": (C.c_int, [C.POINTER(M3GNmaSizes), C.POINTER(M3GNmaParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_double, C.c_void_p]),
    "m3g_nma_read": (C.c_int, [C.POINTER(M3GNmaSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_nma_frame": (C.c_int, [C.POINTER(M3GNmaSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_neb_state_bytes": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "m3g_neb_init": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "m3g_neb_forces": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "m3g_ph_state_bytes": (C.c_int, [C.POINTER(M3GPhSizes), C.POINTER(C.c_size_t)]),
    "m3g_ph_init": (C.c_int, [C.POINTER(M3GPhSizes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                              C.c_size_t, C.c_void_p]),
    "m3g_ph_displace": (C.c_int, [C.POINTER(M3GPhSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "m3g_ph_force_constants": (C.c_int, [C.POINTER(M3GPhSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "m3g_ph_dynmat": (C.c_int, [C.POINTER(M3GPhSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p]),
    "m3g_ph_dynmat_gradient": (C.c_int, [C.POINTER(M3GPhSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_void_p]),
    "m3g_ph_group_velocities": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "m3g_eigh_batched": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_el_state_bytes": (C.c_int, [C.POINTER(M3GElSizes), C.POINTER(C.c_size_t)]),
    "m3g_el_init": (C.c_int, [C.POINTER(M3GElSizes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                              C.c_void_p]),
    "m3g_el_deform": (C.c_int, [C.POINTER(M3GElSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_el_fit_elastic": (C.c_int, [C.POINTER(M3GElSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_el_fit_eos": (C.c_int, [C.POINTER(M3GElSizes), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m3g_profile_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "m3g_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_float),
                                   C.POINTER(C.c_int32)]),
}
MAX_STAGES = 16

_lib = None


def build_library(verbose: bool = False) -> Path:
    """Compile csrc/*.hip for gfx950 with hipcc (make).  Cross-compiles without a GPU."""
    proc = subprocess.run(["make", "-C", str(_PKG_ROOT), "-j8"], capture_output=True, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout[-4000:])
        print(proc.stderr[-4000:])
    if proc.returncode != 0:
        raise RuntimeError("building libm3gnet_hip.so failed")
    return LIB_PATH


def load_library():
    """Load the HIP engine.  Fails loudly when it is missing -- there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `make -C {_PKG_ROOT}` (or __graft_entry__.build()); "
            "torch_m3gnet has no CPU/eager fallback"
        )
    lib = C.CDLL(str(LIB_PATH), mode=os.RTLD_GLOBAL if hasattr(os, "RTLD_GLOBAL") else C.DEFAULT_MODE)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> None:
    """Translate an m3g_status into the exception the reference would raise."""
    if status == M3G_OK:
        return
    msg = load_library().m3g_last_error().decode(errors="replace")
    if status == M3G_ERR_VALUE:
        raise ValueError(msg)
    raise RuntimeError(f"m3gnet_hip error {status}: {msg}")

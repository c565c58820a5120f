/*
 * m3gnet_hip.h -- C ABI of libm3gnet_hip.so: MI355X (gfx950) M3GNet energy/force engine.
 *
 * The reference (lan496/torch-m3gnet) has no FFI: its operator boundary is the Python module
 * protocol `forward(graph) -> graph` over keyed tensors.  This header is the
 * plain-C boundary that protocol binds to in the MI355X build: every entry point names the
 * reference interface it replaces (paths relative to /root/reference/src/torch_m3gnet).
 *
 * Conventions
 *   - all `const float*` / `const int64_t*` / `void*` data arguments are DEVICE pointers unless
 *     the parameter name starts with `host_`;
 *   - buffers are caller-owned; the library never allocates inside a hot call -- scratch comes
 *     from the caller (sizes from m3g_workspace_bytes / m3g_topology_bytes);
 *   - every call takes the HIP stream to enqueue on (`hipStream_t` passed as void*); calls are
 *     asynchronous with respect to the host unless stated otherwise;
 *   - return value: 0 = M3G_OK, otherwise an m3g_status; m3g_last_error() gives a message
 *     (thread-local).  The Python host turns M3G_ERR_VALUE into ValueError (the reference raises
 *     ValueError for too-large l_max/n_max, nn/interaction.py:250-253) and the rest into RuntimeError;
 *   - thread-compatible: no global mutable state; one plan may be used from one thread at a time.
 *
 * Tensor layouts are those of the reference's MaterialGraph (data/material_graph.py:14-107):
 *   pos [N,3] f32, atom_types [N] i64 (Z-1), edge_index [2,E] i64 (row 0 centre i, row 1
 *   neighbour j, SORTED BY CENTRE), edge_cell_shift [E,3] i32, triplet_edge_index [2,T] i64
 *   (row 0 = edge ij, row 1 = edge ik, any order), lattice [S,3,3] f32 row-wise, batch [N] i64.
 */
#ifndef M3GNET_HIP_H
#define M3GNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  M3G_OK = 0,
  M3G_ERR_VALUE = 1,    /* bad hyper-parameter / malformed graph (Python: ValueError) */
  M3G_ERR_STATE = 2,    /* call order violated (e.g. parameters not committed) */
  M3G_ERR_SIZE = 3,     /* caller buffer too small */
  M3G_ERR_HIP = 4,      /* a HIP runtime call failed */
  M3G_ERR_UNSUPPORTED = 5
} m3g_status;

/* Hyper-parameters == arguments of build_model (model/build.py:16-28). */
typedef struct {
  double cutoff;            /* Angstrom, unscaled (Python float == double, as the reference holds it) */
  double threebody_cutoff;  /* Angstrom, unscaled */
  double energy_scale;
  double length_scale;
  int32_t l_max;
  int32_t n_max;
  int32_t num_types;
  int32_t embedding_dim;
  int32_t num_blocks;
  int32_t reserved;
} m3g_config;

typedef struct m3g_plan m3g_plan; /* opaque: packed weights + constants + kernel selection */

/* Library / device probe.  Returns M3G_OK and fills the fields when a gfx950 device is usable. */
typedef struct {
  int32_t abi_version;
  int32_t device_count;
  char arch[32]; /* gcnArchName of the current device, "" when none */
} m3g_info;
int m3g_get_info(m3g_info* out);
const char* m3g_last_error(void);

/* ---- plan: replaces module construction in build_model (model/build.py:37-81) -------------- */
int m3g_plan_create(const m3g_config* cfg, m3g_plan** out);
void m3g_plan_destroy(m3g_plan* plan);

/* Set one parameter by its reference state_dict key ("model.7.concat_edge_update.dense.0.weight",
 * ...).  HOST pointer, row-major as torch stores it, `numel` floats.  Unknown key
 * or wrong size -> M3G_ERR_VALUE. */
int m3g_plan_set_param(m3g_plan* plan, const char* key, const float* host_data, int64_t numel);

/* Constants the reference keeps as plain module attributes (not in state_dict):
 *   "elemental_energies" [num_types]   AtomRef            (nn/atom_ref.py:17-23)
 *   "em" "dm" "coeff"     [n_max]      EdgeFeaturizer     (nn/featurizer.py:61-79)
 *   "factors"             [l_max,n_max] NormalizedSphericalBessel (nn/interaction.py:256-266)
 *   "bessel_zeros"        [l_max,n_max] rows 0..l_max-1 of SPHERICAL_BESSEL_ZEROS (interaction.py:14-135)
 * HOST pointers. */
int m3g_plan_set_const(m3g_plan* plan, const char* name, const float* host_data, int64_t numel);

/* Engine options (not part of the reference):
 *   "precision"   arithmetic of the dense products of the gated MLPs (nn/core.py:61-62: fp32 Linear layers), fp32 accumulate in all modes:
 *                   0 (default) "fp32": every product on v_mfma_f32_16x16x4_f32 -- exact fp32 products accumulated in k order, bitwise
 *                   an fp32 fmaf chain: the reference's arithmetic;
 *                   2 "f16x3" (opt-in, narrower than fp32): every operand scaled by a power of two (weights: one for the model;
 *                   activations and gradients: one per edge and chain, chosen from the data) and split in two fp16 parts that
 *                   together carry 22-24 significant bits, three v_mfma_f32_16x16x32_f16 products per fp32 product (lo x lo
 *                   dropped) -- errors ~1.8 x those of an fp32 fmaf chain, parity inside north_star's tolerances on every case;
 *                   1 "bf16x3" (opt-in): two bf16 parts (16 significant bits), three v_mfma_f32_16x16x32_bf16 products (relative
 *                   product error ~2^-16; the fastest mode, parity within north_star's tolerances on near-linear weights only);
 *                   all weight image sets are resident after a commit, switching costs nothing;
 *   "edge_kernel" = 1 fused MFMA edge blocks (default), 0 = vector-ALU baseline kernels (also M3G_EDGE_KERNEL in the env),
 *                   2 = the any-size path (run-time-sized fp32 kernels; chosen automatically for embedding_dim > 64,
 *                   l_max or n_max > 4, more than 8 blocks -- up to the reference's own limits l_max <= 9, n_max <= 10);
 *   "save_p1" / "save_p2" (fp32 mode, default 1): the forward kernel saves SiLU'(p1) / the layer-2 pre-activations of both conv
 *                   MLPs for the reverse kernel (no recompute MFMAs) -- 0 for A/B measurements;
 *   "rev_kernel"  = 1 one fused reverse kernel per block (default; fp32 mode: k_edge_rev_f32 on the saved activations, bf16x3
 *                   mode: k_edge_rev_fused recomputing them), 0 = node-MLP + edge-MLP kernel pair (both modes, A/B tests);
 *   "stress_mode" = 0 the reference's sum pos (x) F / V (nn/gradient.py:39-62, default), 1 = pair virial
 *                   -(1/V) sum_e r_e (x) dE/dr_e (docs/gradient.md:47-84), invariant under lattice translations;
 *   "readout_f16" = 1 the readout layers run on scaled two-part fp16 chains in the f16x3 mode (5 us per step faster at 10,000 atoms);
 *                   default 0: exact-fp32 MFMA chains in every mode (energies that are the small remainder of larger terms keep
 *                   fp32's 24 bits per product);
 *   "threebody_moments" = 1 (default) the three-body sums run over per-atom moments when m3g_io.topo_hints says every centre's
 *                   triplet list is complete (m3g_topology_hints), 0 = always walk the lists (A/B tests);
 *   "legendre_backward" = 0 (default) d P_l / d cos(theta) is the true derivative; 1 = what the reference's
 *                   LegendreCosPolynomial.backward returns (nn/interaction.py:373-382 multiplies grad_output in at every level of
 *                   its recurrence: inexact for l >= 2), so forces and stresses reproduce the reference's own numbers rather than
 *                   the gradient of its energy.  Not linear in a triplet's incoming gradient: the list kernels run (as with
 *                   "threebody_moments" = 0).  Energies are unaffected;
 *   "overlap"     = 1 the three-body reverse of a block runs on an internal side stream beside the node reverse's gather
 *                   (fork/join with events on the caller's stream), 0 = everything on the caller's stream (default: the
 *                   cross-stream waits measured slower than the overlap gains on the benchmark workload);
 *   "graph_replay" = 1 m3g_energy_forces captures its launch sequence into a hipGraph the first time it sees a given
 *                   (m3g_io contents, workspace, stream, options) and replays it on later identical calls (launch-bound
 *                   small systems); every buffer of the call must stay alive at the same address.  Default 0;
 *   "stamps"      = 1 / 2 / 3: diagnostic builds with in-kernel cycle stamps (m3g_debug_read_stamps), 0 off;
 *   "debug_force_move" = 1 (tests) the next m3g_plan_commit takes the device-move path although the device is unchanged. */
int m3g_plan_set_option(m3g_plan* plan, const char* name, int32_t value);

/* Pack and upload everything set so far (synchronous; drains the device first).  Must be called before any compute
 * call and again after parameters/constants change.  Missing keys -> M3G_ERR_STATE.  The plan's device buffers live on the
 * HIP device that is current at commit; committing again under another device moves them there, and m3g_energy_forces
 * under a device other than the plan's returns M3G_ERR_STATE. */
int m3g_plan_commit(m3g_plan* plan);

/* ---- topology: replaces nothing in the reference nn (which re-gathers by index on every call);
 * it converts MaterialGraph index tensors into the receiver-sorted CSR form the kernels use.
 * Depends on the index tensors only -- reusable across calls while they are unchanged. ---------- */
int m3g_topology_bytes(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs, size_t* bytes);
/* The call waits for the stream once (it reads back whether the triplet list is sorted and symmetric, which decides the
 * sorts); on return host_flags[0] != 0 means the graph is malformed (the remaining kernels of the build may still be running):
 *   bit 0: edge_index[0] not sorted; bit 1: index out of range; bit 2: triplet edges with different centres. */
int m3g_topology_build(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs,
                       const int64_t* edge_index, const int64_t* triplet_edge_index, const int64_t* batch,
                       void* topo, size_t topo_bytes, int32_t* host_flags, void* stream);

/* What the build found out about the graph that lets m3g_energy_forces pick cheaper kernels: an opaque word for m3g_io.topo_hints
 * (0 is always valid).  Today: M3G_TOPO_TB_COMPLETE -- every centre atom's triplet list holds each ordered pair of its active
 * edges exactly once (what compute_threebody emits, data/material_graph.py:196-254), so the three-body sums may run over per-atom
 * moments instead of the lists -- plus the largest window sizes the kernels then need.  The certificate is formed by this call (a
 * few small kernels over the lists, then one wait for the stream: about what the moment kernels save in four steps on a 10k-atom
 * Cu cell, in one step on a dense cell), so ask once per topology that will be used repeatedly and keep the word with the buffer. */
#define M3G_TOPO_TB_COMPLETE 1
int m3g_topology_hints(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs, const void* topo,
                       int32_t* host_hints, void* stream);
/* m3g_topology_build + m3g_topology_hints with ONE wait for the device: for the lists the graph builders emit (triplets sorted by
 * (e1, e2) and symmetric, symmetric edge list) the whole build and the certificate are queued on that assumption and a single
 * read-back confirms it; other lists redo the affected parts.  host_hints may be NULL (then exactly m3g_topology_build). */
int m3g_topology_build_hints(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs,
                             const int64_t* edge_index, const int64_t* triplet_edge_index, const int64_t* batch,
                             void* topo, size_t topo_bytes, int32_t* host_flags, int32_t* host_hints, void* stream);

/* m3g_topology_build_hints for lists THIS LIBRARY's builders have just written (m3g_neighbor_fill / m3g_verlet_fill /
 * m3g_verlet_fill_lists + m3g_threebody_*), untouched since: their triplet lists are symmetric and complete by construction, so the
 * mirror check of the triplet list and the per-row completeness test of the certificate are skipped; index ranges, row order and
 * edge-list symmetry are still checked.  Handing it any other list is a caller error (the moment kernels would then sum over
 * partners the list does not hold).  Replaces the host loops of data/material_graph.py:196-254 on the trajectory path. */
int m3g_topology_build_canonical(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs,
                                 const int64_t* edge_index, const int64_t* triplet_edge_index, const int64_t* batch,
                                 void* topo, size_t topo_bytes, int32_t* host_flags, int32_t* host_hints, void* stream);

/* m3g_topology_build_canonical in two calls, so that the host prepares its next call (workspace, outputs, the m3g_io block) while
 * the device builds: _begin queues the launches and the copy of the verdict words to `pinned_verdict` -- at least 8 int32 of PINNED
 * host memory (hipHostMalloc / torch pin_memory) the caller leaves untouched until _end; _end (same stream, same arguments) waits for
 * the stream and certifies the buffer, or -- when a check failed or _begin did not apply (no triplets, more atoms than its
 * one-workgroup scan takes) -- runs the general build there and then.  Results and errors are those of m3g_topology_build_canonical. */
int m3g_topology_build_canonical_begin(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs,
                                       const int64_t* edge_index, const int64_t* triplet_edge_index, const int64_t* batch,
                                       void* topo, size_t topo_bytes, int32_t* pinned_verdict, void* stream);
int m3g_topology_build_canonical_end(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs,
                                     const int64_t* edge_index, const int64_t* triplet_edge_index, const int64_t* batch,
                                     void* topo, size_t topo_bytes, const int32_t* pinned_verdict, int32_t* host_flags,
                                     int32_t* host_hints, void* stream);

/* Diagnostic / tests: the leading part of a topology buffer that holds the lists the kernels read (the rest is scratch of the build),
 * and which build m3g_topology_build_canonical took on this thread the last time: 1 = the six-launch build for canonical lists,
 * 0 = the general one (a failed check, no hints asked for, no triplets, or more atoms than its one-workgroup scan takes). */
int m3g_topology_data_bytes(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs, size_t* bytes);
int m3g_topology_debug_last_path(int32_t* path);

/* Sticky error bits the hot call left on a topology buffer (0 = none).  M3G_TOPO_ERR_HINTS: m3g_energy_forces was handed a
 * non-zero m3g_io.topo_hints that is not the word m3g_topology_hints certified for THIS buffer (stale after a rebuild, or copied
 * from another topology): the three-body moment kernels then touch nothing (no out-of-bounds access) and the call's three-body
 * terms, hence its results, are INVALID.  m3g_energy_forces itself never reads the word back (that would stall the stream):
 * a caller that passes hints words around must poll this entry point -- once per topology is enough, the bits are sticky (the
 * Python engine does so at the second call with a topology).  Synchronises the stream. */
#define M3G_TOPO_ERR_HINTS 1
#define M3G_TOPO_ERR_SYNC 2    /* an in-launch wait between workgroup roles ran into its bound (never expected; the rows that were waited for
                                * are replaced by NaN, so the call's forces are NaN as well) */
#define M3G_TOPO_ERR_SPECIES 4 /* an atom_types entry outside [0, num_types): the reference raises there (IndexError at
                                * elemental_energies[atom_types], nn/atom_ref.py:27).  The hot call cannot return it without a wait, so it
                                * never indexes with such a value (clamped), stores NaN as that atom's energy -- its structure's energy is
                                * then NaN -- and sets this bit.  m3g_md_step checks the species itself and returns M3G_ERR_VALUE. */
int m3g_topology_status(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs, const void* topo,
                        int32_t* host_status, void* stream);

/* Number of ACTIVE edges of a built topology: edges that appear in either column of triplet_edge_index (the three-body
 * arrays of the workspace hold one row per active edge).  Synchronises the stream. */
int m3g_topology_active_edges(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs, const void* topo,
                              int64_t* host_count, void* stream);

/* ---- the hot call: replaces Gradient.forward over the whole Sequential (nn/gradient.py:25-64,
 * model/build.py:37-81): energies, forces, virial stresses ------------------------------------- */
int m3g_workspace_bytes(const m3g_plan* plan, int64_t n_atoms, int64_t n_edges, int64_t n_triplets,
                        int64_t n_structs, size_t* bytes);

typedef struct {
  /* inputs (MaterialGraph) */
  int64_t n_atoms, n_edges, n_triplets, n_structs;
  const float* pos;               /* [N,3] */
  const int64_t* atom_types;      /* [N] */
  const int32_t* edge_cell_shift; /* [E,3] */
  const float* lattice;           /* [S,3,3] */
  const void* topo;               /* from m3g_topology_build for the same index tensors */
  const int64_t* triplet_edge_index; /* [2,T] original order; only read when triplet_angles != NULL */
  /* required outputs */
  float* total_energy; /* [S]   MaterialGraphKey.TOTAL_ENERGY */
  float* forces;       /* [N,3] MaterialGraphKey.FORCES (may be NULL: energy only, no reverse pass) */
  /* optional outputs (NULL to skip) -- the other keys the reference writes */
  float* stresses;               /* [S,6] Voigt xx,yy,zz,yz,zx,xy (nn/gradient.py:39-62) */
  float* scaled_total_energy;    /* [S] */
  float* scaled_atomic_energies; /* [N] */
  float* node_features;          /* [N,D]  "x" after the last block */
  float* edge_attr;              /* [E,D]  after the last block */
  float* edge_distances;         /* [E] (scaled length units) */
  float* edge_weights;           /* [E,n_max] */
  float* triplet_angles;         /* [T] cos(theta_jik), original triplet order */
  float* mid_edge_features;      /* [num_blocks,E,l_max*n_max] three-body aggregate of every block */
  /* optional input */
  int32_t topo_hints;            /* from m3g_topology_hints for `topo` (0: none -- always valid, the general kernels) */
  int32_t reserved;              /* 0 */
} m3g_io;

int m3g_energy_forces(const m3g_plan* plan, const m3g_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* ---- stage entry points: the reference modules a caller may run on their own ----------------- */
/* ScaleLength + DistanceAndAngle (nn/scale.py:24-29, nn/invariant.py:20-59) */
int m3g_distance_angle(double length_scale, int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs,
                       const float* pos, const float* lattice, const int32_t* edge_cell_shift, const void* topo,
                       const int64_t* triplet_edge_index, float* scratch_unit_vectors /* [E,3] */,
                       float* edge_distances, float* triplet_angles, void* stream);
/* EdgeFeaturizer.forward (nn/featurizer.py:81-100); host_em/dm/coeff are HOST arrays [n_max]; n_max in 1..10, the degrees
 * m3g_plan_commit accepts (1..4 on the kernel of the MFMA path, 5..10 on the any-size path's radial basis: the same terms) */
int m3g_edge_featurizer(int32_t n_max, double scaled_cutoff, const float* host_em, const float* host_dm,
                        const float* host_coeff, int64_t n_edges, const float* edge_distances, float* edge_weights,
                        void* stream);
/* AtomFeaturizer.forward (nn/featurizer.py:33-38): x[a,:] = W[:, types[a]]; weight [D,num_types] DEVICE */
int m3g_atom_featurizer(int32_t num_types, int32_t dim, const float* weight, int64_t n_atoms,
                        const int64_t* atom_types, float* x, void* stream);
/* AtomRef.forward (nn/atom_ref.py:25-29) */
int m3g_atom_ref(int32_t num_types, const float* elemental_energies, int64_t n_atoms, const int64_t* atom_types,
                 float* out, void* stream);

/* ---- stand-alone forward of the block modules (any size; run-time-sized fp32 kernels, csrc/m3g_generic.hip).  The reference's
 * modules can be called one by one (tests/test_model.py:14-38 runs the bare Sequential); these are their kernels. -------------- */
/* torch.nn.Linear + activation: Y = act(X W^T + b); act 0 none, 1 SiLU, 2 sigmoid (nn/core.py:31-59, nn/featurizer.py:128-132) */
int m3g_linear(int64_t n, int32_t in_features, int32_t out_features, const float* x, const float* weight, const float* bias /* or NULL */,
               int32_t act, float* y, void* stream);
/* y = a * b: the dense(x) * gate(x) of GatedMLP.forward (nn/core.py:61-62) */
int m3g_multiply(int64_t n, const float* a, const float* b, float* y, void* stream);
/* NormalizedSphericalBessel.forward (nn/interaction.py:268-281): out [l_max, n_max, n]; host_zeros / host_factors HOST [l_max*n_max] */
int m3g_bessel_basis(int32_t l_max, int32_t n_max, double cutoff, const float* host_zeros, const float* host_factors, int64_t n,
                     const float* rs, float* out, void* stream);
/* ThreeBodyInteration.forward (nn/interaction.py:187-223): edge_attr [E,D] updated in place from the graph's edge_distances,
 * triplet_angles and node features; scratch EXACTLY (N*C + E*C + 2*E*D) floats, C = l_max*n_max, never NULL (one float serves when
 * that is 0); mid (or NULL) receives the aggregate [E,C].  The indices are NOT range-checked on the device: the caller passes
 * edge_index < N and triplet_edge_index < E (torch_m3gnet.nn checks them on the host before the call) */
int m3g_three_body(int32_t l_max, int32_t n_max, int32_t embedding_dim, double scaled_cutoff, double scaled_threebody_cutoff,
                   const float* host_zeros, const float* host_factors, int64_t n_atoms, int64_t n_edges, int64_t n_triplets,
                   const int64_t* edge_index, const int64_t* triplet_edge_index, const float* edge_distances, const float* triplet_angles,
                   const float* x, const float* w_sigmoid, const float* b_sigmoid, const float* w_dense, const float* w_gate, float* scratch,
                   float* edge_attr, float* mid, void* stream);
/* M3GNetConv.forward (nn/conv.py:63-97): x [N,D] and edge_attr [E,D] updated in place.  host_params: HOST array of 18 DEVICE pointers,
 * edge MLP {dense.0.weight, gate.0.weight, dense.0.bias, gate.0.bias, dense.2.weight, gate.2.weight, dense.2.bias, gate.2.bias,
 * edge_linear.weight}, then the node MLP likewise (node_linear.weight last).  scratch: m3g_conv_block_scratch_bytes, i.e.
 * (11*E*D + 1024) floats: eleven [E,D] activation arrays, and 1024 floats so that the buffer is never empty */
int m3g_conv_block_scratch_bytes(int32_t embedding_dim, int64_t n_edges, size_t* bytes);
int m3g_conv_block(int32_t embedding_dim, int32_t n_max, int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs,
                   const void* topo, const float* const* host_params, const float* edge_weights, float* x, float* edge_attr, float* scratch,
                   size_t scratch_bytes, void* stream);
/* AtomWiseReadout.forward (nn/readout.py:39-58).  host_params: HOST array of 12 DEVICE pointers {dense.0.weight, dense.0.bias,
 * dense.2.weight, dense.2.bias, dense.4.weight, dense.4.bias, gate.0.weight, ...}; scratch EXACTLY (4*N*D + 2*N) floats (two hidden
 * layers of two branches, in place of their pre-activations, and the two outputs; may be NULL when N = 0).  batch is NOT
 * range-checked on the device: the caller passes batch < n_structs (torch_m3gnet.nn checks it on the host before the call) */
int m3g_readout(int32_t embedding_dim, int64_t n_atoms, int64_t n_structs, const float* const* host_params, double energy_scale,
                const float* x, const float* elemental_energies_per_atom, const int64_t* batch, float* scaled_atomic_energies,
                float* scaled_total_energy, float* total_energy, float* scratch, void* stream);

/* ---- graph construction on the GPU -------------------------------------
 * Periodic neighbour list: replaces get_all_neighbors_with_cell_shifts (data/material_graph.py:168-193, pymatgen
 * Structure.get_all_neighbors).  pos [N,3] and lattice [S,3,3] are DEVICE fp64 (pymatgen works in double), batch
 * [N] int64 sorted.  Output order: centre atom, edge cell shift (sx, sy, sz) lexicographic, neighbour index
 * (the shift refers to the given coordinates: the order does not depend on which atoms sit outside the home cell).  Two phases because the
 * edge count is data dependent: *_count synchronises the stream and returns E, the caller allocates, *_fill writes.
 * max_images >= (2rx+1)(2ry+1)(2rz+1) of every structure, r_p = ceil((cutoff+1e-8) |a_q x a_r| / V). */
int m3g_neighbor_scratch_bytes(int64_t n_atoms, int64_t n_structs, int64_t max_images, size_t* bytes);
int m3g_neighbor_count(int64_t n_atoms, int64_t n_structs, int64_t max_images, const double* pos, const double* lattice,
                       const int64_t* batch, double cutoff, void* scratch, size_t scratch_bytes, int64_t* host_n_edges,
                       void* stream);
/* m3g_neighbor_count that also returns, from the same pass and the same wait, the number of triplets the list will have under
 * `threebody_cutoff` (valid edges: fp32 length <= it, as compute_threebody thresholds them): a caller building both lists sizes
 * every tensor after ONE wait for the device and follows up with m3g_neighbor_fill + m3g_threebody_build. */
int m3g_neighbor_count_triplets(int64_t n_atoms, int64_t n_structs, int64_t max_images, const double* pos, const double* lattice,
                                const int64_t* batch, double cutoff, float threebody_cutoff, void* scratch, size_t scratch_bytes,
                                int64_t* host_n_edges, int64_t* host_n_triplets, void* stream);
int m3g_neighbor_fill(int64_t n_atoms, int64_t n_structs, int64_t max_images, const int64_t* batch, double cutoff,
                      void* scratch, int64_t n_edges, int64_t* edge_index /* [2,E] */, int32_t* edge_cell_shift /* [E,3] */,
                      double* distances /* [E] */, void* stream);
/* Three-body index: replaces compute_threebody (data/material_graph.py:196-254), same triplet order.  distances are
 * the fp32 edge lengths the reference thresholds (material_graph.py:191,224). */
int m3g_threebody_scratch_bytes(int64_t n_atoms, int64_t n_edges, size_t* bytes);
int m3g_threebody_count(int64_t n_atoms, int64_t n_edges, const int64_t* edge_index, const float* distances,
                        float threebody_cutoff, void* scratch, size_t scratch_bytes, int64_t* host_n_triplets, void* stream);
int m3g_threebody_fill(int64_t n_atoms, int64_t n_edges, const int64_t* edge_index, void* scratch, int64_t n_triplets,
                       int64_t* triplet_edge_index /* [2,T] */, int64_t* num_triplet_i /* [N] or NULL */,
                       int32_t* num_triplet_ij /* [E] or NULL */, void* stream);
/* m3g_threebody_count + m3g_threebody_fill in one call when n_triplets is known already (m3g_neighbor_count_triplets): no wait
 * for the device; scratch from m3g_threebody_scratch_bytes. */
int m3g_threebody_build(int64_t n_atoms, int64_t n_edges, const int64_t* edge_index, const float* distances, float threebody_cutoff,
                        void* scratch, size_t scratch_bytes, int64_t n_triplets, int64_t* triplet_edge_index /* [2,T] */,
                        int64_t* num_triplet_i /* [N] */, int32_t* num_triplet_ij /* [E] */, void* stream);

/* ---- skin ("Verlet") list: repeated evaluation along an MD trajectory without a search per step --------------------
 * The reference rebuilds everything for every structure it sees, in Python (data/material_graph.py:133-254).  For a trajectory
 * the caller keeps CANDIDATES -- the list m3g_neighbor_count/fill return for cutoff + skin at reference positions -- on the
 * device, with their row pointers (m3g_verlet_rows) and one membership byte per candidate.  While no atom has moved by more than
 * skin / 2 since the reference, the candidates that pass d <= cutoff, in candidate order, are EXACTLY the list a fresh search at
 * the current positions returns (same edges, order, shifts, hence the same triplets): the canonical order does not depend on the
 * positions, and every distance is formed by the search's own arithmetic.
 *   m3g_verlet_update   one pass over atoms and candidates at the current positions (DEVICE fp64, unwrapped like pos_ref): the
 *                       largest displacement since pos_ref, whether any candidate's membership (bit 0: in the list; bit 1: fp32
 *                       length within the three-body cutoff) differs from cand_state -- the membership the caller's current lists
 *                       were filled with --, and the sizes E, T the lists have now.  Waits for the stream once.  changed == 0 and
 *                       max_disp < skin / 2: the current edge_index / edge_cell_shift / triplets / topology / hints stay valid,
 *                       only the positions of the next m3g_energy_forces call are new.
 *   m3g_verlet_fill     (changed != 0, max_disp < skin / 2) writes the new list from the candidates and updates cand_state; follow
 *                       with m3g_threebody_build (n_triplets from the update) and m3g_topology_build.  No wait.
 * max_disp >= skin / 2 (or a changed lattice): search again with cutoff + skin, pos_ref = pos, then update with cand_state = NULL
 * (fresh candidates: reported as changed) + fill.
 * cand_row_ptr: int32 [N + 2] (N + 1 pointers and one scratch word). */
int m3g_verlet_scratch_bytes(int64_t n_atoms, int64_t n_candidates, size_t* bytes);
int m3g_verlet_rows(int64_t n_atoms, int64_t n_candidates, const int64_t* cand_edge_index /* [2,Ec] */, int32_t* cand_row_ptr, void* stream);
int m3g_verlet_update(int64_t n_atoms, int64_t n_structs, int64_t n_candidates, const double* pos, const double* pos_ref,
                      const double* lattice, const int64_t* batch, const int64_t* cand_edge_index, const int32_t* cand_shift,
                      const int32_t* cand_row_ptr, double cutoff, float threebody_cutoff, const uint8_t* cand_state, void* scratch,
                      size_t scratch_bytes, double* host_max_disp, int32_t* host_changed, int64_t* host_n_edges,
                      int64_t* host_n_triplets, void* stream);
/* m3g_verlet_update without the wait: the pass and its 48-byte result copy are queued on the stream; host_out (PINNED host memory,
 * SIX words) receives {bits of max_disp^2 as a double, changed, E, T, (internal), the longest candidate row -- what
 * m3g_verlet_fill_lists wants as max_cand_row} when the stream reaches the copy.  A caller may queue the evaluation
 * behind it on the assumption that nothing changed and read the verdict afterwards. */
int m3g_verlet_update_async(int64_t n_atoms, int64_t n_structs, int64_t n_candidates, const double* pos, const double* pos_ref,
                            const double* lattice, const int64_t* batch, const int64_t* cand_edge_index, const int32_t* cand_shift,
                            const int32_t* cand_row_ptr, double cutoff, float threebody_cutoff, const uint8_t* cand_state, void* scratch,
                            size_t scratch_bytes, uint64_t* host_out /* [6] */, void* stream);
int m3g_verlet_fill(int64_t n_atoms, int64_t n_candidates, int64_t n_edges, void* scratch, const int64_t* cand_edge_index,
                    const int32_t* cand_shift, const int32_t* cand_row_ptr, int64_t* edge_index /* [2,E] */,
                    int32_t* edge_cell_shift /* [E,3] */, double* distances /* [E] */, uint8_t* cand_state /* [Ec] out */, void* stream);
/* m3g_verlet_fill + m3g_threebody_build in TWO launches: edge list, shifts, membership bytes, triplet list (the reference's
 * order, data/material_graph.py:239-248) and the per-centre / per-edge triplet counts straight from the candidates and the state the
 * preceding m3g_verlet_update left in `scratch` (n_edges, n_triplets: its E and T).  max_cand_row = the longest candidate row (the
 * caller knows it from cand_row_ptr); rows beyond M3G_VERLET_FILL_LISTS_MAX_ROW or more than 262,144 atoms return
 * M3G_ERR_UNSUPPORTED -- use the two calls above, which have no limits and return identical lists.  No wait.
 * Replaces, for a trajectory, the per-structure rebuild of data/material_graph.py:168-254. */
#define M3G_VERLET_FILL_LISTS_MAX_ROW 1024
/* m3g_verlet_update(_async) runs its whole pass in ONE launch up to this many atoms and in three launches (wrap, rows, totals) above
 * it; both classify every pair through the same device functions and return the same verdict.  Not a limit of any call: it names
 * the regime, so that a test can place itself on either side. */
#define M3G_VERLET_ONE_LAUNCH_MAX_ATOMS 512
int m3g_verlet_fill_lists(int64_t n_atoms, int64_t n_candidates, int64_t n_edges, int64_t n_triplets, int64_t max_cand_row, void* scratch,
                          const int64_t* cand_edge_index, const int32_t* cand_shift, const int32_t* cand_row_ptr,
                          int64_t* edge_index /* [2,E] */, int32_t* edge_cell_shift /* [E,3] */, uint8_t* cand_state /* [Ec] out */,
                          int64_t* triplet_edge_index /* [2,T] */, int64_t* num_triplet_i /* [N] or NULL */,
                          int32_t* num_triplet_ij /* [E] or NULL */, void* stream);

/* ---- one trajectory step per call: skin test, lists + topology when they changed, energies / forces / stresses ------------------
 * Replaces, for a structure followed along a trajectory, the reference's per-frame MaterialGraph.from_structure
 * (data/material_graph.py:132-254) + Gradient.forward (nn/gradient.py:25-64).  The caller searches the candidates (cutoff + skin;
 * m3g_neighbor_*, m3g_verlet_rows) and hands them over with list buffers of the candidates' capacity -- every pointer device memory
 * it owns and keeps alive until the next m3g_md_set_lists / m3g_md_destroy; the library then sequences m3g_verlet_update_async, (when
 * a pair crossed a cutoff) m3g_verlet_fill_lists + m3g_topology_build_canonical, and m3g_energy_forces itself.  Per step the host
 * waits twice at most (the verdict's sizes; the topology's certificate) and allocates nothing.  Same kernels on the same inputs as
 * the separate calls: identical lists, bit-identical results. */
typedef struct m3g_md m3g_md;
typedef struct {
  int64_t n_atoms, n_structs, n_cand;     /* N, S, number of candidate pairs Ec */
  int64_t cap_edges, cap_triplets;        /* capacity of the list buffers below (cap_edges >= n_cand; cap_triplets: an upper bound of
                                           * T for every configuration within skin / 2 of pos_ref, e.g. sum_i c_i (c_i - 1) over the
                                           * candidates within threebody_cutoff + skin) */
  double cutoff, threebody_cutoff, skin;
  const double* pos_ref;                  /* [N,3] positions the candidates were searched at */
  const double* lattice;                  /* [S,3,3] */
  const float* lattice32;                 /* [S,3,3] the same in fp32 (m3g_io.lattice) */
  const int64_t* batch;                   /* [N] */
  const int64_t* atom_types;              /* [N] */
  const int64_t* cand_edge_index;         /* [2,Ec] */
  const int32_t* cand_shift;              /* [Ec,3] */
  const int32_t* cand_row_ptr;            /* [N+2] (m3g_verlet_rows) */
  uint8_t* cand_state;                    /* [Ec+16] membership bytes (written by the library) */
  void* verlet_scratch; size_t verlet_scratch_bytes;   /* m3g_verlet_scratch_bytes(N, Ec) */
  int64_t* edge_index;                    /* [2 * cap_edges]      the lists the library re-derives: read as [2,E] / [E,3] / [2,T] / */
  int32_t* edge_cell_shift;               /* [3 * cap_edges]      [N] / [E] with the E, T of m3g_md_result */
  int64_t* triplet_edge_index;            /* [2 * cap_triplets] */
  int64_t* num_triplet_i;                 /* [N] */
  int32_t* num_triplet_ij;                /* [cap_edges] */
  float* pos32;                           /* [N,3] */
  void* topo; size_t topo_bytes;          /* m3g_topology_bytes(N, cap_edges, cap_triplets, S) */
  void* workspace; size_t workspace_bytes;/* m3g_workspace_bytes(plan, N, cap_edges, cap_triplets, S) */
} m3g_md_lists;
#define M3G_MD_REUSE 0        /* lists unchanged: the step ran on the standing lists */
#define M3G_MD_REFILL 1       /* a pair crossed a cutoff (or first step / asked for): lists and topology re-derived, then the step */
#define M3G_MD_NEED_SEARCH 2  /* an atom moved further than skin / 2: NOTHING was evaluated; search again, m3g_md_set_lists, call again */
#define M3G_MD_UNSUPPORTED 3  /* candidate rows beyond M3G_VERLET_FILL_LISTS_MAX_ROW, or lists beyond the buffers' capacity: NOTHING was
                               * evaluated; use the separate calls for this step */
typedef struct {
  int32_t path, topo_hints;
  int64_t n_edges, n_triplets;            /* of the lists the step ran on (path 0 / 1), of the verdict otherwise */
  double max_displacement;                /* largest |pos - pos_ref| */
} m3g_md_result;
int m3g_md_create(m3g_md** md);
void m3g_md_destroy(m3g_md* md);
int m3g_md_set_lists(m3g_md* md, const m3g_md_lists* lists);
int m3g_md_invalidate(m3g_md* md);   /* the caller has rewritten cand_state / the list buffers through other calls: re-derive at the next step */
/* pos: [N,3] fp64 device positions (unwrapped).  forces / stresses may be NULL (energies only).  force_refill != 0: re-derive the
 * lists whatever the verdict says (tests, timing).  Waits for `stream` (verdict) -- the outputs are queued, not waited for.
 * Behind that one wait the call also learns (ABI 6): whether atom_types lies in [0, num_types) of `plan` -- checked once per list set
 * and model; M3G_ERR_VALUE otherwise, as the reference raises IndexError (nn/atom_ref.py:25-29) -- and whether an EARLIER step left
 * sticky error bits on the topology buffer (M3G_TOPO_ERR_*): M3G_ERR_STATE, nothing evaluated, the next call re-derives lists and
 * topology.  M3G_MD_UNSUPPORTED also answers a workspace that has become too small for the plan's current options (the caller makes
 * buffers again).  cand_state and the list buffers may be NULL when n_cand == 0. */
int m3g_md_step(m3g_md* md, const m3g_plan* plan, const double* pos, float* total_energy, float* forces, float* stresses,
                int32_t force_refill, m3g_md_result* host_result, void* stream);

/* ---- batched structure relaxation: FIRE, fixed or variable cell (csrc/m3g_relax.hip) ---------------------------------------------
 * Replaces the reference's relaxation script (scripts/relax_org.py -> m3gnet's Relaxer: ASE's FIRE over a UnitCellFilter, one
 * optimiser per structure on the host).  Every structure of a batch is relaxed on its own, with the semantics of ASE's FIRE applied to
 * that structure alone (unit masses; the loop of ASE's Optimizer.run: evaluate -> converged? -> step).  relax_cell = 1 relaxes the cell
 * through ASE's UnitCellFilter (linear deformation gradient F = solve(L0, L)^T, cell_factor = the structure's atom count): generalized
 * coordinates X = [pos F^-T ; cell_factor F], generalized forces g = [f F ; W F^-T / cell_factor] with the virial W = V * stresses of
 * the PAIR-VIRIAL stresses (m3g_plan_set_option "stress_mode" = 1: the strain derivative; mode 0 is not one).  Converged means
 * max_i |g_i| < fmax over every row of the structure, cell rows included; a converged structure is FROZEN (positions, cell and FIRE
 * state bitwise unchanged by later calls); a structure whose g holds a non-finite value gets M3G_FIRE_ERROR and is never moved.
 * The state buffer (m3g_fire_state_bytes) is caller-owned device memory holding X, v, L0, F in fp64, the per-structure dt, a, n, flags
 * and step counts, and a chunk table of the batch made by m3g_fire_init (which waits for the stream). */
typedef struct {
  double dt, maxstep, dtmax, finc, fdec, astart, fa;   /* ASE defaults: 0.1, 0.2, 1.0, 1.1, 0.5, 0.1, 0.99 */
  double fmax;                                         /* > 0 */
  int32_t nmin;                                        /* 5 */
  int32_t relax_cell;                                  /* 0 positions only, 1 positions and cell */
} m3g_fire_params;
#define M3G_FIRE_STARTED 1     /* the structure has taken a step (ASE's v is no longer None) */
#define M3G_FIRE_CONVERGED 2   /* frozen: max_i |g_i| < fmax was seen */
#define M3G_FIRE_ERROR 4       /* frozen: its generalized forces held a non-finite value */
int m3g_fire_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes);
/* host_offsets: HOST int64 [S+1], 0 = o_0 < o_1 < ... < o_S = N (atoms of structure s: [o_s, o_s+1)).  pos [N,3] and lattice [S,3,3]
 * (rows = lattice vectors; may be NULL with the cell fixed) DEVICE fp64: the starting point (L0).  Invalid parameters (fmax <= 0, ...) or
 * offsets -> M3G_ERR_VALUE.  Waits for the stream. */
int m3g_fire_init(const m3g_fire_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* pos,
                  const double* lattice, void* state, size_t state_bytes, void* stream);
/* One FIRE iteration of the batch at the forces [N,3] / stresses [S,6] (f32 DEVICE, Voigt xx,yy,zz,yz,zx,xy, pair-virial convention;
 * stresses may be NULL with the cell fixed) evaluated at the current pos: convergence and error verdicts, then one step of every other
 * structure, which updates pos [N,3] fp64 and (relax_cell) lattice [S,3,3] fp64 / lattice32 [S,3,3] f32 (may be NULL) IN PLACE.  params:
 * those of m3g_fire_init.  check_only != 0: the verdicts only, nothing moves (the evaluation after the last step).  `unconverged` (may be
 * NULL; device or pinned host memory) receives the number of structures that are neither converged nor failed after this call.  Three
 * launches whatever S (two with check_only), no allocation and no wait: capture-safe.  A cell relaxation without stresses or lattice
 * -> M3G_ERR_VALUE. */
int m3g_fire_step(const m3g_fire_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                  const float* stresses, double* pos, double* lattice, float* lattice32, int32_t check_only, int32_t* unconverged, void* stream);
/* Per-structure flags (M3G_FIRE_*), step counts, dt, a, n [S] and the generalized coordinates / velocities [N + 3S, 3] (the N atom
 * rows, then three cell rows per structure) to HOST memory; every output may be NULL.  Waits for the stream. */
int m3g_fire_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int32_t* host_steps,
                  double* host_dt, double* host_a, int32_t* host_n, double* host_x, double* host_v, void* stream);

/* ---- batched structure relaxation: L-BFGS beside FIRE, fixed or variable cell (csrc/m3g_lbfgs.hip) ------------------------------
 * ASE's LBFGS without line search, applied to every structure of a batch on its own, over the generalized coordinates X and forces g
 * of the FIRE calls above (the same cell filter, the same verdicts, the same freezing; grad = -g).  Per call and structure: the
 * verdicts; then, once the structure has stepped, the pair s = X - X_prev, y = grad - grad_prev joins its history with rho = 1 / y.s
 * (only the newest `memory` pairs are kept; a pair whose y.s is zero or not finite is NOT stored, where ASE would divide by zero --
 * two equal fp32 force arrays give y = 0; a negative y.s is kept, as in ASE); the two-loop recursion with H0 = 1 / alpha gives the
 * direction p; longest = max over rows |p_row| (cell rows included), p *= maxstep / longest when longest >= maxstep, dr = damping p;
 * a non-finite dr flags the structure M3G_LBFGS_ERROR and does not move it; else X_prev = X, grad_prev = grad, X += dr.
 * The state buffer is caller-owned device memory; with C = ceil(N / 256) + S, R = N + 3 S, M = memory + 1 it holds, each region rounded
 * up to 256 bytes: the chunk table (8 (S+1) + 4 C + 8 C + 4 (S+1)), partial sums 8 * 5 * C * (M + 1) + 8 C, the vectors X, X_prev, grad,
 * grad_prev, p (8 * 3R each), the rings of s and y (8 * 3R * M each: the dominant term, memory * 2 * 3(N+3S) * 8), L0 and F (8 * 9 * S
 * each), per structure two Gram blocks s_i.y_j, y_i.y_j (8 * M * M each) and five coefficient vectors (8 * M each), four int32 words and
 * 16 doubles. */
typedef struct {
  double maxstep, damping, alpha;   /* ASE defaults: 0.2, 1.0, 70.0 (H0 = 1 / alpha); all > 0 */
  double fmax;                      /* > 0 */
  int32_t memory;                   /* 100; 1 <= memory <= M3G_LBFGS_MAX_MEMORY */
  int32_t relax_cell;               /* 0 positions only, 1 positions and cell */
} m3g_lbfgs_params;
#define M3G_LBFGS_STARTED 1     /* the structure has taken a step (X_prev and grad_prev are set); the bits of M3G_FIRE_* */
#define M3G_LBFGS_CONVERGED 2   /* frozen: max_i |g_i| < fmax was seen */
#define M3G_LBFGS_ERROR 4       /* frozen: its generalized forces or its step held a non-finite value */
#define M3G_LBFGS_MAX_MEMORY 2047
int m3g_lbfgs_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t memory, size_t* bytes);
/* Arguments as the FIRE init call.  Invalid parameters (memory < 1, a non-finite or non-positive maxstep, damping, alpha or fmax,
 * relax_cell not 0 or 1), bad offsets or a cell relaxation without lattice -> M3G_ERR_VALUE before any HIP call; a short state buffer
 * -> M3G_ERR_SIZE.  Waits for the stream. */
int m3g_lbfgs_init(const m3g_lbfgs_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* pos,
                   const double* lattice, void* state, size_t state_bytes, void* stream);
/* One L-BFGS iteration of the batch; arguments, units, check_only and `unconverged` as the FIRE step call.  FIVE launches whatever the
 * memory, the history depth reached and the batch (three with check_only), no atomics, no allocation and no wait: capture-safe.  params:
 * those of the init call. */
int m3g_lbfgs_step(const m3g_lbfgs_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                   const float* stresses, double* pos, double* lattice, float* lattice32, int32_t check_only, int32_t* unconverged, void* stream);
/* Per-structure flags (M3G_LBFGS_*), step counts, history depths (pairs stored, <= memory) [S] and the generalized coordinates
 * [N + 3S, 3] (the N atom rows, then three cell rows per structure) to HOST memory; every output may be NULL.  `memory`: that of the
 * init call.  Waits for the stream. */
int m3g_lbfgs_read(int64_t n_atoms, int64_t n_structs, int32_t memory, const void* state, size_t state_bytes, int32_t* host_flags,
                   int32_t* host_steps, int32_t* host_pairs, double* host_x, void* stream);

/* ---- batched molecular dynamics: NVE, NVT (Berendsen, Langevin BAOAB), NPT Berendsen (csrc/m3g_dynamics.hip) -------------------
 * Replaces the m3gnet package's MolecularDynamics (m3gnet.models.MolecularDynamics, the interface the reference stands in for: ASE's
 * VelocityVerlet "nve", NVTBerendsen "nvt" and NPTBerendsen "npt_berendsen" on one structure, on the host) for a whole batch, each
 * structure with its own target temperature and random stream.  Units: A, fs, amu, eV; velocities A/fs (fp64); a_i = kappa F_i / m_i
 * with kappa = 9.648533215665e-3; k_B = 8.617333262e-5 eV/K; KE_s = sum_i m_i |v_i|^2 / (2 kappa); T_s = 2 KE_s / (3 n_s k_B);
 * P_s = (tr W_s + lambda^2 2 KE_s) / (3 V_s) with the virial W = V * stresses of the PAIR-VIRIAL stresses (stress_mode 1).
 * One m3g_dyn_step at the forces F(x_k) of every structure not frozen:
 *   finish  (a structure that has started): v += dt/2 a;
 *   observables at the full step: KE, T, P (lambda = 1; NaN without stresses or lattice), V (NaN without lattice) -> obs[s] =
 *           {KE, T, P, V};
 *   start   (not with finish_only, which instead clears M3G_DYN_STARTED: the next call starts without a finish kick)
 *     NVE            ASE's VelocityVerlet: v += dt/2 a; fix_com: v_i -= pbar / m_i (pbar = sum_j m_j v_j / n after the kick); x += dt v
 *     NVT_BERENDSEN  ASE's NVTBerendsen: lambda = sqrt(max(1 + dt/taut (T0/T - 1), 0)) clamped to [0.9, 1.1] (1.1 when T = 0),
 *                    v = lambda v, then as NVE
 *     NPT_BERENDSEN  ASE's NPTBerendsen, isotropic: lambda as NVT, v = lambda v; mu = 1 - dt compressibility / (3 taup) (pressure -
 *                    P); lattice = mu lattice, x = mu x; then as NVE with the forces of the unscaled positions (as ASE)
 *     NVT_LANGEVIN   BAOAB (NOT ASE's Langevin scheme): v += dt/2 a; x += dt/2 v; v = c1 v + sqrt((1 - c1^2) k_B T0 kappa / m) xi,
 *                    c1 = exp(-friction dt); x += dt/2 v (the next finish is the final B).  xi: Philox4x64-10, key (seed_s, 0), counter
 *                    (k_s, i - o_s, 0, 0) with k_s the structure's count of starts; u_j = ((w_j >> 11) + 0.5) 2^-53, Box-Muller on
 *                    (u0, u1) -> xi_x, xi_y and (u2, u3) -> xi_z: a structure's noise does not depend on the rest of the batch.
 * A structure whose forces (or, in NPT, stresses) hold a non-finite value gets M3G_DYN_ERROR and is FROZEN: positions, cell,
 * velocities and its obs row are never written again.  No atomics: every result is bitwise the same alone or in any batch.
 * The state buffer (m3g_dyn_state_bytes) is caller-owned device memory: masses, velocities, target temperatures, seeds, flags, step
 * counts and the chunk table of the batch (the one of m3g_fire_*). */
typedef struct {
  int32_t ensemble;         /* M3G_DYN_NVE, M3G_DYN_NVT_BERENDSEN, M3G_DYN_NVT_LANGEVIN, M3G_DYN_NPT_BERENDSEN */
  int32_t fix_com;          /* 0 / 1: zero the total momentum at every start (not with NVT_LANGEVIN) */
  double dt;                /* fs, > 0 */
  double taut;              /* fs, > 0 (NVT_BERENDSEN, NPT_BERENDSEN) */
  double friction;          /* 1/fs, >= 0 (NVT_LANGEVIN) */
  double pressure;          /* eV/A^3, finite (NPT_BERENDSEN) */
  double taup;              /* fs, > 0 (NPT_BERENDSEN) */
  double compressibility;   /* A^3/eV, > 0 (NPT_BERENDSEN) */
} m3g_dyn_params;
#define M3G_DYN_NVE 0
#define M3G_DYN_NVT_BERENDSEN 1
#define M3G_DYN_NVT_LANGEVIN 2
#define M3G_DYN_NPT_BERENDSEN 3
#define M3G_DYN_STARTED 1   /* the structure's last call started a step: the next one finishes it */
#define M3G_DYN_ERROR 2     /* frozen: its forces (NPT: or stresses) held a non-finite value */
int m3g_dyn_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes);
/* host_offsets: HOST int64 [S+1] as m3g_fire_init; host_masses [N] (amu, > 0), host_temperatures [S] (target T0_s in K, finite, >= 0;
 * unused by NVE), host_seeds [S] (Philox keys): HOST.  vel [N,3] DEVICE fp64: the starting velocities (copied into the state).
 * Everything is validated on the host before any HIP call: an unknown ensemble, dt / taut / taup / compressibility not finite and > 0
 * where the ensemble uses it, friction < 0, a bad pressure, temperature or mass, bad offsets, or NVT_LANGEVIN with fix_com ->
 * M3G_ERR_VALUE.  Waits for the stream. */
int m3g_dyn_init(const m3g_dyn_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                 const double* host_temperatures, const uint64_t* host_seeds, const double* vel, void* state, size_t state_bytes,
                 void* stream);
/* One call per force evaluation (see above): forces [N,3] f32 DEVICE evaluated at pos; stresses [S,6] f32 DEVICE (Voigt xx,yy,zz,yz,zx,xy,
 * pair-virial convention; may be NULL except in NPT); pos [N,3] fp64 DEVICE (unwrapped), lattice [S,3,3] fp64 / lattice32 [S,3,3] f32
 * DEVICE (may be NULL except in NPT; lattice32 may be NULL always), all updated IN PLACE; obs [S,4] fp64 DEVICE or NULL.  params: those
 * of m3g_dyn_init.  Three launches whatever S, no allocation, copy or wait: capture-safe.  NPT without stresses or lattice ->
 * M3G_ERR_VALUE. */
int m3g_dyn_step(const m3g_dyn_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                 const float* stresses, double* pos, double* lattice, float* lattice32, int32_t finish_only, double* obs, void* stream);
/* Per-structure flags (M3G_DYN_*) and step counts (starts taken) [S] and the velocities [N,3] to HOST memory; every output may be
 * NULL.  Waits for the stream. */
int m3g_dyn_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int64_t* host_steps,
                 double* host_vel, void* stream);
/* Byte offsets, inside a state buffer of these sizes, of the masses [N] and the velocities [N,3] (fp64): a device-side reader (the
 * trajectory sampler below) takes the integrator's velocities without a copy.  Between two m3g_dyn_step calls they are the
 * half-step velocities of the step under way; after a finish_only call the full-step ones. */
int m3g_dyn_state_view(int64_t n_atoms, int64_t n_structs, size_t* mass_offset, size_t* velocity_offset);

/* ---- batched molecular dynamics, deterministic ensembles: Nose-Hoover chain NVT, isotropic MTK NPT (csrc/m3g_nhc.hip) -----------------
 * Time-reversible thermostat and barostat with a conserved quantity (Martyna, Tuckerman, Tobias, Klein, Mol. Phys. 87, 1117 (1996);
 * what ASE's NoseHooverChainNVT and LAMMPS' fix nvt / fix npt iso integrate), for a whole batch, each structure with its own target
 * temperature.  A family of its own beside m3g_dyn_*: that family's structs, state layout and results do not change.  Units and
 * constants as m3g_dyn_*; 2 KE = sum m |v|^2 / kappa in eV; thermostat and barostat velocities vxi, veps in 1/fs, their masses in
 * eV fs^2.  Per structure of n atoms: g = 3 n - 3 with fix_com, else 3 n; kT = k_B T0; particle chain masses Q_1 = g kT taut^2,
 * Q_k>1 = kT taut^2; barostat chain masses kT taup^2; W = (g + 3) kT taup^2; alpha = 1 + 3 / g.
 * One step is T(h) B(h) A(dt) [forces] B(h) T(h), h = dt / 2:
 *   chain half-step chain(Q, xi, vxi, K2, gkT, h) in chain_substeps equal parts d = h / n_c, each:  vxi_M += d/2 G_M;  k = M-1 .. 1:
 *           vxi_k = (vxi_k e + d/2 G_k) e, e = exp(-d/4 vxi_k+1);  s = exp(-d vxi_1), K2 = s^2 K2;  xi += d vxi;  the vxi updates again
 *           in ascending order with the new K2;  G_1 = (K2 - gkT) / Q_1, G_k = (Q_k-1 vxi_k-1^2 - kT) / Q_k.  The particle chain takes
 *           K2 = 2 KE, gkT = g kT and scales every velocity by the product of the s; the barostat chain K2 = W veps^2, gkT = kT, veps;
 *   T(h)    particle chain, then (NPT) barostat chain, then veps += h G_eps, G_eps = (alpha 2 KE + tr W - 3 V pressure) / W with
 *           tr W = V (s_0 + s_1 + s_2) of the PAIR-VIRIAL stresses; the closing T(h) of a step runs the three in the opposite order;
 *   B(h)    NVT v += h a;  NPT v = v exp(-2 y) + h a exp(-y) sinhc(y), y = alpha veps h / 2;  fix_com: v_i -= pbar / m_i after the
 *           opening kick (pbar = sum_j m_j v_j / n);
 *   A(dt)   NVT x += dt v;  NPT x = x exp(2 y) + dt v exp(y) sinhc(y), y = veps h, and lattice = exp(2 y) lattice;
 *           sinhc(y) = sinh(y) / y as its series to y^6 (|y| << 1).
 * One m3g_nhc_step at the forces F(x_k): the B(h) T(h) that close the step under way, obs[s] = {KE, T = 2 KE / (3 n k_B), P = (tr W +
 * 2 KE) / (3 V), V, extended, 0} -- T in the 3 n convention of m3g_dyn_*, so its canonical mean is T0 g / (3 n); extended = g kT xi_1
 * + kT sum_k>1 xi_k + 1/2 sum Q vxi^2, in NPT + pressure V + 1/2 W veps^2 + kT sum xib + 1/2 sum Qb vxib^2: E_pot + KE + extended is
 * conserved -- then the T(h) B(h) A(dt) that open the next step (not with finish_only, which clears M3G_DYN_STARTED instead).  The
 * kinetic energy after a uniform scale is known in closed form, so the atoms are passed over once per launch.  Flags are the
 * M3G_DYN_* bits: a structure whose forces (NPT: or stresses) hold a non-finite value gets M3G_DYN_ERROR and is frozen, bitwise.  No
 * atomics: every result is bitwise the same alone or in any batch. */
typedef struct {
  int32_t ensemble;         /* M3G_NHC_NVT, M3G_NHC_NPT_MTK */
  int32_t fix_com;          /* 0 / 1: zero the total momentum at every start; g = 3 n - 3 */
  int32_t chain_length;     /* M: 1 .. M3G_NHC_MAX_CHAIN thermostats per chain (particles, and in NPT the barostat) */
  int32_t chain_substeps;   /* n_c: 1 .. 8 equal parts of every chain half-step */
  double dt;                /* fs, > 0 */
  double taut;              /* fs, > 0 */
  double pressure;          /* eV/A^3, finite (NPT_MTK) */
  double taup;              /* fs, > 0 (NPT_MTK) */
} m3g_nhc_params;
#define M3G_NHC_NVT 0
#define M3G_NHC_NPT_MTK 1
#define M3G_NHC_MAX_CHAIN 8
#define M3G_NHC_OBS 6       /* columns of an obs row */
/* The state buffer is caller-owned device memory, one carve: the chunk table, chunk partials, masses, velocities (fp64), target
 * temperatures, flags, step counts, coefficients, then per structure xi[M], vxi[M], xib[M], vxib[M], veps.  Bad sizes (n_structs >
 * n_atoms, either < 1, chain_length outside 1 .. M3G_NHC_MAX_CHAIN) -> M3G_ERR_VALUE. */
int m3g_nhc_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* bytes);
/* Byte offsets of the masses [N] and the velocities [N,3] (fp64) inside a state buffer of these sizes, as m3g_dyn_state_view. */
int m3g_nhc_state_view(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* mass_offset, size_t* velocity_offset);
/* Arguments as m3g_dyn_init (no seeds: nothing here is random).  Validated on the host before any HIP call, with the reason in
 * m3g_last_error: an unknown ensemble, chain_length or chain_substeps outside 1 .. 8, dt / taut (NPT: taup) not finite and > 0, a bad
 * pressure or mass, bad offsets, a target temperature that is not finite and > 0 (the chain masses are proportional to it), or a
 * structure of one atom with fix_com -> M3G_ERR_VALUE.  Chain positions and velocities and veps start at 0.  Waits for the stream. */
int m3g_nhc_init(const m3g_nhc_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                 const double* host_temperatures, const double* vel, void* state, size_t state_bytes, void* stream);
/* One call per force evaluation; arguments as m3g_dyn_step, obs [S, M3G_NHC_OBS] fp64 DEVICE or NULL.  params: those of m3g_nhc_init.
 * Three launches whatever S and N, no allocation, copy or wait: capture-safe.  NPT without stresses or lattice -> M3G_ERR_VALUE. */
int m3g_nhc_step(const m3g_nhc_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                 const float* stresses, double* pos, double* lattice, float* lattice32, int32_t finish_only, double* obs, void* stream);
/* Flags and step counts [S], the velocities [N,3] and the chain rows [S, 4 M + 1] (xi, vxi, xib, vxib, veps) to HOST memory; every
 * output may be NULL.  Waits for the stream. */
int m3g_nhc_read(int64_t n_atoms, int64_t n_structs, int32_t chain_length, const void* state, size_t state_bytes, int32_t* host_flags,
                 int64_t* host_steps, double* host_vel, double* host_chain, void* stream);

/* ---- batched molecular dynamics, flexible-cell MTK NPT: the anisotropic barostat (csrc/m3g_mtk.hip) ----------------------------------
 * The fully flexible Martyna-Tobias-Klein barostat with Nose-Hoover chains (Martyna, Tobias, Klein, J. Chem. Phys. 101, 4177 (1994);
 * Mol. Phys. 87, 1117 (1996)): the cell changes shape as well as size.  A third family beside m3g_dyn_* and m3g_nhc_*: their structs,
 * state layouts and results do not change.  Units, flags, the 3 n temperature convention and the chain half-step are those of
 * m3g_nhc_*.  Positions and lattice rows are row vectors, so a symmetric 3x3 matrix acts from the right; such matrices are 6 numbers
 * in Voigt order xx, yy, zz, yz, zx, xy.  Per structure of n atoms: g = 3 n - 3 with fix_com, else 3 n; kT = k_B T0; Q_1 = g kT
 * taut^2, Q_k>1 = kT taut^2; the barostat variable is a symmetric rate vg (1/fs); cell_mask FULL moves all 6 of its components
 * (n_c = 6), ORTHORHOMBIC the diagonal only (n_c = 3; for cells whose vectors lie along the axes); W_g = (g + 3) kT taup^2 / 3 (the
 * isotropic family's W / 3: vg = veps I has the same kinetic energy); barostat chain masses Qb_1 = n_c kT taup^2, Qb_k>1 = kT taup^2.
 *   G       = mask o [K + W_vir - V pressure I + (tr K / g) I] / W_g, K = sum m v v^T / kappa (tr K = 2 KE), W_vir = V * the
 *             PAIR-VIRIAL stresses; tr G / 3 is the isotropic family's G_eps;
 *   T(h)    particle chain on tr K against g kT (scales v), barostat chain on W_g sum_ab vg_ab^2 against n_c kT (first thermostat;
 *           kT for the rest; scales vg), then vg += h G; the closing T(h) of a step runs the three in the opposite order;
 *   B(h)    v = v exp(-B) + h a phi1(-B), B = (vg + (tr vg / g) I) h;  fix_com: v_i -= pbar / m_i after the opening kick;
 *   A(dt)   x = x exp(A) + dt v phi1(A), A = vg dt, and lattice = lattice exp(A);
 *           phi1(A) = sum_k A^k / (k + 1)!; exp and phi1 by Horner at the fixed order 12, no eigensolver and no branch.
 * One step is T(h) B(h) A(dt) [forces] B(h) T(h), h = dt / 2, split over calls as m3g_nhc_step: one m3g_mtk_step at the forces F(x_k)
 * closes the step under way, writes obs[s] = {KE, T = 2 KE / (3 n k_B), P = tr / 3, V, extended, 0, then the pressure tensor (W_vir +
 * K) / V in Voigt order}, and opens the next (not with finish_only, which clears M3G_DYN_STARTED instead).  extended = g kT xi_1 + kT
 * sum_k>1 xi_k + 1/2 sum Q vxi^2 + pressure V + 1/2 W_g sum_ab vg_ab^2 + n_c kT xib_1 + kT sum_k>1 xib_k + 1/2 sum Qb vxib^2: E_pot +
 * KE + extended is conserved.  A structure whose forces or stresses hold a non-finite value, or whose max |vg_ab| dt exceeds 0.05 at
 * the end of the call's thermostat arithmetic (the series above are exact to fp64 below it), gets M3G_DYN_ERROR and is frozen, bitwise:
 * nothing of that call is kept.  The pressure is hydrostatic only.  A symmetric vg does not forbid a slow rigid rotation of the cell
 * (products of symmetric matrices are not symmetric); the physics does not see it.  No atomics: every result is bitwise the same alone
 * or in any batch. */
typedef struct {
  int32_t cell_mask;        /* M3G_MTK_CELL_FULL, M3G_MTK_CELL_ORTHORHOMBIC */
  int32_t fix_com;          /* 0 / 1: zero the total momentum at every start; g = 3 n - 3 */
  int32_t chain_length;     /* M: 1 .. M3G_NHC_MAX_CHAIN thermostats per chain (particles and barostat) */
  int32_t chain_substeps;   /* 1 .. 8 equal parts of every chain half-step */
  double dt;                /* fs, > 0 */
  double taut;              /* fs, > 0 */
  double pressure;          /* eV/A^3, finite; hydrostatic */
  double taup;              /* fs, > 0 */
} m3g_mtk_params;
#define M3G_MTK_CELL_FULL 0
#define M3G_MTK_CELL_ORTHORHOMBIC 1
#define M3G_MTK_OBS 12      /* columns of an obs row */
/* The state buffer is caller-owned device memory, one carve: the chunk table, chunk partials, masses, velocities (fp64), target
 * temperatures, flags, step counts, coefficients, then per structure xi[M], vxi[M], xib[M], vxib[M], vg[6].  Bad sizes as
 * m3g_nhc_state_bytes -> M3G_ERR_VALUE. */
int m3g_mtk_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* bytes);
/* Byte offsets of the masses [N] and the velocities [N,3] (fp64) inside a state buffer of these sizes, as m3g_dyn_state_view. */
int m3g_mtk_state_view(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* mass_offset, size_t* velocity_offset);
/* Arguments as m3g_nhc_init.  Validated on the host before any HIP call, with the reason in m3g_last_error: an unknown cell_mask,
 * fix_com not 0 / 1, chain_length or chain_substeps outside 1 .. 8, dt / taut / taup not finite and > 0, a bad pressure or mass, bad
 * offsets, a target temperature that is not finite and > 0, or a structure of one atom with fix_com -> M3G_ERR_VALUE.  Chain
 * positions and velocities and vg start at 0.  Waits for the stream. */
int m3g_mtk_init(const m3g_mtk_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                 const double* host_temperatures, const double* vel, void* state, size_t state_bytes, void* stream);
/* One call per force evaluation; arguments as m3g_nhc_step, obs [S, M3G_MTK_OBS] fp64 DEVICE or NULL.  params: those of m3g_mtk_init.
 * Three launches whatever S and N, no allocation, copy or wait: capture-safe.  Missing stresses or lattice -> M3G_ERR_VALUE. */
int m3g_mtk_step(const m3g_mtk_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                 const float* stresses, double* pos, double* lattice, float* lattice32, int32_t finish_only, double* obs, void* stream);
/* Flags and step counts [S], the velocities [N,3] and the chain rows [S, 4 M + 6] (xi, vxi, xib, vxib, vg) to HOST memory; every
 * output may be NULL.  Waits for the stream. */
int m3g_mtk_read(int64_t n_atoms, int64_t n_structs, int32_t chain_length, const void* state, size_t state_bytes, int32_t* host_flags,
                 int64_t* host_steps, double* host_vel, double* host_chain, void* stream);

/* ---- batched path-integral molecular dynamics: ring polymers under PILE-L (csrc/m3g_pimd.hip) ---------------------------------------
 * Nuclear quantum effects by imaginary-time path integrals (Ceriotti, Parrinello, Markland, Manolopoulos, J. Chem. Phys. 133, 124104
 * (2010)).  A fourth family beside m3g_dyn_*, m3g_nhc_* and m3g_mtk_*: their structs, state layouts and results do not change.  Units,
 * constants and flag bits as m3g_dyn_*; hbar = 0.6582119569 eV fs.  The S = R P structures of the batch are R ring polymers laid out
 * ring by ring: bead j of ring g is structure g P + j, and all P beads of a ring hold the same number of atoms n_g with the same
 * masses.  Temperatures, seeds, flags, step counts and obs rows are per RING.  Ring g at target temperature T samples
 *   H_P = sum_j [KE_j + 1/2 sum_i m_i w_P^2 |q_i,j - q_i,j+1|^2 + V(q_j)],  w_P = P k_B T / hbar,  at temperature P T,
 * so every bead feels the full force.  Normal modes: the real orthogonal C[j][k] = sqrt(1/P) (k = 0), sqrt(2/P) cos(2 pi j k / P)
 * (0 < 2 k < P), sqrt(1/P) (-1)^j (2 k = P), sqrt(2/P) sin(2 pi j k / P) (2 k > P), applied as the direct O(P^2) product, any P in
 * 1 .. M3G_PIMD_MAX_BEADS; mode frequencies w_k = 2 w_P sin(k pi / P).  One step is BAOAB, h = dt / 2:
 *   B(h)   v += h kappa F / m for every bead;
 *   A(h)   in normal modes: mode 0 drifts, x += h v; mode k >= 1 rotates exactly, x' = cos(w_k h) x + sin(w_k h) / w_k v,
 *          v' = cos(w_k h) v - w_k sin(w_k h) x;
 *   O(dt)  in normal modes (PILE_L only): v' = c1_k v + c2_k sqrt(P k_B T kappa / m_i) xi, c1_k = exp(-gamma_k dt), c2_k = sqrt(1 -
 *          c1_k^2), gamma_0 = centroid_friction, gamma_k = 2 pile_lambda w_k.  xi: Philox4x64-10, key (seed_g, 3), counter (the ring's
 *          count of starts before this one, the atom's index inside the ring, k, 0), u and Box-Muller as NVT_LANGEVIN of m3g_dyn_*;
 *   A(h), back to beads, [forces], B(h).
 * Thermostat NONE skips O (microcanonical ring-polymer MD, which conserves H_P); centroid_friction = 0 under PILE_L is TRPMD.  The
 * step is split over calls as m3g_dyn_step: one m3g_pimd_step at the forces F(x_k) closes the step under way with B(h), writes
 * obs[g] = {KE of all beads, T = 2 KE / (3 n P^2 k_B) (canonical mean: the target), E_spring, K_prim = 3 n P k_B T / 2 - E_spring / P,
 * K_cv = 3 n k_B T / 2 - 1 / (2 P) sum_j sum_i (q_i,j - qbar_i) . F_i,j with qbar the centroid of the unwrapped positions, heat, 0, 0},
 * then opens the next with B A O A (not with finish_only, which clears M3G_DYN_STARTED instead).  heat is the running sum, over the
 * O steps of all earlier calls, of the ring kinetic energy the thermostat added: sum_j E_j + KE + E_spring - heat is conserved up to
 * the integrator's O(dt^2).  A ring with a non-finite force on any bead gets M3G_DYN_ERROR and is frozen, all beads bitwise.  No
 * atomics: every result is bitwise the same alone or in any batch. */
typedef struct {
  int32_t thermostat;         /* M3G_PIMD_NONE, M3G_PIMD_PILE_L */
  int32_t n_beads;            /* P: 1 .. M3G_PIMD_MAX_BEADS, the same for every ring of the batch */
  double dt;                  /* fs, > 0 */
  double centroid_friction;   /* 1/fs, >= 0: gamma of mode 0 */
  double pile_lambda;         /* >= 0: gamma_k = 2 pile_lambda w_k for k >= 1 */
} m3g_pimd_params;
#define M3G_PIMD_NONE 0
#define M3G_PIMD_PILE_L 1
#define M3G_PIMD_MAX_BEADS 64
#define M3G_PIMD_OBS 8      /* columns of an obs row */
/* The state buffer is caller-owned device memory, one carve: the chunk table over RINGS, chunk partials, masses, velocities (fp64),
 * per ring the target temperature, seed, flags, step count and heat, the [P,P] table and per ring and mode cos(w_k h), sin(w_k h) /
 * w_k, w_k sin(w_k h), c1_k, c2_k (formed on the host in fp64 by the init call).  Bad sizes (as m3g_dyn_state_bytes, n_beads outside
 * 1 .. M3G_PIMD_MAX_BEADS or not a divisor of n_structs and n_atoms) -> M3G_ERR_VALUE. */
int m3g_pimd_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t n_beads, size_t* bytes);
/* Byte offsets of the masses [N] and the velocities [N,3] (fp64) inside a state buffer of these sizes, as m3g_dyn_state_view. */
int m3g_pimd_state_view(int64_t n_atoms, int64_t n_structs, int32_t n_beads, size_t* mass_offset, size_t* velocity_offset);
/* host_offsets [S+1], host_masses [N] as m3g_dyn_init; host_temperatures [R] (K), host_seeds [R], R = S / n_beads: HOST.  vel [N,3]
 * DEVICE fp64.  Validated on the host before any HIP call, with the reason in m3g_last_error: n_beads outside 1 .. 64 or not a
 * divisor of n_structs, beads of a ring with unequal atom counts or unequal masses, an unknown thermostat, dt not finite and > 0,
 * centroid_friction or pile_lambda not finite and >= 0, a temperature not finite and > 0, a bad mass, bad offsets -> M3G_ERR_VALUE;
 * a short state buffer -> M3G_ERR_SIZE.  Waits for the stream. */
int m3g_pimd_init(const m3g_pimd_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                  const double* host_temperatures, const uint64_t* host_seeds, const double* vel, void* state, size_t state_bytes,
                  void* stream);
/* One call per force evaluation: forces [N,3] f32 DEVICE evaluated at pos [N,3] fp64 DEVICE (unwrapped, moved IN PLACE); obs
 * [R, M3G_PIMD_OBS] fp64 DEVICE or NULL.  params: those of m3g_pimd_init.  Three launches whatever R, P and N, no allocation, copy,
 * wait or atomics: capture-safe.  Missing forces or pos -> M3G_ERR_VALUE. */
int m3g_pimd_step(const m3g_pimd_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                  double* pos, int32_t finish_only, double* obs, void* stream);
/* Flags, step counts and heat [R] and the velocities [N,3] to HOST memory; every output may be NULL.  heat holds the O steps up to
 * the one before the last call's.  Waits for the stream. */
int m3g_pimd_read(int64_t n_atoms, int64_t n_structs, int32_t n_beads, const void* state, size_t state_bytes, int32_t* host_flags,
                  int64_t* host_steps, double* host_heat, double* host_vel, void* stream);

/* ---- batched thermodynamic integration to an Einstein crystal (csrc/m3g_ti.hip) ---------------------------------------------------------
 * Anharmonic Helmholtz free energies by Frenkel-Ladd integration, at fixed coupling or by non-equilibrium switching (Freitas, Asta,
 * de Koning, Comput. Mater. Sci. 112, 333 (2016)).  A fifth family beside m3g_dyn_*, m3g_nhc_*, m3g_mtk_* and m3g_pimd_*: their
 * structs, state layouts and results do not change.  Units, kappa, k_B and the flag bits are those of m3g_dyn_*.  Every structure
 * moves under H(lambda) = KE + lambda E_model(x) + (1 - lambda) U_s(x), U_s = 1/2 sum_i k_i |x_i - r0_i|^2 (k_i in eV/A^2 per atom,
 * r0 the reference sites), by BAOAB Langevin dynamics whose centre of mass is held exactly: with u_i = x_i - r0_i and G_i = lambda F_i
 * - (1 - lambda) k_i u_i the force on atom i is G_i - (m_i / M) sum_j G_j, and the O step is v_i <- c1 v_i + sigma_i xi_i - pbar / M,
 * c1 = exp(-friction dt), sigma_i = sqrt((1 - c1^2) k_B T kappa / m_i), pbar = sum_j m_j sigma_j xi_j (xi: Philox4x64-10 under key
 * (seed, 4), counter (step, atom of the structure, 0, 0), the Box-Muller of m3g_dyn_*).  friction = 0 is velocity Verlet on the
 * constrained force.  A structure follows its path (lambda_b, lambda_e, n_switch, n_discard) by its step index c: lambda = lambda_b +
 * (lambda_e - lambda_b) g(min(c, n_switch) / n_switch) (lambda_b when n_switch = 0), g(t) = t (LINEAR) or t^5 (70 t^4 - 315 t^3 +
 * 540 t^2 - 420 t + 126) (SMOOTH).  One m3g_ti_step at the forces and energies of x_k closes the step under way with B(h), h = dt / 2,
 * forms D = dH/dlambda = E - U_s, adds (lambda - lambda_prev) (D + D_prev) / 2 to the work W (not on the first call of a path), puts D
 * into Welford's count / mean / M2 and |u_i|^2 into per-atom sums when c >= n_discard, writes obs[s] = {KE, T = 2 KE / ((3 n - 3) k_B),
 * U_s, D, lambda, W, 0, 0} and (not with finish_only) starts the next step with B(h) A(h) O(dt) A(h) and c += 1.  A non-finite force or
 * energy flags the structure M3G_DYN_ERROR and leaves it untouched from then on.  No atomics: every result is bitwise the same alone
 * or in any batch.  The calls remove no centre-of-mass velocity or displacement: the caller starts from sum m_i v_i = 0. */
typedef struct {
  int32_t schedule;   /* M3G_TI_LINEAR, M3G_TI_SMOOTH */
  int32_t reserved;   /* 0 */
  double dt;          /* fs, > 0 */
  double friction;    /* 1/fs, >= 0 */
} m3g_ti_params;
#define M3G_TI_LINEAR 0
#define M3G_TI_SMOOTH 1
#define M3G_TI_OBS 8      /* columns of an obs row */
/* The state buffer is caller-owned device memory, one carve: the chunk table, chunk partials, per atom the mass, velocity, reference
 * site, spring constant and sum of |u|^2, per structure the temperature, total mass, seed, flags, step count, path, work and
 * accumulators.  Bad sizes (as m3g_dyn_state_bytes, or fewer than two atoms per structure) -> M3G_ERR_VALUE. */
int m3g_ti_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes);
/* Byte offsets of the masses [N] and the velocities [N,3] (fp64) inside a state buffer of these sizes, as m3g_dyn_state_view. */
int m3g_ti_state_view(int64_t n_atoms, int64_t n_structs, size_t* mass_offset, size_t* velocity_offset);
/* host_offsets [S+1], host_masses [N], host_springs [N] (eV/A^2), host_temperatures [S] (K), host_seeds [S]: HOST.  vel, reference
 * [N,3] DEVICE fp64, both copied.  The path starts as lambda = 1 throughout (n_switch = n_discard = 0).  Validated on the host before
 * any HIP call, with the reason in m3g_last_error: an unknown schedule, dt not finite and > 0, friction not finite and >= 0, a
 * temperature not finite and > 0, a bad mass, a spring constant not finite and >= 0 or all of a structure's zero, bad offsets, a
 * structure of fewer than two atoms (the held centre of mass leaves 3 n - 3 degrees of freedom) -> M3G_ERR_VALUE; a short state
 * buffer -> M3G_ERR_SIZE.  Waits for the stream. */
int m3g_ti_init(const m3g_ti_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                const double* host_springs, const double* host_temperatures, const uint64_t* host_seeds, const double* vel,
                const double* reference, void* state, size_t state_bytes, void* stream);
/* A new path for every structure that has not failed: host_lambda_begin, host_lambda_end [S] HOST, each in [0, 1] (equal: fixed
 * coupling), n_switch, n_discard >= 0, else M3G_ERR_VALUE.  Sets c = 0, W = 0 and clears the accumulators and the per-atom sums; a
 * step under way is finished by the next m3g_ti_step at the new path's lambda.  Waits for the stream. */
int m3g_ti_path(int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const double* host_lambda_begin,
                const double* host_lambda_end, int64_t n_switch, int64_t n_discard, void* stream);
/* One call per force evaluation: forces [N,3] and energies [S] f32 DEVICE evaluated at pos [N,3] fp64 DEVICE (unwrapped, moved IN
 * PLACE); obs [S, M3G_TI_OBS] fp64 DEVICE or NULL.  params: those of m3g_ti_init.  Three launches whatever S and N, no allocation,
 * copy, wait or atomics: capture-safe.  Missing forces, energies or pos -> M3G_ERR_VALUE. */
int m3g_ti_step(const m3g_ti_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                const float* energies, double* pos, int32_t finish_only, double* obs, void* stream);
/* Flags, step counts, work, Welford count / mean / M2 of D [S], the velocities [N,3] and the per-atom sums of |u|^2 [N] (over the
 * `count` samples) to HOST memory; every output may be NULL.  Waits for the stream. */
int m3g_ti_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int64_t* host_steps,
                double* host_work, int64_t* host_count, double* host_mean, double* host_m2, double* host_vel, double* host_msd_sum,
                void* stream);

/* ---- batched replica-exchange MD (parallel tempering) over an m3g_dyn_* batch (csrc/m3g_remd.hip) -----------------------------------
 * The S structures of an NVT_LANGEVIN batch are cut into G ladders by ladder_offsets [G+1] (0 = o_0 < ... < o_G = S): ladder g is the
 * contiguous run of R_g = o_{g+1} - o_g >= 2 replicas of one system, with strictly ascending temperatures T_g[0..R_g) > 0 and one
 * 64-bit seed; replica o_g + k starts holding temperature index k (the caller gives m3g_dyn_init the same temperatures).  An exchange
 * swaps TEMPERATURES, not configurations: positions never move between rows, so neighbour lists stay valid.
 * One m3g_remd_exchange is attempt a = 0, 1, ... of every ladder (the count lives on the device), at the energies E [S]:
 *   1. E of every replica without M3G_DYN_ERROR whose E is finite joins count / mean / M2 (Welford, fp64) of the index it holds,
 *      before any swap;
 *   2. the pairs (k, k+1) with k % 2 == a % 2: i holds k, j holds k+1, Delta = (1/(k_B T_k) - 1/(k_B T_{k+1})) (E_i - E_j) in fp64 (k_B
 *      of m3g_dyn_*); accepted iff Delta >= 0 or u < exp(Delta), u = ((w_0 >> 11) + 0.5) 2^-53 of Philox4x64-10 with counter (a, k, 0, 0)
 *      and key (ladder seed, 1) -- the Langevin draws use key word 0;
 *   3. a pair with M3G_DYN_ERROR or M3G_DYN_STARTED on either replica, or a non-finite energy, is NOT attempted: not counted, nothing
 *      of it written.  STARTED means half-step velocities: make the call after a finish_only m3g_dyn_step;
 *   4. on accept the held indices and the holder map are swapped, the new targets are written into the dyn state's target
 *      temperatures (read by the next m3g_dyn_step), and the velocities are scaled by sqrt(T_new / T_old); every other replica's
 *      velocities stay bitwise untouched;
 *   5. round trips: a replica that reaches index R-1 after last touching index 0, and then reaches 0 again, has completed one;
 *   6. row a of `history` (the held index of every replica) is written if a < history_rows; the attempt counter becomes a + 1.
 * No atomics: a ladder's results depend on its own replicas only, bitwise the same alone or beside any other ladders.
 * Per-(ladder, index) and per-pair arrays are [S]: row o_g + k is index k (pair (k, k+1)) of ladder g; the row o_g + R_g - 1 of a pair
 * array is unused. */
int m3g_remd_state_bytes(int64_t n_structs, int64_t n_ladders, size_t* bytes);
/* host_ladder_offsets [G+1] int64, host_temperatures [S] (K; replica order, ladder after ladder), host_seeds [G]: HOST.  Null pointers,
 * offsets that do not run from 0 to S or do not increase strictly, a ladder of fewer than 2 replicas, a temperature that is not
 * finite, <= 0 or not strictly ascending within its ladder -> M3G_ERR_VALUE, a short buffer -> M3G_ERR_SIZE, before any HIP call.
 * Waits for the stream. */
int m3g_remd_init(int64_t n_structs, int64_t n_ladders, const int64_t* host_ladder_offsets, const double* host_temperatures,
                  const uint64_t* host_seeds, void* state, size_t state_bytes, void* stream);
/* remd_state: of m3g_remd_init; dyn_state: of m3g_dyn_init over the same S structures (N atoms); energies [S] f32 DEVICE; history
 * [history_rows, S] int32 DEVICE or NULL.  TWO launches whatever S and G, no atomics, no allocation, copy or wait: capture-safe. */
int m3g_remd_exchange(int64_t n_atoms, int64_t n_structs, int64_t n_ladders, void* remd_state, size_t remd_bytes, void* dyn_state,
                      size_t dyn_bytes, const float* energies, int32_t* history, int64_t history_rows, void* stream);
/* To HOST memory, every output may be NULL: held index of every replica and the replica holding every index (int32 [S], replica
 * numbers of the batch), attempts / accepts of every pair (int64 [S]), count (int64), mean and M2 (fp64) of the energy at every index
 * [S], round trips of every replica (int64 [S]) and the attempt counters (int64 [G]).  Waits for the stream. */
int m3g_remd_read(int64_t n_structs, int64_t n_ladders, const void* state, size_t state_bytes, int32_t* host_held, int32_t* host_holder,
                  int64_t* host_attempts, int64_t* host_accepts, int64_t* host_count, double* host_mean, double* host_m2,
                  int64_t* host_round_trips, int64_t* host_counters, void* stream);
/* Byte offset, inside an m3g_dyn_* state buffer of these sizes, of the target temperatures [S] (fp64) the exchange writes. */
int m3g_remd_target_view(int64_t n_atoms, int64_t n_structs, size_t* temperature_offset);

/* ---- batched canonical atom-swap Monte Carlo, alone or interleaved with m3g_dyn_* MD (csrc/m3g_mc.hip) -------------------------------
 * A batch of S structures with N atoms in all (offsets [S+1] as m3g_fire_init), each with a temperature T_s > 0 (K) and a 64-bit seed.
 * `active` [N] (uint8) marks the rows that take part, fixed for the run (only the cation sublattice, say).  Rows are SITES: a trial
 * exchanges the occupants of two rows of one structure -- two entries of atom_types and, with a dynamics state, their masses and
 * velocities (the atoms trade places and each keeps its own velocity, so the kinetic energy is unchanged and the acceptance needs
 * the potential energy only).  Positions never move: neighbour and triplet lists stay valid, and the multiset of species is
 * preserved, so a range check of atom_types made once stays true.
 * Draws: structure s keeps a proposal counter a_s = 0, 1, ... on the device; proposal a_s draws Philox4x64-10 with counter
 * (a_s, 0, 0, 0) and key (seed_s, 2) -- key word 0 is the Langevin noise, word 1 replica exchange; u_k = ((w_k >> 11) + 0.5) 2^-53.
 * m3g_mc_propose, per structure: n_p = its active rows; row i = the active row of rank min((int64)(u_0 n_p), n_p - 1) in row order;
 *   m = the active rows whose species differs from that of i; row j = the one of rank min((int64)(u_1 m), m - 1) among those.  The
 *   pair is drawn with probability (1/n_p) [1/(n_p - n_s(i)) + 1/(n_p - n_s(j))], which the swap leaves unchanged: the proposal is
 *   symmetric for unequal compositions too.  The occupants of i and j are exchanged in place, (i, j) and u_2 of the SAME Philox
 *   output are recorded, M3G_MC_PENDING is set.  a_s advances for every structure at every call, attempted or not, so a structure's
 *   stream depends on its own history only; a_s - 1 is also the index of the call.
 *   A structure is NOT attempted, nothing of it written but a_s (and the flag named), when it is already PENDING (sets the sticky
 *   M3G_MC_ERR_ORDER), when a dynamics state is given and it has M3G_DYN_ERROR or M3G_DYN_STARTED (half-step velocities: call after a
 *   finish_only m3g_dyn_step), when its current energy is not finite, or when its active rows hold fewer than two species (sets
 *   M3G_MC_NO_PAIR; the init call sets it for fewer than two active rows).
 * m3g_mc_decide, per PENDING structure, at the trial energies E' [S] (the engine's output for the swapped species) and the current
 *   energies E [S] (caller-owned, updated in place): dE = (double)E' - (double)E; a non-finite E' is rejected explicitly (-inf too)
 *   and counted in `nonfinite`; otherwise accepted iff dE <= 0 or u_2 < exp(-dE / (k_B T_s)), k_B of m3g_dyn_*.  Reject: rows i, j
 *   are exchanged back -- species, masses and velocities bitwise what they were.  Accept: E[s] = E'[s], and the structure's rows of
 *   the current forces [N,3] / stresses [S,6], when given, are overwritten with the trial ones (a rejected structure's stay bitwise
 *   untouched).  Then attempts, accepts and count / mean / M2 (Welford, fp64) of the current energy after the verdict are updated
 *   and PENDING is cleared.  Row a of history [rows, S, 3] (int32), a the index of the last propose call, gets (i - o_s, j - o_s,
 *   1 | 0), or (-1, -1, -1) for a structure that call did not attempt, if a < rows; a second decide without a new proposal changes
 *   nothing.
 * No atomics: a structure's results are bitwise the same alone or in any batch. */
#define M3G_MC_NO_PAIR 1     /* fewer than two active rows, or fewer than two species on them: never attempted */
#define M3G_MC_PENDING 2     /* proposed, not yet decided: atom_types (masses, velocities) hold the trial configuration */
#define M3G_MC_ERR_ORDER 4   /* sticky: a proposal was asked for while one was pending */
int m3g_mc_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes);
/* host_offsets [S+1] int64, host_temperatures [S] (K), host_seeds [S], host_active [N] uint8: HOST.  Null pointers, bad offsets, a
 * temperature that is not finite and > 0 -> M3G_ERR_VALUE, a short buffer -> M3G_ERR_SIZE, before any HIP call.  Waits for the
 * stream. */
int m3g_mc_init(int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_temperatures, const uint64_t* host_seeds,
                const uint8_t* host_active, void* state, size_t state_bytes, void* stream);
/* atom_types [N] int64 DEVICE (the array the engine reads), exchanged in place; dyn_state: of m3g_dyn_init over the same batch, or
 * NULL (pure lattice Monte Carlo); energies [S] f32 DEVICE: the current ones.  ONE launch whatever S, no allocation, copy or wait:
 * capture-safe. */
int m3g_mc_propose(int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, int64_t* atom_types, void* dyn_state, size_t dyn_bytes,
                   const float* energies, void* stream);
/* trial_energies [S], trial_forces [N,3], trial_stresses [S,6] (f32 DEVICE): the evaluation of the trial; energies, forces, stresses:
 * the current ones, updated in place.  forces and stresses are optional, each given together with its trial partner (else
 * M3G_ERR_VALUE); history [history_rows, S, 3] int32 DEVICE or NULL.  TWO launches (the verdict with the revert, the row copy over the
 * chunk table), ONE when forces and stresses are NULL; no allocation, copy or wait: capture-safe. */
int m3g_mc_decide(int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, int64_t* atom_types, void* dyn_state, size_t dyn_bytes,
                  const float* trial_energies, const float* trial_forces, const float* trial_stresses, float* energies, float* forces,
                  float* stresses, int32_t* history, int64_t history_rows, void* stream);
/* To HOST memory, every output may be NULL: flags (M3G_MC_*, int32), proposal counters, attempts, accepts, non-finite trials, count
 * (int64), mean and M2 (fp64) of the current energy [S], and the last attempted pair [S,2] (int32, rows relative to the structure).
 * Waits for the stream. */
int m3g_mc_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int64_t* host_counters,
                int64_t* host_attempts, int64_t* host_accepts, int64_t* host_nonfinite, int64_t* host_count, double* host_mean, double* host_m2,
                int32_t* host_pairs, void* stream);

/* ---- batched reverse non-equilibrium MD over an m3g_dyn_* batch: imposed heat or momentum flux (csrc/m3g_rnemd.hip) -----------------
 * Mueller-Plathe's method (J. Chem. Phys. 106, 6082 (1997); Phys. Rev. E 59, 4894 (1999)) with the unequal-mass exchange of
 * Nieto-Draghi and Avalos (Mol. Phys. 101, 2303 (2003)).  A batch of S structures with N atoms in all (offsets [S+1] as m3g_dyn_init),
 * each cut into n_slabs slabs along lattice direction `axis`.  The calls act on the m3g_dyn_* state of the same batch at a synchronous
 * point, after a finish_only m3g_dyn_step, as m3g_remd_exchange does.
 * Slab of a row: g_s = column `axis` of the inverse lattice (rows = lattice vectors), computed by m3g_rnemd_init on the host in fp64;
 *   on the device f = (x g0 + y g1) + z g2, f -= floor(f), slab = min((int)(f n_slabs), n_slabs - 1): a wrapped f of exactly 1.0 lands
 *   in the last slab.  No product is contracted with a sum anywhere in this family.  Slab 0 is the cold (sink) slab, slab n_slabs / 2
 *   the hot (source) slab.
 * Selection: the candidates of a slab are its rows with active != 0 and a finite key.  kind HEAT: key = m ((vx vx + vy vy) + vz vz);
 *   MOMENTUM: key = v[flow_axis].  Slab 0 is ordered by (key descending, row ascending), slab n_slabs / 2 by (key ascending, row
 *   ascending).  Pair p = 0 .. n_swaps - 1 takes the p-th entry of each list while both lists hold one, and is exchanged iff
 *   key0 > keyMid strictly.
 * Exchange of rows i (slab 0) and j: with mi == mj bitwise the velocity vectors (HEAT) or their flow_axis components (MOMENTUM) trade
 *   places; else vcm = (mi vi + mj vj) / (mi + mj), vi' = 2 vcm - vi, vj' = 2 vcm - vj on those components.  Both conserve sum m v and
 *   sum m |v|^2 exactly in real arithmetic.  `transferred` gains 0.5 mi (|vi|^2 - |vi'|^2) / kappa (HEAT, eV; |v|^2 = (vx vx + vy vy) +
 *   vz vz, kappa of m3g_dyn_*) or mi (vi - vi') (MOMENTUM, amu A/fs), pairs in the order p = 0, 1, ...
 * Sampling (do_sample): per slab the number of rows and the sums of m, m vx, m vy, m vz, m ((vx vx + vy vy) + vz vz) over ALL its rows
 *   (inactive ones too), from the velocities BEFORE the exchange of the same call: per run of 64 consecutive rows of the
 *   structure in row order from zero, the four runs of a chunk of 256 rows in row order from zero, the chunks' partials in chunk
 *   order from zero, and that total added to the accumulator.
 * A structure whose dyn flags carry M3G_DYN_ERROR or M3G_DYN_STARTED is left bitwise untouched: not exchanged, not sampled, none of
 *   its counters advanced.  Otherwise n_calls advances at every call that swaps or samples, n_samples at every sampling one, and
 *   last_pairs is rewritten by every swapping one.
 * No atomics: every result of a structure depends on its own rows only, bitwise the same alone or in any batch. */
typedef struct { int32_t kind, axis, flow_axis, n_slabs, n_swaps, reserved; } m3g_rnemd_params;   /* 24 bytes */
#define M3G_RNEMD_HEAT 0
#define M3G_RNEMD_MOMENTUM 1
#define M3G_RNEMD_MAX_SWAPS 8
#define M3G_RNEMD_MAX_SLABS 64
/* Null `bytes`, bad sizes, n_slabs odd, < 2 or > M3G_RNEMD_MAX_SLABS -> M3G_ERR_VALUE. */
int m3g_rnemd_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t n_slabs, size_t* bytes);
/* host_offsets [S+1] int64, host_lattices [S,3,3] fp64 (rows = lattice vectors), host_active [N] uint8 or NULL (every row takes part):
 * HOST.  Null pointers, bad sizes or offsets, an unknown kind, axis or flow_axis outside 0 .. 2, MOMENTUM with flow_axis == axis,
 * n_slabs odd, < 2 or > 64, n_swaps < 1 or > 8, a singular or non-finite lattice -> M3G_ERR_VALUE, a short buffer -> M3G_ERR_SIZE,
 * before any HIP call.  Waits for the stream. */
int m3g_rnemd_init(const m3g_rnemd_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets,
                   const double* host_lattices, const uint8_t* host_active, void* state, size_t state_bytes, void* stream);
/* state: of m3g_rnemd_init; dyn_state: of m3g_dyn_init over the same batch; pos [N,3] fp64 DEVICE, unwrapped (the integrator's own);
 * params: those of m3g_rnemd_init (n_swaps may differ from call to call).  do_swap / do_sample: exchange, accumulate the profile, or
 * both (neither: nothing is launched).  TWO launches whatever N, S, n_slabs and n_swaps, no atomics, no allocation, copy or wait:
 * capture-safe. */
int m3g_rnemd_exchange(const m3g_rnemd_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes,
                       void* dyn_state, size_t dyn_bytes, const double* pos, int32_t do_swap, int32_t do_sample, void* stream);
/* To HOST memory, every output may be NULL: n_calls, n_exchanged (int64 [S]), transferred (fp64 [S]), n_samples (int64 [S]),
 * last_pairs [S, n_swaps, 2] (int32: the rows, relative to the structure, exchanged by the last swapping call at params->n_swaps,
 * slab-0 row first, -1 where pair p was not exchanged), slab count [S, n_slabs] (int64) and sums [S, n_slabs, 5] (fp64).  Waits for
 * the stream. */
int m3g_rnemd_read(const m3g_rnemd_params* params, int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes,
                   int64_t* host_n_calls, int64_t* host_n_exchanged, double* host_transferred, int64_t* host_n_samples,
                   int32_t* host_last_pairs, int64_t* host_count, double* host_sums, void* stream);

/* ---- batched collective-variable biasing: metadynamics, restraints and walls (csrc/m3g_meta.hip) -----------------------------------
 * A bias layer over any MD family: one m3g_meta_bias takes the integrator's unwrapped pos [N,3] (fp64) and the engine's forces [N,3]
 * (f32) and writes forces_out [N,3] (f32, may be `forces` itself), which goes to m3g_dyn_step / m3g_nhc_step unchanged.  The S
 * structures (offsets [S+1] as m3g_dyn_init) are cut into G walker groups by group_offsets [G+1] (structure indices, 0 .. S, strictly
 * increasing; a group of one walker is legal); the walkers of a group share one hill list of at most max_hills hills.
 * Collective variables: n_cv = 1 .. M3G_META_MAX_CV per call, one set for the whole batch.  membership [n_cv, N] uint8: 0 none, 1 = A,
 *   2 = B, 3 = both; weights [N] fp64 >= 0 (the masses, usually); c_X = sum_X w x / sum_X w over UNWRAPPED positions, no minimum image.
 *   M3G_CV_DISTANCE      s = |c_A - c_B|; at distance 0 the gradient is zero.
 *   M3G_CV_PROJECTION    s = (c_A - c_B - origin_s) . direction, direction a unit vector (|n|^2 within 1e-12 of 1), origin [3] per
 *                        structure and CV; an empty B means c_B = 0.
 *   M3G_CV_COORDINATION  s = sum_{i in A} sum_{j in B, j != i} f(r_ij), sigma(r) = 1 / (1 + (r^2 / r0^2)^power), power = 1 .. 6 by
 *                        repeated multiplication, f = (sigma(r) - sigma(r_cut)) / (1 - sigma(r_cut)) for r < r_cut and 0 from r_cut
 *                        on.  r_ij under the minimum image of the FIXED cell given at init (rint of the fractional difference,
 *                        fp64: exact below half the smallest perpendicular width of the cell, which r_cut must not exceed).
 *                        O(|A| |B|) per call.  NVE / NVT only: the cells never change.
 * Bias of structure s: V = V_hills + sum_k [ kappa_sk / 2 (s_k - centre_sk)^2 + walls ], walls [S, n_cv, 4] = (lower, kappa_lower,
 *   upper, kappa_upper): kappa_lower / 2 (s - lower)^2 where s < lower, kappa_upper / 2 (s - upper)^2 where s > upper; a kappa of 0
 *   switches its term off.  V_hills(s) = sum_h w_h exp(-1/2 sum_k (s_k - c_hk)^2 / sigma_gk^2) over the hills of the structure's group.
 * Deposits (calls with deposit != 0): every walker appends a hill at its own s of height height_g exp(-V_hills(s) inv_kdt_g) --
 *   inv_kdt = 1 / (kB DeltaT): well-tempered; 0: plain metadynamics -- with V_hills over the list as it stood BEFORE the call, as are
 *   the forces and the obs row of that call.  Walker r of a group of R writes slot c R + r, c the deposits it has made.  A group whose
 *   list cannot take R more hills sets the sticky M3G_META_FULL on its walkers, deposits nothing and goes on.
 * A walker with a non-finite CV (or a non-finite position in any of its groups' rows) gets M3G_META_ERROR (sticky), no bias force
 *   in that call -- forces_out = forces -- an obs row of its CVs and zeros, and on a deposit appends a hill of height 0 at centre 0.
 * obs [S, M3G_META_OBS] fp64 or NULL: s_0, s_1, V, V_hills, V_restraints + walls, dV/ds_0, dV/ds_1, the height deposited (0: none).
 * All arithmetic is fp64, no product is contracted with a sum; the only f32 operation is forces_out = (float)(forces - sum_k dV/ds_k
 *   ds_k/dx).  Rows that belong to no group of any CV pass through bitwise.  Sums: rows over a chunk of 256 in a fixed tree, chunks
 *   lane-strided over 64 lanes in chunk order, then a butterfly; COORDINATION rows walk their partners in row order; hills
 *   lane-strided in list order, then the butterfly.  No atomics: a group's results are bitwise the same alone or in any batch. */
#define M3G_META_MAX_CV 2
#define M3G_META_OBS 8
#define M3G_CV_DISTANCE 0
#define M3G_CV_PROJECTION 1
#define M3G_CV_COORDINATION 2
#define M3G_META_ERROR 1
#define M3G_META_FULL 2
typedef struct {
  int32_t n_cv, reserved;
  int64_t max_hills;                       /* per group, as given to m3g_meta_state_bytes */
  int32_t kind[M3G_META_MAX_CV];           /* M3G_CV_* */
  int32_t power[M3G_META_MAX_CV];          /* COORDINATION */
  double r0[M3G_META_MAX_CV], r_cut[M3G_META_MAX_CV];   /* COORDINATION */
  double direction[M3G_META_MAX_CV][3];    /* PROJECTION */
} m3g_meta_params;                         /* 112 bytes */
/* Null `bytes`, bad sizes (1 <= n_groups <= n_structs <= n_atoms), n_cv outside 1 .. 2, max_hills < 0 -> M3G_ERR_VALUE. */
int m3g_meta_state_bytes(int64_t n_atoms, int64_t n_structs, int64_t n_groups, int32_t n_cv, int64_t max_hills, size_t* bytes);
/* The byte offset, within the state, of the COORDINATION gradients [n_cv, N, 3] fp64 (d s_k / d x_i as the last m3g_meta_bias left
 * them; only the rows with membership != 0 of a COORDINATION CV are ever written). */
int m3g_meta_state_view(int64_t n_atoms, int64_t n_structs, int64_t n_groups, int32_t n_cv, int64_t max_hills, size_t* gradient_offset);
/* All arrays HOST: offsets [S+1], group_offsets [G+1] int64; lattices [S,3,3] fp64 (rows = lattice vectors); membership [n_cv,N] uint8;
 * weights [N]; origins [S,n_cv,3], centres [S,n_cv], kappas [S,n_cv], walls [S,n_cv,4] (each may be NULL: zeros); sigmas [G,n_cv],
 * heights [G], inv_kdt [G].  Validated before any HIP call, the reason in m3g_last_error: null pointers, bad sizes, offsets or
 * lattices, an unknown kind, n_cv outside 1 .. 2, a direction that is no unit vector, power outside 1 .. 6, r0 or r_cut not finite
 * and > 0, r_cut above half the smallest perpendicular width of any cell, membership > 3, an empty group A (B too for DISTANCE and
 * COORDINATION) in any structure, a weight that is negative or a group of a centre CV whose total weight is not > 0, sigma <= 0, a
 * negative kappa, height or inv_kdt, a restraint or wall that is on without a finite position -> M3G_ERR_VALUE; a short buffer ->
 * M3G_ERR_SIZE.  The hill lists start empty.  Waits for the stream. */
int m3g_meta_init(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, const int64_t* host_offsets,
                  const int64_t* host_group_offsets, const double* host_lattices, const uint8_t* host_membership, const double* host_weights,
                  const double* host_origins, const double* host_centres, const double* host_kappas, const double* host_walls,
                  const double* host_sigmas, const double* host_heights, const double* host_inv_kdt, void* state, size_t state_bytes,
                  void* stream);
/* params: those of m3g_meta_init.  pos, forces, forces_out, obs: DEVICE.  THREE launches whatever N, S, G and the number of hills, no
 * atomics, no allocation, copy or wait: capture-safe. */
int m3g_meta_bias(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, void* state, size_t state_bytes,
                  const double* pos, const float* forces, float* forces_out, int32_t deposit, double* obs, void* stream);
/* Replaces the hill lists (a restart): HOST group_offsets [G+1] (those of init), counts [G] (each a multiple of the group's walkers,
 * <= max_hills), centres [G, max_hills, n_cv], heights [G, max_hills] (finite below the count).  Waits for the stream. */
int m3g_meta_set_hills(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, void* state, size_t state_bytes,
                       const int64_t* host_group_offsets, const int64_t* host_counts, const double* host_centres, const double* host_heights,
                       void* stream);
/* To HOST memory, every output may be NULL: flags [S] (int32, M3G_META_*), deposits made [S] and hill counts [G] (int64), centres
 * [G, max_hills, n_cv] and heights [G, max_hills] (fp64; beyond the count zeros, or what m3g_meta_set_hills was given).  Waits for the stream. */
int m3g_meta_read(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, const void* state, size_t state_bytes,
                  int32_t* host_flags, int64_t* host_deposits, int64_t* host_hill_counts, double* host_centres, double* host_heights,
                  void* stream);

/* ---- trajectory observables: RDF, MSD and VACF accumulated on the device (csrc/m3g_trajectory.hip) ---------------------------------
 * Fed one frame per m3g_traj_sample (from the MD loop, or any frames): per structure and species pair (a <= b) the INTEGER histogram
 * of minimum-image pair distances below r_max in rdf_bins bins (unordered pairs i < j; bin = (int)(r rdf_bins / r_max) taken only
 * where r < r_max, so a non-finite distance is counted nowhere), the sum of the cell volumes, and over a ring of the last n_lags
 * sampled frames the sums, per species a and lag l, of |r_i(now) - r_i(now - l)|^2 and v_i(now) . v_i(now - l) over the atoms of
 * species a, with the number of samples that contributed to lag l.  Division by atom counts and by lag_count is the caller's.
 * The minimum image comes from rounding the fractional difference (fp64): exact for every pair closer than half the smallest
 * perpendicular width w_min = V / max |a_j x a_k| of the cell; a sample taken with r_max > w_min / 2 in the CURRENT cell of a
 * structure sets M3G_TRAJ_RDF_RANGE in its flags (compared with a relative slack of 1e-12, for the rounding of w_min itself).
 * With remove_com the mass-weighted centre-of-mass position and velocity of the atom's own structure are subtracted from every
 * stored frame.  Velocities: with `forces` the sampler stores v + kick kappa F / m
 * (the finish kick of m3g_dyn_step: give the state's velocities -- m3g_dyn_state_view -- and the forces BEFORE the m3g_dyn_step
 * call of the same positions, with kick = dt / 2, or 0 before the first step); without forces, `vel` as given.
 * No float atomics: integer counts, fixed-order sums; every number is bitwise the same alone or in any batch. */
typedef struct {
  int64_t n_atoms;       /* N */
  int64_t n_structs;     /* S */
  int32_t max_species;   /* 1 .. 8: species indices are local, 0 .. max_species - 1 */
  int32_t rdf_bins;      /* 0 (no RDF) .. 4096 */
  int32_t n_lags;        /* 0 (no correlations) .. 4096: ring of n_lags frames, n_lags * N * 48 bytes */
} m3g_traj_sizes;
typedef struct {
  double r_max;          /* A, finite and > 0 when rdf_bins > 0 */
  int32_t remove_com;    /* 0 / 1 */
} m3g_traj_params;
#define M3G_TRAJ_RDF_RANGE 1   /* a sample saw r_max above half the smallest perpendicular width of the structure's cell */
/* Sizes outside their limits, or rdf_bins == n_lags == 0 -> M3G_ERR_VALUE.  The size follows from `sizes` alone (no offsets), so the
 * table of tile pairs (24 B each) and the grid of the RDF launch take the most pairs any batch of these sizes can have: t (t + 1) / 2
 * + S - 1 with t = ceil(N / 256) + 1, reached when one structure holds nearly every atom.  Batches of many small structures launch
 * workgroups that return at once; one structure of 10^6 atoms has 7.6e6 pairs, 183 MB of table (beside a ring of 48 MB per lag). */
int m3g_traj_state_bytes(const m3g_traj_sizes* sizes, size_t* bytes);
/* HOST host_offsets [S+1] (int64, as m3g_dyn_init), host_species [N] (int32, 0 .. max_species - 1), host_masses [N] (amu, > 0).
 * Uploads the tables (the chunk table and the table of 256-atom tile pairs the RDF launch runs over) and zeroes the accumulators.
 * Everything is checked on the host before any HIP call -> M3G_ERR_VALUE; a short state buffer -> M3G_ERR_SIZE.  Waits for the
 * stream. */
int m3g_traj_init(const m3g_traj_sizes* sizes, const m3g_traj_params* params, const int64_t* host_offsets, const int32_t* host_species,
                  const double* host_masses, void* state, size_t state_bytes, void* stream);
/* One sample: pos [N,3] fp64, lattice [S,3,3] fp64 (may be NULL when rdf_bins == 0), vel [N,3] fp64 (may be NULL when n_lags == 0),
 * forces [N,3] f32 or NULL, all DEVICE.  One launch for the RDF and three (four with remove_com) for the correlations, whatever S;
 * the ring position and the sample counts live in the state buffer: no allocation, copy or wait, capture-safe. */
int m3g_traj_sample(const m3g_traj_sizes* sizes, const m3g_traj_params* params, void* state, size_t state_bytes, const double* pos,
                    const double* lattice, const double* vel, const float* forces, double kick, void* stream);
/* The accumulators to HOST memory; every output may be NULL: hist [S, P, rdf_bins] uint64 with P = max_species (max_species + 1) / 2,
 * pair (a <= b) in row-major upper-triangle order; msd, vacf [S, max_species, n_lags] fp64; lag_count [S, n_lags] int64; n_samples [S]
 * int64; volume_sum [S] fp64; flags [S] int32 (M3G_TRAJ_*).  Waits for the stream. */
int m3g_traj_read(const m3g_traj_sizes* sizes, const void* state, size_t state_bytes, uint64_t* host_hist, double* host_msd,
                  double* host_vacf, int64_t* host_lag_count, int64_t* host_n_samples, double* host_volume_sum, int32_t* host_flags,
                  void* stream);
/* The stored frame `lag` samples back (0: the last sample; < n_lags and < the samples taken, else M3G_ERR_VALUE) to HOST memory:
 * host_pos, host_vel [N,3] fp64 -- what the correlations are formed from: the full-step velocities, centre of mass removed where
 * asked for.  Waits for the stream. */
int m3g_traj_frame(const m3g_traj_sizes* sizes, const void* state, size_t state_bytes, int32_t lag, double* host_pos, double* host_vel,
                   void* stream);

/* ---- scattering observables: S(q), F(q,t) and current correlations accumulated on the device (csrc/m3g_scattering.hip) ----------------
 * The reciprocal-space companion of the trajectory observables above, fed one frame per m3g_sq_sample.  Structure s has its own list
 * of Q_s integer Miller triples h != 0.  With L the CURRENT cell (rows = lattice vectors), q = 2 pi h L^-T, so that q . r = 2 pi h . f
 * with f = r L^-1: every h is commensurate with every cell, so a moving cell (NPT) needs no special case.  Per species a (local
 * indices as in m3g_traj_*):
 *   rho_a(q) = sum_{j in a} exp(-i q . r_j)        j_a(q) = sum_{j in a} v_j exp(-i q . r_j)
 *   j_L = qhat . j                                 j_T = j - qhat j_L            (qhat from the cell current at that sample)
 * v is `vel` as given, or with `forces` vel + kick kappa F / m, the completion of m3g_traj_sample.  With remove_com positions and
 * velocities are relative to the structure's mass-weighted centre of mass: under Langevin dynamics the centre of mass diffuses,
 * and a displacement d of it multiplies rho(q, t) by exp(-i q . d), a spurious phase that would decay F(q,t) at a rate that is no
 * property of the material.
 * Phases: positions are the integrator's unwrapped ones; f is reduced to f - rint(f) in fp64 before h . f is formed, h . f is
 * reduced again, and sincospi only ever sees an argument in [-1, 1].
 * Accumulated over a ring of the last n_lags samples, per structure, q, species pair (a <= b, row-major upper triangle as the RDF's
 * histogram rows) and lag l -- sums only, normalisation is the caller's:
 *   F_sum [q,ab,l] += Re[rho_a(t) rho_b*(t-l) + rho_b(t) rho_a*(t-l)] / 2
 *   CL_sum[q,ab,l] += Re[j_L,a(t) j_L,b*(t-l) + j_L,b(t) j_L,a*(t-l)] / 2
 *   CT_sum[q,ab,l] += 1/2 Re[j_T,a(t) . j_T,b*(t-l) + j_T,b(t) . j_T,a*(t-l)] / 2     (the mean over the two transverse directions)
 * with lag_count[s,l] and n_samples[s] per structure.  A sample whose cell is not invertible (|det| < 1e-12 or not finite) sets
 * M3G_SQ_CELL in the structure's flags and takes no part in any sum, now or as the older frame of a later lag; n_samples and
 * lag_count do not count it.  No float atomics, fixed-order sums: every number depends on the structure's own rows only, bitwise
 * the same alone or in any batch. */
typedef struct {
  int64_t n_atoms;       /* N */
  int64_t n_structs;     /* S */
  int64_t n_q;           /* total number of q-vectors over the structures, >= 1 */
  int32_t max_species;   /* 1 .. 4 (M3G_SQ_MAX_SPECIES): species indices are local, 0 .. max_species - 1 */
  int32_t n_lags;        /* 1 .. 4096: ring of n_lags entries of 80 bytes per (q, species) */
} m3g_sq_sizes;
typedef struct {
  int32_t remove_com;    /* 0 / 1 */
  int32_t reserved;      /* 0 */
} m3g_sq_params;
#define M3G_SQ_MAX_INDEX 128     /* |h_k| at most */
#define M3G_SQ_MAX_Q 4096        /* q-vectors of one structure at most */
#define M3G_SQ_MAX_SPECIES 4
#define M3G_SQ_MAX_LAGS 4096
#define M3G_SQ_CELL 1            /* a sample saw a cell that is not invertible: it was left out */
/* Sizes outside their limits -> M3G_ERR_VALUE.  The size follows from `sizes` alone: the per-chunk partial sums are laid out for
 * min(n_q, M3G_SQ_MAX_Q) vectors in every one of the ceil(N / 256) + S chunks a batch of these sizes can have (64 max_species bytes
 * each). */
int m3g_sq_state_bytes(const m3g_sq_sizes* sizes, size_t* bytes);
/* HOST host_offsets [S+1], host_species [N], host_masses [N] as m3g_traj_init; host_q_offsets [S+1] (int64, 0 = o_0 <= o_1 <= ... <=
 * o_S = n_q: a structure without vectors is legal and costs nothing), host_hkl [n_q,3] int32.  Everything is checked on the host
 * before any HIP call -> M3G_ERR_VALUE: h = 0, |h_k| > M3G_SQ_MAX_INDEX, more than M3G_SQ_MAX_Q vectors in one structure, offsets
 * that do not end at n_q; a short state buffer -> M3G_ERR_SIZE.  Uploads the tables, zeroes the accumulators, waits for the stream. */
int m3g_sq_init(const m3g_sq_sizes* sizes, const m3g_sq_params* params, const int64_t* host_offsets, const int32_t* host_species,
                const double* host_masses, const int64_t* host_q_offsets, const int32_t* host_hkl, void* state, size_t state_bytes,
                void* stream);
/* One sample: pos [N,3], lattice [S,3,3], vel [N,3] fp64, forces [N,3] f32 or NULL, all DEVICE.  Three launches (four with
 * remove_com) whatever S, Q, N and n_lags; the ring position lives in the state buffer (the two counters of m3g_traj_sample): no
 * allocation, copy or wait, capture-safe. */
int m3g_sq_sample(const m3g_sq_sizes* sizes, const m3g_sq_params* params, void* state, size_t state_bytes, const double* pos,
                  const double* lattice, const double* vel, const float* forces, double kick, void* stream);
/* The accumulators to HOST memory; every output may be NULL: f, cl, ct [n_q, P, n_lags] fp64 with P = max_species (max_species + 1)
 * / 2; lag_count [S, n_lags] int64; n_samples [S] int64; flags [S] int32 (M3G_SQ_*).  Waits for the stream. */
int m3g_sq_read(const m3g_sq_sizes* sizes, const void* state, size_t state_bytes, double* host_f, double* host_cl, double* host_ct,
                int64_t* host_lag_count, int64_t* host_n_samples, int32_t* host_flags, void* stream);
/* The stored ring entry `lag` samples back (0: the last sample; < n_lags and < the samples taken, else M3G_ERR_VALUE) to HOST
 * memory, complex numbers as (re, im) pairs of fp64: rho, j_L [n_q, max_species], j_T [n_q, max_species, 3]; every output may be
 * NULL.  The first stage (densities and projected currents) on its own.  Waits for the stream. */
int m3g_sq_frame(const m3g_sq_sizes* sizes, const void* state, size_t state_bytes, int32_t lag, double* host_rho, double* host_jl,
                 double* host_jt, void* stream);

/* ---- local-order observables: Steinhardt q_l, their neighbour average, solid-like atoms and clusters (csrc/m3g_local_order.hip) -------
 * The per-atom companion of the two families above, fed one frame per m3g_lo_sample; positions and cells only, no velocities.
 * Neighbours: for structure s with cut-off r_cut[s] (A), atom j != i is a neighbour of i when the minimum-image distance r_ij <
 *   r_cut[s] (strict); all species count.  Minimum image as in the RDF of m3g_traj_*: the fractional difference minus its rint, in
 *   fp64, valid only while r_cut <= half the smallest perpendicular width of the CURRENT cell -- checked per sample on the device with
 *   the allowance 1 + 1e-12 of M3G_TRAJ_RDF_RANGE.  N_b(i) is the neighbour count; the list of an atom holds its first
 *   M3G_LO_MAX_NEIGHBORS neighbours in ascending structure-local index j, the count is kept uncapped.
 * Spherical harmonics Y_lm(rhat) with the Condon-Shortley phase, orthonormal on the sphere; only m = 0 .. l is stored, since
 *   Y_l,-m = (-1)^m Y_lm*.
 * Per atom:  q_lm(i) = (1/N_b) sum_{j in nb(i)} Y_lm(rhat_ij)   (j ascending),
 *            q_l(i)  = sqrt( 4 pi / (2l+1) ( |q_l0|^2 + 2 sum_{m>0} |q_lm|^2 ) );      N_b(i) = 0: q_lm = 0, q_l = 0.
 * Neighbour average (Lechner and Dellago, J. Chem. Phys. 129, 114707 (2008)):
 *            qbar_lm(i) = ( q_lm(i) + sum_{j in nb(i)} q_lm(j) ) / (N_b(i) + 1), j ascending; qbar_l from qbar_lm as q_l from q_lm.
 * Global:    Q_lm = sum_i N_b(i) q_lm(i) / sum_i N_b(i) over the structure, Q_l as above; 0 when the structure has no bond.
 * Solid-like bond (ten Wolde, Ruiz-Montero and Frenkel, J. Chem. Phys. 104, 9932 (1996)), L = solid_degree:
 *            s_ij = Re sum_{m=-L..L} q_Lm(i) q_Lm*(j) / ( |q_L(i)| |q_L(j)| ),  |q_L(i)|^2 = sum_m |q_Lm(i)|^2,  -1 <= s_ij <= 1;
 *            the bond is connected when s_ij > solid_threshold (a zero norm: not connected); n_conn(i) counts the connected bonds of
 *            i, and atom i is solid-like when n_conn(i) >= solid_bonds.
 * Clusters:  two solid-like atoms that are neighbours belong to the same cluster; its label is the smallest structure-local atom
 *            index in it, non-solid atoms carry -1.  Per sample: n_solid, n_clusters, largest_cluster.
 * Accumulated per structure over the samples: per species and degree integer histograms (hist_bins bins on [0, 1], the last bin closed)
 * of q_l and qbar_l and the sums of q_l, q_l^2, qbar_l, qbar_l^2; per species a histogram of N_b (0 .. 32); and for the first
 * series_cap samples a series row (n_solid, n_clusters, largest_cluster; Q_l and the mean of qbar_l over the atoms per degree).
 * A sample of a structure that raises any M3G_LO_* flag takes no part in any histogram, sum or series row of that structure
 * (n_skipped counts it, n_samples the others); the flags are sticky and the per-atom frame is still written as computed.  No float
 * atomics, fixed-order sums: every number depends on the structure's own rows only, bitwise the same alone or in any batch. */
typedef struct {
  int64_t n_atoms;       /* N */
  int64_t n_structs;     /* S */
  int32_t max_species;   /* 1 .. 4 (M3G_LO_MAX_SPECIES): species indices are local, 0 .. max_species - 1 */
  int32_t n_degrees;     /* 1 .. 3 (M3G_LO_MAX_DEGREES) */
  int32_t hist_bins;     /* 1 .. 1024 (M3G_LO_MAX_BINS) */
  int32_t series_cap;    /* 1 .. 65536 (M3G_LO_MAX_SERIES): later samples enter the histograms and sums, not the series */
} m3g_lo_sizes;
#define M3G_LO_MAX_DEGREE 12
#define M3G_LO_MAX_DEGREES 3
#define M3G_LO_MAX_NEIGHBORS 32
#define M3G_LO_MAX_SPECIES 4
#define M3G_LO_MAX_BINS 1024
#define M3G_LO_MAX_SERIES 65536
typedef struct {
  int32_t degrees[M3G_LO_MAX_DEGREES];   /* the first n_degrees: distinct, each 1 .. 12 (M3G_LO_MAX_DEGREE); the others are ignored */
  int32_t solid_degree;                  /* one of them */
  int32_t solid_bonds;                   /* 1 .. 32 */
  double solid_threshold;                /* -1 .. 1 */
} m3g_lo_params;
#define M3G_LO_CELL 1            /* a sample saw a cell that is singular (|det| < 1e-12) or not finite */
#define M3G_LO_RANGE 2           /* r_cut beyond half the smallest perpendicular width of a sample's cell */
#define M3G_LO_NEIGHBORS 4       /* an atom had more than M3G_LO_MAX_NEIGHBORS neighbours */
#define M3G_LO_NONFINITE 8       /* a pair distance was not finite, or 0 */
/* Sizes outside their limits -> M3G_ERR_VALUE.  The size follows from `sizes` alone: 936 + 224 n_degrees bytes per atom for the lists
 * and the frame beside the accumulators. */
int m3g_lo_state_bytes(const m3g_lo_sizes* sizes, size_t* bytes);
/* HOST host_offsets [S+1] and host_species [N] as m3g_traj_init, host_r_cut [S] (A, finite and > 0).  Everything is checked on the
 * host before any HIP call -> M3G_ERR_VALUE; a short state buffer -> M3G_ERR_SIZE.  Uploads the tables (the normalisation of Y_lm
 * among them, computed here in fp64), zeroes the accumulators, waits for the stream. */
int m3g_lo_init(const m3g_lo_sizes* sizes, const m3g_lo_params* params, const int64_t* host_offsets, const int32_t* host_species,
                const double* host_r_cut, void* state, size_t state_bytes, void* stream);
/* One sample: pos [N,3] (unwrapped or not), lattice [S,3,3] fp64, both DEVICE.  Six launches whatever S, N and the species; the
 * counters live in the state buffer (the two counters of m3g_traj_sample): no allocation, copy or wait, capture-safe on one stream. */
int m3g_lo_sample(const m3g_lo_sizes* sizes, const m3g_lo_params* params, void* state, size_t state_bytes, const double* pos,
                  const double* lattice, void* stream);
/* The accumulators to HOST memory; every output may be NULL: hist_q, hist_qbar [S, max_species, n_degrees, hist_bins] uint64;
 * hist_nb [S, max_species, 33] uint64; moments [S, max_species, n_degrees, 4] fp64 (sums of q_l, q_l^2, qbar_l, qbar_l^2);
 * series_counts [S, series_cap, 3] int64 (n_solid, n_clusters, largest_cluster); series_order [S, series_cap, 2, n_degrees] fp64 (Q_l,
 * mean qbar_l); n_samples, n_skipped [S] int64; flags [S] int32 (M3G_LO_*).  Series rows from n_samples on are zero.  Waits. */
int m3g_lo_read(const m3g_lo_sizes* sizes, const void* state, size_t state_bytes, uint64_t* host_hist_q, uint64_t* host_hist_qbar,
                uint64_t* host_hist_nb, double* host_moments, int64_t* host_series_counts, double* host_series_order,
                int64_t* host_n_samples, int64_t* host_n_skipped, int32_t* host_flags, void* stream);
/* The per-atom arrays of the last sample to HOST memory (before any sample: M3G_ERR_VALUE); every output may be NULL: qlm
 * [N, n_degrees, 13, 2] fp64 ((re, im) of m = 0 .. 12, zero beyond l), ql, qbar [N, n_degrees] fp64, n_neighbors (uncapped), n_conn,
 * solid (0 / 1), label [N] int32.  Waits for the stream. */
int m3g_lo_frame(const m3g_lo_sizes* sizes, const void* state, size_t state_bytes, double* host_qlm, double* host_ql, double* host_qbar,
                 int32_t* host_n_neighbors, int32_t* host_n_conn, int32_t* host_solid, int32_t* host_label, void* stream);

/* ---- thermodynamic fluctuation observables and Green-Kubo stress correlations (csrc/m3g_thermo.hip) ---------------------------------
 * The per-structure companion of the three families above, fed one sample per m3g_thermo_sample at the synchronous point of a step:
 * the engine's energies and pair-virial stresses, the cell, and the kinetic part from one of two sources.
 * (a) `vel` (with `forces`: v = vel + kick kappa F / m, the completion of m3g_traj_sample).  Over the rows of structure s, with the
 *     Voigt order c = xx, yy, zz, yz, zx, xy:  R_c = sum m v_a v_b,  M = sum m,  Q_a = sum m v_a  (a fixed tree inside a 256-row
 *     chunk, then the chunks in order);  K_c = R_c / kappa, or with remove_com (R_c - Q_a Q_b / M) / kappa  (eV);
 *     ke = ((K_xx + K_yy) + K_zz) / 2;  P_c = (double)stresses[s][c] + K_c / V;  p = ((P_xx + P_yy) + P_zz) / 3.
 * (b) `kinetic` (a device fp64 value per structure, kinetic[s * kinetic_stride]: the obs row of an integrator):  ke is read; with
 *     `pressure_tensor` P_c = pressure_tensor[s * tensor_stride + c] and p as in (a); without it no tensor is defined (n_lags must
 *     be 0) and p = (V ((s_xx + s_yy) + s_zz) + 2 ke) / (3 V) with s = (double)stresses[s]: the pressure of m3g_nhc_step.
 * V = |det L| of `lattice` [s] (rows = lattice vectors).  The row of the sample, x [M3G_THERMO_ROW = 11], fp64:
 *     x0 = e_pot = (double)energies[s];  x1 = ke;  x2 = V;  x3 = h = (e_pot + ke) + p_ext[s] V;  x4 = p;
 *     x5 .. x10 = the Green-Lagrange strain eps = (A A^T - 1) / 2 against the reference cell L0, A = L0^-1 L (A_ij = sum_k
 *     L0inv_ik L_kj, (A A^T)_ij = sum_k A_ik A_jk, k ascending), components xx, yy, zz, yz, zx, xy (tensor components, no factor 2);
 *     L0^-1 is formed once by the init call on the host in fp64 (adjugate over determinant).
 * The tensor of the sample, u [M3G_THERMO_TENSOR = 7] = (P_xx, P_yy, P_zz, P_yz, P_zx, P_xy, p); (b) without a tensor: not formed.
 * A sample of a structure whose x or u holds a non-finite value (or, in (a), that has a row with a non-finite velocity) sets
 * M3G_THERMO_NONFINITE (sticky), is counted in n_skipped, enters no accumulator and EMPTIES the ring of that structure, so that no
 * lag spans the gap.  Otherwise, with n = n_samples + 1 (Welford; exactly this order, i <= j, the 66 co-moments row-major over the
 * upper triangle, (i, j) at i * 11 - i (i - 1) / 2 + (j - i)):
 *     d_i = x_i - mean_i;   mean_i <- mean_i + d_i / n;   C_ij <- C_ij + d_i * (x_j - mean_j)   with the NEW mean_j;   n_samples <- n
 * so that Cov(x_i, x_j) = C_ij / n_samples (the fluctuation formulas want the population form).  With n_lags > 0 u is pushed into
 * the structure's ring of the last n_lags tensors, and for every lag l = 0 .. min(entries in the ring, n_lags) - 1 and component c:
 *     uu[l][c] += u_c(now) * u_c(now - l);   now[l][c] += u_c(now);   old[l][c] += u_c(now - l);   lag_count[l] += 1
 * (lag 0 is the sample against itself), from which the mean-subtracted correlation at lag l is uu / k - (now / k)(old / k), k =
 * lag_count[l].  The row is kept as the last row whether the sample was skipped or not.  fp64 throughout, no float atomics,
 * fixed-order sums: every number depends on the structure's own rows only, bitwise the same alone or in any batch. */
typedef struct {
  int64_t n_atoms;     /* N */
  int64_t n_structs;   /* S */
  int32_t n_lags;      /* 0 .. 4096 (M3G_THERMO_MAX_LAGS); 0: no stress correlations, no ring */
} m3g_thermo_sizes;
typedef struct {
  int32_t remove_com;  /* 0 / 1: mode (a) subtracts the centre-of-mass term Q_a Q_b / M */
} m3g_thermo_params;
#define M3G_THERMO_ROW 11
#define M3G_THERMO_COMOMENTS 66
#define M3G_THERMO_TENSOR 7
#define M3G_THERMO_MAX_LAGS 4096
#define M3G_THERMO_NONFINITE 1   /* a sample held a non-finite value: skipped, the ring emptied */
/* Sizes outside their limits -> M3G_ERR_VALUE.  The size follows from `sizes` alone, every region rounded up to 256 bytes: the
 * chunk table; masses [N], p_ext [S], L0^-1 [S,9] fp64; two int64 counters; flags [S] int32; n_samples, n_skipped [S] int64;
 * ring fill and ring position [S] int32; mean [S,11], co-moments [S,66], last row [S,11] fp64; lag_uu, lag_now, lag_old
 * [S, n_lags, 7] fp64, lag_count [S, n_lags] int64, the ring [S, n_lags, 7] fp64; 11 fp64 partials per chunk. */
int m3g_thermo_state_bytes(const m3g_thermo_sizes* sizes, size_t* bytes);
/* HOST host_offsets [S+1] and host_masses [N] (amu, finite and > 0) as m3g_traj_init; host_p_ext [S] (eV/A^3, finite): the external
 * pressure of the enthalpy; host_reference_cells [S,3,3] (A, finite, |det| >= 1e-12): the L0 of the strain.  Everything is checked
 * on the host before any HIP call -> M3G_ERR_VALUE; a short state buffer -> M3G_ERR_SIZE.  Uploads the tables, zeroes the
 * accumulators, waits for the stream. */
int m3g_thermo_init(const m3g_thermo_sizes* sizes, const m3g_thermo_params* params, const int64_t* host_offsets, const double* host_masses,
                    const double* host_p_ext, const double* host_reference_cells, void* state, size_t state_bytes, void* stream);
/* One sample, all pointers DEVICE: energies [S] and stresses [S,6] float32 (pair-virial convention of the integrators), lattice
 * [S,3,3] fp64; then exactly one of vel [N,3] fp64 (mode (a); forces [N,3] float32 or NULL, kick finite) and kinetic (mode (b);
 * kinetic_stride >= 1 doubles between structures; pressure_tensor or NULL, tensor_stride >= 6; forces must be NULL) -- both or
 * neither, or n_lags > 0 in mode (b) without a tensor -> M3G_ERR_VALUE.  Two launches in mode (a), one in mode (b), whatever S, N
 * and n_lags; ring positions and counts live in the state buffer: no allocation, copy or wait, capture-safe on one stream. */
int m3g_thermo_sample(const m3g_thermo_sizes* sizes, const m3g_thermo_params* params, void* state, size_t state_bytes,
                      const float* energies, const float* stresses, const double* lattice, const double* vel, const float* forces,
                      double kick, const double* kinetic, int64_t kinetic_stride, const double* pressure_tensor, int64_t tensor_stride,
                      void* stream);
/* The accumulators to HOST memory; every output may be NULL: mean [S,11], comoments [S,66] fp64; lag_uu, lag_now, lag_old
 * [S, n_lags, 7] fp64; lag_count [S, n_lags], n_samples, n_skipped [S] int64; flags [S] int32 (M3G_THERMO_*).  Waits. */
int m3g_thermo_read(const m3g_thermo_sizes* sizes, const void* state, size_t state_bytes, double* host_mean, double* host_comoments,
                    double* host_lag_uu, double* host_lag_now, double* host_lag_old, int64_t* host_lag_count, int64_t* host_n_samples,
                    int64_t* host_n_skipped, int32_t* host_flags, void* stream);
/* The last row [S,11] and the ring entry `lag` samples back [S,7] (0: the last one pushed; a structure whose ring holds no such
 * entry: NaN) to HOST memory; either may be NULL.  host_tensor needs n_lags > 0 and 0 <= lag < n_lags; before any sample:
 * M3G_ERR_VALUE.  Waits for the stream. */
int m3g_thermo_frame(const m3g_thermo_sizes* sizes, const void* state, size_t state_bytes, int32_t lag, double* host_row,
                     double* host_tensor, void* stream);

/* ---- normal-mode analysis of MD: the trajectory projected on harmonic eigenvectors (csrc/m3g_nma.hip) -------------------------------
 * Normal-mode decomposition (Ladd, Moran and Hoover, Phys. Rev. B 34, 5058 (1986); McGaughey and Kaviany, Phys. Rev. B 69, 094303
 * (2004); the spectral energy density of Thomas et al., Phys. Rev. B 81, 081411 (2010)), fed one frame per m3g_nma_sample, as the
 * trajectory observables above are.  Structure s: a unit cell of n_u atoms with masses m_b, repeated in a diagonal MD supercell
 * (c1, c2, c3) in the order of the phonon family below: atom j = l n_u + b, l = (l1 c2 + l2) c3 + l3, N_c = c1 c2 c3 cells, N_s = N_c n_u
 * atoms.  Equilibrium site r0_j = f_j L (L the unit cell, rows = lattice vectors) with f_j = f_b + (l1, l2, l3) the fractional
 * coordinate in unit-cell units.  Q_s q-points in fractional coordinates of the unit cell's reciprocal lattice, each with an
 * eigenvector matrix E[q] [3 n_u, 3 n_u] complex128 (interleaved re, im; row-major): column nu is the mode, rows 3b .. 3b + 2 belong
 * to atom b -- what m3g_eigh_batched returns for a dynamical matrix of m3g_ph_dynmat (phonopy's convention: the phase on atomic
 * positions).  Mode velocity and mode displacement:
 *   Qdot[q,nu] = N_c^(-1/2) sum_j sqrt(m_j) exp(-2 pi i q.f_j) sum_a conj(E[q][3b+a, nu]) v[j,a]
 *   Q   [q,nu] = the same with u_j = r_j - r0_j - (mass-weighted mean of r - r0 over the structure) in place of v
 * v: `vel` as given, or with `forces` vel + kick kappa F / m (the completion of m3g_traj_sample); with remove_com minus the
 * structure's mass-weighted mean velocity.  Positions are the integrator's unwrapped ones.
 * Two stages, no 3 N_s x 3 N_s projector: W[q,b,a] = N_c^(-1/2) sqrt(m_b) sum_l phase v (per thread the cells l = g, g + G', ... in
 * order with G' = floor(256 / 3 n_u) groups, then the groups in order; the same for u), then Qdot = E[q]^H W with E[q] in LDS (rows in
 * order).  The phase table exp(-2 pi i q.f_j), Q_s N_s 16 bytes per structure, is built once by the init call on the host in fp64
 * from x = (q0 f0 + q1 f1) + q2 f2 reduced by its nearest integer.
 * Accumulators per structure: n_samples; kinetic_sum = sum_t sum_j m_j |v_j|^2 (from the velocities of stage 1, not from the modes:
 * with unitary E and all commensurate q it equals the sum over modes of qdot2_sum); per mode qdot2_sum = sum_t |Qdot|^2 and q2_sum =
 * sum_t |Q|^2; a ring of the last n_lags Qdot; acf[mode, lag] = sum_t conj(Qdot(t - lag)) Qdot(t); lag_count[lag]; flags.
 * A sample with a non-finite position, velocity or force in a structure sets M3G_NMA_NONFINITE in that structure's flags and is not
 * accumulated; a flagged structure accumulates nothing more.  The others are unaffected.
 * No atomics, fixed-order sums over the structure's own rows: every number is bitwise the same alone or in any batch. */
typedef struct {
  int64_t n_atoms;       /* N = sum_s N_s */
  int64_t n_structs;     /* S */
  int64_t n_unit_atoms;  /* U = sum_s n_u */
  int64_t n_qpoints;     /* sum_s Q_s (every structure has at least one) */
  int64_t n_modes;       /* sum_s Q_s 3 n_u */
  int64_t n_eig;         /* sum_s Q_s (3 n_u)^2: complex elements of the eigenvector matrices */
  int64_t n_phase;       /* sum_s Q_s N_s: complex elements of the phase table */
  int32_t max_n;         /* max_s 3 n_u, 3 .. M3G_NMA_MAX_N */
  int32_t n_lags;        /* 0 (no autocorrelation) .. M3G_NMA_MAX_LAGS: ring and acf of n_lags * n_modes * 16 bytes each */
} m3g_nma_sizes;
typedef struct { int32_t remove_com, reserved; } m3g_nma_params;
#define M3G_NMA_MAX_N 64         /* 3 n_u at most: E[q] is 64 KiB of LDS there (M3G_EIGH_MAX_N) */
#define M3G_NMA_MAX_LAGS 4096
#define M3G_NMA_NONFINITE 1      /* flag: a sample of the structure held a non-finite position, velocity or force */
/* Sizes outside their limits or inconsistent among themselves -> M3G_ERR_VALUE. */
int m3g_nma_state_bytes(const m3g_nma_sizes* sizes, size_t* bytes);
/* HOST: host_unit_offsets [S+1] and host_q_offsets [S+1] (int64, from 0, strictly increasing), host_supercells [S,3] (int32, >= 1),
 * host_lattices [S,3,3] fp64 (unit cells), host_frac [U,3] fp64 (f_b), host_masses [U] fp64 (amu, > 0), host_qpoints [sum Q_s, 3] fp64,
 * host_eigenvectors [n_eig] complex128 (structure after structure, q after q).  Everything is checked on the host before any HIP
 * call (sizes that do not follow from the offsets and supercells, non-finite values, remove_com not 0 / 1) -> M3G_ERR_VALUE; a short
 * state buffer -> M3G_ERR_SIZE.  Uploads the tables and zeroes the accumulators.  Waits for the stream. */
int m3g_nma_init(const m3g_nma_sizes* sizes, const m3g_nma_params* params, const int64_t* host_unit_offsets, const int32_t* host_supercells,
                 const double* host_lattices, const double* host_frac, const double* host_masses, const int64_t* host_q_offsets,
                 const double* host_qpoints, const double* host_eigenvectors, void* state, size_t state_bytes, void* stream);
/* One sample: pos, vel [N,3] fp64, forces [N,3] f32 or NULL, all DEVICE; kick finite.  THREE launches whatever the batch, the
 * q-points and the lags; the ring positions and the counts live in the state buffer: no allocation, copy or wait, capture-safe. */
int m3g_nma_sample(const m3g_nma_sizes* sizes, const m3g_nma_params* params, void* state, size_t state_bytes, const double* pos,
                   const double* vel, const float* forces, double kick, void* stream);
/* The accumulators to HOST memory; every output may be NULL: n_samples [S] int64, kinetic_sum [S] fp64, qdot2_sum and q2_sum [n_modes]
 * fp64, acf [n_modes, n_lags] complex128, lag_count [S, n_lags] int64, flags [S] int32 (M3G_NMA_*).  Modes run structure after
 * structure, q after q, nu fastest.  Waits for the stream. */
int m3g_nma_read(const m3g_nma_sizes* sizes, const void* state, size_t state_bytes, int64_t* host_n_samples, double* host_kinetic_sum,
                 double* host_qdot2_sum, double* host_q2_sum, double* host_acf, int64_t* host_lag_count, int32_t* host_flags, void* stream);
/* Qdot and Q [n_modes] complex128 of the last sample every structure accumulated (zeros before its first) to HOST memory.  Waits for
 * the stream. */
int m3g_nma_frame(const m3g_nma_sizes* sizes, const void* state, size_t state_bytes, double* host_qdot, double* host_q, void* stream);

/* ---- batched nudged elastic band: climbing-image NEB force projection (csrc/m3g_neb.hip) ----------------------------------------
 * Replaces ASE's NEB.get_forces (NEB(images, k, climb, method="improvedtangent"), the forces an ASE optimiser drives on the host, one
 * image at a time) for a whole batch of bands.  A band has M >= 3 images: fixed endpoints 0 and M-1 (given once, to m3g_neb_init) and
 * M-2 interior images (the rows of `pos`); all images of a band share the atom count, species order and cell.  For interior image i
 * with energies V and positions R (3n vectors, never wrapped):
 *   tau+ = R_i+1 - R_i, tau- = R_i - R_i-1;
 *   tau  = tau+ if V_i+1 > V_i > V_i-1;  tau- if V_i+1 < V_i < V_i-1;  otherwise, with dVmax / dVmin the max / min of |V_i+1 - V_i| and
 *          |V_i-1 - V_i|: dVmax tau+ + dVmin tau- if V_i+1 > V_i-1, else dVmin tau+ + dVmax tau-  (the f32 energies, compared exactly);
 *   ordinary image:  F_neb = F - (F.tau_hat) tau_hat + k (|tau+| - |tau-|) tau_hat  (ASE's improved parallel spring, one k per band);
 *   climbing image (a band with climb = 1: its interior image of highest energy, LOWEST index on ties -- ASE takes the last entry of
 *          an argsort -- re-chosen at every call):  F_neb = F - 2 (F.tau_hat) tau_hat, no spring.
 * Every F_neb is F + alpha tau+ + beta tau- with two scalars per image, which follow in closed form from five per-image sums (|tau+|^2,
 * |tau-|^2, tau+.tau-, F.tau+, F.tau-).  An image with a non-finite position (its own or a neighbour's), energy or force, or with
 * |tau| = 0, gets NaN rows: m3g_fire_step then flags its band M3G_FIRE_ERROR and freezes it.  The optimiser is ASE's: m3g_fire_step
 * with relax_cell = 0 over the NEB forces, with FIRE offsets of one structure per band covering all of its interior atoms (ASE's FIRE
 * over the NEB optimizable: one dt / v per band, maxstep clipped over the norm of the whole band, converged when max |F_neb| < fmax
 * over the band's interior rows).  No atomics: a band's results are bitwise the same alone or in any batch.
 * The state buffer (m3g_neb_state_bytes) is caller-owned device memory: the chunk table of the interior images, the neighbour table,
 * k, climb, the endpoint rows and energies, per-image scalars. */
#define M3G_NEB_ROWS 5   /* observables per interior image: |tau+|, |tau-|, F.tau_hat, spring term (0 at the climbing image), climbing (0 / 1) */
/* 1 <= n_bands <= n_images <= n_atoms, else M3G_ERR_VALUE. */
int m3g_neb_state_bytes(int64_t n_atoms, int64_t n_images, int64_t n_bands, size_t* bytes);
/* n_atoms: interior atoms of the batch; n_images: interior images I; n_bands: B.  HOST host_image_offsets [I+1] (int64, 0 = o_0 < ... <
 * o_I = n_atoms: atoms of interior image i), host_band_images [B+1] (int32, 0 = b_0 < ... < b_B = I: interior images of band b; the images
 * of a band in path order), host_k [B] (eV/A^2, finite, > 0), host_climb [B] (0 / 1), host_endpoint_energies [2B] (initial, final per
 * band; finite).  endpoint_pos DEVICE fp64 [2 sum_b n_b, 3]: per band its initial image rows, then its final image rows (copied into the
 * state).  Everything is checked on the host before any HIP call: bad offsets, a band without interior image, images of one band with
 * different atom counts, k <= 0 or not finite, climb not 0 / 1, non-finite endpoint energies -> M3G_ERR_VALUE.  Waits for the stream. */
int m3g_neb_init(int64_t n_atoms, int64_t n_images, int64_t n_bands, const int64_t* host_image_offsets, const int32_t* host_band_images,
                 const double* host_k, const int32_t* host_climb, const double* endpoint_pos, const double* host_endpoint_energies,
                 void* state, size_t state_bytes, void* stream);
/* NEB forces of every interior image: pos [N,3] fp64, energies [I] f32, forces [N,3] f32 (evaluated at pos) DEVICE; neb_forces [N,3]
 * f32 DEVICE (written: the forces m3g_fire_step takes); rows [I, M3G_NEB_ROWS] fp64 DEVICE or NULL.  Three launches whatever the batch,
 * no allocation, copy or wait: capture-safe. */
int m3g_neb_forces(int64_t n_atoms, int64_t n_images, int64_t n_bands, void* state, size_t state_bytes, const double* pos,
                   const float* energies, const float* forces, float* neb_forces, double* rows, void* stream);

/* ---- batched finite-displacement phonons: force constants and dynamical matrices (csrc/m3g_phonons.hip) ---------------------------
 * Replaces phonopy's finite-displacement workflow over an ASE calculator (Phonopy(unitcell, supercell_matrix=diag(n1, n2, n3))
 * .generate_displacements(distance=delta, is_plusminus=True, no symmetry) -> one calculator call per displaced supercell ->
 * produce_force_constants -> symmetrize nothing but the acoustic sum rule -> get_dynamical_matrix_at_q) for a whole batch of structures.
 * Structure s: n_u unit atoms at r_b (Cartesian, A), cell L (rows = lattice vectors), diagonal supercell n1 x n2 x n3, N_s = n_u n1 n2 n3.
 *   supercell atom j = l n_u + b, l = (l1 n2 + l2) n3 + l3, at r_b + l1 L_0 + l2 L_1 + l3 L_2 (the home copy of atom u is j = u);
 *   displaced batch: per structure 1 + 6 n_u copies of its N_s rows -- copy 0 undisplaced (the residual forces), copy 1 + 6u + 2a + k
 *          with the home atom u moved by +delta (k = 0) or -delta (k = 1) along Cartesian axis a; structures one after another;
 *   force constants (phonopy's compact layout, fp64 from the fp32 forces): Phi[u, j, a, b] = -(F+_jb - F-_jb) / (2 delta) over the
 *          copies of (u, a); with asr the self term Phi[u, u] is replaced so that sum_j Phi[u, j, a, b] = 0; the raw sums over j are
 *          reported either way.  A structure with a non-finite force in any of its copies gets NaN force constants and sums and a
 *          non-zero count; the others are unaffected;
 *   dynamical matrix (phonopy's convention, q in fractional coordinates of the reciprocal lattice of the unit cell):
 *          D_ua,vb(q) = sum_l sum_m w_m Phi[u, l n_u + v, a, b] exp(2 pi i q.d_m) / sqrt(m_u m_v), d_m the shortest vectors from home
 *          atom u to supercell atom l n_u + v in the supercell's periodicity (unit-cell fractional coordinates; supercell translations
 *          {-2..2}^3 searched, images within 1e-5 A of the shortest tied), w_m = 1 / multiplicity; then (D + D^H) / 2.
 * The image table is built once by m3g_ph_init on the host in fp64.  No atomics: a structure's results are bitwise the same alone or in
 * any batch. */
#define M3G_PH_MAX_MULTIPLICITY 27   /* tied shortest images per (u, j) pair the table holds */
typedef struct {
  int64_t n_structs;      /* S */
  int64_t n_unit_atoms;   /* U = sum_s n_u */
  int64_t n_super_atoms;  /* sum_s N_s; the displaced batch has 6 n_pairs + n_super_atoms rows */
  int64_t n_pairs;        /* sum_s n_u N_s: rows of Phi */
} m3g_ph_sizes;
/* 1 <= n_structs <= n_unit_atoms <= n_super_atoms <= n_pairs, else M3G_ERR_VALUE. */
int m3g_ph_state_bytes(const m3g_ph_sizes* sizes, size_t* bytes);
/* HOST host_unit_offsets [S+1] (int64, 0 = o_0 < ... < o_S = U), host_supercells [S,3] (int32, >= 1), host_lattices [S,3,3] fp64,
 * host_positions [U,3] fp64 (unit cells, Cartesian), host_masses [U] fp64 (amu); delta (A).  Everything is checked on the host before
 * any HIP call: bad offsets, supercell dims < 1, delta not finite or <= 0, masses not finite or <= 0, a singular or non-finite cell,
 * non-finite positions, sizes that do not match the offsets and supercells, more than M3G_PH_MAX_MULTIPLICITY tied images of one pair
 * -> M3G_ERR_VALUE.  Waits for the stream. */
int m3g_ph_init(const m3g_ph_sizes* sizes, const int64_t* host_unit_offsets, const int32_t* host_supercells, const double* host_lattices,
                const double* host_positions, const double* host_masses, double delta, void* state, size_t state_bytes, void* stream);
/* The positions of every row of the displaced batch: pos [6 n_pairs + n_super_atoms, 3] fp64 DEVICE (written).  One launch, no
 * allocation, copy or wait: capture-safe. */
int m3g_ph_displace(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, double* pos, void* stream);
/* forces [6 n_pairs + n_super_atoms, 3] f32 DEVICE (of the displaced batch, in its row order); asr 0 / 1; phi [n_pairs, 3, 3] fp64, sums
 * [U, 9] fp64 (raw sum_j Phi[u, j]), nonfinite [S] int32 (non-finite force values of the structure) DEVICE, written.  One launch,
 * capture-safe. */
int m3g_ph_force_constants(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, const float* forces, int32_t asr, double* phi,
                           double* sums, int32_t* nonfinite, void* stream);
/* Dynamical matrices of n_q q-points: q [n_q, 3] fp64 (fractional), q_struct [n_q] int32 (the structure of each q) DEVICE; dynmat
 * [n_q, 3 max_unit_atoms, 3 max_unit_atoms] complex128 (interleaved re, im) DEVICE: the leading 3 n_u x 3 n_u block of each q is
 * written, the rest left as it is; a q whose structure has more than max_unit_atoms atoms or lies outside [0, S) is skipped.  One
 * launch, capture-safe. */
int m3g_ph_dynmat(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, const double* phi, int64_t n_q, const double* q,
                  const int32_t* q_struct, int32_t max_unit_atoms, double* dynmat, void* stream);

/* ---- batched Hermitian eigensolver for small matrices (csrc/m3g_eigh.h, csrc/m3g_eigh.hip) ------------------------------------------
 * Replaces numpy.linalg.eigh (UPLO = 'U') over a batch of small complex Hermitian matrices.  Cyclic Jacobi with complex rotations in
 * fp64, matrix and eigenvectors in LDS, one workgroup per matrix.  The rotation order is the round-robin (circle) pairing, which
 * depends on n only; a rotation is skipped when |a_pq| <= DBL_EPSILON ||H||_F / n (the norm taken once, over the entries read); the
 * solver stops after a sweep without a rotation, at most M3G_EIGH_MAX_SWEEPS sweeps.  No atomics: a matrix's outputs have the same
 * bits alone, at any position of a batch and for any batch size.
 *   a [M, n, n] complex128 (interleaved re, im; row-major) DEVICE: only the upper triangle and the real part of the diagonal are read;
 *   eigenvalues [M, n] fp64 ascending (ties in index order); eigenvectors [M, n, n] complex128, column k belonging to eigenvalue k,
 *   orthonormal (NULL allowed with want_vectors = 0: the eigenvalues have the same bits either way); info [M] int32: the sweeps run
 *   (the last of them found nothing to rotate) in the bits M3G_EIGH_SWEEPS_MASK, M3G_EIGH_NONFINITE (an entry read, or the norm, is
 *   not finite) and M3G_EIGH_NOT_CONVERGED (the last allowed sweep still rotated) above them.  A flagged matrix gets NaN eigenvalues
 *   and eigenvectors; the others are unaffected.
 * n < 1, n > M3G_EIGH_MAX_N, n_matrices < 0 or a null pointer -> M3G_ERR_VALUE; n_matrices == 0 does nothing.  One launch, no
 * allocation, copy or wait: capture-safe. */
#define M3G_EIGH_MAX_N 64
#define M3G_EIGH_MAX_SWEEPS 30
#define M3G_EIGH_SWEEPS_MASK 0xff
#define M3G_EIGH_NONFINITE 0x100
#define M3G_EIGH_NOT_CONVERGED 0x200
int m3g_eigh_batched(int64_t n_matrices, int32_t n, const double* a, int32_t want_vectors, double* eigenvalues, double* eigenvectors,
                     int32_t* info, void* stream);

/* ---- phonon group velocities (csrc/m3g_phonons.hip) ------------------------------------------------------------------------------
 * Replaces phonopy's DerivativeOfDynamicalMatrix (the analytic derivative) and GroupVelocity.
 * m3g_ph_dynmat_gradient: the arguments, checks and launch shape of m3g_ph_dynmat; gradient [n_q, 3, 3 max_unit_atoms,
 * 3 max_unit_atoms] complex128: dD / dq_alpha for the CARTESIAN q in 1/A without 2 pi (q_cart = q_frac L^-T), that is every image term
 * of D times 2 pi i r_alpha with r = d L; eV / (A amu).  3 n_q blocks-per-q must fit one launch, else M3G_ERR_VALUE. */
int m3g_ph_dynmat_gradient(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, const double* phi, int64_t n_q,
                           const double* q, const int32_t* q_struct, int32_t max_unit_atoms, double* gradient, void* stream);
/* Group velocities v = d f / d q_cart (THz A; 1 THz A = 100 m/s) of n_q q-points, one workgroup each.  DEVICE: eigenvalues [n_q, n]
 * (of D, eV / (A^2 amu), ascending), eigenvectors [n_q, n, n] complex128 (columns), gradient [n_q, 3, n, n] complex128 as above;
 * velocities [n_q, n, 3] fp64 written.  HOST: direction [3], a Cartesian unit vector (| |d| - 1 | <= 1e-12).
 * f_i = sign(lambda_i) sqrt(|lambda_i|) M3G_PH_THZ.  A degenerate set is a maximal run of consecutive f whose neighbouring gaps are
 * below degeneracy_tolerance (THz, finite, >= 0).  In a set of more than one mode, W = E_S^H (sum_alpha direction_alpha dD_alpha) E_S
 * is diagonalised by the solver above and E_S U stands for E_S (in LDS only: the caller's eigenvectors are not modified).  Then
 * v[i, alpha] = Re(e_i^H dD_alpha e_i) M3G_PH_THZ^2 / (2 f_i); a mode with f_i < cutoff_frequency (THz, finite, >= 0; imaginary ones
 * included) gets exactly 0.  A q with a non-finite eigenvalue (a matrix the solver flagged) gets NaN, and so do the modes of a set of
 * more than M3G_PH_GV_MAX_SET modes or whose W the solver flags.  Sums: lane-strided, then a fixed tree; a q's result has the same
 * bits alone or in any batch.  n < 1 or n > M3G_PH_GV_MAX_N, n_q < 0, a null pointer or a bad scalar -> M3G_ERR_VALUE; n_q == 0 does
 * nothing.  One launch, capture-safe. */
#define M3G_PH_THZ 15.63330423985619   /* sqrt(eV / (A^2 amu)) / (2 pi) in THz (CODATA 2018) */
#define M3G_PH_GV_MAX_N 256
#define M3G_PH_GV_MAX_SET 16
int m3g_ph_group_velocities(int64_t n_q, int32_t n, const double* eigenvalues, const double* eigenvectors, const double* gradient,
                            double degeneracy_tolerance, double cutoff_frequency, const double* direction, double* velocities,
                            void* stream);

/* ---- batched finite-strain elastic constants and equation of state (csrc/m3g_elastic.hip) ------------------------------------------
 * Replaces the host loop of pymatgen's DeformedStructureSet / matcalc's ElasticityCalc and EOSCalc over an ASE calculator (deform a
 * cell, evaluate, copy the stress back, 25 times per structure, fit in numpy) for a whole batch of structures.
 * Conventions: rows of a lattice are lattice vectors and a deformation acts on the right, L' = L D, r' = r D, D = I + eps symmetric.
 * Voigt order xx, yy, zz, yz, zx, xy.  The engine's pair-virial `stresses` are -(1/V) dE/d eps; the Cauchy stress (tension positive)
 * is sigma = -stresses, and every quantity below is stated in sigma.
 *   deformed batch: structure s (n_s atoms, cell L, positions r) has 1 + M copies of its n_s rows: copy 0 undeformed, copy m = 1..M
 *          deformed by D_m, which component[m-1] and magnitude[m-1] define: component j in 0..5 -- eps holds that one Voigt
 *          component, eps_jj = d for j < 3, the two off-diagonal entries d / 2 for j >= 3 (d is the engineering shear) -- or
 *          M3G_EL_VOLUMETRIC -- eps = d I (d the linear strain).  Structures one after another: row = (1 + M) o_s + c n_s + b.
 *          r'_c = (r_0 D_0c + r_1 D_1c) + r_2 D_2c in exactly this order with no fused multiply-add, cells likewise;
 *   elastic fit (mode M3G_EL_MODE_ELASTIC; fp64 from the fp32 stresses [copies, 6]): for every strained component j and stress
 *          component i the slope of the least-squares straight line with intercept through (0, sigma_i of copy 0) and (d, sigma_i)
 *          of the copies of component j, in copy order: C_raw[i][j] (eV/A^3).  C = (C_raw + C_raw^T) / 2, S = C^-1 (Gauss-Jordan
 *          with partial pivoting), Voigt / Reuss / Hill bulk and shear moduli, E = 9 K G / (3 K + G) and nu = (3 K - 2 G) /
 *          (2 (3 K + G)) from the Hill values, the universal anisotropy 5 G_V / G_R + K_V / K_R - 6, the eigenvalues of C (cyclic
 *          Jacobi, row-major sweeps, ascending) and stable = smallest eigenvalue > 0.  This is the stress-strain tensor at the given
 *          cell (what pymatgen / matcalc report); it is the second strain derivative of the energy only at zero residual stress.
 *          A structure with a non-finite stress gets NaN in its whole row and a non-zero count; the others are unaffected;
 *   EOS fit (mode M3G_EL_MODE_EOS; fp64 from the fp32 energies [copies]): third-order Birch-Murnaghan, which is exactly a cubic in
 *          t = (V / V_ref)^(-2/3) - 1 = (1 + d)^-2 - 1 (V_ref = |det L|): least squares by Householder QR over the 1 + M points in
 *          u = t / max |t| with the energy of copy 0 subtracted; t0 = the root of dE/dt that is a minimum; V0 = V_ref (1 + t0)^(-3/2),
 *          E0 = E(t0), and with a2 = E''(t0) (1 + t0)^2 / 2, a3 = E'''(t0) (1 + t0)^3 / 6: B0 = 8 a2 / (9 V0), B0' = 4 + 2 a3 / a2.
 *          Error bits: M3G_EL_EOS_NONFINITE (an energy is not finite: the row is NaN), M3G_EL_EOS_NO_MINIMUM (no minimum of the fitted
 *          cubic inside the sampled range of t: the row holds NaN but for v_ref, rms and the point count).
 * No atomics: a structure's results are bitwise the same alone or in any batch. */
#define M3G_EL_VOLUMETRIC 6       /* component value of an isotropic deformation */
#define M3G_EL_MODE_ELASTIC 0
#define M3G_EL_MODE_EOS 1
#define M3G_EL_MAX_DEFORM 64      /* deformations per structure */
#define M3G_EL_MAX_STRAIN 0.2     /* |magnitude| below this */
/* result row of m3g_el_fit_elastic (doubles): C_raw [36] row-major, C [36], S [36], residual sigma [6], eigenvalues [6], then */
#define M3G_EL_ROW_CRAW 0
#define M3G_EL_ROW_C 36
#define M3G_EL_ROW_S 72
#define M3G_EL_ROW_SIGMA0 108
#define M3G_EL_ROW_EIG 114
#define M3G_EL_ROW_ASYMMETRY 120
#define M3G_EL_ROW_FIT_RESIDUAL 121
#define M3G_EL_ROW_KV 122
#define M3G_EL_ROW_KR 123
#define M3G_EL_ROW_KH 124
#define M3G_EL_ROW_GV 125
#define M3G_EL_ROW_GR 126
#define M3G_EL_ROW_GH 127
#define M3G_EL_ROW_YOUNG 128
#define M3G_EL_ROW_POISSON 129
#define M3G_EL_ROW_ANISOTROPY 130
#define M3G_EL_ROW_STABLE 131     /* 1.0 or 0.0 */
#define M3G_EL_ROW 132
/* result row of m3g_el_fit_eos (doubles): v0, e0, b0, b0', rms residual, v_ref, t0, number of points */
#define M3G_EL_EOS_ROW 8
#define M3G_EL_EOS_NONFINITE 1
#define M3G_EL_EOS_NO_MINIMUM 2
typedef struct {
  int64_t n_structs;   /* S */
  int64_t n_atoms;     /* U = sum_s n_s; the deformed batch has (1 + M) U rows and (1 + M) S copies */
  int32_t n_deform;    /* M, 1 .. M3G_EL_MAX_DEFORM */
  int32_t mode;        /* M3G_EL_MODE_* */
} m3g_el_sizes;
/* 1 <= n_structs <= n_atoms, 1 <= n_deform <= M3G_EL_MAX_DEFORM, mode 0 / 1, else M3G_ERR_VALUE. */
int m3g_el_state_bytes(const m3g_el_sizes* sizes, size_t* bytes);
/* HOST host_offsets [S+1] (int64, 0 = o_0 < ... < o_S = U), host_lattices [S,3,3] fp64, host_positions [U,3] fp64 (Cartesian),
 * host_components [M] int32, host_magnitudes [M] fp64.  Everything is checked on the host before any HIP call: bad offsets, a singular
 * or non-finite cell, non-finite positions, a magnitude that is not finite, zero or with |d| >= M3G_EL_MAX_STRAIN; elastic mode: a
 * component outside 0..5, a component with fewer than two distinct magnitudes; EOS mode: a component other than M3G_EL_VOLUMETRIC,
 * fewer than 5 distinct volumes (copy 0 counted) -> M3G_ERR_VALUE.  Waits for the stream. */
int m3g_el_init(const m3g_el_sizes* sizes, const int64_t* host_offsets, const double* host_lattices, const double* host_positions,
                const int32_t* host_components, const double* host_magnitudes, void* state, size_t state_bytes, void* stream);
/* The deformed batch: pos [(1 + M) U, 3] fp64 and lattices [(1 + M) S, 3, 3] fp64 (copy c of structure s at (1 + M) s + c) DEVICE,
 * written.  One launch, no allocation, copy or wait: capture-safe. */
int m3g_el_deform(const m3g_el_sizes* sizes, const void* state, size_t state_bytes, double* pos, double* lattices, void* stream);
/* stresses [(1 + M) S, 6] f32 DEVICE (the engine's pair-virial stresses of the copies); rows [S, M3G_EL_ROW] fp64, nonfinite [S] int32
 * DEVICE, written.  Elastic mode only.  One launch, capture-safe. */
int m3g_el_fit_elastic(const m3g_el_sizes* sizes, const void* state, size_t state_bytes, const float* stresses, double* rows,
                       int32_t* nonfinite, void* stream);
/* energies [(1 + M) S] f32 DEVICE (total energies of the copies); rows [S, M3G_EL_EOS_ROW] fp64, error [S] int32 (M3G_EL_EOS_* bits)
 * DEVICE, written.  EOS mode only.  One launch, capture-safe. */
int m3g_el_fit_eos(const m3g_el_sizes* sizes, const void* state, size_t state_bytes, const float* energies, double* rows, int32_t* error,
                   void* stream);

/* ---- measurement: per-stage device time from HIP events recorded on the call's own stream ---------
 * m3g_profile_enable(plan, 1) makes every following m3g_energy_forces record an event pair around each
 * stage launch; m3g_profile_read synchronises those events, returns per-stage totals since the last
 * read and resets.  `names[i]` points to static strings.  Off by default (no events, no overhead). */
#define M3G_MAX_STAGES 16
int m3g_profile_enable(m3g_plan* plan, int32_t enable);
int m3g_profile_read(m3g_plan* plan, int32_t* n_stages, const char** names /* [M3G_MAX_STAGES] */,
                     float* total_ms /* [M3G_MAX_STAGES] */, int32_t* launches /* [M3G_MAX_STAGES] */);

/* Diagnostic only: with option "stamps" = 1 the forward edge kernel runs a stamped variant (s_memtime per
 * phase), = 2 the reverse edge-MLP kernel of the two-kernel reverse, = 3 the fused reverse kernel (f16x3 mode; its waves ADD
 * their sums over the launches since the option was set); this copies the per-wave phase cycle sums [256 workgroups][16 wave
 * slots][12 phases] to the host. */
int m3g_debug_read_stamps(m3g_plan* plan, uint64_t* host_out);
/* Diagnostic only: number of HIP streams / events the plan currently owns (internal side stream, fork / join events, profiler
 * event pool).  They are bound to the plan's device: a commit that moves the plan to another device releases all of them. */
int m3g_debug_live_handles(const m3g_plan* plan, int32_t* out);

/* Test hooks for the library's own device-wide exclusive scan and stable radix sort (csrc/m3g_prims.h: the primitives behind the
 * neighbour search and the list / topology construction).  elem_bytes / key_bytes: 4 or 8 (integers); in == out allowed for the
 * scan; the sort works in place on `keys` (+ `vals`, int32, may be NULL) over the key bits [begin_bit, end_bit).  Both allocate their
 * temporary storage and wait for the stream: diagnostics only. */
int m3g_debug_exclusive_scan(int32_t elem_bytes, int64_t n, const void* in, void* out, void* stream);
int m3g_debug_radix_sort(int32_t key_bytes, int64_t n, void* keys, int32_t* vals, int32_t begin_bit, int32_t end_bit, void* stream);
/* Test hook, host only (no device call): where each array of the topology buffer lies, from the very function the builds carve the
 * buffer with.  Regions in the buffer's order:
 *   src, dst, row_ptr, in_ptr, in_edge, in_pair, in_pos, t1_ptr, t1_e2, t2_ptr, t2_e1, act_list, act_scan, act_id, arow_ptr, act_dst,
 *   tb_win, tb_fast, t1_e2c, t2_e1c, t1_b, t2_b, batch, struct_ptr, flags
 * byte_offset[i] from the start of the buffer, n_elems[i] the documented length (E, N + 1, T, 2 E for in_pair, 6 and 2 words per window
 * record over n_edges / 128 + 1 records for tb_win and tb_fast, 16 for flags; act_list and act_dst: E, of which the first A =
 * m3g_topology_active_edges are written) -- not the padded allocation --, elem_bytes[i] 4 (int32) or 1 (t1_b, t2_b).  *n_regions is
 * the number of regions (25); at most max_regions entries are written, so a call with max_regions = 0 asks for the count alone. */
int m3g_debug_topology_layout(int64_t n_atoms, int64_t n_edges, int64_t n_triplets, int64_t n_structs, int32_t max_regions,
                              int64_t* byte_offset, int64_t* n_elems, int32_t* elem_bytes, int32_t* n_regions);

/* Measurement: what ONE m3g_energy_forces call with these arguments puts on a stream -- kernel launches and other operations (memsets,
 * copies) -- counted by capturing the call's own launch sequence into a HIP graph on an internal stream (nothing executes, no buffer
 * is touched) and counting the graph's nodes.  The sequence counted is the un-profiled one (the stage profiler changes it). */
int m3g_count_launches(const m3g_plan* plan, const m3g_io* io, void* workspace, size_t workspace_bytes, int32_t* kernel_launches,
                       int32_t* other_operations);

#define M3G_ABI_VERSION 11  /* 2: m3g_io.topo_hints, m3g_topology_hints; 3: m3g_verlet_*, m3g_topology_status, hints word certified on the buffer,
                             * canonical edge order by the shift relative to the given coordinates, default precision fp32;
                             * 4: m3g_verlet_fill_lists, m3g_topology_build_canonical, M3G_TOPO_ERR_SYNC, options small_tiles / small_launches / fuse_node_tb;
                             * 5: m3g_topology_build_canonical_begin / _end, m3g_topology_data_bytes, option legendre_backward, m3g_md_*;
                             * 6: M3G_TOPO_ERR_SPECIES (species checked on the library side, m3g_md_step returns M3G_ERR_VALUE), m3g_count_launches,
                             *    m3g_debug_exclusive_scan / m3g_debug_radix_sort (the library's own scan and sort: no hipCUB);
                             * 7: m3g_fire_* (batched FIRE relaxation, fixed or variable cell);
                             * 8: m3g_dyn_* (batched molecular dynamics: NVE, NVT Berendsen / Langevin, NPT Berendsen);
                             * 9: m3g_neb_* (batched climbing-image NEB force projection, improved tangent; replaces ASE's NEB.get_forces);
                             * 10: m3g_ph_* (batched finite-displacement phonons: displaced supercells, force constants, dynamical matrices);
                             * 11: m3g_el_* (batched finite-strain elastic constants and Birch-Murnaghan equation of state: deformed copies, both fits);
                             *     additive, same version: m3g_eigh_batched (batched Hermitian Jacobi eigensolver), m3g_ph_dynmat_gradient,
                             *     m3g_ph_group_velocities (phonon eigenvectors and group velocities);
                             *     additive, same version: m3g_traj_state_bytes / _init / _sample / _read / _frame (trajectory observables) and
                             *     m3g_dyn_state_view;
                             *     additive, same version: m3g_lbfgs_state_bytes / _init / _step / _read (batched L-BFGS relaxation beside
                             *     FIRE) -- new exports only: no existing struct, constant or call changes, so a caller built
                             *     against 11 runs unchanged;
                             *     additive, same version: m3g_remd_state_bytes / _init / _exchange / _read / _target_view (batched
                             *     replica-exchange MD over an m3g_dyn_* batch);
                             *     additive, same version: m3g_mc_state_bytes / _init / _propose / _decide / _read (batched atom-swap
                             *     Monte Carlo, alone or over an m3g_dyn_* batch);
                             *     additive, same version: m3g_nhc_state_bytes / _state_view / _init / _step / _read (Nose-Hoover chain NVT
                             *     and isotropic MTK NPT, a family beside m3g_dyn_*);
                             *     additive, same version: m3g_mtk_state_bytes / _state_view / _init / _step / _read (flexible-cell MTK NPT:
                             *     the anisotropic barostat, a third MD family beside m3g_dyn_* and m3g_nhc_*);
                             *     additive, same version: m3g_pimd_state_bytes / _state_view / _init / _step / _read: path-integral MD,
                             *     ring polymers under PILE-L, a fourth MD family;
                             *     additive, same version: m3g_ti_state_bytes / _state_view / _init / _path / _step / _read: thermodynamic
                             *     integration to an Einstein crystal under centre-of-mass-conserving Langevin dynamics, a fifth MD family;
                             *     additive, same version: m3g_rnemd_state_bytes / _init / _exchange / _read (reverse non-equilibrium MD
                             *     over an m3g_dyn_* batch: imposed heat or momentum flux, slab profiles);
                             *     additive, same version: m3g_meta_state_bytes / _state_view / _init / _bias / _set_hills / _read
                             *     (collective-variable biasing over any MD family: metadynamics, restraints, walls);
                             *     additive, same version: m3g_sq_state_bytes / _init / _sample / _read / _frame (scattering observables:
                             *     S(q), F(q,t) and the longitudinal and transverse current correlations);
                             *     additive, same version: m3g_lo_state_bytes / _init / _sample / _read / _frame (local-order observables:
                             *     Steinhardt q_l, their neighbour average, solid-like atoms and their clusters);
                             *     additive, same version: m3g_thermo_state_bytes / _init / _sample / _read / _frame (thermodynamic
                             *     fluctuation observables: Welford co-moments of e_pot, ke, V, h, p and the strain; stress correlations);
                             *     additive, same version: m3g_debug_topology_layout (test hook: the regions of the topology buffer) */

#ifdef __cplusplus
}
#endif
#endif /* M3GNET_HIP_H */

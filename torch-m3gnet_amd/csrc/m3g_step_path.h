// Which kernels one m3g_energy_forces step runs: the plan's options and resolve_step_path(), the ONE place where options, sizes
// and topology hints turn into a kernel path.  Plain host C++ (nothing from HIP): tests/c_abi/m3g_step_path_check.cpp builds it
// with a host compiler and prints the path of a table of cases.
#pragma once
#include <cstdint>

#include "../../include/m3gnet_hip.h"

namespace m3g {

constexpr int kMaxBlocks = 8;
// arithmetic of the dense chains (plan option "precision"; m3g_edge_mfma.hip: chain_p)
constexpr int kPrecF32 = 0;      // v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulate -- the reference's arithmetic (default)
constexpr int kPrecBf16x3 = 1;   // 3 v_mfma_f32_16x16x32_bf16 products of 2-way bf16 splits per fp32 product, fp32 accumulate
constexpr int kPrecF16x3 = 2;    // 3 v_mfma_f32_16x16x32_f16 products of 2-way fp16 splits of power-of-two SCALED operands: both parts of
                                 // an operand together carry 22-24 significant bits (an fp32 value to within its own rounding), fp32 accumulate
constexpr int kNumPrec = 3;

constexpr int kSyncWords = 16;
constexpr int kSyncForceTail = 0, kSyncReadout = 1, kSyncNodeRev = 2;   // (+ block index for the per-block ones)
// fused launches: the per-structure sums (energies after the readout, virial after the force gather) are formed by the LAST
// workgroup of the producing launch when the batch has at most this many structures (it walks them one after the other)
constexpr int64_t kForceTailMaxStructs = 8;
// ... and at most this many atoms: the last workgroup's 256 threads then read <= 4 atoms each (measured on the 10,000-atom cell: 40
// dependent reads per thread of values other XCDs have just written cost 24 us after the readout and 65 us after the force gather,
// against 6 and 10 us for the stand-alone sum kernels)
constexpr int64_t kFusedSumsMaxAtoms = 1024;   // (2,000 atoms: readout + sums 23 us against ~20 separately, gather + virial 19 against 17: no gain any more)
// k_node_tb_reverse (two roles in one launch).  Small cells only.  Measured: 32 atoms 20.7 -> 15.8 us for the pair, 108 atoms a gain,
// 256 atoms a small loss, 864 atoms 24 -> 47 us, 10,000 atoms 2.40 -> 2.62 ms per step: publishing costs an L2 write-back per
// three-body workgroup and an L2 invalidate per waiting wave (the XCDs' L2s are not coherent with each other), which a launch
// boundary does once for everybody.
constexpr int64_t kNodeTbFusedMaxAtoms = 128;

// The topology hints word (m3g_io.topo_hints; described in include/m3gnet_hip.h): M3G_TOPO_TB_COMPLETE, then the largest window the
// moment kernels will meet, one byte each -- rows in bits 8-15, centre atoms in bits 16-23.  Formed from the certificate's
// statistics (windows that may not use the moment path, largest window in rows and in atoms); 0 = no certificate.
constexpr int32_t topo_hints_word(int32_t bad, int32_t rows, int32_t atoms) {
  return (bad == 0 && rows > 0) ? (M3G_TOPO_TB_COMPLETE | ((rows & 0xff) << 8) | ((atoms & 0xff) << 16)) : 0;
}
constexpr int topo_hints_rows(int hints) { return (hints >> 8) & 0xff; }
constexpr int topo_hints_atoms(int hints) { return (hints >> 16) & 0xff; }

// ---- plan options (m3g_plan_set_option), all plain ints: their bytes are part of the captured-graph key ----
struct Options {
  int precision = kPrecF32;      // option "precision" (default: exact fp32 MFMA products = the reference's arithmetic; 1 / 2 = the split modes, opt-in)
  int save_p1 = 1;               // option "save_p1" (fp32 mode only): 0 = recompute layer 1 in the reverse kernels (A/B tests)
  int save_p2 = 1;               // option "save_p2" (fp32 mode, fused reverse): 0 = recompute layer 2 in the reverse kernel
  int small_tiles_fwd = 3072;    // option "small_tiles_fwd": the same threshold for the forward kernel alone (measured: a gain up to ~900 atoms, equal at 1,372)
  int small_tiles = 1536;        // option "small_tiles": graphs of at most this many 16-edge tiles run the split-tile edge kernels
                                 // (m3g_edge_small.hip: a tile over the four SIMDs of a CU, operands in registers); 0 = never
  int dp1_by_dst = 0;            // option "dp1_by_dst": dp1 rows of the exact-fp32 fused reverse kernels stored by the edge's position in the by-neighbour
                                 // list.  Measured on the 10k-atom cell: node reverse 205 -> 207 us, reverse edge kernels 1.012 -> 1.017 ms per step --
                                 // the gather of whole 1-KB rows is not what bounds the node reverse; off by default
  int split_node_tiles = 128;    // option "split_node_tiles": 16-atom tiles (2,048 atoms) up to which the node tables and the readout take their split forms
                                 // (m3g_node_mfma.hip; measured at 625 tiles: node tables 58 -> 85 us, readout 28 -> 36 us per step -- not beyond)
  int species_tables = 1;        // option "species_tables": block 0's node rows (x^0, v^0, TA^0, TB^0) depend on the committed weights and the
                                 // atom's species only -- formed once per species at commit (m3g_plan::d_species_tab) and copied per atom
                                 // beside the geometry stage; 0 = block 0's node kernel in every step (A/B tests; bit-identical either way)
  int fuse_node_tb = 1;          // option "fuse_node_tb": three-body reverse (moment path) + node reverse of a block as two workgroup roles of
                                 // one launch (k_node_tb_reverse, m3g_threebody.hip)
  int debug_node_tb_polls = 0;   // option "debug_node_tb_polls" (tests): see launch_node_tb_reverse
  int split_tail = 1;            // option "split_tail": see k_edge_rev_f32 (the tiles of a workgroup's last, part-filled round through the four-way split)
  int small_launches = 1;        // option "small_launches": small systems take fused launches (force tail, readout + energy sums, ...)
  int rev_kernel = 1;            // MFMA path: 1 = fused reverse kernel per block, 0 = node-MLP + edge-MLP kernel pair
  int readout_f16 = 0;           // option "readout_f16": the readout layers on scaled two-part fp16 chains in the f16x3 mode (5 us faster at 10,000
                                 // atoms); default: exact-fp32 chains in every mode -- the per-atom energy can be the ill-conditioned remainder of its
                                 // last layer's terms, where 22 against 24 bits per product show (fuzz case 84)
  int legendre_ref = 0;          // option "legendre_backward" = 1: the reference's own (inexact) backward of P_l, list kernels only
  int tb_moments = 1;            // option "threebody_moments": per-atom moment sums where the partner lists are complete (m3g_threebody.hip)
  int stress_mode = 0;           // 0: reference formula sum pos (x) F / V; 1: pair virial (PBC consistent)
  int edge_kernel = 1;           // 0 = VALU baseline (m3g_edge_simple.hip), 1 = MFMA (m3g_edge_mfma.hip), 2 = any-size path (m3g_generic.hip)
  int stamp_target = 0;          // option "stamps": 0 = off, else the kernel that runs its stamped variant (the stamp buffer exists exactly then):
                                 // 1 forward edge block, 2 reverse edge-MLP kernel, 3 fused reverse (f16x3)
  int overlap = 0;               // option "overlap": 1 = use the side stream (measured 2 % SLOWER on the 10k-atom step: two fork/join
                                 // pairs of cross-stream event waits cost more than the ~40 us of kernel time they hide), default off
  // hipGraph replay (option "graph_replay"): the launch sequence of one m3g_energy_forces call is captured once per
  // distinct (io, workspace, stream, options) and replayed while those stay identical -- for small systems the ~36
  // launches of a step are launch-bound.  The caller must then keep every buffer of the call alive and at the same address.
  int graph_replay = 0;
};
static_assert(sizeof(Options) == 21 * sizeof(int), "Options: twenty-one ints, no padding (its bytes are compared as a key)");

// dp1 hand-over formats of k_node_reverse: fp32 rows, 24-bit floating rows (bf16x3 fused kernel), 24-bit fixed-point rows + scales
// (f16x3 fused kernel)
enum { kDp1F32 = 0, kDp1Packed = 1, kDp1Fixed = 2, kDp1F32ByDst = 3 /* fp32 rows stored by position in the by-neighbour list */ };

enum Pipeline { kPipeValu = 0, kPipeMfma = 1, kPipeAnySize = 2 };
// reverse edge kernel of a block.  One fused kernel per block: k_edge_rev_fused (bf16x3 / f16x3, dual-use images) or, in the fp32
// mode, k_edge_rev_f32 / k_edge_rev_split (they need the saved layer-1 pre-activations); otherwise the node-MLP + edge-MLP pair
enum RevEdge { kRevValu = 0, kRevPair, kRevFused, kRevF32, kRevSplit };
enum Readout { kReadoutValu = 0, kReadoutSplit, kReadoutF32, kReadoutF16 };
// what follows a block's reverse edge kernel
enum RevTail {
  kTailSeparate = 0,   // three-body reverse, then (b > 0) node reverse
  kTailOverlap,        // three-body reverse on the side stream beside the node reverse's dp1 gather, then the v-gradient term
  kTailNodeTb,         // CANDIDATE: both as two roles of one launch, if the runtime says all its workgroups are resident; else separate
  kTailFinalTb,        // block 0: the step's last three-body reverse also forms dE/dr of every edge (no k_geometry_reverse)
};
// how block 0's node rows are formed (its x^0 is the species embedding: nothing in them depends on the call's geometry)
enum Block0Tables {
  kBlock0Kernel = 0,         // the node kernel, like every other block (beside the geometry stage where geom_with_node_pre says so)
  kBlock0ExpandBesideGeom,   // rows of the plan's per-species tables copied per atom, as the second workgroup role of the geometry launch
  kBlock0ExpandAlone,        // ... in a launch of their own (stage profiler on, or no edge and so no geometry launch)
};
enum StressKernel { kStressNone = 0, kStressInGather /* the force gather's last workgroup */, kStressPair, kStressRef };

struct ModelDims { int L, R, C, B; };

struct StepPath {
  int pipeline = kPipeMfma;    // kPipeAnySize: nothing else is set (m3g_generic.hip decides for itself)
  bool fused_rev = false;      // one reverse edge kernel per block that also forms e0 and its reverse (no embedded-edge image)
  int saved_acts = 0;          // workspace: 0 none, 1 layer-1 pre-activations, 2 both layers (fp32 mode)
  int fwd_save = 0;            // what the forward edge kernel stores of them (0 in an energy-only call)
  int dp1 = kDp1F32;           // what the reverse edge kernels hand to the node reverse
  bool dp1_by_dst = false;
  int tb_hints = 0;            // the hints word the three-body kernels see (0: the list kernels, always valid; the reference's Legendre
                               // backward is not linear in the incoming gradient of a triplet, so the moment sums cannot carry it)
  bool moments = false;        // three-body moment kernels (else the list kernels)
  bool long_lists = false;     // list kernels: the long-list instantiation
  bool geom_with_node_pre = false;   // geometry stage and block 0's node tables as two roles of one launch
  int block0 = kBlock0Kernel;  // Block0Tables; anything else: the per-species tables replace the node kernel of block 0, whatever geom_with_node_pre says
  bool node_split = false;     // node tables: a tile and pass per workgroup (else groups of four tiles)
  bool fwd_split = false;      // forward edge kernel: split-tile (else persistent)
  int rev_edge = kRevValu;
  int split_tail = 0;          // kRevF32: its split_tail argument
  int readout = kReadoutValu;
  bool readout_sums = false;   // the readout's last workgroup forms the per-structure energy sums
  bool energy_deferred = false;   // ... nobody has after the readout: k_struct_stress forms them (else, without readout_sums, k_struct_energy)
  int tail[kMaxBlocks] = {};   // RevTail per block
  bool node_rev_small = false;
  bool gather_virial = false;  // the force gather ends with the reference virial
  int stress = kStressNone;    // the stress kernel after the force gather
};

inline StepPath resolve_step_path(const Options& o, const ModelDims& m, int64_t N, int64_t E, int64_t T, int64_t S, int topo_hints,
                                  bool want_forces, bool want_stresses, bool profile) {
  StepPath p;
  p.pipeline = o.edge_kernel;
  if (o.edge_kernel == 2) return p;
  const bool mfma = o.edge_kernel == 1, f32 = o.precision == kPrecF32, stamps = o.stamp_target != 0;
  // fp32 mode is bound by the matrix pipe: its forward kernel saves the layer-1 pre-activations of both MLPs (1 KB per edge and
  // block) and the reverse kernels start from them instead of recomputing that layer (a quarter of their MFMAs)
  const bool saves_p1 = mfma && f32 && o.save_p1 != 0;
  // ... and, with the fused fp32 reverse kernel, the layer-2 pre-activations as well (another 1 KB per edge and block): the
  // reverse kernel then issues no recompute MFMA at all (576 instead of 832 per tile)
  const bool saves_p2 = saves_p1 && o.rev_kernel == 1 && o.save_p2 != 0;
  p.saved_acts = saves_p2 ? 2 : saves_p1 ? 1 : 0;
  p.fwd_save = want_forces ? p.saved_acts : 0;
  p.fused_rev = mfma && o.rev_kernel == 1 && (!f32 || saves_p1);
  p.dp1_by_dst = o.dp1_by_dst && p.fused_rev && f32;
  // the fused kernels write 24-bit rows (floating in the bf16x3 mode, fixed point + scales in the f16x3 mode), everything else fp32 rows
  p.dp1 = !p.fused_rev ? kDp1F32 : p.dp1_by_dst ? kDp1F32ByDst : o.precision == kPrecBf16x3 ? kDp1Packed : o.precision == kPrecF16x3 ? kDp1Fixed : kDp1F32;

  // the moment kernels apply when the topology build found every window complete (hint bit, read back by the caller once per
  // topology: m3g_topology_hints) and l_max <= 3 (their instantiations); no triplets: no three-body launch at all
  p.tb_hints = o.tb_moments && !o.legendre_ref ? topo_hints : 0;
  p.moments = (p.tb_hints & M3G_TOPO_TB_COMPLETE) && m.L >= 1 && m.L <= 3 && m.R >= 1 && m.R <= 4 && topo_hints_rows(p.tb_hints) > 0 &&
              topo_hints_atoms(p.tb_hints) > 0;
  // Long partner lists?  Triplets per edge is a host-side lower bound of triplets per ACTIVE edge (the number of active edges
  // lives on the device); either choice is correct, the wrong one only costs time (global-memory fallback or LDS footprint).
  p.long_lists = T > 24 * E;
  const bool tb_mom = p.moments && E != 0 && T != 0;

  const int64_t etiles = (E + 15) / 16, ntiles = (N + 15) / 16;   // 16-edge / 16-atom tiles
  const bool small_nodes = o.small_launches && ntiles <= o.split_node_tiles;
  const bool few = N <= kFusedSumsMaxAtoms && S > 0 && S <= kForceTailMaxStructs;   // the last workgroup of a launch may form per-structure sums
  if (mfma) {
    p.node_split = f32 && small_nodes;
    p.geom_with_node_pre = !profile && p.node_split && m.B != 0 && E != 0 && N != 0;
    // the copy role needs no LDS and few registers: it sits beside the geometry role at any size
    if (o.species_tables && m.B != 0 && N != 0) p.block0 = !profile && E != 0 ? kBlock0ExpandBesideGeom : kBlock0ExpandAlone;
    // the split-tile kernels cover the exact-fp32 default only (not: another precision / an A-B option of the persistent kernels / stamps)
    p.fwd_split = etiles > 0 && etiles <= o.small_tiles_fwd && f32 && p.fwd_save != 1 && !stamps;
    p.rev_edge = !p.fused_rev ? kRevPair : !f32 ? kRevFused : (etiles > 0 && etiles <= o.small_tiles && saves_p2 && !stamps) ? kRevSplit : kRevF32;
    p.split_tail = o.split_tail;
    const bool f16_readout = o.precision == kPrecF16x3 && o.readout_f16;
    p.readout = f16_readout ? kReadoutF16 : small_nodes ? kReadoutSplit : kReadoutF32;
    p.readout_sums = o.small_launches && N > 0 && few;
    // a step that ends with the reference virial forms the per-structure energy sums in that launch (nothing in between reads them)
    p.energy_deferred = o.small_launches && want_forces && want_stresses && o.stress_mode == 0 && !profile && !p.readout_sums && N > 0;
  }
  if (!want_forces) return p;
  for (int b = 0; b < m.B && b < kMaxBlocks; ++b) {
    if (b > 0 && p.fused_rev && o.overlap && !profile) p.tail[b] = kTailOverlap;
    else if (b > 0 && p.fused_rev && o.fuse_node_tb && !profile && N <= kNodeTbFusedMaxAtoms && N != 0 && tb_mom && kSyncNodeRev + b < kSyncWords)
      p.tail[b] = kTailNodeTb;
    else if (b == 0 && p.fused_rev && o.small_launches && !profile && tb_mom) p.tail[b] = kTailFinalTb;
  }
  p.node_rev_small = o.small_launches && N <= kFusedSumsMaxAtoms;
  // few structures: the force-gather launch ends with the reference virial (one launch less, bit-identical)
  p.gather_virial = mfma && o.small_launches && o.stress_mode == 0 && want_stresses && N > 0 && few;
  p.stress = !want_stresses ? kStressNone : p.gather_virial ? kStressInGather : o.stress_mode == 1 ? kStressPair : kStressRef;
  return p;
}

}  // namespace m3g

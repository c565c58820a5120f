// Internal declarations shared by the translation units of libm3gnet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/m3gnet_hip.h"
#include "m3g_step_path.h"

namespace m3g {

constexpr int kDP = 64;      // padded feature width (embedding_dim <= kDP; zero padding is exact)
constexpr int kLCap = 4;     // l_max <= kLCap
constexpr int kRCap = 4;     // n_max <= kRCap
constexpr int kRAnyCap = 10; // n_max of the any-size path (m3g_generic.hip): the columns of the reference's Bessel-root table
constexpr int kCP = 16;      // padded l_max*n_max
constexpr int kRP = 4;       // padded n_max

void set_error(const char* fmt, ...);
#define M3G_HIP_CHECK(expr)                                                               \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      ::m3g::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return M3G_ERR_HIP;                                                                 \
    }                                                                                     \
  } while (0)

// ---- small constants passed to kernels by value -------------------------------------------------
struct Consts {
  int L, R, C, D, B, num_types;
  float inv_len;        // 1 / length_scale is NOT used for pos (reference divides); kept for forces
  float length_scale, energy_scale;
  float rc, rc3;        // scaled cutoffs
  float a1[kRCap], a2[kRCap];          // (m+1)*pi/rc, (m+2)*pi/rc formed in fp32 like the reference
  float coeff[kRCap];
  float rec_mul[kRCap], rec_div[kRCap]; // sqrt(em[m]/dm[m-1]), sqrt(dm[m])
  float zeros[kLCap][kRCap];
  float factors[kLCap][kRCap];
  float ynorm[kLCap];   // sqrt((2l+1)/(4 pi))
};

// ---- packed weight blob: offsets in floats from the blob base -------------------------------------
struct MlpW {
  // forward orientation, k-major ("_t" = transposed w.r.t. torch's [out,in])
  size_t w1a_t, w1b_t, w1c_t;  // [kDP][2*kDP]  columns: dense | gate
  size_t b1;                   // [2*kDP]
  size_t w2d_t, w2g_t;         // [kDP][kDP]
  size_t b2d, b2g;             // [kDP]
  size_t wl_t;                 // [kRP][kDP]
  // reverse orientation, out-major (torch layout, padded)
  size_t w1a, w1b, w1c;        // [2*kDP][kDP]
  size_t w2d, w2g;             // [kDP][kDP]
  size_t wl;                   // [kDP][kRP]
};
struct BlockW {
  size_t tb_w1_t;   // [kDP][kCP]   v = sigmoid(x W1^T + b1)
  size_t tb_b1;     // [kCP]
  size_t tb_w1;     // [kCP][kDP]
  size_t tb_wd_t, tb_wg_t;  // [kCP][kDP]
  size_t tb_wd, tb_wg;      // [kDP][kCP]
  MlpW e, n;
};
struct ReadoutW {
  size_t w1d_t, w1g_t, w2d_t, w2g_t;  // [kDP][kDP] k-major
  size_t w1d, w1g, w2d, w2g;          // [kDP][kDP] out-major
  size_t b1d, b1g, b2d, b2g;          // [kDP]
  size_t w3d, w3g;                    // [kDP]
  size_t b3;                          // [2]  (dense, gate)
};
struct WeightLayout {
  size_t emb;      // [num_types][kDP]
  size_t adj_t;    // [kRP][kDP]
  size_t adj;      // [kDP][kRP]
  size_t elemental;  // [num_types]
  BlockW blk[kMaxBlocks];
  ReadoutW ro;
  size_t total;
};

// ---- MFMA edge-block weight images (one per block), copied verbatim into LDS by the kernels -----------
// v_mfma_f32_16x16x4_f32: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15], D col = lane&15,
// row = 4*(lane>>4) + reg.  A tile is 16 edges (lane & 15); lane quarter qd = lane>>4 holds, in register `reg`
// of 16-feature block `blk`, feature blk*16 + 4*qd + reg.
// "chain" image of a layer with OB 16-row output blocks and KB 16-wide k blocks (accumulator feeds next layer):
//   img[((ob*KB + kb)*4 + reg)*64 + lane] = W[ob*16 + (lane&15)][kb*16 + 4*(lane>>4) + reg]
// "direct" image (k straight from memory, S steps of 4):
//   img[(ob*S + s)*64 + lane] = W[ob*16 + (lane&15)][4*s + (lane>>4)]
constexpr int kTbSteps = 4;             // three-body MLP: k = l_max*n_max padded to 16 -> 4 k-steps of 4
struct MfmaMlpFwd {                     // offsets in floats inside the forward image
  int w1c;   // chain [8][4]   rows: dense 0-63 | gate 64-127, k: edge features      (8192 floats)
  int w2d;   // chain [4][4]                                                         (4096)
  int w2g;   // chain [4][4]
  int b2;    // [2 (dense,gate)][4 ob][64]  bias as a k-step: lanes < 16 hold b[ob*16+lane], others 0
  int wl;    // direct [4 ob][1 step][64]   W_l [64][R<=4]
};
struct MfmaFwdLayout {
  int tb;    // direct [8 ob][kTbSteps][64]: dense ob0-3, gate ob4-7
  MfmaMlpFwd mlp[2];
  int adj;   // direct [4 ob][1][64]: edge embedding W_adj [64][R<=4] (block 0 forms e0 = SiLU(W_adj h) itself)
  int total;
};
// reverse images: one per conv MLP (two kernels per block: node MLP first, then edge MLP + three-body update)
struct MfmaMlpRev {
  int w1c;           // forward layer-1 image: nothing is saved by the forward pass, both layers are recomputed
  int w2d, w2g, b2;  // forward layer-2 images
  int w2dT;  // chain [4][4]   rows: hidden k, cols: out o
  int w2gT;
  int w1cT;  // chain [4][8]   rows: edge feature k, cols: layer-1 outputs (dense 0-63 | gate 64-127)
  int wl;    // [64][4] plain
  int total; // floats of the MLP part (the node-MLP kernel's whole image)
};
struct MfmaRevLayout {
  MfmaMlpRev mlp;   // offsets inside either image
  int tb;           // edge-MLP image only: forward three-body image
  int tbT;          // edge-MLP image only: chain [1][8] rows: c
  int total_n;      // node-MLP image size
  int total_e;      // edge-MLP image size (MLP part + tb + tbT)
  int per_block;    // total_e + total_n; block b: [edge image | node image]
};
// fused reverse kernel (one per block): dual-use images (m3g_dual_image.h) serve the recompute and the transposed
// products from one LDS copy, so both MLPs fit together
struct MfmaMlpFused {
  int w1c;        // dual image, 128 rows (dense 0-63 | gate 64-127 layer-1 outputs) x 64 edge features
  int w2d, w2g;   // dual images, 64 x 64
  int b2;         // bias images (as the forward kernel's)
  int wl;         // [64][4] plain
  int wld;        // direct [4 ob][64] image of the same W_l (A operand of the W_l h product)
};
struct MfmaRevFusedLayout {
  int tb;    // direct three-body image (forward recompute)
  int tbT;   // chain [1][8] rows: c
  MfmaMlpFused mlp[2];   // 0: edge update, 1: node message
  int adj;   // direct [4 ob][1][64] edge embedding W_adj (block 0 only: e0 and its reverse are formed in the kernel)
  int adjp;  // [64][4] plain copy of W_adj for the dL/dh accumulation
  int total;
};
// fused fp32 reverse kernel (m3g_edge_rev_f32.hip): it starts from the saved layer-1 pre-activations, so it needs W2 in both
// orientations (dual-use fp32 images, m3g_dual_f32.h) but W1c only transposed
struct MfmaMlpRevF32 {
  int w2d, w2g;   // dual fp32 images [64][64]
  int w1cT;       // f32 chain image [4 ob][32 k-steps]: rows = edge feature, k = layer-1 outputs (dense 0-63 | gate 64-127)
  int b2;         // bias images (as the forward kernel's)
  int wl;         // [64][4] plain
  int wld;        // direct [4 ob][64] image of W_l
};
struct MfmaRevF32Layout {
  int tb;    // direct three-body image (forward recompute)
  int tbT;   // f32 chain image [1][32 k-steps] rows: c
  MfmaMlpRevF32 mlp[2];   // 0: edge update, 1: node message
  int adj;   // direct edge-embedding image (block 0)
  int adjp;  // [64][4] plain copy
  int total;
};
MfmaRevF32Layout mfma_rev_f32_layout();
// k_node_pre_mfma image: the 528 x 64 matrix [W1a (TA columns 0-255) | W1b (TB columns) | W_sigmoid1 (v, 16 rows)] as three
// bf16x3 chain images of 11 row blocks (hi + lo parts, the size of an fp32 image), followed by the 528 row biases (b1 for
// TA, 0 for TB, b_sigmoid1)
constexpr int kNodeRowBlocks = 33;
constexpr int kNodeImgFloats = kNodeRowBlocks * 16 * 64 + kNodeRowBlocks * 16;
// per-species rows of block 0 (m3g_plan::d_species_tab, build_species_tables): four arrays of num_types rows one after the other,
// x^0 [kDP] | v^0 [kCP] | TA^0 [4*kDP] | TB^0 [4*kDP], each with the row stride of its per-atom twin in Work
constexpr int kSpeciesRowFloats = kDP + kCP + 2 * 4 * kDP;
constexpr size_t species_tab_v(int num_types) { return (size_t)num_types * kDP; }
constexpr size_t species_tab_ta(int num_types) { return (size_t)num_types * (kDP + kCP); }
constexpr size_t species_tab_tb(int num_types) { return (size_t)num_types * (kDP + kCP + 4 * kDP); }
// k_readout_mfma image (floats): exact-fp32 chain images (f32_chain_image) of the readout GatedMLP (nn/readout.py:39-58)
// and its transposes, then the small vectors
struct ReadoutImg {
  static constexpr int w1 = 0;                 // [8 ob][16 k-steps]  rows: dense 0-63 | gate 64-127 first-layer outputs, k: x
  static constexpr int w2d = w1 + 8 * 2 * 512;   // chain [4][2]
  static constexpr int w2g = w2d + 4 * 2 * 512;
  static constexpr int w2dT = w2g + 4 * 2 * 512; // chain [4][2]  rows: hidden input k, cols: second-layer output
  static constexpr int w2gT = w2dT + 4 * 2 * 512;
  static constexpr int w1T = w2gT + 4 * 2 * 512; // chain [4][4]  rows: x feature, k: dense 0-63 | gate 64-127
  static constexpr int b1 = w1T + 4 * 4 * 512;   // [128]
  static constexpr int b2 = b1 + 128;            // [128] dense | gate
  static constexpr int w3 = b2 + 128;            // [128] dense | gate final weights
  static constexpr int b3 = w3 + 128;            // [2] (+2 pad)
  static constexpr int total = b3 + 4;
};
MfmaFwdLayout mfma_fwd_layout();
MfmaRevLayout mfma_rev_layout();
MfmaRevFusedLayout mfma_rev_fused_layout();

}  // namespace m3g

struct m3g_plan {
  m3g_config cfg;
  m3g::Consts consts;
  m3g::WeightLayout wl;
  std::map<std::string, std::vector<float>> params;  // raw state_dict tensors (host)
  std::map<std::string, std::vector<float>> cvals;   // raw constants (host)
  float* d_weights = nullptr;
  // MFMA weight images, one set per precision mode (same layouts and sizes: an fp32 image is as large as a bf16 hi + lo pair)
  float* d_mfma_fwd[m3g::kNumPrec] = {nullptr, nullptr, nullptr};   // [num_blocks][MfmaFwdLayout.total]
  float* d_mfma_rev[m3g::kNumPrec] = {nullptr, nullptr, nullptr};   // [num_blocks][MfmaRevLayout.total]
  float* d_mfma_revf = nullptr;  // [num_blocks][MfmaRevFusedLayout.total] (bf16x3 dual-use images)
  float* d_mfma_revf_h = nullptr;  // the same layout holding fp16 parts of the scaled weights (f16x3 mode)
  float* d_mfma_revf32 = nullptr;  // [num_blocks][MfmaRevF32Layout.total] (fused fp32 reverse kernel)
  float* d_node_img[m3g::kNumPrec] = {nullptr, nullptr, nullptr};   // [num_blocks][kNodeImgFloats]: node-table weights as MFMA A-operand images (k_node_pre_mfma)
  float* d_species_tab[m3g::kNumPrec] = {nullptr, nullptr, nullptr};   // [num_types][kSpeciesRowFloats]: block 0's node rows per species, formed by
                                                                       // k_node_pre_mfma at every commit from d_node_img, the embedding and w_scale_inv
  m3g::Options opt;           // every option of m3g_plan_set_option that shapes the step (m3g_step_path.h)
  float w_scale_inv = 1.f;       // f16x3 mode: 1 / (the power of two all chain-image weights were multiplied by), set by pack_mfma_images
  int device = -1;               // HIP device the plan's buffers live on (set by m3g_plan_commit)
  // generic path (m3g_generic.hip): raw state_dict tensors, unpadded, in one device blob; offsets by key
  bool generic = false;          // sizes beyond the MFMA kernels' tiles (or option "edge_kernel" = 2)
  float* d_generic = nullptr;
  std::map<std::string, size_t> generic_off;
  float* d_readout_img = nullptr;   // [ReadoutImg::total]: readout MLP weights as exact-fp32 chain images (k_readout_mfma; fp32 and bf16x3 modes)
  float* d_readout_img_h = nullptr; // the same layout as scaled two-part fp16 chain images (f16x3 mode), weights scaled by 1 / ro_w_scale_inv
  float ro_w_scale_inv = 1.f;
  unsigned long long* d_stamps = nullptr;  // option "stamps": diagnostic phase-cycle sums [256][16][12]; non-null exactly while opt.stamp_target != 0
  bool committed = false;
  // opt-in stage profiler (m3g_profile_*): event pairs recorded around stage launches
  // side stream: the three-body reverse of a block (short, latency-bound, does not fill the chip) runs beside the node
  // reverse's dp1 gather (HBM-bound); fork/join with events, created on first use
  bool debug_force_move = false;        // option debug_force_move (tests): the next commit runs the device-move path
  mutable hipStream_t side_stream = nullptr;
  mutable hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // captured launch sequences (option "graph_replay"), keyed by (io, workspace, stream, opt)
  struct GraphEntry { std::vector<unsigned char> key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
  mutable std::vector<GraphEntry> graphs;
  bool profile = false;                 // written by m3g_profile_enable only
  mutable std::vector<hipEvent_t> ev_pool;
  mutable std::vector<int> ev_stage;   // stage id of pair k (events 2k, 2k+1)
  mutable size_t ev_used = 0;          // pairs used since the last read
};

namespace m3g {

// ---- host helpers shared by the launchers ----------------------------------------------------------------
// sizes of carved sub-buffers: every array starts on a 256-byte boundary
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
// grid of a launch with one thread (or one group of `per`) per item
inline dim3 grid_for(int64_t n, int per = 256) { return dim3((unsigned)((n + per - 1) / per)); }
// carving a caller's buffer into arrays, one after the other from `base`.  A null base measures: `off` ends as the bytes needed,
// and what take() returned are the byte offsets themselves (integer arithmetic, so no pointer is formed from null + n).
struct Carve {
  uintptr_t base;
  size_t off = 0;
  explicit Carve(const void* b) : base((uintptr_t)b) {}
  template <class T> T* take(size_t count) { T* r = (T*)(base + off); off += align_up(sizeof(T) * count); return r; }
  void* take(size_t bytes) { return take<char>(bytes); }
};
// the byte offset of a pointer taken from a Carve over a null base
inline size_t carve_offset(const void* p) { return (size_t)(uintptr_t)p; }

// ---- the fp32 basis constants, for Consts and the any-size path's GenConsts alike ---------------------------------------
// fp32 arithmetic in the reference's order (see oracle make_constants / radial_basis): parity rests on these lines.
// radial basis of n_max = R terms over the scaled cutoff rc (nn/featurizer.py:87-96)
template <class C>
inline void fill_radial_consts(C& c, int R, double rc, const float* coeff, const float* em, const float* dm) {
  const float pi_f = (float)M_PI;
  for (int m = 0; m < R; ++m) {
    c.a1[m] = ((float)(m + 1) * pi_f) / (float)rc;
    c.a2[m] = ((float)(m + 2) * pi_f) / (float)rc;
    c.coeff[m] = coeff[m];
    c.rec_mul[m] = m > 0 ? sqrtf(em[m] / dm[m - 1]) : 0.f;
    c.rec_div[m] = sqrtf(dm[m]);
  }
}
// three-body bases: the scaled cutoffs, sqrt((2l+1)/(4 pi)) (nn/interaction.py:198) and the [L, R] tables of Bessel roots and factors
template <class C>
inline void fill_angular_consts(C& c, int L, int R, double rc, double rc3, const float* zeros, const float* factors) {
  c.rc = (float)rc;
  c.rc3 = (float)rc3;
  for (int l = 0; l < L; ++l) {
    c.ynorm[l] = (float)std::sqrt((2 * l + 1) / (4.0 * M_PI));
    for (int n = 0; n < R; ++n) {
      c.zeros[l][n] = zeros[l * R + n];
      c.factors[l][n] = factors[l * R + n];
    }
  }
}

// ---- device helper shared by the graph-side units -----------------------------------------------------------
// One thread's binary search: the first index of the sorted a[0..n) whose key is not below `key`, n when there is none.  `key_of`
// projects an element onto what the array is sorted by (the high word of a 64-bit (row, partner) key, say).
struct KeyItself { template <class T> __device__ T operator()(T v) const { return v; } };
template <class T, class K, class KeyOf = KeyItself>
__device__ __forceinline__ int64_t lower_bound(const T* a, int64_t n, K key, KeyOf key_of = {}) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key_of(a[mid]) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- topology view (device arrays carved from the caller's topo buffer) -----------------------------
// compile-time dispatch on (l_max, n_max) <= (4, 4): BODY sees constexpr int L, R
#define M3G_LR_CASE(l, r, ...) case l * 8 + r: { constexpr int L = l, R = r; __VA_ARGS__; } break;
#define M3G_LR_ROW(l, ...) M3G_LR_CASE(l, 1, __VA_ARGS__) M3G_LR_CASE(l, 2, __VA_ARGS__) M3G_LR_CASE(l, 3, __VA_ARGS__) M3G_LR_CASE(l, 4, __VA_ARGS__)
#define M3G_DISPATCH_LR(L_, R_, BODY) \
  switch ((L_) * 8 + (R_)) { M3G_LR_ROW(1, BODY) M3G_LR_ROW(2, BODY) M3G_LR_ROW(3, BODY) M3G_LR_ROW(4, BODY) default: break; }
// ... on l_max <= 3 only (the three-body moment kernels; an `if constexpr (L <= 3)` body would still instantiate their L = 4 forms)
#define M3G_DISPATCH_LR3(L_, R_, BODY) \
  switch ((L_) * 8 + (R_)) { M3G_LR_ROW(1, BODY) M3G_LR_ROW(2, BODY) M3G_LR_ROW(3, BODY) default: break; }

constexpr int kTbRows = 128;  // active edge rows per three-body workgroup (m3g_threebody.hip; windows precomputed in the topology)
constexpr int kTbCap = 255;  // staged three-body window: the rows of the workgroup + the other rows of the centres they belong to;
                                     // < 256 so a window-relative partner id fits a byte (rows beyond it are read from global memory)
// staged partner ids per row and list (one byte each; longer lists continue from global memory).  Two instantiations of the
// three-body kernels: the short lists of the usual 3-body cutoff (r_3 = 4 A: ~17 partners per active edge) and the long ones of
// dense neighbourhoods (BASELINE config 5, r_3 = 6 A: ~58 per edge) -- sweep in profiles/r02_config5_sweep.txt: staging 96
// ids per row takes the dense case from 61 to 24 us (forward) and 137 to 86 us (reverse) per launch, but costs the 10k-atom
// Cu cell 25 % of its three-body reverse (LDS footprint -> fewer resident workgroups), hence the choice per launch.
constexpr int kTbListShort = 32, kTbListLong = 96;
constexpr int kTbCapShort = kTbRows + 64 < kTbCap ? kTbRows + 64 : kTbCap;   // window rows the short-list instantiation stages
constexpr int kTbFastAtoms = 64;   // most centre atoms per workgroup window the moment path keeps sums for (more: the list path)
static_assert(kTbCap <= 255 && kTbFastAtoms <= 255, "topo_hints_word packs the largest window (rows, atoms) in 8 bits each");
// The window record of one three-body workgroup (Topo::tb_win): the compacted-row window [lo, hi) it stages in LDS, then the ranges
// of its rows' partner lists in t1_e2c and in t2_e1c.  Word w of block b is tb_win[tb_win_at(b, w)]; the buffer holds a record
// for every block index a grid can reach plus one.
enum TbWinWord : int { kTbWinLo, kTbWinHi, kTbWinT1Lo, kTbWinT1Hi, kTbWinT2Lo, kTbWinT2Hi, kTbWinWords };
template <class I>
constexpr I tb_win_at(I blk, int word) { return kTbWinWords * blk + word; }
constexpr int64_t tb_win_blocks(int64_t E) { return E / kTbRows + 1; }   // block indices with a window record
constexpr int kTopoFlags = 16;     // Topo::flags words
struct Topo {
  int64_t N, E, T, S;
  int32_t* src;      // [E] centre of each edge
  int32_t* dst;      // [E] neighbour of each edge
  int32_t* row_ptr;  // [N+1] edges of centre i: row_ptr[i] .. row_ptr[i+1]
  int32_t* in_ptr;   // [N+1] incoming edges of atom j (dst == j)
  int32_t* in_edge;  // [E]
  int32_t* in_pos;   // [E] position of edge e in the by-neighbour list: in_edge[in_pos[e]] == e (dp1 rows are stored by that position in the
                     // exact-fp32 fused path, so the node reverse STREAMS the rows of an atom instead of gathering them)
  int32_t* in_pair;  // [E][2] (in_edge[k], act_id[in_edge[k]]): the k-th incoming edge and its compact three-body row (-1: none),
                     // one 8-byte load in the node reverse gather
  int32_t* t1_ptr;   // [E+1] triplets grouped by first edge e1
  int32_t* t1_e2;    // [T]
  int32_t* t2_ptr;   // [E+1] triplets grouped by second edge e2
  int32_t* t2_e1;    // [T]
  // "active" edges = edges that take part in at least one triplet (d <= three-body cutoff and a partner exists); the
  // three-body kernels run over this compacted list so no lane idles on the edges beyond the three-body cutoff
  int32_t* act_list;   // [A] active edge ids, ascending
  int32_t* act_scan;   // [E+1] number of active edges before e (compacted id of e when e is active)
  int32_t* act_id;     // [E] compacted id of edge e, -1 for an edge without triplets: the per-edge three-body arrays
                       // (q, q', m, dm, dg) hold rows for ACTIVE edges only, indexed by this id
  int32_t* arow_ptr;   // [N+1] compacted rows of centre i: arow_ptr[i] .. arow_ptr[i+1]
  int32_t* t1_e2c;     // [T] t1_e2 in compacted ids
  int32_t* t2_e1c;     // [T] t2_e1 in compacted ids
  uint8_t* t1_b;       // [T] the same partners as byte-sized ids relative to the LDS window of the row's workgroup
  uint8_t* t2_b;       //     (255: outside the staged window -> the kernels fall back to the int32 list)
  int32_t* act_dst;    // [A] neighbour atom of each active edge (saves a dependent load when staging)
  int32_t* tb_win;     // [kTbWinWords * blocks] the window record of each three-body workgroup (TbWinWord)
  int32_t* tb_fast;    // [2 * blocks] per three-body workgroup: {number of centre atoms spanned by its window, first of them} when every
                       // one of those atoms has COMPLETE partner lists (each active edge paired with every other active edge of its
                       // centre exactly once, in both roles) and there are at most kTbFastAtoms of them -- the workgroup may then use
                       // per-atom moment sums instead of walking the lists (m3g_threebody.hip); {0, x} otherwise
  int32_t* n_act;      // device scalar A (= flags + 2)
  int32_t* batch;    // [N]
  int32_t* struct_ptr;  // [S+1] atoms of structure s: struct_ptr[s] .. struct_ptr[s+1] (valid when `batch` is non-decreasing, flags[3] == 0)
  int32_t* flags;    // [kTopoFlags] [0] malformed-graph bits (bits 0-2; bit 3, "sort the incoming edges after all", is the build's own and
                     // cleared before it returns: 0 after a build of well-formed lists); [1] the build's order / symmetry verdicts, 0 after
                     // it; [2] = A; [3] != 0: `batch` is not sorted (per-structure sums then use atomics);
                     // [4] three-body workgroups that may NOT use the moment path, [5] largest window (rows), [6] most atoms per window
                     // (m3g_topology_hints packs 4..6 for the caller); [7] the hints word m3g_topology_hints certified for this
                     // buffer (0 after a build); [8] sticky error bits set by the hot call (M3G_TOPO_ERR_*, m3g_topology_status);
                     // [9..15] reserved, 0
  void* sort_tmp;    // scratch for the radix sorts
  size_t sort_tmp_bytes;
  size_t total_bytes;
};
Topo topo_carve(int64_t N, int64_t E, int64_t T, int64_t S, void* base);
size_t topo_sort_tmp_bytes(int64_t E, int64_t T);

// ---- workspace view ---------------------------------------------------------------------------------
// 24-bit dp1 rows (768 B per edge) leave the last quarter of the [E,4*kDP] fp32 buffer free: the f16x3 mode's per-row inverse
// scales ([E][4] floats) live at its start
inline float* dp1_scale_of(float* dp1, int64_t E) { return dp1 ? dp1 + (size_t)E * 192 : nullptr; }
struct Work {
  // per-edge geometry / bases
  float *u, *d, *h, *hp, *q, *qp, *fc3, *fc3p;  // [E,3] [E] [E,kRP] [E,kRP] [E,kCP] [E,kCP] [E] [E]
  float* x[kMaxBlocks + 1];   // [N,kDP] node features before block b (x[B] = final)
  float* v[kMaxBlocks];       // [N,kCP]
  float *TA, *TB;             // [N,4*kDP]
  float* e;                   // [E,kDP] edge features (updated in place)
  float* m[kMaxBlocks];       // [E,kCP]
  float* act[kMaxBlocks];     // [E,8*kDP] saved pre-activations: e:{p1[2DP],p2d,p2g} n:{p1[2DP],p2d,p2g}
  // reverse pass
  float *dx, *dx2;            // [N,kDP]
  float* de;                  // [E,kDP]
  float* dm;                  // [E,kCP]
  float* g;                   // [E,kCP] q * v[dst] of the current block
  float* dg;                  // [E,kCP]
  float* dh;                  // [E,kRP]
  float* dd;                  // [E]
  float* du;                  // [E,3]
  float* dp1;                 // [E,4*kDP]  (packed 24-bit rows use the first 3/4 of it, dp1_scale_of() the start of the rest)
  float* dr;                  // [E,3]
  // MFMA path: tile-SoA images ([tile of 16 edges][4 blk][64 lanes][4]) of the edge features BEFORE each block
  // (e_blk[b]; e_blk[B] = final) and of dL/de, per-block node tables, row-major messages.  No activations saved.
  float* e_blk[kMaxBlocks + 1];
  float* p2_blk[kMaxBlocks];  // fp32 mode, StepPath::saved_acts == 2: layer-2 pre-activations, same shape; p1_blk then holds SiLU'(p1)
  float* p1_blk[kMaxBlocks];  // fp32 mode: layer-1 pre-activations of both conv MLPs saved by the forward kernel,
                              // [tiles][2 mlp][8 blk][64 lanes][4] (the reverse kernels start from them: StepPath::saved_acts >= 1)
  float* TAb[kMaxBlocks];     // [N,4*kDP] per block (the reverse pass recomputes layer 1 from them)
  float* TBb[kMaxBlocks];
  float* de_soa;
  float* dcn;                 // tile-SoA: node-MLP kernel's contribution to dL/de2 (store-only there, loaded by the edge-MLP kernel)
  float* dh_parts;            // [2B+1][E,kRP]: every reverse kernel stores its dL/dh share in its own slice (no read-modify-write)
  // per-centre sums formed inside the MFMA edge kernels (rows of a centre are consecutive edges): seg_head[t] = sum of the
  // tile's first run (the centre owning column 0), seg_first[i] = sum of the run in which centre i's row starts mid-tile
  float* seg_head;            // [tiles][4*kDP]
  float* seg_first;           // [N][4*kDP]
  float* tail;                // [N + 2 S] scratch for the optional outputs the caller did not ask for (per-atom energies, per-structure sums)
  int32_t* sync;              // [kSyncWords] "last workgroup" counters of the step's fused launches: cleared by k_geometry, the first
                              // kernel of every step (nullptr when carved without a base)
  size_t total_bytes;
};
Work work_carve(int B, const StepPath& path /* pipeline, saved_acts */, int64_t N, int64_t E, int64_t S, void* base);

// ---- kernel launchers (each in its own .hip) -----------------------------------------------------------
// geometry.hip
void launch_geometry(const Consts& c, const Topo& t, const float* pos, const float* lattice, const int32_t* shift,
                     const Work& w, hipStream_t s);
void launch_geometry_reverse(const Consts& c, const Topo& t, const Work& w, const float* dh, int dh_parts, float* forces,
                             float* stresses, hipStream_t s, bool gather_virial = false, const float* pos = nullptr, const float* lattice = nullptr,
                             bool dr_done = false);
void launch_stress(const Consts& c, const Topo& t, const float* pos, const float* lattice, const float* forces,
                   float* stresses, hipStream_t s, const float* ea = nullptr, float* scaled_total = nullptr, float* total = nullptr);
void launch_stress_pair(const Topo& t, const Work& w, const float* lattice, float* stresses, hipStream_t s);
void launch_force_gather(float length_scale, const Topo& t, const float* dr, float* forces, float* stresses, hipStream_t s);
// generic.hip: any-size path (embedding_dim, l_max, n_max beyond the MFMA kernels' tiles)
size_t generic_workspace_bytes(const m3g_plan* plan, int64_t N, int64_t E, int64_t T, int64_t S);
int generic_commit(m3g_plan* plan);
void generic_free(m3g_plan* plan);
int generic_energy_forces(const m3g_plan* plan, const m3g_io* io, void* workspace, size_t workspace_bytes, hipStream_t s);
void generic_edge_featurizer(int n_max, double rc, const float* coeff, const float* em, const float* dm, int64_t E, const float* d, float* out,
                             hipStream_t s);   // kRCap < n_max <= kRAnyCap
void launch_triplet_angles(const Topo& t, const int64_t* tei, const float* u, float* out, hipStream_t s);
void launch_distance_only(float length_scale, const Topo& t, const float* pos, const float* lattice,
                          const int32_t* shift, float* u, float* d, hipStream_t s);
void launch_edge_featurizer(const Consts& c, int64_t E, const float* d, float* out, int out_stride, hipStream_t s);
// node.hip
void launch_embed(const Consts& c, const float* W, const WeightLayout& wl, const Topo& t, const int64_t* types,
                  const Work& w, hipStream_t s);
void launch_embed_reverse(const Consts& c, const float* W, const WeightLayout& wl, const Topo& t, const Work& w,
                          hipStream_t s);
void launch_node_pre(const Consts& c, const float* W, const BlockW& bw, const Topo& t, const Work& w, const float* x_prev, float* x,
                     float* v, float* TA, float* TB, hipStream_t s);
void launch_node_pre_mfma(const m3g_plan* plan, bool split, const Consts& c, const Topo& t, const Work& w, int b, const float* x_prev, float* x,
                          float* v, float* TA, float* TB, const int64_t* types, const float* emb, hipStream_t s);
void launch_geometry_node_pre(const m3g_plan* plan, const Consts& c, const Topo& t, const Work& w, const float* pos, const float* lattice,
                              const int32_t* shift, const int64_t* types, const float* emb, hipStream_t s);
// block 0 from the plan's per-species tables (StepPath::block0), and the tables themselves (m3g_plan_commit, after pack_mfma_images)
void launch_species_expand(const m3g_plan* plan, const Consts& c, const Topo& t, const Work& w, const int64_t* types, hipStream_t s);
void launch_geometry_species(const m3g_plan* plan, const Consts& c, const Topo& t, const Work& w, const float* pos, const float* lattice,
                             const int32_t* shift, const int64_t* types, hipStream_t s);
int build_species_tables(m3g_plan* plan);
void launch_energy_sums(const Consts& c, const Topo& t, const float* scaled_atomic, float* scaled_total, float* total, hipStream_t s);
// (p.readout, p.readout_sums; without the latter the caller forms the energy sums: launch_energy_sums or, deferred, k_struct_stress)
void launch_readout_mfma(const m3g_plan* plan, const StepPath& p, const Consts& c, const WeightLayout& wl, const Topo& t, const int64_t* types,
                         const float* x_prev, float* x, const Work& w, float* scaled_atomic, float* scaled_total, float* total,
                         bool want_grad, hipStream_t s);
void launch_node_reverse(const Consts& c, const float* W, const BlockW& bw, const Topo& t, const Work& w,
                         const float* v, const float* dx_new, float* dx_out, bool row_sums_in_seg, int dp1_packed, bool with_v_term,
                         hipStream_t s, bool small = false);
void launch_node_reverse_v_term(const Consts& c, const float* W, const BlockW& bw, const Topo& t, const Work& w, const float* v,
                                float* dx_out, hipStream_t s);
void launch_readout(const Consts& c, const float* W, const WeightLayout& wl, const Topo& t, const int64_t* types,
                    const float* x_prev, float* x, const Work& w, float* scaled_atomic, float* scaled_total, float* total,
                    bool want_grad, hipStream_t s);
void launch_gather_rows(const float* table, int64_t n, int width, int table_stride, int table_rows, bool transposed,
                        const int64_t* idx, float* out, hipStream_t s);
void launch_copy_expand_rows(const int32_t* row_id, const float* in, int in_stride, float* out, int out_stride, int width, int64_t n,
                             hipStream_t s);
void launch_copy_strided(const float* in, int in_stride, float* out, int out_stride, int width, int64_t rows,
                         hipStream_t s);
// threebody.hip
// (p.moments with p.tb_hints, else the list kernels by p.long_lists)
void launch_threebody(const StepPath& p, const Consts& c, const Topo& t, const Work& w, const float* v, float* m, hipStream_t s);
void launch_threebody_reverse(const StepPath& p, const Consts& c, const Topo& t, const Work& w, const float* v, bool first, hipStream_t s,
                              bool ref_legendre = false);
void launch_threebody_reverse_final(const Consts& c, const Topo& t, const Work& w, const float* v, bool first, const float* dh, int dh_parts,
                                    hipStream_t s, int topo_hints);
// the one launcher that may decline (false: the runtime cannot hold all its workgroups at once -- the caller launches the two kernels)
bool launch_node_tb_reverse(const Consts& c, const float* W, const BlockW& bw, const Topo& t, const Work& w, const float* v, bool first,
                            const float* dx_new, float* dx_out, int dp1_packed, int block, hipStream_t s, int topo_hints, int debug_polls = 0);
// pack_mfma.hip / edge_mfma.hip
int pack_mfma_images(m3g_plan* plan);
void free_mfma_images(m3g_plan* plan);
void launch_edge_block_mfma(const m3g_plan* plan, const StepPath& p, const Consts& c, const Topo& t, const Work& w, int b, hipStream_t s,
                            bool e_out_read = true);
void launch_edge_rev_node_mlp(const m3g_plan* plan, const StepPath& p, const Consts& c, const Topo& t, const Work& w, int b, const float* dx_new,
                              hipStream_t s);
void launch_edge_rev_edge_mlp(const m3g_plan* plan, const StepPath& p, const Consts& c, const Topo& t, const Work& w, int b, const float* dx_new,
                              bool de_is_zero, hipStream_t s);
void launch_edge_rev_fused(const m3g_plan* plan, const Consts& c, const Topo& t, const Work& w, int b, const float* dx_new,
                           bool de_is_zero, hipStream_t s);
void launch_edge_rev_f32(const m3g_plan* plan, const StepPath& p, const Consts& c, const Topo& t, const Work& w, int b, const float* dx_new,
                         bool de_is_zero, hipStream_t s);
// edge_small.hip: the exact-fp32 edge kernels with one tile split over the four waves of a workgroup (small systems)
void launch_edge_fwd_split(const m3g_plan* plan, const StepPath& p, const Consts& c, const Topo& t, const Work& w, int b, hipStream_t s);
void launch_edge_rev_split(const m3g_plan* plan, const StepPath& p, const Consts& c, const Topo& t, const Work& w, int b, const float* dx_new, bool de_is_zero,
                           hipStream_t s);
void launch_embed_edges_soa(const Consts& c, const float* adj_t, const float* h, float* soa, int64_t E, hipStream_t s);
void launch_embed_edges_reverse_soa(const float* adj, const float* h, const float* de_soa, float* dh_slice, int64_t E, hipStream_t s);
void launch_embed_nodes_only(const Consts& c, const float* W, const WeightLayout& wl, const Topo& t, const int64_t* types,
                             const Work& w, hipStream_t s);
void launch_rows_to_soa(const float* rows, float* soa, int64_t E, hipStream_t s);
void launch_soa_to_rows(const float* soa, float* rows, int row_stride, int width, int64_t E, hipStream_t s);
// edge_simple.hip
void launch_edge_block(const Consts& c, const float* W, const BlockW& bw, const Topo& t, const Work& w, int b,
                       const float* x_old, float* x_new, hipStream_t s);
void launch_edge_block_reverse(const Consts& c, const float* W, const BlockW& bw, const Topo& t, const Work& w, int b,
                               const float* dx_new, hipStream_t s);

}  // namespace m3g

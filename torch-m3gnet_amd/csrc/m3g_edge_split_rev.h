// Reverse edge kernel of the exact-fp32 mode with ONE 16-edge tile worked on by FOUR waves (one per SIMD), each owning a quarter of
// every layer's output rows -- the body of k_edge_rev_split (m3g_edge_small.hip: small systems), also run by the persistent kernel
// k_edge_rev_f32 (m3g_edge_rev_f32.hip) on the tiles its waves cannot share out evenly (its "tail").
// Reference: nn/conv.py:63-97, nn/interaction.py:220-221, nn/featurizer.py:128-132; algebra: oracle/staged.py.
#pragma once
#include "m3g_edge_common.h"

namespace m3g {

constexpr int kSplitWaves = 4;
// LDS floats one group of four waves needs: dL/dp2 and dL/dp1 exchange buffers and the per-wave partial dL/dm / dL/dh rows
constexpr int kRevSplitGroupFloats = 3 * 8 * 256;
constexpr int kRevSplitTabFloats = 3 * 256;   // plain W_l of both MLPs, plain W_adj (block 0): shared by all groups

// acc += sum_{blk < 4, r < 4} A[blk*4 + r] * x[XOFF + blk][r]   (chain_f32 restricted to one 16-row output block: same k order)
template <int XOFF, int NX>
__device__ __forceinline__ void chain_reg16(const float (&A)[16], const f32x4 (&x)[NX], f32x4& acc) {
  static_assert(XOFF + 4 <= NX, "chain_reg16 operand out of range");
  static_for<4>([&]<int blk>() { static_for<4>([&]<int r>() { acc = mfma16(A[blk * 4 + r], x[XOFF + blk][r], acc); }); });
}

// The split-tile exchange: what the next layer needs of the other waves' rows (its B operand is the whole activation vector) crosses
// through LDS.  Every wave stores its dense block w and its gate block 4 + w to `hs` (8 blocks x 256 floats), then a workgroup barrier ...
__device__ __forceinline__ void split_publish(float* hs, int w, int lane, const f32x4& dense, const f32x4& gate) {
  *(f32x4*)(hs + w * 256 + lane * 4) = dense;
  *(f32x4*)(hs + (4 + w) * 256 + lane * 4) = gate;
  __syncthreads();
}
// ... and every wave reads all eight blocks (or, short of registers, block by block inside its chain)
__device__ __forceinline__ void split_collect(const float* hs, int lane, f32x4 (&all)[8]) {
  static_for<8>([&]<int ob>() { all[ob] = *(const f32x4*)(hs + ob * 256 + lane * 4); });
}
// (k_readout_split and node_pre_split_body, m3g_node_mfma.hip, spell both out: through these helpers their compiled code changes by
//  more than register names -- profiles/device_idioms.txt)

// ------------------------------------------------------------------------------------------------------------- reverse
struct RevMlpA {
  float wld;          // direct image row block w of W_l (A operand of W_l h)
  float w2t[2][16];   // W2d^T / W2g^T: this wave's 16 input-feature rows, k over the 64 outputs of the branch
  float w1ct[32];     // W1c^T: this wave's 16 edge-feature rows, k over the 128 layer-1 outputs
  const float* wl;    // LDS copy of the plain W_l [64][4] (dL/dh accumulation: rows w*16 + 4 qd + {0..3}); in registers these 16
                      // values per MLP (+ 16 of W_adj in block 0) put the kernel at 292 registers = one workgroup per CU
};
__device__ __forceinline__ void load_rev_mlp(const float* __restrict__ img, const MfmaMlpRevF32& L, int w, int lane, RevMlpA& A, const float* wl_lds) {
  const int m = lane & 15, q = lane >> 4;
  const int base = q * 256 + (m ^ (((q & 1) << 4) | ((q >> 1) << 3)));   // chain_dual32_t's lane offset (m3g_dual_f32.h)
  A.wld = img[L.wld + w * 64 + lane];
  static_for<2>([&]<int hf>() {
    static_for<4>([&]<int blk>() {
      static_for<4>([&]<int r>() { A.w2t[hf][blk * 4 + r] = img[(hf == 0 ? L.w2d : L.w2g) + blk * 1024 + r * 64 + (base ^ ((w * 16) ^ r))]; });
    });
  });
  static_for<32>([&]<int k>() { A.w1ct[k] = img[L.w1cT + (w * 32 + k) * 64 + lane]; });   // f32 chain image [4 ob][32 k-steps]
  A.wl = wl_lds + (w * 16 + 4 * q) * 4;
}

// reverse of one conv GatedMLP from its saved activations, split over the four waves: d_upd = this wave's block of
// dL/d(output); returns this wave's block of contrib = W1c^T dL/dp1; accumulates the wave's share of dL/dh into dhv.
template <bool NEED_DP1, int MLP>
__device__ __forceinline__ f32x4 mlp_reverse_split(const RevMlpA& A, const RevArgs& a, int64_t edge, int64_t drow, int64_t tile, int64_t ci, const SegMasks& sk,
                                                   float hb_sel, const f32x4& d_upd, f32x4& dhv, float* hs1, float* hs2, int w, int lane) {
  const int qd = lane >> 4;
  const float* p2_src = a.p2 + tile * (2 * kP1TileFloats) + MLP * kP1TileFloats + lane * 4;
  const float* p1_src = a.p1 + tile * (2 * kP1TileFloats) + MLP * kP1TileFloats + lane * 4;
  f32x4 d2d = load_tile4(p2_src + w * 256), d2g = load_tile4(p2_src + (4 + w) * 256);   // saved layer-2 pre-activations
  // gating derivatives; W_l h on the matrix pipe, dL/dh on the vector ALU (as mlp_reverse_f32, for row block w)
  const f32x4 sl = mfma16(A.wld, hb_sel, zero4());
  gated_out_reverse(d2d, d2g, d_upd, sl, A.wl, dhv);
  // dL/dp2 of all waves -> every wave (B operand of the W2^T products)
  split_publish(hs1, w, lane, d2d, d2g);
  f32x4 dp1h[2];
  static_for<2>([&]<int hf>() {
    f32x4 dp1 = zero4();
    const f32x4 ds1 = load_tile4(p1_src + (4 * hf + w) * 256);   // saved SiLU'(p1), this wave's block of this half (requested ahead of its chain)
    __builtin_amdgcn_s_setprio(1);
    static_for<4>([&]<int blk>() {   // (B operands block by block from LDS: all eight blocks at once are 32 live registers)
      const f32x4 d2b = *(const f32x4*)(hs1 + (4 * hf + blk) * 256 + lane * 4);
      static_for<4>([&]<int r>() { dp1 = mfma16(A.w2t[hf][blk * 4 + r], d2b[r], dp1); });
    });
    __builtin_amdgcn_s_setprio(0);
    dp1 *= ds1;
    if (NEED_DP1 && edge < a.E) *(f32x4*)(a.dp1 + drow * (4 * kDP) + MLP * (2 * kDP) + hf * kDP + 4 * qd + w * 16) = dp1;
    dp1h[hf] = dp1;
    if (NEED_DP1) {   // per-centre sums of the dp1 rows (x_i half of the node reverse)
      f32x4 t[1] = {edge < a.E ? dp1 : zero4()};
      seg_scan(t, sk);
      seg_store(t, sk, a.seg_head, a.seg_first, tile, ci, qd, MLP * 8 + 4 * hf + w);
    }
  });
  // dL/dp1 of all waves -> every wave (B operand of the W1c^T product)
  split_publish(hs2, w, lane, dp1h[0], dp1h[1]);
  f32x4 contrib = zero4();
  __builtin_amdgcn_s_setprio(1);
  static_for<8>([&]<int blk>() {
    const f32x4 db = *(const f32x4*)(hs2 + blk * 256 + lane * 4);
    static_for<4>([&]<int r>() { contrib = mfma16(A.w1ct[blk * 4 + r], db[r], contrib); });
  });
  __builtin_amdgcn_s_setprio(0);
  return contrib;
}

// The tiles t0, t0 + step, ... < t1 through the four waves of group `g` (wave `w` of it).  EVERY wave of the workgroup that is still
// running calls this together -- it synchronises with workgroup barriers; a group that has run out of tiles simply returns (a wave
// that has ended no longer counts at a barrier).  `scratch`: LDS, groups x kRevSplitGroupFloats + kRevSplitTabFloats floats, free
// for this function once every caller has arrived (the first barrier below) -- it may be the very LDS the image `img` sits in: every
// operand is in registers before that barrier.  The A operands a wave needs -- its quarter of the weight images -- come ONCE from the
// packed image `img` (the L2-resident global copy, or a workgroup's LDS copy) straight into registers (145 per lane).
template <int TBS, bool NEED_DP1>
__device__ __forceinline__ void rev_split_run(const RevArgs& a, const MfmaRevF32Layout& L, const float* img, float* scratch, int groups, int g, int w,
                                              int lane, int64_t t0, int64_t t1, int64_t step) {
  const int qd = lane >> 4;
  float* hs1 = scratch + (size_t)g * kRevSplitGroupFloats;   // dL/dp2 of one MLP, two blocks per wave
  float* hs2 = hs1 + 8 * 256;                                // dL/dp1 of one MLP
  float* part = hs2 + 8 * 256;                               // per-wave partial dL/dm rows, then partial dL/dh rows
  float* small_tabs = scratch + (size_t)groups * kRevSplitGroupFloats;   // plain W_l of both MLPs, plain W_adj (block 0)
  constexpr bool FIRST = !NEED_DP1;   // block 0: its input is the edge embedding e0 = SiLU(W_adj h), reversed here
  float a_tb[2][TBS], a_tbt[2][4];
  static_for<2>([&]<int hf>() {
    static_for<TBS>([&]<int s>() { a_tb[hf][s] = img[L.tb + ((hf * 4 + w) * kTbSteps + s) * 64 + lane]; });
    static_for<4>([&]<int r>() { a_tbt[hf][r] = img[L.tbT + ((hf * 4 + w) * 4 + r) * 64 + lane]; });   // f32 chain image [1][32 k-steps]
  });
  RevMlpA A0, A1;
  load_rev_mlp(img, L.mlp[0], w, lane, A0, small_tabs);
  load_rev_mlp(img, L.mlp[1], w, lane, A1, small_tabs + 256);
  float a_adj = 0.f;
  const float* adjp = small_tabs + 512 + (w * 16 + 4 * qd) * 4;
  if (FIRST) a_adj = img[L.adj + w * 64 + lane];
  float tab0 = 0.f, tab1 = 0.f, tab2 = 0.f;
  const bool tab_writer = threadIdx.x < 256;
  if (tab_writer) {
    tab0 = img[L.mlp[0].wl + threadIdx.x];
    tab1 = img[L.mlp[1].wl + threadIdx.x];
    tab2 = FIRST ? img[L.adjp + threadIdx.x] : 0.f;
  }
  __syncthreads();   // every wave of the workgroup is here (or has ended): `scratch` is free
  if (tab_writer) {
    small_tabs[threadIdx.x] = tab0;
    small_tabs[256 + threadIdx.x] = tab1;
    small_tabs[512 + threadIdx.x] = tab2;
  }
  __syncthreads();
  for (int64_t tile = t0; tile < t1; tile += step) {
    const int64_t edge = tile * kTileEdges + (lane & 15);
    const int64_t ec = edge < a.E ? edge : a.E - 1;
    const int64_t ci = a.src[ec];
    const int64_t drow = (NEED_DP1 && a.in_pos) ? (int64_t)a.in_pos[ec] : edge;   // row of this edge in the dp1 array (see RevArgs::in_pos)
    const SegMasks sk = seg_masks((int)ci, lane);
    const f32x4 hv = *(const f32x4*)(a.h + ec * kRP);
    const float hb_sel = qd == 0 ? hv[0] : qd == 1 ? hv[1] : qd == 2 ? hv[2] : hv[3];
    const int arow = a.act_id[ec];   // < 0: the edge takes part in no triplet, its aggregate is zero
    float mb[TBS];
    static_for<TBS>([&]<int s>() { mb[s] = arow >= 0 ? a.m[(int64_t)arow * kCP + 4 * s + qd] : 0.f; });
    f32x4 dhv = zero4();
    // node-message MLP (nn/conv.py:77-89): d msg[e] = dx_new[centre(e)]
    const f32x4 dmsg = *(const f32x4*)(a.dx_new + ci * kDP + 4 * qd + w * 16);
    f32x4 de;
    if (!a.de_is_zero) de = load_tile4(a.de_soa + tile * kTileFloats + w * 256 + lane * 4);
    f32x4 contrib = mlp_reverse_split<NEED_DP1, 1>(A1, a, edge, drow, tile, ci, sk, hb_sel, dmsg, dhv, hs1, hs2, w, lane);
    // dL/d e2 = what flows in from later blocks + the node MLP's contribution
    if (a.de_is_zero) de = contrib;
    else de = de + contrib;
    // edge-update MLP (nn/conv.py:68-75)
    contrib = mlp_reverse_split<NEED_DP1, 0>(A0, a, edge, drow, tile, ci, sk, hb_sel, de, dhv, hs1, hs2, w, lane);
    de += contrib;   // dL/d e1
    if (!FIRST) *(f32x4*)(a.de_soa + tile * kTileFloats + w * 256 + lane * 4) = de;
    if (FIRST) {
      // edge embedding, reverse: dL/dh += W_adj^T (dL/de0 * SiLU'(W_adj h)), rows of block w
      const f32x4 pe = mfma16(a_adj, hb_sel, zero4());
      static_for<4>([&]<int r>() {
        const f32x4 wr = *(const f32x4*)(adjp + r * 4);
        const float t = de[r] * fdsilu(pe[r]);
        dhv[0] += t * wr[0]; dhv[1] += t * wr[1]; dhv[2] += t * wr[2]; dhv[3] += t * wr[3];
      });
    }
    // three-body gated update, reverse (nn/interaction.py:220-221): rows w (dense) and 4 + w (gate)
    f32x4 pd = zero4(), pg = zero4();
    static_for<TBS>([&]<int s>() {
      pd = mfma16(a_tb[0][s], mb[s], pd);
      pg = mfma16(a_tb[1][s], mb[s], pg);
    });
    gated_reverse(pd, pg, de);
    // dL/dm = W_tb^T d8 over the 128 rows: this wave's 32 rows (blocks w, 4 + w), partial results added in wave order below
    f32x4 dmv = zero4();
    static_for<4>([&]<int r>() { dmv = mfma16(a_tbt[0][r], pd[r], dmv); });
    static_for<4>([&]<int r>() { dmv = mfma16(a_tbt[1][r], pg[r], dmv); });
    static_for<4>([&]<int rr>() { dhv[rr] = sum_lane_quarters(dhv[rr]); });   // the wave's rows of every lane quarter
    *(f32x4*)(part + w * 256 + lane * 4) = dmv;
    *(f32x4*)(part + (4 + w) * 256 + lane * 4) = dhv;
    __syncthreads();
    if (w == 0) {
      f32x4 dm = *(const f32x4*)(part + lane * 4);
      f32x4 dh = *(const f32x4*)(part + 4 * 256 + lane * 4);
      static_for<3>([&]<int k>() {
        dm += *(const f32x4*)(part + (k + 1) * 256 + lane * 4);
        dh += *(const f32x4*)(part + (5 + k) * 256 + lane * 4);
      });
      if (edge < a.E && arow >= 0) *(f32x4*)(a.dm + (int64_t)arow * kCP + 4 * qd) = dm;
      if (qd == 0 && edge < a.E) *(f32x4*)(a.dh + edge * kRP) = dh;
    }
    // (`part` of the next tile is written after four more barriers, all of which wave 0 reaches after the reads above)
  }
}


}  // namespace m3g

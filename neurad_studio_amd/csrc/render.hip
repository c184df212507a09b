// F1 (+C1+C2) fused: multi-resolution hash-grid lookup -> tiny MLPs on the matrix cores -> SDF/density
// head -> transmittance scan -> feature/depth/accumulation compositing, one wavefront per ray.
//
// Wave layout (tile = 16 consecutive samples of one ray):   lane = 16*g + j
//     j = lane & 15  : sample inside the tile          g = lane >> 4 : "k-group" (0..3)
//   * gather: the 4 lanes (j, g=0..3) of a sample each look up L/4 levels  -> 8 features per lane (grids with L*F < 32:
//     ceil(L/4) levels, zero-padded to the same 8 registers -- EncFrame).  Those 8
//     registers ARE the MFMA B-fragments of geo-layer 1 (v_mfma_f32_16x16x4_f32: B[k = lane>>4][n = lane&15]),
//     the weight matrix is the A operand with its K axis permuted to match (done once, at LDS staging).
//   * transposed chaining H^T = W . X^T : the D tile comes out as D[neuron = 4g + r][sample = j]  (r = 0..3),
//     i.e. lane (j,g) again holds 4 activations of ITS sample per 16-neuron block -> they feed the next layer's
//     B operand directly.  No cross-lane traffic, no LDS round trip between the five layers.
//   * compositing: the 16 samples of a tile live in one DPP row (16 lanes) -> exclusive transmittance scan
//     with row_shr DPP ops; the four rows (g) carry identical copies, each accumulates for its own channels.
// Exact fp32 (f32-input MFMA == fmaf chain): the parity target is the reference's fp32 torch path.
//
// What bounds this kernel on MI355X: the far tiles of a ray by the chip's random-line miss rate (every fine-level corner
// is a new 128-byte line for 8-16 useful bytes), the near tiles -- since the MLP products run as fp16 pairs -- by vector
// instruction issue, VALU and MFMA together filling the SIMD's cycles.  Hence:
//   * BLOCK GEOMETRY.  What depends on a sample alone (interval, gaussian, contraction: nine IEEE divisions and two cube
//     roots) is computed once per sample, by the 64 lanes of the wave for a block of four consecutive tiles, and parked
//     in the wave's own LDS rows (Lds::GEO) -- not once per tile by the four lanes that share a sample.  The blend reads
//     the rows again instead of carrying position and std through the MLPs in registers (fill_block, get_block).
//   * SOFTWARE PIPELINE.  A wave's (ray, tile) sequence is flattened; the 8*L/4 corner gathers of the NEXT tile (the
//     next tile of this ray or the first tile of the wave's next ray) are issued right after the current tile's blend,
//     BEFORE its ~170 MFMAs, and stay in flight in VGPRs during the MLP (2 waves / SIMD, ~220 VGPRs); the tile after
//     that already has its sample interval and ray constants requested.  A wave therefore keeps requests in the
//     memory system all the time instead of idling on memory for the ~2 us of its MFMA phase.  Ray constants are
//     read at wave-uniform addresses from `const __restrict__` arguments -> scalar loads, no VGPRs, no vmcnt.
//   * DEFERRED LAST LAYER (composited output).  The last feature layer (H -> 32, no activation) is linear and followed
//     only by sum_s w_s * (.), so the kernel accumulates sum_s w_s*h2_s (H channels) and sum_s w_s*e_s per ray and
//     applies fw2 / fb2 ONCE per ray:  sum_s w_s (fw2 h2_s + fb2 + e_s) = fw2 (sum w h2) + fb2 sum w + sum w e.
//     -32 of 192 MFMAs per tile at H=64; reassociation only (~1e-7 relative).
//   * XCD-COHERENT RAY RANGES.  Workgroup b runs on XCD b % 8 (dispatch order; a wrong guess costs speed only), so the
//     processing order is cut into 8 contiguous ranges and XCD x walks range x with its own workgroups: rays that are
//     neighbours in the order (a 32x32 camera patch; any batch after nrhip_ray_order) share ONE L2 instead of leaving
//     copies of their lines in all eight.  `rays.order` (optional permutation) supplies that order without moving data.
//   * EARLY RAY TERMINATION (eval option, off by default = exact): a ray stops once the transmittance entering a tile
//     is below `stop_eps`; what is skipped weighs less than stop_eps in total.
//   * DYNAMIC ACTORS (ACT instantiations, eval): a sample inside an actor's box reads THAT actor's hash grid at its
//     box-frame position instead of the static grid (neurad_encoding.py:150-187: per-sample table select, highest actor
//     index wins, features zero-padded to 32) and feeds its box-frame direction to the SH encoding.  The ray's candidate
//     list (nrhip_actor_prepare) is walked with scalar loads -- empty for most rays -- and only tiles that contain a hit
//     replace the per-ray SH bias row by four extra k-steps with per-sample SH values.
//   * PACKED SAMPLES (Lay::Packed instantiations, eval: nrhip_render_fwd_packed): the occupancy march's ragged output.  A
//     ray's base and sample count are two scalar loads of `segments`; the pipeline's "wrap to the next ray" decisions use the
//     PENDING ray's own tile count; the ray constants stay per ray, so no per-sample copy of them and no per-sample feature
//     exists anywhere on the route.  Compositing is nrhip_packed_composite_fwd's: no sky residual, depth over all samples,
//     zeros for a ray without samples (which costs one dead tile's gathers and no MLP).  The per-sample kernel (Lay::PackedRows, training:
//     nrhip_field_fwd_train_packed) stores at the packed sample index and carries no compositing state: a lane past the
//     ray's end and a ray without samples store nothing.
//   * PACKED SAMPLES WITH ACTORS (Lay::PackedActors instantiations, eval: nrhip_render_fwd_packed_actors): the two above
//     together -- the pending tile of a packed ray also carries the ray's candidate count, the candidate walk is the dense actor
//     kernel's, the compositing the packed kernel's.  One candidate list per RAY; nothing is sized by the sample count.
//   * PACKED ROWS WITH OVERRIDES (Lay::PackedRowsOvr instantiations, training: nrhip_field_fwd_train_packed_ovr): the
//     per-sample packed kernel of a scene with dynamic actors -- a sample whose entry of ovr_row [M] (read at the packed
//     sample index) is >= 0 takes its encoding row and view direction from the caller, as in the dense Overrides kernels.
// The sky residual (models/neurad.py:381: w_{S-1} += 1 - sum w) is folded into the last tile -- the accumulated weight is
// complete there, so no copy of the last sample's features has to be kept.
#include "common.h"
#include "render_variants.h"

namespace nrhip {

struct FieldDev {
  GridDev grid;
  const void* table;
  float scale;
  const float* gw0; const float* gb0;   // geo layer 0: [H][L*F], [H]
  const float* gw1; const float* gb1;   // geo layer 1: [33][H], [33]
  const float* fw0; const float* fb0;   // feat layer 0: [H][48]
  const float* fw1; const float* fb1;   // feat layer 1: [H][H]
  const float* fw2; const float* fb2;   // feat layer 2: [32][H]
  int use_sdf;
  float beta;
  uint32_t lay[NRHIP_MAX_LEVELS * 4];  // Src::EvalTable kernels: {mulY, mulZ, mask, row0} per level of the eval table (eval_layout.hip)
};

// Training forward (nrhip_field_fwd_train): what the hand-written backward needs, written in the layouts the
// operator-level kernels read ([N, width] row-major).  All null for inference.
struct SaveDev {
  float* enc;  // [N, L*F]  rescaled grid features = input of the geometry MLP
  float* hg;   // [N, H]    geometry MLP hidden activations (post-ReLU)
  float* xf;   // [N, 48]   feature MLP input: geometry embedding (32) | SH of the ray direction (16)
  float* hf;   // [N, 2H]   feature MLP hidden activations, layer 0 | layer 1
};

// LDS carve (floats), H = hidden width.  Fragment-ordered weights use [mb][s/4][lane][s%4] so that one
// ds_read_b128 fetches the A fragments of 4 consecutive k-steps.
// Prod::Bf16Split: the four per-tile matrices are stored as 3-way bf16 splits (6 bytes per weight instead of 4, see
// mfma_layer_split); Prod::F16Pairs: as fp16 pairs (hi image | lo image, 4 bytes per weight, see mfma_layer_pairs).
constexpr int kBlockGeo = 4 * 64;  // floats of one wave's block geometry: x | y | z | std of 64 samples
template <int H, Prod PROD = Prod::F32>
struct Lds {
  static constexpr int NB = H / 16;        // 16-neuron blocks of a hidden layer
  static constexpr int WS(int n) { return PROD == Prod::Bf16Split ? n + n / 2 : n; }
  static constexpr int G0 = 0;             // geo L0 : NB blocks x 8 steps
  static constexpr int G1 = G0 + WS(H * 32);   // geo L1 (rows 1..32): 2 blocks x H/4 steps
  static constexpr int F0 = G1 + WS(32 * H);   // feat L0 (geo part): NB blocks x 8 steps
  static constexpr int F1 = F0 + WS(H * 32);   // feat L1: NB blocks x H/4 steps
  static constexpr int F2 = F1 + WS(H * H);    // feat L2: 2 blocks x H/4 steps (always fp32: applied once per ray)
  static constexpr int SHW = F2 + 32 * H;  // feat L0 SH part: [16 c][NB][4 g][4 r]
  static constexpr int SDFW = SHW + 16 * H;  // geo L1 row 0: [NB][4 g][4 r]
  static constexpr int BG0 = SDFW + H;     // biases, [blk][g][r] == natural order
  static constexpr int BG1 = BG0 + H;      // 33 -> [0] = sdf bias, [1..32]
  static constexpr int BF0 = BG1 + 36;
  static constexpr int BF1 = BF0 + H;
  static constexpr int BF2 = BF1 + H;
  static constexpr int SCAL = BF2 + 32;    // per-level scalings
  static constexpr int RB = SCAL + NRHIP_MAX_LEVELS;  // per wave: this ray's bias of feat L0 (fb0 + SH part), 4 x H
  static constexpr int LAY = RB + 4 * H;   // Src::EvalTable: per-level {mulY, mulZ, mask, row0} (uint32), 16-byte aligned
  static constexpr int FLG = LAY + 4 * NRHIP_MAX_LEVELS;  // Prod::F16Pairs: a weight does not fit the fp16 pair (int, 0 / 1)
  static constexpr int GEO = FLG + 4;      // per wave: contracted position / std of the 64 samples of a block, [4][64]
  static constexpr int TOTAL = GEO + 4 * kBlockGeo;
  // Src::Actors / Src::Overrides instantiations only:
  static constexpr int SHF = TOTAL;             // feat L0 SH part in fragment order: NB blocks x 4 steps
  static constexpr int ASCAL = SHF + 16 * H;    // actor grid: per-level scalings
  static constexpr int AGEO = ASCAL + NRHIP_MAX_LEVELS;  // Src::Actors, per wave: the block's gaussians before the contraction
  static constexpr int TOTAL_ACT = AGEO + 4 * kBlockGeo;
};

// Fused-kernel view of the dynamic actors.  The arrays that are read at wave-uniform addresses are separate
// `const __restrict__` kernel arguments (scalar loads); this struct carries the scalars.
struct ActorFieldDev {
  int K;        // row length of the candidate lists
  int La;       // actor grid levels (<= L; same features per level as the static grid)
  int log2T;    // actor table rows per level
  float scale;  // actor_scale of the actor-frame contraction
  float scal[NRHIP_MAX_LEVELS];  // actor grid scalings
};

// Weight staging.  W[row_off + 16mb + i][col(g,s)] goes to fragment order [mb][s4][lane][s3]; CHAIN: col =
// 16*(s/4) + 4g + s%4 (input is a D tile of the previous layer), else col = 8g + s (input is the gathered feature
// registers).
template <bool CHAIN, int NBLK, int NSTEP>
__device__ __forceinline__ float frag_src(const float* __restrict__ W, int ldw, int row_off, int e) {
  const int s3 = e & 3, lane = (e >> 2) & 63, rest = e >> 8;
  const int s4 = rest % (NSTEP / 4), mb = rest / (NSTEP / 4);
  const int s = 4 * s4 + s3, i = lane & 15, g = lane >> 4;
  const int col = CHAIN ? (16 * (s >> 2) + 4 * g + (s & 3)) : (8 * g + s);
  return W[(size_t)(row_off + 16 * mb + i) * ldw + col];
}

// The encoding frame.  Geo layer 0 always takes K = 32 inputs: lane group g holds 8 feature slots of its sample, owns
// levels LPL g .. LPL g + LPL - 1 (LPL = ceil(L / 4) levels per lane) and puts level LPL g + q, feature f in slot F q + f.
// At L * F == 32 every slot holds a feature.  A smaller grid leaves the slots past LPL F, and the lane groups past L / LPL,
// as zero padding: those lanes issue no gathers, and the padding meets zero weights.  The frame is private to the kernel:
// what crosses the ABI (geo.weight[0] [H, L F], save_enc [N, L F], the override rows [P, L F]) is in the dense order.
template <int L, int F>
struct EncFrame {
  static constexpr int LPL = (L + 3) / 4;          // levels per lane group
  static constexpr int W = LPL * F;                // feature slots of a busy group
  static constexpr int NG = L / LPL;               // busy lane groups
  static constexpr int LF = L * F;                 // dense encoding width
  static constexpr bool FULL = W == 8 && NG == 4;  // no padding (L * F == 32)
  static_assert(W <= 8 && L % LPL == 0, "encoding frame: at most 8 features per lane group, whole levels per group");
  static __device__ __forceinline__ bool busy(int g) { return FULL || g < NG; }
};

// element e of geo layer 0's fragment image (frag_src's order, 8 k-steps): dense column W g + s of the weight, or 0 for
// a padding slot
template <int L, int F, int NBLK>
__device__ __forceinline__ float enc_frag_src(const float* __restrict__ W, int e) {
  using EF = EncFrame<L, F>;
  if constexpr (EF::FULL) {
    return frag_src<false, NBLK, 8>(W, EF::LF, 0, e);
  } else {
    const int s3 = e & 3, lane = (e >> 2) & 63, rest = e >> 8;
    const int s = 4 * (rest & 1) + s3, mb = rest >> 1, i = lane & 15, g = lane >> 4;
    return (s < EF::W && g < EF::NG) ? W[(size_t)(16 * mb + i) * EF::LF + EF::W * g + s] : 0.f;
  }
}

// ---- the matrix work on the matrix cores: 3-way split bf16 ------------------------------------------------------------
// On gfx950 v_mfma_f32_16x16x4_f32 executes at the fp32 VECTOR rate on the vector ALU and overlaps with no other VALU work
// (profiles/r02_mfma_overlap_probe.txt); v_mfma_f32_16x16x16_bf16 is a real second pipe (8 cycles, hides behind VALU
// work).  x = h + m + l with h, m, l bf16 obtained by TRUNCATION (each remainder is exact in fp32), likewise w; the six
// products h.h, h.m, m.h, h.l, l.h, m.m carry every term above 2^-24 of the full product and each is exact in the MFMA's
// fp32 accumulation -- an fp32-equivalent dot product (measured 6e-8 representational error vs 1.4e-7 rounding error of an
// fp32 GEMM), unlike plain bf16 (4e-3) or a 2-way split (3e-5).
using bf16x4 = __attribute__((ext_vector_type(4))) short;

struct Split4 {  // four consecutive k values of one lane, as the three bf16 operands
  bf16x4 h, m, l;
};

__device__ __forceinline__ uint32_t pack_hi16(uint32_t lo_src, uint32_t hi_src) {  // {hi_src[31:16], lo_src[31:16]}
  return __builtin_amdgcn_perm(hi_src, lo_src, 0x07060302u);
}

__device__ __forceinline__ Split4 split4(float x0, float x1, float x2, float x3) {
  const float x[4] = {x0, x1, x2, x3};
  uint32_t h[4], m[4], l[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    h[k] = __float_as_uint(x[k]) & 0xffff0000u;
    const float r1 = x[k] - __uint_as_float(h[k]);  // exact
    m[k] = __float_as_uint(r1) & 0xffff0000u;
    l[k] = __float_as_uint(r1 - __uint_as_float(m[k]));  // exact; its upper half is taken at the packing
  }
  Split4 s;
  s.h = __builtin_bit_cast(bf16x4, uint2{pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3])});
  s.m = __builtin_bit_cast(bf16x4, uint2{pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3])});
  s.l = __builtin_bit_cast(bf16x4, uint2{pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3])});
  return s;
}

// One layer on a 16-sample tile: acc[mb] += W[16 mb .. +15][:] . x, K = 16 KB inputs.  Weights: LDS image
// [mb][kb][split h|m|l][lane] of 8-byte A fragments (lane (i, g): row 16 mb + i, k = 16 kb + 4 g + 0..3 in the layer's own
// input order, see stage_split_matrix; stored as a (h | m) 16-byte image followed by an l 8-byte image); activations
// b[4 kb + v]: this lane's inputs of k-block kb.
template <int NBLK, int KB>
__device__ __forceinline__ void mfma_layer_split(const float* __restrict__ wf, int lane, const float (&b)[4 * KB],
                                                 f32x4 (&acc)[NBLK]) {
  const uint2* w2 = reinterpret_cast<const uint2*>(wf);
  // Consecutive MFMAs go to DIFFERENT accumulators: a dependent bf16 MFMA waits ~3 issue slots for its predecessor, so the
  // six terms of one block issued back to back run no faster than the fp32 MFMA they replace.  Two-block layers get a second
  // accumulator set for that (terms 0-2 | 3-5), summed at the end.
  constexpr bool kTwoSets = NBLK < 4;
  f32x4 acc2[kTwoSets ? NBLK : 1];
  if constexpr (kTwoSets) {
#pragma unroll
    for (int mb = 0; mb < NBLK; ++mb) acc2[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const Split4 x = split4(b[4 * kb], b[4 * kb + 1], b[4 * kb + 2], b[4 * kb + 3]);
    bf16x4 ah[NBLK], am[NBLK], al[NBLK];
#pragma unroll
    for (int mb = 0; mb < NBLK; ++mb) {  // one 16-byte read (h | m) + one 8-byte read (l) per block
      const uint4 hm = reinterpret_cast<const uint4*>(wf)[(mb * KB + kb) * 64 + lane];
      ah[mb] = __builtin_bit_cast(bf16x4, uint2{hm.x, hm.y});
      am[mb] = __builtin_bit_cast(bf16x4, uint2{hm.z, hm.w});
      al[mb] = __builtin_bit_cast(bf16x4, w2[NBLK * KB * 128 + (mb * KB + kb) * 64 + lane]);
    }
#define NR_TERM(ACC, A_, X_)                                                                          \
  _Pragma("unroll") for (int mb = 0; mb < NBLK; ++mb) ACC[mb] =                                        \
      __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(A_[mb], X_, ACC[mb], 0, 0, 0);
    if constexpr (kTwoSets) {
      NR_TERM(acc2, al, x.h) NR_TERM(acc, ah, x.h) NR_TERM(acc2, ah, x.l) NR_TERM(acc, ah, x.m)
      NR_TERM(acc2, am, x.m) NR_TERM(acc, am, x.h)
    } else {  // small terms first
      NR_TERM(acc, al, x.h) NR_TERM(acc, ah, x.l) NR_TERM(acc, am, x.m) NR_TERM(acc, am, x.h) NR_TERM(acc, ah, x.m)
      NR_TERM(acc, ah, x.h)
    }
#undef NR_TERM
  }
  if constexpr (kTwoSets) {
#pragma unroll
    for (int mb = 0; mb < NBLK; ++mb) acc[mb] += acc2[mb];
  }
}

// W[row_off + 16 mb + i][col] -> the split image above.  CHAIN: the layer's input is the previous layer's D tile (lane (j,g)
// holds neurons 16 kb + 4 g + v of block kb): col = 16 kb + 4 g + v; else the gathered features (lane holds 8 g .. 8 g + 7,
// k-block kb takes its features 4 kb .. 4 kb + 3): col = 8 g + 4 kb + v.
template <bool CHAIN, int NBLK, int KB>
__device__ __forceinline__ void stage_split_matrix(float* __restrict__ dst, const float* __restrict__ W, int ldw,
                                                   int row_off) {
  unsigned short* d16 = reinterpret_cast<unsigned short*>(dst);
  for (int e = threadIdx.x; e < NBLK * KB * 64 * 4; e += 256) {
    const int v = e & 3, lane = (e >> 2) & 63, rest = e >> 8;
    const int kb = rest % KB, mb = rest / KB;
    const int i = lane & 15, g = lane >> 4;
    const int col = CHAIN ? (16 * kb + 4 * g + v) : (8 * g + 4 * kb + v);
    const float w = W[(size_t)(row_off + 16 * mb + i) * ldw + col];
    const uint32_t h = __float_as_uint(w) & 0xffff0000u;
    const float r1 = w - __uint_as_float(h);
    const uint32_t m = __float_as_uint(r1) & 0xffff0000u;
    const uint32_t l = __float_as_uint(r1 - __uint_as_float(m));
    // in bf16 units: [mb][kb][lane][h0..h3 m0..m3] (16 bytes per lane), then [mb][kb][lane][l0..l3] (8 bytes per lane)
    const int blk = (mb * KB + kb) * 64 + lane;
    d16[blk * 8 + v] = (unsigned short)(h >> 16);
    d16[blk * 8 + 4 + v] = (unsigned short)(m >> 16);
    d16[NBLK * KB * 64 * 8 + blk * 4 + v] = (unsigned short)(l >> 16);
  }
}

// ---- the matrix work on the matrix cores, second form: fp16 PAIRS -------------------------------------------------------
// x = h + l with h = fp16(x) and l = fp16(x - h) (both round-to-nearest; the remainder is exact in fp32): 22-24 significant
// bits, and the three products h.h, l.h, h.l carry every term above 2^-22 of the full product, each exact in the MFMA's
// fp32 accumulation.  One v_mfma_f32_16x16x32_f16 per 32 inputs and term: 60 MFMAs per 16-sample tile at H = 64, on a pipe of
// their own, where the fp32 form issues 160 v_mfma_f32_16x16x4_f32 on the vector ALU and the 3-way bf16 split 240 of K = 16;
// 2.5 VALU instructions per activation for the split instead of the bf16 split's 5.4 (gfx950 converts and subtracts PAIRS:
// v_cvt_pk_f16_f32, v_pk_add_f32).  fp16's exponent range is the price; it is spent where the network lives --
//   * the whole tile runs in units of kPairAct = 2^6 (ReLU MLPs are positively homogeneous: the biases and the feature inputs
//     are staged / blended x 2^6, the three exits -- sdf row, deferred last layer, embedding sum -- x 2^-6; all exact), so an
//     activation keeps its full precision from 1e-6 up to 1000;
//   * the weights are staged x kPairW = 2^7 and the biases x 2^7 on top, so that the scaled sum accumulates onto the bias in
//     place and comes back through one multiplication by 2^-7 per output;
//   * a tile with an input that does not fit (|x| >= 1000 in true units, infinities) or a matrix with |w| >= 500 takes the
//     fp32 MFMA with its A fragments read from global memory: slow, and the fp32-MFMA kernel's numbers.
// numpy emulation (scripts/pairs_emulation.py, profiles/r05_pairs_emulation.txt): rel. error of a 64-term product sum
// 0.7-1.0e-7 for activations >= 1e-2 (2.7e-7 at 1e-3) -- the fp32 product sum's own 1.0e-7 -- against 1.7e-6 .. 1.7e-4
// without the two recentrings.  On the bench batch the two forms' outputs are 1.0e-7 apart (bench.py: mlp_products).
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
constexpr float kPairAct = 64.f, kPairW = 128.f, kPairFit = 65000.f;
constexpr bool kPairsDefault = true;  // NRHIP_MLP_PAIRS unset (=0: the fp32 MFMA)

// source of element e of a pair image: [mb][q][lane][t] halves (lane (i, g) slot t of the K = 32 step q: row 16 mb + i,
// input of (g, 8 q + t) in the layer's own order -- CHAIN: the previous layer's D tiles (lane (j, g) holds neurons
// 16 kb + 4 g + v of block kb = 2 q + t / 4, v = t % 4), else the gathered features 8 g + t)
template <bool CHAIN, int NBLK, int KQ>
__device__ __forceinline__ float pair_src(const float* __restrict__ W, int ldw, int row_off, int e) {
  const int t = e & 7, lane = (e >> 3) & 63, rest = e >> 9;
  const int q = rest % KQ, mb = rest / KQ;
  const int i = lane & 15, g = lane >> 4;
  const int col = CHAIN ? (16 * (2 * q + (t >> 2)) + 4 * g + (t & 3)) : (8 * g + t);
  return W[(size_t)(row_off + 16 * mb + i) * ldw + col];
}
// element e of a region of N weights: hi image at halves [0, N), lo image at [N, 2 N).  -> does not fit
__device__ __forceinline__ bool pair_store(float* __restrict__ region, int N, int e, float w) {
  _Float16* d16 = reinterpret_cast<_Float16*>(region);
  const float ws = w * kPairW;
  const _Float16 h = (_Float16)ws;
  d16[e] = h;
  d16[N + e] = (_Float16)(ws - (float)h);
  return !(fabsf(ws) < kPairFit);
}

// One layer on a 16-sample tile: acc[mb] = (acc[mb] + kPairW W[row_off + 16 mb .. +15][:] . b) / kPairW, K = 32 KQ inputs
// (b in the layer's own order, see pair_src); acc arrives holding kPairW x the bias (staged so), which makes the scaled
// product sum accumulate in place: no second accumulator set in a kernel at 213 VGPRs.  The accumulation order (hi.hi,
// lo.hi, hi.lo per K step) is immaterial: every addition rounds at 2^-24 of the running sum, as in any fp32 product sum.
// W / ldw / row_off: the fp32 matrix in global memory for the tiles that do not fit.
template <bool CHAIN, int NBLK, int KQ>
__device__ __forceinline__ void mfma_layer_pairs(const float* __restrict__ wf, const float* __restrict__ W, int ldw,
                                                 int row_off, bool wbad, int lane, const float (&b)[8 * KQ],
                                                 f32x4 (&acc)[NBLK]) {
  float mx = 0.f;
#pragma unroll
  for (int k = 0; k < 8 * KQ; ++k) mx = fmaxf(mx, fabsf(b[k]));
  if (__builtin_expect(wbad || __builtin_amdgcn_ballot_w64(!(mx < kPairFit)) != 0ull, 0)) {  // wave-uniform, rare
    // (the fragment addresses depend on the lane only: without the opaque offset they are hoisted out of the TILE loop,
    // 2 VGPRs each, and the fast path spills)
    int opaque = 0;
    asm volatile("" : "+v"(opaque));
    const int g = lane >> 4;
    const float* Wl = W + (size_t)(row_off + (lane & 15)) * ldw + opaque;
#pragma unroll
    for (int s = 0; s < 8 * KQ; ++s) {
      const int col = CHAIN ? (16 * (s >> 2) + 4 * g + (s & 3)) : (8 * g + s);
#pragma unroll
      for (int mb = 0; mb < NBLK; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(Wl[(size_t)16 * mb * ldw + col] * kPairW, b[s], acc[mb], 0, 0, 0);
    }
  } else {
    const f16x8* w8 = reinterpret_cast<const f16x8*>(wf);
    constexpr int LO = NBLK * KQ * 64;  // f16x8 units from the hi image to the lo image
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      f16x8 xh, xl;
#pragma unroll
      for (int k = 0; k < 8; k += 2) {
        const f32x2 v = {b[8 * q + k], b[8 * q + k + 1]};
        const f16x2 h = __builtin_convertvector(v, f16x2);
        const f16x2 l = __builtin_convertvector(v - __builtin_convertvector(h, f32x2), f16x2);  // (the remainder is exact)
        xh[k] = h[0], xh[k + 1] = h[1], xl[k] = l[0], xl[k + 1] = l[1];
      }
      // consecutive MFMAs go to different accumulators (a dependent one waits for its predecessor's passes)
#pragma unroll
      for (int mb = 0; mb < NBLK; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w8[(mb * KQ + q) * 64 + lane], xh, acc[mb], 0, 0, 0);
#pragma unroll
      for (int mb = 0; mb < NBLK; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w8[LO + (mb * KQ + q) * 64 + lane], xh, acc[mb], 0, 0, 0);
#pragma unroll
      for (int mb = 0; mb < NBLK; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w8[(mb * KQ + q) * 64 + lane], xl, acc[mb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int mb = 0; mb < NBLK; ++mb) acc[mb] *= 1.f / kPairW;
}

// One per-tile layer on the variant's products: acc (+)= W . b, K inputs per lane in the layer's own order (CHAIN: the
// previous layer's D tiles, else the gathered features).  W / ldw / row_off / wbad: the pair form's fp32 way out.
template <Prod PROD, bool CHAIN, int NBLK, int K>
__device__ __forceinline__ void tile_layer(const float* __restrict__ wf, const float* __restrict__ W, int ldw, int row_off,
                                           bool wbad, int lane, const float (&b)[K], f32x4 (&acc)[NBLK]) {
  if constexpr (PROD == Prod::F16Pairs) mfma_layer_pairs<CHAIN, NBLK, K / 8>(wf, W, ldw, row_off, wbad, lane, b, acc);
  else if constexpr (PROD == Prod::Bf16Split) mfma_layer_split<NBLK, K / 4>(wf, lane, b, acc);
  else mfma_layer<NBLK, K>(wf, lane, b, acc);
}

// Stage all weights of the field into LDS (256-thread workgroup; caller barriers afterwards).  Every thread first
// ISSUES all of its global loads (one register each, ~60 in flight), then stores: one memory round trip for the whole
// 54 KB image instead of one per loop iteration.
template <int L, int F, int H, Prod PROD = Prod::F32>
__device__ __forceinline__ void stage_field_weights(const FieldDev& fd, float* __restrict__ lds) {
  using Ld = Lds<H, PROD>;
  constexpr int LF = EncFrame<L, F>::LF;  // row length of geo layer 0
  static_assert(PROD == Prod::F32 || EncFrame<L, F>::FULL, "split / pair products: L * F == 32 only");
  constexpr int NB = H / 16;
  constexpr int T = 256;  // == blockDim.x
  constexpr int N_G0 = H * 32 / T, N_G1 = 32 * H / T, N_F0 = H * 32 / T, N_F1 = H * H / T, N_F2 = 32 * H / T,
                N_SH = 16 * H / T;
  static_assert((H * 32) % T == 0 && (H * H) % T == 0 && (16 * H) % T == 0, "regions are whole passes of the block");
  const int tid = threadIdx.x;
  float vg0[N_G0], vg1[N_G1], vf0[N_F0], vf1[N_F1], vf2[N_F2], vsh[N_SH], vs[7];
  if constexpr (PROD == Prod::Bf16Split) {
    stage_split_matrix<false, NB, 2>(lds + Ld::G0, fd.gw0, LF, 0);
    stage_split_matrix<true, 2, NB>(lds + Ld::G1, fd.gw1, H, 1);
    stage_split_matrix<true, NB, 2>(lds + Ld::F0, fd.fw0, 48, 0);
    stage_split_matrix<true, NB, NB>(lds + Ld::F1, fd.fw1, H, 0);
  } else if constexpr (PROD == Prod::F16Pairs) {
    static_assert(H % 32 == 0, "fp16 pairs: K = 32 steps");
    if (tid == 0) reinterpret_cast<int*>(lds)[Ld::FLG] = 0;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < N_G0; ++it) vg0[it] = pair_src<false, NB, 1>(fd.gw0, LF, 0, it * T + tid);
#pragma unroll
    for (int it = 0; it < N_G1; ++it) vg1[it] = pair_src<true, 2, H / 32>(fd.gw1, H, 1, it * T + tid);
#pragma unroll
    for (int it = 0; it < N_F0; ++it) vf0[it] = pair_src<true, NB, 1>(fd.fw0, 48, 0, it * T + tid);
#pragma unroll
    for (int it = 0; it < N_F1; ++it) vf1[it] = pair_src<true, NB, H / 32>(fd.fw1, H, 0, it * T + tid);
  } else {
#pragma unroll
    for (int it = 0; it < N_G0; ++it) vg0[it] = enc_frag_src<L, F, NB>(fd.gw0, it * T + tid);
#pragma unroll
    for (int it = 0; it < N_G1; ++it) vg1[it] = frag_src<true, 2, H / 4>(fd.gw1, H, 1, it * T + tid);
#pragma unroll
    for (int it = 0; it < N_F0; ++it) vf0[it] = frag_src<true, NB, 8>(fd.fw0, 48, 0, it * T + tid);
#pragma unroll
    for (int it = 0; it < N_F1; ++it) vf1[it] = frag_src<true, NB, H / 4>(fd.fw1, H, 0, it * T + tid);
  }
#pragma unroll
  for (int it = 0; it < N_F2; ++it) vf2[it] = frag_src<true, 2, H / 4>(fd.fw2, H, 0, it * T + tid);
#pragma unroll
  for (int it = 0; it < N_SH; ++it) {  // SHW[c][n] = fw0[n][32+c]
    const int e = it * T + tid, c = e / H, n = e - c * H;
    vsh[it] = fd.fw0[(size_t)n * 48 + 32 + c];
  }
  const int th = tid < H ? tid : 0, t33 = tid < 33 ? tid : 0, t32 = tid & 31;
  vs[0] = fd.gw1[th];
  vs[1] = fd.gb0 ? fd.gb0[th] : 0.f;
  vs[2] = fd.fb0 ? fd.fb0[th] : 0.f;
  vs[3] = fd.fb1 ? fd.fb1[th] : 0.f;
  vs[4] = fd.gb1 ? fd.gb1[t33] : 0.f;
  vs[5] = fd.fb2 ? fd.fb2[t32] : 0.f;
  vs[6] = fd.grid.scal[t32];
  if constexpr (PROD == Prod::F16Pairs) {
    // the tile runs in units of kPairAct (see mfma_layer_pairs): biases in, the three exits out -- all powers of two
    // ... and the biases of the four pair layers x kPairW on top (mfma_layer_pairs accumulates onto them in place)
    constexpr float kB = kPairAct * kPairW;
    vs[0] *= 1.f / kPairAct, vs[1] *= kB, vs[2] *= kB, vs[3] *= kB;
    if (t33 != 0) vs[4] *= kB;
#pragma unroll
    for (int it = 0; it < N_F2; ++it) vf2[it] *= 1.f / kPairAct;
#pragma unroll
    for (int it = 0; it < N_SH; ++it) vsh[it] *= kB;
    bool bad = false;
#pragma unroll
    for (int it = 0; it < N_G0; ++it) bad |= pair_store(lds + Ld::G0, H * 32, it * T + tid, vg0[it]);
#pragma unroll
    for (int it = 0; it < N_G1; ++it) bad |= pair_store(lds + Ld::G1, 32 * H, it * T + tid, vg1[it]);
#pragma unroll
    for (int it = 0; it < N_F0; ++it) bad |= pair_store(lds + Ld::F0, H * 32, it * T + tid, vf0[it]);
#pragma unroll
    for (int it = 0; it < N_F1; ++it) bad |= pair_store(lds + Ld::F1, H * H, it * T + tid, vf1[it]);
    if (bad) reinterpret_cast<int*>(lds)[Ld::FLG] = 1;
  }
  if constexpr (PROD == Prod::F32) {
#pragma unroll
    for (int it = 0; it < N_G0; ++it) lds[Ld::G0 + it * T + tid] = vg0[it];
#pragma unroll
    for (int it = 0; it < N_G1; ++it) lds[Ld::G1 + it * T + tid] = vg1[it];
#pragma unroll
    for (int it = 0; it < N_F0; ++it) lds[Ld::F0 + it * T + tid] = vf0[it];
#pragma unroll
    for (int it = 0; it < N_F1; ++it) lds[Ld::F1 + it * T + tid] = vf1[it];
  }
#pragma unroll
  for (int it = 0; it < N_F2; ++it) lds[Ld::F2 + it * T + tid] = vf2[it];
#pragma unroll
  for (int it = 0; it < N_SH; ++it) lds[Ld::SHW + it * T + tid] = vsh[it];
  if (tid < H) {
    lds[Ld::SDFW + tid] = vs[0];
    lds[Ld::BG0 + tid] = vs[1];
    lds[Ld::BF0 + tid] = vs[2];
    lds[Ld::BF1 + tid] = vs[3];
  }
  if (tid < 33) lds[Ld::BG1 + tid] = vs[4];
  if (tid < 32) {
    lds[Ld::BF2 + tid] = vs[5];
    lds[Ld::SCAL + tid] = vs[6];
  }
}

// Streaming store of 16 bytes: the activations a training forward saves (1.2 KB per sample) are read again only by the
// backward, a whole kernel later -- marked non-temporal so that they do not evict the hash-table lines the gathers live on
// from the L2.
__device__ __forceinline__ void stream_store(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }

template <int N>
__device__ __forceinline__ float row_shr(float v, float fill) {
  return dpp_row_shr<N>(v, fill);
}
// sum over the 16 lanes of a DPP row (result valid in every lane of the row)
__device__ __forceinline__ float row_sum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

// ---- the three pipeline stages' state ------------------------------------------------------------------------------
template <int LPL, int F>
struct TileFetch {
  float fv[LPL][8][F];  // corner entries, in flight until the blend
  float x, y, z, std;   // contracted sample position / std: the trilinear offsets and the H4 weights are re-derived from
                        // them at blend time (3 VALU per level and axis) instead of holding 4*LPL more registers.
                        // ACT kernels only (a sample inside a box has its own frame); the others read Lds::GEO again
  float t0, t1;
};
// An ACT tile carries, next to its fetch, one register: the slot (in the ray's candidate list) of the actor whose box
// contains the lane's sample, -1 = static scene.

// Range of the processing order one wave walks.  The ray-side pointers are separate `const __restrict__` kernel
// arguments: the per-ray constants are read at wave-uniform addresses, and only noalias/readonly arguments let the
// compiler turn those reads into scalar loads inside a loop that also stores.
struct RayRange {
  int64_t end;  // one past the last position of this wave's range
  int S, stride;
};

// The tile that will be issued NEXT iteration: its sample interval (vector loads, per lane) and ray constants (scalar
// loads) are requested one iteration ahead, so issuing its gathers never waits on a memory round trip.
// The interval is that of the tile's BLOCK (four consecutive tiles = 64 samples of the ray): lane l holds sample
// 64 (t / 4) + l, one coalesced load when the wave enters the block (t % 4 == 0); the block's other tiles keep it.
struct PendingTile {
  int64_t pos;  // position in the processing order
  int64_t ray;  // ray index = order[pos] (or pos)
  int t;
  bool valid;
  float t0, t1;
  float ox, oy, oz, dx, dy, dz, area;
  int ncand;  // ACT: number of candidate actors of the ray (wave-uniform)
};

// Everything that depends on the sample alone, computed ONCE per sample: lane l of the wave holds sample 64 b + l of the
// block the pending tile lies in (the four lanes of a tile's sample would each repeat the same divisions and cube roots,
// tile after tile, with a quarter of the lanes doing distinct work).  Written when the block's first tile is issued; tile
// k of the block takes its values from lane 16 k + j: position and std through the wave's own LDS rows (Lds::GEO; no
// register is held across the MLPs for them, and a wave's LDS accesses execute in order: no barrier), the interval by a
// cross-lane move out of the pending tile's registers.  A wave issues the tiles of a ray in order and always enters a ray
// at tile 0 (early termination skips to the next ray's tile 0), so one block is live at a time.
// Same instruction sequence on the same inputs as the per-tile form: the values are bit-identical.
__device__ __forceinline__ float from_lane(float v, int byte_addr) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(byte_addr, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ void put_block(float* geo, int lane, const SamplePos& p) {
  geo[lane] = p.x, geo[64 + lane] = p.y, geo[128 + lane] = p.z, geo[192 + lane] = p.std;
}
__device__ __forceinline__ SamplePos get_block(const float* geo, int src) {
  SamplePos p;
  p.x = geo[src], p.y = geo[64 + src], p.z = geo[128 + src], p.std = geo[192 + src];
  return p;
}

// ACT: ageo takes the gaussian before the contraction as well (box tests, actor-frame contraction)
template <bool ACT>
__device__ __forceinline__ void fill_block(float* geo, float* ageo, int lane, const PendingTile& pt, float scale) {
  if constexpr (ACT) {
    const SamplePos gs = sample_gaussian(pt.ox, pt.oy, pt.oz, pt.dx, pt.dy, pt.dz, pt.area, pt.t0, pt.t1);
    put_block(ageo, lane, gs);
    put_block(geo, lane, contract_gaussian(gs.x, gs.y, gs.z, gs.std, scale));
  } else {
    put_block(geo, lane, sample_position(pt.ox, pt.oy, pt.oz, pt.dx, pt.dy, pt.dz, pt.area, pt.t0, pt.t1, scale));
  }
}

__device__ __forceinline__ void load_pending(PendingTile& p, int64_t pos, int t, const RayRange& rr, int lane,
                                             const int32_t* __restrict__ order, const float* __restrict__ ro,
                                             const float* __restrict__ rd, const float* __restrict__ rarea,
                                             const float* __restrict__ rstarts, const float* __restrict__ rends,
                                             const int32_t* __restrict__ cand_count = nullptr) {
  // Past the end of this wave's range the loads still go out (clamped to the last position, tile 0) and their gathers
  // are issued and dropped: an `if (valid)` around them makes every fetched register a phi at the join, and the copies
  // the compiler puts there wait for ALL gathers before the MFMA phase -- exactly the stall the pipeline removes.
  p.pos = pos, p.t = t, p.valid = pos < rr.end;
  const int64_t pc = p.valid ? pos : rr.end - 1;
  const int64_t ray = order ? (int64_t)order[pc] : pc;
  p.ray = ray;
  const int s = p.valid ? 64 * (t >> 2) + lane : lane;  // the tile's block, one sample per lane
  const int64_t si = ray * rr.stride + (s < rr.S ? s : rr.S - 1);
  if ((t & 3) == 0) {  // wave-uniform: entering a block (a tile inside one keeps the block's interval)
    p.t0 = rstarts[si];
    p.t1 = rends[si];
  }
  p.ox = ro[3 * ray], p.oy = ro[3 * ray + 1], p.oz = ro[3 * ray + 2];
  p.dx = rd[3 * ray], p.dy = rd[3 * ray + 1], p.dz = rd[3 * ray + 2];
  p.area = rarea[ray];
  p.ncand = cand_count ? cand_count[ray] : 0;
}

// Lay::Packed: the layout of PackedRaysDev (common.h) read through the kernel's own arguments (packed_launch_rays below):
// M = rr.S >= 1.  This pipeline clamps for itself -- the index of every load stays inside [0, M): a lane past the ray's end reads
// the ray's last sample; an empty segment gives b - 1 <= M - 1, which is -1 only for b == 0, where sample 0 stands in.
// The last clamp holds the reads inside the arrays even for segments that break their precondition.
__device__ __forceinline__ void load_pending_packed(PendingTile& p, int64_t pos, int t, const RayRange& rr, int lane,
                                                    const int32_t* __restrict__ order, const float* __restrict__ ro,
                                                    const float* __restrict__ rd, const float* __restrict__ rarea,
                                                    const float* __restrict__ rstarts, const float* __restrict__ rends,
                                                    const int64_t* __restrict__ segs, int& first, int& count,
                                                    const int32_t* __restrict__ cand_count = nullptr) {
  p.pos = pos, p.t = t, p.valid = pos < rr.end;
  const int64_t pc = p.valid ? pos : rr.end - 1;
  const int64_t ray = order ? (int64_t)order[pc] : pc;
  p.ray = ray;
  const int b = (int)segs[ray], n = (int)segs[ray + 1] - b;  // (M < 2^31)
  first = b, count = n;
  const int s = p.valid ? 64 * (t >> 2) + lane : lane;  // the tile's block, one sample per lane
  int si = b + (s < n ? s : n - 1);
  si = si < 0 ? 0 : si;
  si = si < rr.S ? si : rr.S - 1;
  if ((t & 3) == 0) {  // wave-uniform: entering a block (a tile inside one keeps the block's interval)
    p.t0 = rstarts[si];
    p.t1 = rends[si];
  }
  p.ox = ro[3 * ray], p.oy = ro[3 * ray + 1], p.oz = ro[3 * ray + 2];
  p.dx = rd[3 * ray], p.dy = rd[3 * ray + 1], p.dz = rd[3 * ray + 2];
  p.area = rarea[ray];
  p.ncand = cand_count ? cand_count[ray] : 0;  // (Lay::PackedActors)
}

// H2 + H3 + the hash of H1 for one pending tile, then all gathers issued back to back (no waits in here beyond the
// pending tile's own small loads, which were issued a whole tile earlier).
// hash_corners with the level's own multipliers and mask (eval_layout.hip): the reference hash for the levels that keep it,
// ix | iy << s | iz << 2s for the shadow levels -- one code path; the offsets are re-derived at blend time as before
__device__ __forceinline__ void layout_corners(float x, float y, float z, float scale, uint32_t my, uint32_t mz,
                                               uint32_t mask, uint32_t (&idx)[8]) {
  const float sx = __fmul_rn(x, scale), sy = __fmul_rn(y, scale), sz = __fmul_rn(z, scale);
  const uint32_t ifx = (uint32_t)(int)floorf(sx), ify = (uint32_t)(int)floorf(sy), ifz = (uint32_t)(int)floorf(sz);
  const uint32_t icx = (uint32_t)(int)ceilf(sx), icy = (uint32_t)(int)ceilf(sy), icz = (uint32_t)(int)ceilf(sz);
  const uint32_t hyc = icy * my, hyf = ify * my, hzc = icz * mz, hzf = ifz * mz;
  idx[0] = (icx ^ hyc ^ hzc) & mask;
  idx[1] = (icx ^ hyf ^ hzc) & mask;
  idx[2] = (ifx ^ hyf ^ hzc) & mask;
  idx[3] = (ifx ^ hyc ^ hzc) & mask;
  idx[4] = (icx ^ hyc ^ hzf) & mask;
  idx[5] = (icx ^ hyf ^ hzf) & mask;
  idx[6] = (ifx ^ hyf ^ hzf) & mask;
  idx[7] = (ifx ^ hyc ^ hzf) & mask;
}

template <int L, int F, bool HALF, bool RELAY = false>
__device__ __forceinline__ void issue_tile(const FieldDev& fd, const PendingTile& pt, int g, uint32_t mask,
                                           const float* scal_lds, TileFetch<EncFrame<L, F>::LPL, F>& tf,
                                           float* geo, int lane, const uint32_t* lay_lds = nullptr) {
  constexpr int LPL = EncFrame<L, F>::LPL;
  if ((pt.t & 3) == 0) fill_block<false>(geo, nullptr, lane, pt, fd.scale);  // wave-uniform: the block's first tile
  const int src = 16 * (pt.t & 3) + (lane & 15);  // lane 16 k + j holds this lane's sample
  const SamplePos p = get_block(geo, src);
  tf.t0 = from_lane(pt.t0, src << 2);
  tf.t1 = from_lane(pt.t1, src << 2);  // (tf.x .. tf.std stay unset: the blend reads the block's rows again)
  if (!EncFrame<L, F>::busy(g)) return;  // a lane group without levels (L < 4) loads nothing
#pragma unroll
  for (int q = 0; q < LPL; ++q) {
    if constexpr (RELAY) {
      const uint4 ly = *reinterpret_cast<const uint4*>(lay_lds + 4 * q);  // mulY, mulZ, mask, row0 of this lane's level
      uint32_t idx[8];
      layout_corners(p.x, p.y, p.z, scal_lds[q], ly.x, ly.y, ly.z, idx);
#pragma unroll
      for (int k = 0; k < 8; ++k) Entry<F, HALF>::load(fd.table, ly.w + idx[k], tf.fv[q][k]);
    } else {
      const Corners cs = hash_corners(p.x, p.y, p.z, scal_lds[q], mask);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        Entry<F, HALF>::load(fd.table, ((uint32_t)(LPL * g + q) << fd.grid.log2T) + cs.idx[k], tf.fv[q][k]);
    }
  }
}

// ACT: (1) the ray's candidate actors are walked -- a wave-uniform loop over scalar loads, empty for most rays -- and
// every lane notes the LAST candidate whose box contains its sample (ascending actor index: the highest wins,
// neurad_encoding.py:184-185 on CPU); (2) the static gathers go out for every lane exactly as above; (3) in the rare tile
// with a hit, the lanes inside a box re-issue their gathers against that actor's table, one wave-uniform pass per
// distinct winner, so the table base stays in SGPRs and the loads keep the SGPR-base + 32-bit-offset form.  Vector loads
// return in order: the later (actor) data is what the registers end up holding.  Nothing of (1)/(3) is live across the
// gathers on the common path except one register (the winning slot).
template <int L, int F, bool HALF>
__device__ __forceinline__ void issue_tile_actors(const FieldDev& fd, const ActorFieldDev& ad, const PendingTile& pt, int g,
                                                  uint32_t mask, const float* scal_lds, const float* ascal_lds,
                                                  const int32_t* __restrict__ cand_actor,
                                                  const float* __restrict__ cand_w2b, const float* __restrict__ bounds,
                                                  const void* const* __restrict__ tables,
                                                  TileFetch<EncFrame<L, F>::LPL, F>& tf, int& slot_out,
                                                  float* geo, float* ageo, int lane) {
  constexpr int LPL = EncFrame<L, F>::LPL;
  const bool busy = EncFrame<L, F>::busy(g);  // lanes of a group without levels load nothing
  const int n = __builtin_amdgcn_readfirstlane(pt.ncand);
  // 32-bit row index, made scalar explicitly: a 64-bit multiply has no scalar form
  const uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)pt.ray * (uint32_t)ad.K));
  // the block's geometry (all lanes active here: the cross-lane moves of the interval read every lane of the wave)
  if ((pt.t & 3) == 0) fill_block<true>(geo, ageo, lane, pt, fd.scale);
  const int src = 16 * (pt.t & 3) + (lane & 15);
  // this lane's sample: the gaussian, and its contraction in the static scene
  const SamplePos gs = get_block(ageo, src), ps = get_block(geo, src);
  tf.t0 = from_lane(pt.t0, src << 2);
  tf.t1 = from_lane(pt.t1, src << 2);
  int slot = -1;
  if (n > 0) {
    for (int c = 0; c < n; ++c) {
      const float* w = cand_w2b + (row + (uint32_t)c) * 12u;
      const int act = cand_actor[row + (uint32_t)c];
      const float bx = w[0] * gs.x + w[1] * gs.y + w[2] * gs.z + w[3];
      const float by = w[4] * gs.x + w[5] * gs.y + w[6] * gs.z + w[7];
      const float bz = w[8] * gs.x + w[9] * gs.y + w[10] * gs.z + w[11];
      if (fabsf(bx) < bounds[3 * act] && fabsf(by) < bounds[3 * act + 1] && fabsf(bz) < bounds[3 * act + 2]) slot = c;
    }
  }
  slot_out = slot;
  unsigned long long todo = __ballot(slot >= 0);
  const uint32_t amask = (1u << ad.log2T) - 1u;
  while (todo) {  // rare: the lanes inside a box, one pass per distinct winner
    const int c = __builtin_amdgcn_readlane(slot, (int)__builtin_ctzll(todo));
    const bool mine = slot == c;
    todo &= ~__ballot(mine);
    const float* w = cand_w2b + (row + (uint32_t)c) * 12u;
    const int act = cand_actor[row + (uint32_t)c];
    const void* tb = tables[act];  // scalar load: the table base stays in SGPRs
    if (mine) {
      const float bx = w[0] * gs.x + w[1] * gs.y + w[2] * gs.z + w[3];
      const float by = w[4] * gs.x + w[5] * gs.y + w[6] * gs.z + w[7];
      const float bz = w[8] * gs.x + w[9] * gs.y + w[10] * gs.z + w[11];
      const SamplePos p = contract_gaussian(bx, by, bz, gs.std, ad.scale);
      tf.x = p.x, tf.y = p.y, tf.z = p.z, tf.std = p.std;
      if (busy) {
#pragma unroll
        for (int q = 0; q < LPL; ++q) {
          // levels beyond the actor grid are the zero padding of F.pad (neurad_encoding.py:183): their fetch goes to the
          // last actor level and is weighted 0 at the blend
          const int lv = LPL * g + q, alv = lv < ad.La ? lv : ad.La - 1;
          const Corners cs = hash_corners(p.x, p.y, p.z, ascal_lds[alv], amask);
#pragma unroll
          for (int k = 0; k < 8; ++k) Entry<F, HALF>::load(tb, ((uint32_t)alv << ad.log2T) + cs.idx[k], tf.fv[q][k]);
        }
      }
    }
  }
  // the static scene: the lanes outside every box, i.e. all lanes of nearly every tile.  Issued LAST so that whatever
  // bookkeeping the compiler attaches to the rare passes above (waits, copies) sits in front of these gathers, where
  // nothing is in flight, and not between them and the MLPs.
  if (slot < 0) {
    const SamplePos p = ps;
    tf.x = p.x, tf.y = p.y, tf.z = p.z, tf.std = p.std;
    if (busy) {
#pragma unroll
      for (int q = 0; q < LPL; ++q) {
        const Corners cs = hash_corners(p.x, p.y, p.z, scal_lds[q], mask);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          Entry<F, HALF>::load(fd.table, ((uint32_t)(LPL * g + q) << fd.grid.log2T) + cs.idx[k], tf.fv[q][k]);
      }
    }
  }
}

// ACT, tile with a hit: a sample inside an actor box sees the view direction in the box frame (neurad_encoding.py:203-208),
// so the tile takes its SH inputs per sample.  -> this lane's B values of the four extra k-steps of feat layer 0: SH
// components 4g..4g+3 of its sample's direction.  One wave-uniform pass per distinct winning actor (scalar loads of w2b).
__device__ __forceinline__ void actor_tile_sh(int slot, uint32_t row, int g, float dx, float dy, float dz,
                                              const float* __restrict__ cand_w2b, float (&shb)[4]) {
  float bx = dx, by = dy, bz = dz;
  unsigned long long todo = __ballot(slot >= 0);
  while (todo) {
    const int c = __builtin_amdgcn_readlane(slot, (int)__builtin_ctzll(todo));
    const bool mine = slot == c;
    todo &= ~__ballot(mine);
    const float* w = cand_w2b + (row + (uint32_t)c) * 12u;
    const float ddx = w[0] * dx + w[1] * dy + w[2] * dz;
    const float ddy = w[4] * dx + w[5] * dy + w[6] * dz;
    const float ddz = w[8] * dx + w[9] * dy + w[10] * dz;
    const float nn = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz) + 1e-7f;  // neurad_encoding.py:207
    if (mine) bx = ddx / nn, by = ddy / nn, bz = ddz / nn;
  }
  float sh[16];
  sh4((bx + 1.f) / 2.f, (by + 1.f) / 2.f, (bz + 1.f) / 2.f, sh);
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if ((c >> 2) == g) shb[c & 3] = sh[c];
}

template <int L, int F>
__device__ __forceinline__ void blend_tile_actors(const TileFetch<EncFrame<L, F>::LPL, F>& tf, int slot, int g, int La,
                                                  const float* scal_lds, const float* ascal_lds, float (&feat)[8]) {
  using EF = EncFrame<L, F>;
  constexpr int LPL = EF::LPL;
  const bool in_box = slot >= 0;
#pragma unroll
  for (int q = 0; q < LPL; ++q) {
    const int lv = LPL * g + q, alv = lv < La ? lv : La - 1;
    const float sc = in_box ? ascal_lds[alv] : scal_lds[q];
    Corners c;
    const float sx = __fmul_rn(tf.x, sc), sy = __fmul_rn(tf.y, sc), sz = __fmul_rn(tf.z, sc);
    c.ox = __fsub_rn(sx, floorf(sx)), c.oy = __fsub_rn(sy, floorf(sy)), c.oz = __fsub_rn(sz, floorf(sz));
    float v[F];
    lerp_corners<F>(c, tf.fv[q], v);
    const float rw = (in_box && lv >= La) ? 0.f : rescale_weight(sc, tf.std);
#pragma unroll
    for (int f = 0; f < F; ++f) feat[q * F + f] = EF::busy(g) ? v[f] * rw : 0.f;
  }
#pragma unroll
  for (int k = EF::W; k < 8; ++k) feat[k] = 0.f;  // padding slots of the frame
}

template <int L, int F>
__device__ __forceinline__ void blend_tile(const TileFetch<EncFrame<L, F>::LPL, F>& tf, const SamplePos& p, int g,
                                           const float* scal_lds, float (&feat)[8]) {
  using EF = EncFrame<L, F>;
  constexpr int LPL = EF::LPL;
#pragma unroll
  for (int q = 0; q < LPL; ++q) {
    const float sc = scal_lds[q];
    Corners c;  // offsets rounded exactly as hash_corners does (encodings.py:431-446)
    const float sx = __fmul_rn(p.x, sc), sy = __fmul_rn(p.y, sc), sz = __fmul_rn(p.z, sc);
    c.ox = __fsub_rn(sx, floorf(sx)), c.oy = __fsub_rn(sy, floorf(sy)), c.oz = __fsub_rn(sz, floorf(sz));
    float v[F];
    lerp_corners<F>(c, tf.fv[q], v);
    const float rw = rescale_weight(sc, p.std);
#pragma unroll
    for (int f = 0; f < F; ++f) feat[q * F + f] = EF::busy(g) ? v[f] * rw : 0.f;  // (idle groups fetched nothing)
  }
#pragma unroll
  for (int k = EF::W; k < 8; ++k) feat[k] = 0.f;  // padding slots of the frame
}

// L levels, F features/level (L*F <= 32, see EncFrame), H hidden width, HALF = fp16 table; OUT / SRC / PROD / LAY: the
// variant (render_variants.h).  Lay::Packed takes the sample count M in `S` and the segments [R + 1] through `tables`
// (no new argument: the existing kernels keep their argument block), and composites as nrhip_packed_composite_fwd does:
// no sky-residual sample, depth over all samples, zeros for a ray without samples.  Lay::PackedActors is Lay::Packed with
// Src::Actors: `tables` is the actors' own, the segments come through `sv.enc`.  A lane past its ray's end holds the ray's
// last sample (load_pending_packed), so it walks the candidate list like a live lane and weighs nothing; the candidate
// row index is ray * K with ray < R, the slot < cand_count[ray] <= K: inside [0, R K), as in the dense actor kernel.
// Lay::PackedRowsOvr is Lay::PackedRows with Src::Overrides: the two features' argument slots do not collide (overrides in
// `cand_count` / `cand_w2b` / `bounds`, segments in `tables`), and ovr_row [M] is read at the packed sample index of a live
// lane only -- inside [0, M).
template <int L, int F, int H, bool HALF, Out OUT, Src SRC, Prod PROD, Lay LAY = Lay::Dense>
__global__ __launch_bounds__(256, 2) void render_kernel(
    FieldDev fd, int64_t n_rays, int S, int stride, const int32_t* __restrict__ order, const float* __restrict__ ro,
    const float* __restrict__ rd, const float* __restrict__ rarea, const float* __restrict__ rstarts,
    const float* __restrict__ rends, float* __restrict__ out_feat, float* __restrict__ out_depth,
    float* __restrict__ out_acc, float* __restrict__ out_w, float* __restrict__ out_sdf, float* __restrict__ out_alpha,
    SaveDev sv, float stop_eps, const int32_t* __restrict__ range, ActorFieldDev ad,
    const int32_t* __restrict__ cand_count,
    const int32_t* __restrict__ cand_actor, const float* __restrict__ cand_w2b, const float* __restrict__ bounds,
    const void* const* __restrict__ tables) {
  using EF = EncFrame<L, F>;  // (asserts L * F <= 32 in whole levels per lane group)
  static_assert(render_variant_ok(L, F, OUT, SRC, PROD, LAY), "not a legal variant: see render_variant_ok");
  static_assert(H % 16 == 0 && H >= 16 && H <= 128, "hidden width");
  constexpr bool COMPOSITE = OUT == Out::Composite;
  constexpr bool ACT = SRC == Src::Actors, RELAY = SRC == Src::EvalTable, OVR = SRC == Src::Overrides;
  constexpr bool PAIRS = PROD == Prod::F16Pairs;
  constexpr bool PACKED = LAY != Lay::Dense;  // (Packed / PackedActors: composited, PackedRows: per-sample rows)
  // PACKED: [R + 1].  The actor kernel needs `tables` for its table pointers: its segments travel in the first of the save
  // pointers, which no composited kernel reads
  const int64_t* const segs = LAY == Lay::PackedActors ? reinterpret_cast<const int64_t*>(sv.enc)
                                                       : reinterpret_cast<const int64_t*>(tables);
  const int32_t* const pcand = ACT ? cand_count : nullptr;  // PACKED: the candidate counts the pending tile reads
  // OVR (training forward of a scene with dynamic actors): samples inside an actor box take their encoding row and view
  // direction from the caller (the differentiable actor branch computed them for the few hit samples) instead of the
  // static lookup.  The three actor-only pointer arguments carry the overrides:
  const int32_t* const ovr_row = cand_count;  // [N] row index or -1
  const float* const ovr_rows = cand_w2b;     // [P, L*F]
  const float* const ovr_dirs = bounds;       // [P, 3]
  using Ld = Lds<H, PROD>;
  constexpr int NB = H / 16;
  constexpr int LPL = EF::LPL;       // levels per lane
  constexpr bool DEFER = COMPOSITE;  // last feature layer applied once per ray
  extern __shared__ __attribute__((aligned(16))) float lds[];

  // ---- stage weights (once per workgroup; the grid is persistent over rays) ----------------------
  stage_field_weights<L, F, H, PROD>(fd, lds);
  if constexpr (ACT || OVR) {
    for (int e = threadIdx.x; e < 16 * H; e += 256) lds[Ld::SHF + e] = frag_src<true, NB, 4>(fd.fw0 + 32, 48, 0, e);
  }
  if constexpr (ACT) {
    if (threadIdx.x < ad.La) lds[Ld::ASCAL + threadIdx.x] = ad.scal[threadIdx.x];
  }
  if constexpr (RELAY) {
    if (threadIdx.x < 4 * L) reinterpret_cast<uint32_t*>(lds + Ld::LAY)[threadIdx.x] = fd.lay[threadIdx.x];
  }
  __syncthreads();
  bool wbad = false;  // PAIRS: some weight does not fit its fp16 pair -> every tile takes the fp32 products
  if constexpr (PAIRS) wbad = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(lds)[Ld::FLG]) != 0;

  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const uint32_t mask = (1u << fd.grid.log2T) - 1u;
  const int ntile = (S + 15) >> 4;

  // XCD-coherent ranges of the processing order (see the header)
  const int nx = (int)gridDim.x < 8 ? (int)gridDim.x : 8;
  const int xcd = (int)blockIdx.x % nx, lb = (int)blockIdx.x / nx;
  const int nblk = ((int)gridDim.x - xcd + nx - 1) / nx;  // workgroups that share this range
  // `range` (device memory, optional): the slice [range[0], range[1]) of the processing order this launch renders -- a
  // scene with actors is rendered as two launches over one order, split on the device (nrhip_render_fwd_actors)
  const int64_t first = range ? range[0] : 0, count = range ? range[1] - range[0] : n_rays;
  const int64_t lo = first + count * xcd / nx;
  const RayRange rr{first + count * (xcd + 1) / nx, S, stride};
  const int64_t pos_step = (int64_t)nblk * 4;

  const float* scal_l = lds + Ld::SCAL + LPL * g;  // this lane's levels (re-read per tile: 1 ds_read, no VGPRs held)
  const uint32_t* lay_l = reinterpret_cast<const uint32_t*>(lds + Ld::LAY) + 4 * LPL * g;  // RELAY: their layout constants
  float* rbw = lds + Ld::RB + wid * H;              // this wave's per-ray bias row
  int64_t pos = lo + (int64_t)lb * 4 + wid;
  if (pos >= rr.end) return;
  int t = 0;
  // three-stage pipeline over this wave's flattened (ray, tile) sequence:
  //   tf = gathered corners of the CURRENT tile | q = next tile (interval + ray constants loaded, gathers not yet
  //   issued) | the tile after q has its small loads requested at the end of the issue step
  TileFetch<LPL, F> tf;
  if constexpr (!EF::FULL) tf = TileFetch<LPL, F>{};  // (the idle lane groups never load theirs)
  int ta = -1;  // ACT: candidate slot of the actor containing this lane's sample of the tile in `tf` (-1: none)
  const float* ascal_l = lds + Ld::ASCAL;
  PendingTile q;
  // geometry of the block q's tile lies in, this wave's rows (written at the block's first tile: fill_block)
  float* geo_w = lds + Ld::GEO + wid * kBlockGeo;
  float* ageo_w = lds + (ACT ? Ld::AGEO : Ld::GEO) + wid * kBlockGeo;  // (only ACT kernels carve and touch AGEO)
  int qb = 0, qn = 0;  // PACKED: first sample and sample count of q's ray (wave-uniform)
  auto tiles_of = [](int n) { return n > 16 ? (n + 15) >> 4 : 1; };  // PACKED: a ray without samples walks one dead tile
  if constexpr (PACKED) load_pending_packed(q, pos, 0, rr, lane, order, ro, rd, rarea, rstarts, rends, segs, qb, qn, pcand);
  else load_pending(q, pos, 0, rr, lane, order, ro, rd, rarea, rstarts, rends, cand_count);
  int64_t ray = q.ray;
  int cb = 0, cn = 0;  // PACKED: first sample and sample count of the ray in `tf`
  if constexpr (PACKED) cb = qb, cn = qn;
  if constexpr (ACT) issue_tile_actors<L, F, HALF>(fd, ad, q, g, mask, scal_l, ascal_l, cand_actor, cand_w2b, bounds, tables, tf, ta, geo_w, ageo_w, lane);
  else issue_tile<L, F, HALF, RELAY>(fd, q, g, mask, scal_l, tf, geo_w, lane, lay_l);
  // override row of this lane's sample of `tf` (PACKED: at the packed sample index; q's segment is still qb / qn here)
  if constexpr (OVR && PACKED) ta = (q.valid && j < qn && qb + j >= 0 && qb + j < S) ? ovr_row[qb + j] : -1;
  else if constexpr (OVR) ta = (q.valid && j < S) ? ovr_row[q.ray * S + j] : -1;
  {
    const bool wrap = (PACKED ? tiles_of(cn) : ntile) == 1;
    if constexpr (PACKED) load_pending_packed(q, wrap ? pos + pos_step : pos, wrap ? 0 : 1, rr, lane, order, ro, rd, rarea, rstarts, rends, segs, qb, qn, pcand);
    else load_pending(q, wrap ? pos + pos_step : pos, wrap ? 0 : 1, rr, lane, order, ro, rd, rarea, rstarts, rends, cand_count);
  }

  // per-ray state
  f32x4 shq = f32x4{0.f, 0.f, 0.f, 0.f};
  float carry = 0.f, acc_w = 0.f, acc_d = 0.f;
  constexpr int NHA = DEFER ? H / 4 : 1;
  float ha[NHA];  // DEFER: sum_s w_s * h2_s (this lane's sample column)
  f32x4 fa[2];    // DEFER: sum_s w_s * geo_embedding_s

  while (true) {
    if (t == 0) {
      // per-ray part of feat layer 0:  rb[n] = fb0[n] + sum_c fw0[n][32+c] * SH_c((d+1)/2)   (neurad_field.py:140-141)
      const float dx = rd[3 * ray], dy = rd[3 * ray + 1], dz = rd[3 * ray + 2];
      float sh[16];
      sh4((dx + 1.f) / 2.f, (dy + 1.f) / 2.f, (dz + 1.f) / 2.f, sh);
      if constexpr (!COMPOSITE) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if ((c >> 2) == g) shq[c & 3] = sh[c];
      }
      f32x4 rb[NB];
#pragma unroll
      for (int mb = 0; mb < NB; ++mb) rb[mb] = *reinterpret_cast<const f32x4*>(lds + Ld::BF0 + 16 * mb + 4 * g);
#pragma unroll
      for (int c = 0; c < 16; ++c)
#pragma unroll
        for (int mb = 0; mb < NB; ++mb) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(lds + Ld::SHW + c * H + 16 * mb + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) rb[mb][r] = fmaf(w[r], sh[c], rb[mb][r]);
        }
      // parked in this wave's LDS row (the 16 lanes of a DPP row hold identical copies; every lane stores its own ->
      // same value to the same address) and re-read as the accumulator init of feat layer 0 in every tile
#pragma unroll
      for (int mb = 0; mb < NB; ++mb) *reinterpret_cast<f32x4*>(rbw + 16 * mb + 4 * g) = rb[mb];
      carry = COMPOSITE ? (fd.use_sdf ? 1.f : 0.f) : 0.f;  // running transmittance (product) / optical depth (sum)
      acc_w = 0.f, acc_d = 0.f;
      fa[0] = fa[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NHA; ++k) ha[k] = 0.f;
    }

    // The weights in LDS are loop invariant: without this opaque offset the compiler hoists ~200 LDS
    // loads out of the tile loop and spills them.  `lw` re-derives the LDS base once per tile.
    int opaque = 0;
    asm volatile("" : "+v"(opaque));
    const float* lw = lds + opaque;
    const int s = 16 * t + j;
    const bool live = s < (PACKED ? cn : S);
    const float t0 = tf.t0, t1 = tf.t1;

    // ---- blend the fetched corners (H1 + H4): the only wait on the gathers ---------------------------
    float feat[8];
    bool tile_hit = false;
    float shb[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (ACT) {
      blend_tile_actors<L, F>(tf, ta, g, ad.La, scal_l, ascal_l, feat);
      tile_hit = __ballot(ta >= 0) != 0ull;  // wave-uniform
      if (tile_hit)  // here, where few registers are live -- not in the middle of the MLPs
        actor_tile_sh(ta, (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)ray * (uint32_t)ad.K)), g, rd[3 * ray],
                      rd[3 * ray + 1], rd[3 * ray + 2], cand_w2b, shb);
    } else {
      // position / std of this tile's samples: still in the block's LDS rows (the issue step below is what overwrites
      // them, when the NEXT tile opens a block), so no register carries them across the MLPs
      blend_tile<L, F>(tf, get_block(geo_w, 16 * (t & 3) + j), g, scal_l, feat);
      if constexpr (PAIRS) {
#pragma unroll
        for (int k = 0; k < 8; ++k) feat[k] *= kPairAct;
      }
      if constexpr (OVR) {
        tile_hit = __ballot(ta >= 0) != 0ull;  // wave-uniform; rare
        if (tile_hit) {
          float bx = rd[3 * ray], by = rd[3 * ray + 1], bz = rd[3 * ray + 2];
          if (ta >= 0) {
            const float* rp = ovr_rows + (size_t)ta * EF::LF + EF::W * g;  // this lane's columns of the override row
            if constexpr (EF::FULL) {
              const f32x4 r0 = *reinterpret_cast<const f32x4*>(rp), r1 = *reinterpret_cast<const f32x4*>(rp + 4);
#pragma unroll
              for (int k = 0; k < 4; ++k) feat[k] = r0[k], feat[4 + k] = r1[k];
            } else if (EF::busy(g)) {  // (the padding slots stay 0)
#pragma unroll
              for (int k = 0; k < EF::W; ++k) feat[k] = rp[k];
            }
            bx = ovr_dirs[3 * (size_t)ta], by = ovr_dirs[3 * (size_t)ta + 1], bz = ovr_dirs[3 * (size_t)ta + 2];
          }
          float sh[16];
          sh4((bx + 1.f) / 2.f, (by + 1.f) / 2.f, (bz + 1.f) / 2.f, sh);
#pragma unroll
          for (int c = 0; c < 16; ++c)
            if ((c >> 2) == g) shb[c & 3] = sh[c];
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- early ray termination (eval option): the transmittance ENTERING this tile is already below stop_eps, so
    // everything behind it weighs less than stop_eps in total -> this (already fetched) tile is the ray's last.
    // The test lags one tile behind the carry so that the fetch below never has to be re-issued.
    bool stop_here = false;
    if constexpr (COMPOSITE) {
      if (stop_eps > 0.f) {
        const float c = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, carry)));
        stop_here = fd.use_sdf ? (c < stop_eps) : (c > -__logf(stop_eps));  // wave-uniform -> scalar branch
      }
    }
    const bool last_tile = t == (PACKED ? tiles_of(cn) : ntile) - 1;
    const bool ray_done = last_tile || stop_here;

    // ---- issue the next tile's gathers: they fly while this tile runs through the MLPs ---------------
    if (ray_done && q.valid && q.pos == pos) {  // terminated early: q still points into this ray -> skip to the next ray
      // (one exposed round trip)
      if constexpr (PACKED) load_pending_packed(q, pos + pos_step, 0, rr, lane, order, ro, rd, rarea, rstarts, rends, segs, qb, qn, pcand);
      else load_pending(q, pos + pos_step, 0, rr, lane, order, ro, rd, rarea, rstarts, rends, cand_count);
    }
    const bool have_next = q.valid;
    const int64_t npos = q.pos, nray = q.ray;
    const int nt = q.t;
    int nb = 0, nn = 0;
    if constexpr (PACKED) nb = qb, nn = qn;
    // unconditional (see load_pending)
    if constexpr (ACT) issue_tile_actors<L, F, HALF>(fd, ad, q, g, mask, scal_l, ascal_l, cand_actor, cand_w2b, bounds, tables, tf, ta, geo_w, ageo_w, lane);
    else issue_tile<L, F, HALF, RELAY>(fd, q, g, mask, scal_l, tf, geo_w, lane, lay_l);
    if constexpr (OVR && PACKED) {
      const int s2 = 16 * q.t + j;
      ta = (q.valid && s2 < qn && qb + s2 >= 0 && qb + s2 < S) ? ovr_row[qb + s2] : -1;
    } else if constexpr (OVR) {
      ta = (q.valid && 16 * q.t + j < S) ? ovr_row[q.ray * S + 16 * q.t + j] : -1;
    }
    {
      const bool wrap = nt + 1 == (PACKED ? tiles_of(nn) : ntile);  // request the small loads of the tile after it
      if constexpr (PACKED)
        load_pending_packed(q, wrap ? npos + pos_step : npos, wrap ? 0 : nt + 1, rr, lane, order, ro, rd, rarea, rstarts, rends, segs, qb, qn, pcand);
      else
        load_pending(q, wrap ? npos + pos_step : npos, wrap ? 0 : nt + 1, rr, lane, order, ro, rd, rarea, rstarts, rends,
                     cand_count);
    }
    __builtin_amdgcn_sched_barrier(0);

    if constexpr (PACKED) {
      if (cn <= 0) {  // wave-uniform: a ray without samples writes its zeros (per-sample output: nothing) and runs no MLP
        if (COMPOSITE && j == 0) {
          float* fp = out_feat + ray * 32;
          *reinterpret_cast<f32x4*>(fp + 4 * g) = f32x4{0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<f32x4*>(fp + 16 + 4 * g) = f32x4{0.f, 0.f, 0.f, 0.f};
          if (g == 0) {
            out_acc[ray] = 0.f;
            out_depth[ray] = 0.f;
          }
        }
        if (!have_next) break;
        pos = npos, ray = nray, t = nt, cb = nb, cn = nn;
        continue;
      }
    }

    bool saving = false;
    int64_t srow = 0;
    if constexpr (!COMPOSITE) {
      saving = sv.enc != nullptr && live;
      srow = PACKED ? (int64_t)cb + s : ray * S + s;  // (PACKED: the packed sample index; the ray constants stay per ray)
      if (saving) {
        constexpr float u = PAIRS ? 1.f / kPairAct : 1.f;  // (tile units -> true units: a power of two, exact)
        float* ep = sv.enc + srow * EF::LF + EF::W * g;  // dense [N, L*F]: this lane group's W columns
        if constexpr (EF::FULL) {
          stream_store(ep, f32x4{feat[0] * u, feat[1] * u, feat[2] * u, feat[3] * u});
          stream_store(ep + 4, f32x4{feat[4] * u, feat[5] * u, feat[6] * u, feat[7] * u});
        } else if (EF::busy(g)) {
          if constexpr (EF::W == 4) {
            stream_store(ep, f32x4{feat[0] * u, feat[1] * u, feat[2] * u, feat[3] * u});
          } else {
#pragma unroll
            for (int k = 0; k < EF::W; ++k) __builtin_nontemporal_store(feat[k] * u, ep + k);
          }
        }
      }
    }

    // ---- geo MLP layer 0 (L*F in the 32-slot frame -> H, ReLU) -----------------------------------
    f32x4 h[NB];
#pragma unroll
    for (int mb = 0; mb < NB; ++mb) h[mb] = *reinterpret_cast<const f32x4*>(lw + Ld::BG0 + 16 * mb + 4 * g);
    tile_layer<PROD, false>(lw + Ld::G0, fd.gw0, EF::LF, 0, wbad, lane, feat, h);
    float hb[H / 4];
#pragma unroll
    for (int mb = 0; mb < NB; ++mb)
#pragma unroll
      for (int r = 0; r < 4; ++r) hb[4 * mb + r] = fmaxf(h[mb][r], 0.f);

    if constexpr (!COMPOSITE) {
      if (saving) {
        constexpr float u = PAIRS ? 1.f / kPairAct : 1.f;
#pragma unroll
        for (int mb = 0; mb < NB; ++mb)
          stream_store(sv.hg + srow * H + 16 * mb + 4 * g,
                       f32x4{hb[4 * mb] * u, hb[4 * mb + 1] * u, hb[4 * mb + 2] * u, hb[4 * mb + 3] * u});
      }
    }

    // ---- geo MLP layer 1 (H -> 1 + 32): row 0 (sdf / raw density) on the VALU, rows 1..32 on MFMA --
    float sdf = 0.f;
#pragma unroll
    for (int mb = 0; mb < NB; ++mb) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(lw + Ld::SDFW + 16 * mb + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) sdf = fmaf(w[r], hb[4 * mb + r], sdf);
    }
    sdf += __shfl_xor(sdf, 16, 64);
    sdf += __shfl_xor(sdf, 32, 64);
    sdf += lw[Ld::BG1];
    f32x4 e[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const float* bp = lw + Ld::BG1 + 1 + 16 * mb + 4 * g;
      e[mb] = f32x4{bp[0], bp[1], bp[2], bp[3]};
    }
    tile_layer<PROD, true>(lw + Ld::G1, fd.gw1, H, 1, wbad, lane, hb, e);
    float eb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) eb[k] = e[k >> 2][k & 3];

    // ---- feature MLP (32 [+16 SH folded into the per-ray bias] -> H -> H -> 32), residual add ------
    if constexpr (!COMPOSITE) {
      if (saving) {
        constexpr float u = PAIRS ? 1.f / kPairAct : 1.f;
        float* xp = sv.xf + srow * 48;
        stream_store(xp + 4 * g, e[0] * u);
        stream_store(xp + 16 + 4 * g, e[1] * u);
        stream_store(xp + 32 + 4 * g, tile_hit ? f32x4{shb[0], shb[1], shb[2], shb[3]} : shq);
      }
    }
    if (!tile_hit) {
#pragma unroll
      for (int mb = 0; mb < NB; ++mb) h[mb] = *reinterpret_cast<const f32x4*>(lw + Ld::RB + wid * H + 16 * mb + 4 * g);
    } else {
      // per-sample SH inputs (actor_tile_sh): four more k-steps instead of the per-ray bias row
#pragma unroll
      for (int mb = 0; mb < NB; ++mb) h[mb] = *reinterpret_cast<const f32x4*>(lw + Ld::BF0 + 16 * mb + 4 * g);
      mfma_layer<NB, 4>(lw + Ld::SHF, lane, shb, h);
    }
    tile_layer<PROD, true>(lw + Ld::F0, fd.fw0, 48, 0, wbad, lane, eb, h);
#pragma unroll
    for (int mb = 0; mb < NB; ++mb)
#pragma unroll
      for (int r = 0; r < 4; ++r) hb[4 * mb + r] = fmaxf(h[mb][r], 0.f);
    if constexpr (!COMPOSITE) {
      if (saving) {
        constexpr float u = PAIRS ? 1.f / kPairAct : 1.f;
#pragma unroll
        for (int mb = 0; mb < NB; ++mb)
          stream_store(sv.hf + srow * (2 * H) + 16 * mb + 4 * g,
                       f32x4{hb[4 * mb] * u, hb[4 * mb + 1] * u, hb[4 * mb + 2] * u, hb[4 * mb + 3] * u});
      }
    }
#pragma unroll
    for (int mb = 0; mb < NB; ++mb) h[mb] = *reinterpret_cast<const f32x4*>(lw + Ld::BF1 + 16 * mb + 4 * g);
    tile_layer<PROD, true>(lw + Ld::F1, fd.fw1, H, 0, wbad, lane, hb, h);
#pragma unroll
    for (int mb = 0; mb < NB; ++mb)
#pragma unroll
      for (int r = 0; r < 4; ++r) hb[4 * mb + r] = fmaxf(h[mb][r], 0.f);
    if constexpr (!COMPOSITE) {
      if (saving) {
        constexpr float u = PAIRS ? 1.f / kPairAct : 1.f;
#pragma unroll
        for (int mb = 0; mb < NB; ++mb)
          stream_store(sv.hf + srow * (2 * H) + H + 16 * mb + 4 * g,
                       f32x4{hb[4 * mb] * u, hb[4 * mb + 1] * u, hb[4 * mb + 2] * u, hb[4 * mb + 3] * u});
      }
    }

    // ---- head (F4 / trunc_exp) -------------------------------------------------------------------
    float a_or_d;  // alpha (sdf mode) or density
    if (fd.use_sdf) a_or_d = __builtin_amdgcn_rcpf(1.f + __expf(sdf * fd.beta));  // sigmoid(-sdf*beta)
    else a_or_d = expf(sdf);

    if constexpr (!COMPOSITE) {
      // per-sample output: feature = geo_embedding + mlp_feature(...)   (neurad_field.py:141)
      f32x4 o[2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) o[mb] = *reinterpret_cast<const f32x4*>(lw + Ld::BF2 + 16 * mb + 4 * g);
      mfma_layer<2, H / 4>(lw + Ld::F2, lane, hb, o);  // (PAIRS: fw2 is staged x 1 / kPairAct -- true units)
      if constexpr (PAIRS) {
        o[0] += e[0] * (1.f / kPairAct);
        o[1] += e[1] * (1.f / kPairAct);
      } else {
        o[0] += e[0];
        o[1] += e[1];
      }
      if (live) {
        const int64_t si = PACKED ? (int64_t)cb + s : ray * S + s;
        float* fp = out_feat + si * 32;
        stream_store(fp + 4 * g, o[0]);
        stream_store(fp + 16 + 4 * g, o[1]);
        if (g == 0) {
          out_sdf[si] = sdf;
          out_alpha[si] = a_or_d;
        }
      }
    } else {
      // ---- C1: transmittance scan over the 16 samples of the DPP row, carried across tiles -------
      float w, T;
      if (fd.use_sdf) {
        const float alpha = live ? a_or_d : 0.f;
        float incl = 1.f - alpha;
        incl *= row_shr<1>(incl, 1.f);
        incl *= row_shr<2>(incl, 1.f);
        incl *= row_shr<4>(incl, 1.f);
        incl *= row_shr<8>(incl, 1.f);
        const float excl = row_shr<1>(incl, 1.f);
        T = carry * excl;
        w = T * alpha;
        carry *= __shfl(incl, (lane & 48) | 15, 64);
      } else {
        const float sd = live ? a_or_d * (t1 - t0) : 0.f;
        float incl = sd;
        incl += row_shr<1>(incl, 0.f);
        incl += row_shr<2>(incl, 0.f);
        incl += row_shr<4>(incl, 0.f);
        incl += row_shr<8>(incl, 0.f);
        const float excl = row_shr<1>(incl, 0.f);
        T = expf(-(carry + excl));
        w = T * (1.f - expf(-sd));
        carry += __shfl(incl, (lane & 48) | 15, 64);
      }
      if (out_w && live && g == 0) out_w[PACKED ? (int64_t)cb + s : ray * S + s] = w;
      // ---- C2 accumulation ------------------------------------------------------------------------
      acc_w += w;
      if (PACKED || s < S - 1) acc_d += w * ((t0 + t1) / 2.f);  // (PACKED: every sample; a dead lane has w = 0)
      float wf = w;  // weight of this sample's FEATURES: the sky residual 1 - sum w goes on sample S-1 (not PACKED)
      float acc = 0.f;
      if (ray_done) {
        acc = row_sum16(acc_w);
        if constexpr (!PACKED) {
          if (last_tile && s == S - 1) wf += 1.f - acc;
        }
      }
#pragma unroll
      for (int k = 0; k < H / 4; ++k) ha[k] = fmaf(hb[k], wf, ha[k]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        fa[0][r] = fmaf(e[0][r], wf, fa[0][r]);
        fa[1][r] = fmaf(e[1][r], wf, fa[1][r]);
      }

      if (ray_done) {
        const float dep = row_sum16(acc_d);
        if (!last_tile && out_w)  // terminated early: the rest of the ray contributes nothing
          for (int s2 = 16 * (t + 1) + lane; s2 < (PACKED ? cn : S); s2 += 64)
            out_w[(PACKED ? (int64_t)cb : ray * S) + s2] = 0.f;
        // features = fw2 . (sum w h2) + fb2 * sum w' + sum w' e ;  sum w' = acc + (1 - acc) on a completed ray (PACKED: acc)
        const float wsum = (!PACKED && last_tile) ? acc + (1.f - acc) : acc;
        f32x4 of2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        mfma_layer<2, H / 4>(lw + Ld::F2, lane, ha, of2);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          const f32x4 b2 = *reinterpret_cast<const f32x4*>(lw + Ld::BF2 + 16 * mb + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float es = PAIRS ? fa[mb][r] * (1.f / kPairAct) : fa[mb][r];  // (the embedding sum ran in tile units)
            of2[mb][r] = fmaf(b2[r], wsum, row_sum16(of2[mb][r] + es));
          }
        }
        if (j == 0) {
          float* fp = out_feat + ray * 32;
          *reinterpret_cast<f32x4*>(fp + 4 * g) = of2[0];
          *reinterpret_cast<f32x4*>(fp + 16 + 4 * g) = of2[1];
          if (g == 0) {
            out_acc[ray] = acc;
            out_depth[ray] = dep;
          }
        }
      }
    }

    if (!have_next) break;
    pos = npos, ray = nray, t = nt;
    if constexpr (PACKED) cb = nb, cn = nn;
  }
}

// ---- host side: which variant, and its launch -----------------------------------------------------------------------
struct Variant {  // one row of render_variants.h
  int L, F, H;
  Out out;
  Src src;
  Prod prod;
};
constexpr Variant kVariants[] = {
#define X(L_, F_, H_, O_, S_, P_) {L_, F_, H_, Out::O_, Src::S_, Prod::P_},
    NRHIP_RENDER_VARIANTS(X)
#undef X
};

static bool same(const Variant& a, const Variant& b) {
  return a.L == b.L && a.F == b.F && a.H == b.H && a.out == b.out && a.src == b.src && a.prod == b.prod;
}
static bool has_variant(const Variant& v) {
  for (const Variant& r : kVariants)
    if (same(r, v)) return true;
  return false;
}

static int validate_field(const nrhip_field* f) {
  NR_REQUIRE(f, NRHIP_ERR_INVALID_ARG, "field descriptor is NULL");
  if (int e = validate_grid(&f->grid)) return e;
  NR_REQUIRE(f->table && f->static_scale > 0.f, NRHIP_ERR_INVALID_ARG, "field: NULL table or non-positive scale");
  const nrhip_mlp& a = f->geo;
  const nrhip_mlp& b = f->feat;
  const int L = f->grid.num_levels, F = f->grid.n_features, in = L * F;
  // (the table holds every static fp32 shape for both outputs: tests/test_fused_shapes_gate.py)
  NR_REQUIRE(has_variant({L, F, a.hidden_dim, Out::Composite, Src::Static, Prod::F32}), NRHIP_ERR_UNSUPPORTED,
             "fused field kernel: no instantiation for L=%d F=%d H=%d (the grids and hidden widths: csrc/render_variants.h); "
             "use the unfused ops",
             L, F, a.hidden_dim);
  NR_REQUIRE(a.num_layers == 2 && b.num_layers == 3 && a.in_dim == in && a.out_dim == 33 && b.in_dim == 48 &&
                 b.out_dim == 32 && a.hidden_dim == b.hidden_dim,
             NRHIP_ERR_UNSUPPORTED,
             "fused field kernel needs geo L*F->H->33 (2 layers, L*F=%d) and feat 48->H->H->32 (3 layers); use the "
             "unfused ops",
             in);
  for (int l = 0; l < 2; ++l) NR_REQUIRE(a.weight[l], NRHIP_ERR_INVALID_ARG, "geo weight %d is NULL", l);
  for (int l = 0; l < 3; ++l) NR_REQUIRE(b.weight[l], NRHIP_ERR_INVALID_ARG, "feat weight %d is NULL", l);
  return NRHIP_OK;
}

static FieldDev to_dev(const nrhip_field& f) {
  FieldDev d;
  d.grid = to_dev(f.grid);
  d.table = f.table;
  d.scale = f.static_scale;
  d.gw0 = f.geo.weight[0], d.gb0 = f.geo.bias[0];
  d.gw1 = f.geo.weight[1], d.gb1 = f.geo.bias[1];
  d.fw0 = f.feat.weight[0], d.fb0 = f.feat.bias[0];
  d.fw1 = f.feat.weight[1], d.fb1 = f.feat.bias[1];
  d.fw2 = f.feat.weight[2], d.fb2 = f.feat.bias[2];
  d.use_sdf = f.use_sdf;
  d.beta = f.beta;
  for (int i = 0; i < NRHIP_MAX_LEVELS * 4; ++i)
    d.lay[i] = (f.eval_table && f.eval_layout && i < 4 * f.grid.num_levels) ? f.eval_layout[i] : 0u;
  return d;
}

// the candidate lists + actor tables a Src::Actors launch reads (all device pointers)
struct ActorLaunch {
  ActorFieldDev ad;
  const int32_t* cand_count;
  const int32_t* cand_actor;
  const float* cand_w2b;
  const float* bounds;
  const void* const* tables;
};
// the caller's rows a Src::Overrides launch reads (device pointers)
struct OverrideLaunch {
  const int32_t* row;  // [N] row index of the sample, or -1
  const float* rows;   // [P, L*F]
  const float* dirs;   // [P, 3]
};
// What a launch hands to the kernel beside the field and the rays, whatever the variant (value-initialise: all off)
struct RenderArgs {
  float *feat, *depth, *acc, *w;  // composited: w optional | per-sample: feat, sdf, alpha
  float *sdf, *alpha;
  SaveDev sv;
  float stop_eps;
  const int32_t* range;  // [2] device: slice of the processing order (NULL = all rays)
  const int64_t* segments;  // Lay::Packed: [R + 1] device
  ActorLaunch actors;
  OverrideLaunch ovr;
  hipStream_t stream;
};

template <int L, int F, int H, bool HALF, Out OUT, Src SRC, Prod PROD, Lay LAY = Lay::Dense>
static int launch_render(const FieldDev& fd, const RaysDev& rd, const RenderArgs& a) {
  constexpr bool OVR = SRC == Src::Overrides;
  constexpr bool PACKED = LAY == Lay::Packed || LAY == Lay::PackedRows || LAY == Lay::PackedRowsOvr;
  constexpr size_t lds = ((SRC == Src::Actors || OVR) ? Lds<H, PROD>::TOTAL_ACT : Lds<H, PROD>::TOTAL) * sizeof(float);
  auto kern = render_kernel<L, F, H, HALF, OUT, SRC, PROD, LAY>;
  static int cap = 0;  // persistent grid: CUs x resident workgroups per CU, queried once per instantiation
  if (!cap) {
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    int dev = 0, n_cu = 256, nb = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n_cu = p.multiProcessorCount;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)kern, 256, lds) != hipSuccess || nb < 1) nb = 2;
    cap = n_cu * (nb > 4 ? 4 : nb);
  }
  const int64_t want = (rd.R + 3) / 4;
  const int blocks = (int)(want < cap ? want : cap);
  const ActorLaunch& al = a.actors;
  SaveDev sv = a.sv;
  // (Lay::PackedActors: `tables` is taken, the segments go through the first save pointer -- read, never written)
  if constexpr (LAY == Lay::PackedActors) sv.enc = reinterpret_cast<float*>(const_cast<int64_t*>(a.segments));
  // (the override kernel reads its three arrays through the actor kernel's pointer arguments, the packed kernel its
  // segments through the last of them and M = rd.S: see render_kernel)
  kern<<<blocks, 256, lds, a.stream>>>(fd, rd.R, rd.S, rd.stride, rd.order, rd.o, rd.d, rd.area, rd.starts, rd.ends, a.feat,
                                       a.depth, a.acc, a.w, a.sdf, a.alpha, sv, a.stop_eps, a.range, al.ad,
                                       OVR ? a.ovr.row : al.cand_count, al.cand_actor, OVR ? a.ovr.rows : al.cand_w2b,
                                       OVR ? a.ovr.dirs : al.bounds,
                                       PACKED ? reinterpret_cast<const void* const*>(a.segments) : al.tables);
  return check_launch("render/field fused kernel");
}

// THE preference order among the variants of one (L, F, H, output).  Actors and overrides are the caller's choice (fp32
// products only); for the static scene the first of these that has a row in the table wins:
static Variant choose_variant(const nrhip_field* f, Out out, Src src) {
  const int L = f->grid.num_levels, F = f->grid.n_features, H = f->geo.hidden_dim;
  if (src != Src::Static) return {L, F, H, out, src, Prod::F32};
  const bool composite = out == Out::Composite;
  const bool split_bf16 = tuning().mlp_split_bf16;
  const bool pairs = tuning().mlp_pairs >= 0 ? tuning().mlp_pairs == 1 : kPairsDefault;
  const struct {
    bool on;
    Src src;
    Prod prod;
  } order[] = {
      // 1. eval table given (nrhip_field.eval_table / eval_layout): the coarse levels are read from their shadow copies.
      // Decided FIRST: a caller that hands the table over asked for this kernel; it exists with fp32-MFMA products only
      // (render_variant_ok: the relayout and the split / pair products do not combine), so it wins over the pair default.
      {composite && f->eval_table && f->eval_layout, Src::EvalTable, Prod::F32},
      // 2. NRHIP_MLP_PAIRS (default 1): the products as fp16 pairs (mfma_layer_pairs) in the composited kernels -- at H = 64,
      // and at NeuRAD's own width, where the arithmetic mostly hid under the memory time already (c2's render stage
      // 72 -> 60-67 us).  In the per-sample kernel (field forward / training forward with saved activations) the same pair
      // products are OPT-IN (NRHIP_MLP_PAIRS_TRAIN=1).  Round 6 measured no gain: the kernel stores 516 B of activations per
      // sample beside its gathers and is bound by them -- 1.03-1.09 ms with pairs against 1.01-1.03 ms with the fp32 MFMA on
      // the c3 batch, the step unchanged (profiles/r06_ab_pairs_train.txt)
      {pairs && !split_bf16 && (composite || tuning().mlp_pairs_train), Src::Static, Prod::F16Pairs},
      // 3. NRHIP_MLP_SPLIT_BF16=1 (64-wide MLPs, composited output): the per-tile matrix products run as 3-way split bf16
      // on the matrix cores (mfma_layer_split) instead of the fp32 MFMA.  Same results to fp32 accuracy; NOT the default
      // because it measured no faster (163 vs 163 us on config[1]: the splitting costs the vector ALU what the matrix pipe
      // saves -- DESIGN.md §9).
      {split_bf16 && composite, Src::Static, Prod::Bf16Split},
  };
  for (const auto& c : order)
    if (c.on && has_variant({L, F, H, out, c.src, c.prod})) return {L, F, H, out, c.src, c.prod};
  return {L, F, H, out, Src::Static, Prod::F32};  // 4. the fp32 MFMA
}

// The layout a variant takes on packed samples.  The packed kernels have no rows of their own in the table: a row is
// instantiated in this layout as well wherever render_variant_ok admits it.
constexpr Lay packed_lay(Out out, Src src) {
  return src == Src::Actors ? Lay::PackedActors
         : src == Src::Overrides ? Lay::PackedRowsOvr
         : out == Out::Composite ? Lay::Packed
                                 : Lay::PackedRows;
}

// One row of the table, for dense samples or (packed: rd.S carries M, a.segments the segments) in its packed layout
template <int L, int F, int H, bool HALF, Out OUT, Src SRC, Prod PROD>
static int launch_row(const char* who, bool packed, const FieldDev& fd, const RaysDev& rd, const RenderArgs& a) {
  if (!packed) return launch_render<L, F, H, HALF, OUT, SRC, PROD>(fd, rd, a);
  constexpr Lay LAY = packed_lay(OUT, SRC);
  if constexpr (render_variant_ok(L, F, OUT, SRC, PROD, LAY)) {
    return launch_render<L, F, H, HALF, OUT, SRC, PROD, LAY>(fd, rd, a);
  } else {
    set_error("%s: no packed form of this variant", who);
    return NRHIP_ERR_UNSUPPORTED;
  }
}

// Looks the chosen variant up in the table and launches it (fp32 or fp16 table by the grid's storage type).  Packed
// samples: choose_variant's preference among the rows that have a packed form -- where the preferred row has none (the
// split products, the pair products per sample, the eval table) the fp32 MFMA row of the same source runs.  `entry` is
// the entry point's name: the override kernels' messages carry it.
static int dispatch_render(const char* entry, const nrhip_field* f, const RaysDev& rd, bool packed, Out out, Src src,
                           const RenderArgs& a) {
  Variant v = choose_variant(f, out, src);
  if (packed && !render_variant_ok(v.L, v.F, v.out, v.src, v.prod, packed_lay(out, src))) v.src = src, v.prod = Prod::F32;
  FieldDev fd = to_dev(*f);
  if (v.src == Src::EvalTable) fd.table = f->eval_table;
  const bool half = f->grid.param_dtype == 1;
  const char* who = src == Src::Actors ? "fused field kernel with actors" : src == Src::Overrides ? entry : "fused field kernel";
#define X(L_, F_, H_, O_, S_, P_)                                                                 \
  if (same(v, {L_, F_, H_, Out::O_, Src::S_, Prod::P_}))                                          \
    return half ? launch_row<L_, F_, H_, true, Out::O_, Src::S_, Prod::P_>(who, packed, fd, rd, a) \
                : launch_row<L_, F_, H_, false, Out::O_, Src::S_, Prod::P_>(who, packed, fd, rd, a);
  NRHIP_RENDER_VARIANTS(X)
#undef X
  set_error("%s: no instantiation for L=%d F=%d H=%d", who, v.L, v.F, v.H);
  return NRHIP_ERR_UNSUPPORTED;
}

// Stable partition of the processing order into [rays no actor can touch | rays with candidate actors] + the two slices
// as device-side ranges {0, n0, n0, R}.  One workgroup: per-thread chunk counts -> block scan -> ordered writes, so each
// half keeps the locality order it was given.
constexpr int kPartThreads = 1024;
__global__ __launch_bounds__(kPartThreads) void actor_partition_kernel(const int32_t* __restrict__ cand_count,
                                                                       const int32_t* __restrict__ order_in, int64_t n,
                                                                       int32_t* __restrict__ order_out,
                                                                       int32_t* __restrict__ ranges) {
  __shared__ uint32_t wave_tot[kPartThreads / 64];
  const int tid = threadIdx.x;
  const int64_t per = (n + kPartThreads - 1) / kPartThreads, b = per * tid, e = b + per < n ? b + per : n;
  uint32_t free_rays = 0;
  for (int64_t i = b; i < e; ++i) free_rays += cand_count[order_in ? order_in[i] : i] == 0 ? 1u : 0u;
  uint32_t incl = free_rays;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off, 64);
    if ((tid & 63) >= off) incl += up;
  }
  if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
  __syncthreads();
  uint32_t before = incl - free_rays, total = 0;
  for (int w = 0; w < kPartThreads / 64; ++w) {
    if (w < (tid >> 6)) before += wave_tot[w];
    total += wave_tot[w];
  }
  // position i of the input is preceded by `before` free rays and (b - before) actor rays
  int64_t pf = before, pa = (int64_t)total + (b < n ? b : n) - before;
  for (int64_t i = b; i < e; ++i) {
    const int32_t r = order_in ? order_in[i] : (int32_t)i;
    if (cand_count[r] == 0) order_out[pf++] = r;
    else order_out[pa++] = r;
  }
  if (tid == 0) ranges[0] = 0, ranges[1] = (int32_t)total, ranges[2] = (int32_t)total, ranges[3] = (int32_t)n;
}

}  // namespace nrhip

using namespace nrhip;

// ---- what the entry points share.  Each of them validates its own ray descriptor, turns it into a RaysDev (to_dev, or
// packed_launch_rays with the segments beside it in RenderArgs), handles the empty batches of its layout and goes on here.
static int check_stop_eps(const char* who, float eps) {
  NR_REQUIRE(eps >= 0.f && eps < 1.f, NRHIP_ERR_INVALID_ARG, "%s: early_stop_eps %g not in [0,1)", who, (double)eps);
  return NRHIP_OK;
}

// a packed batch whose segments are all empty: no sample pointer (and no segment) is read, the per-ray outputs are zeroed
static int zero_ray_outputs(const char* who, int64_t R, float* features, float* depth, float* acc, hipStream_t st) {
  if (hipMemsetAsync(features, 0, (size_t)R * 32 * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(depth, 0, (size_t)R * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(acc, 0, (size_t)R * sizeof(float), st) != hipSuccess) {
    set_error("%s: zeroing the outputs failed", who);
    return NRHIP_ERR_LAUNCH;
  }
  return NRHIP_OK;
}

// composited output (segments: packed samples only)
static RenderArgs composite_args(float* features, float* depth, float* acc, float* weights, float stop_eps,
                                 const int64_t* segments, void* stream) {
  RenderArgs a{};
  a.feat = features, a.depth = depth, a.acc = acc, a.w = weights;
  a.stop_eps = stop_eps, a.segments = segments, a.stream = (hipStream_t)stream;
  return a;
}

// The four training forwards past their ray descriptor: every output and save buffer present, the save buffers aligned
// for 16-byte stores.  segments: packed samples only.  ovr (or NULL): the caller's rows for the samples inside an actor
// box; a row index is 32 bits (packed: M < 2^31 is the descriptor's own check).
static int field_fwd_train(const char* who, const nrhip_field* f, const RaysDev& rd, const int64_t* segments,
                           const OverrideLaunch* ovr, float* feature, float* sdf, float* alpha, const SaveDev& sv,
                           void* stream) {
  NR_REQUIRE(feature && sdf && alpha && sv.enc && sv.hg && sv.xf && sv.hf, NRHIP_ERR_INVALID_ARG, "%s: NULL output", who);
  NR_REQUIRE(((reinterpret_cast<uintptr_t>(sv.enc) | reinterpret_cast<uintptr_t>(sv.hg) |
               reinterpret_cast<uintptr_t>(sv.xf) | reinterpret_cast<uintptr_t>(sv.hf)) & 15) == 0,
             NRHIP_ERR_INVALID_ARG, "%s: save buffers must be 16-byte aligned", who);
  RenderArgs a{};
  a.feat = feature, a.sdf = sdf, a.alpha = alpha, a.sv = sv, a.segments = segments, a.stream = (hipStream_t)stream;
  if (ovr) {
    a.ovr = *ovr;
    NR_REQUIRE(ovr->row && ovr->rows && ovr->dirs, NRHIP_ERR_INVALID_ARG, "%s: NULL pointer", who);
    NR_REQUIRE((reinterpret_cast<uintptr_t>(ovr->rows) & 15) == 0, NRHIP_ERR_INVALID_ARG,
               "%s: override rows must be 16-byte aligned", who);
    NR_REQUIRE(segments || rd.R * rd.S < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "%s: N >= 2^31", who);
  }
  return dispatch_render(who, f, rd, segments != nullptr, Out::PerSample, ovr ? Src::Overrides : Src::Static, a);
}

// per-sample table select keeps the gather shape: one storage type, same features per level, no more levels than the
// static grid
static int check_actor_grid(const char* who, const nrhip_field* f, const nrhip_actors* a) {
  NR_REQUIRE(f->grid.param_dtype == a->grid.param_dtype, NRHIP_ERR_UNSUPPORTED,
             "%s: the static and the actor tables must share one storage type (fp32 or fp16)", who);
  NR_REQUIRE(a->grid.n_features == f->grid.n_features && a->grid.num_levels <= f->grid.num_levels, NRHIP_ERR_UNSUPPORTED,
             "%s: actor grid (L=%d F=%d) must have the static grid's features per level (F=%d) and at most its levels "
             "(L=%d); use the unfused ops",
             who, a->grid.num_levels, a->grid.n_features, f->grid.n_features, f->grid.num_levels);
  return NRHIP_OK;
}

static bool actor_inputs_present(const nrhip_actors* a, const int32_t* cand_count, const int32_t* cand_actor,
                                 const float* cand_w2b, const int32_t* workspace) {
  return cand_count && cand_actor && cand_w2b && workspace && a->bounds && a->tables && a->n_actors >= 1 &&
         a->actor_scale > 0.f;
}

// Most rays of a street scene pass no actor at all.  The processing order is split on the device into those rays and
// the rays with candidates (no host round trip): the first slice runs through the plain static kernel at full speed,
// the second through the ACT instantiation, which pays for the candidate walk in registers and latency.
// workspace: int32 [R + 4] (the split order, then the two ranges)
static int render_split_by_candidates(const char* who, const nrhip_field* f, const nrhip_actors* a, RaysDev rd,
                                      bool packed, RenderArgs ra, const int32_t* cand_count, const int32_t* cand_actor,
                                      const float* cand_w2b, int32_t* workspace) {
  ActorLaunch al;
  al.ad.K = a->max_candidates > 0 ? a->max_candidates : NRHIP_DEFAULT_ACTOR_CANDIDATES;
  al.ad.La = a->grid.num_levels, al.ad.log2T = a->grid.log2_table_size, al.ad.scale = a->actor_scale;
  for (int l = 0; l < NRHIP_MAX_LEVELS; ++l) al.ad.scal[l] = a->grid.scalings[l];
  al.cand_count = cand_count, al.cand_actor = cand_actor, al.cand_w2b = cand_w2b, al.bounds = a->bounds, al.tables = a->tables;
  int32_t* order2 = workspace;
  int32_t* ranges = workspace + rd.R;
  actor_partition_kernel<<<1, kPartThreads, 0, ra.stream>>>(cand_count, rd.order, rd.R, order2, ranges);
  if (int e = check_launch("actor_partition")) return e;
  rd.order = order2;
  ra.range = ranges;
  if (int e = dispatch_render(who, f, rd, packed, Out::Composite, Src::Static, ra)) return e;
  ra.range = ranges + 2, ra.actors = al;
  return dispatch_render(who, f, rd, packed, Out::Composite, Src::Actors, ra);
}

// The RaysDev that launch_render takes for the packed layouts: `S` carries the sample count M, the stride is 0, and the
// segments travel beside it in RenderArgs (the kernel reads them through its `tables` argument or its first save pointer).
static RaysDev packed_launch_rays(const nrhip_packed_rays& rays) {
  const PackedRaysDev p = to_dev(rays);
  return RaysDev{p.R, p.M, 0, p.o, p.d, p.area, p.starts, p.ends, rays.order};
}

extern "C" int nrhip_field_fwd(const nrhip_field* f, const nrhip_rays* rays, float* feature, float* sdf, float* alpha,
                               void* stream) {
  if (int e = validate_field(f)) return e;
  if (int e = validate_rays(rays)) return e;
  if (rays->n_rays == 0 || rays->n_samples == 0) return NRHIP_OK;
  NR_REQUIRE(feature && sdf && alpha, NRHIP_ERR_INVALID_ARG, "field_fwd: NULL output");
  RenderArgs a{};
  a.feat = feature, a.sdf = sdf, a.alpha = alpha, a.stream = (hipStream_t)stream;
  return dispatch_render("field_fwd", f, to_dev(*rays), false, Out::PerSample, Src::Static, a);
}

extern "C" int nrhip_field_fwd_train(const nrhip_field* f, const nrhip_rays* rays, float* feature, float* sdf,
                                     float* alpha, float* save_enc, float* save_geo_hidden, float* save_feat_in,
                                     float* save_feat_hidden, void* stream) {
  if (int e = validate_field(f)) return e;
  if (int e = validate_rays(rays)) return e;
  if (rays->n_rays == 0 || rays->n_samples == 0) return NRHIP_OK;
  return field_fwd_train("field_fwd_train", f, to_dev(*rays), nullptr, nullptr, feature, sdf, alpha,
                         SaveDev{save_enc, save_geo_hidden, save_feat_in, save_feat_hidden}, stream);
}

extern "C" int nrhip_field_fwd_train_ovr(const nrhip_field* f, const nrhip_rays* rays, const int32_t* ovr_row,
                                         const float* ovr_rows, const float* ovr_dirs, float* feature, float* sdf,
                                         float* alpha, float* save_enc, float* save_geo_hidden, float* save_feat_in,
                                         float* save_feat_hidden, void* stream) {
  if (int e = validate_field(f)) return e;
  if (int e = validate_rays(rays)) return e;
  if (rays->n_rays == 0 || rays->n_samples == 0) return NRHIP_OK;
  const OverrideLaunch ovr{ovr_row, ovr_rows, ovr_dirs};
  return field_fwd_train("field_fwd_train_ovr", f, to_dev(*rays), nullptr, &ovr, feature, sdf, alpha,
                         SaveDev{save_enc, save_geo_hidden, save_feat_in, save_feat_hidden}, stream);
}

extern "C" int nrhip_render_fwd_ex(const nrhip_field* f, const nrhip_rays* rays, float* out_features, float* out_depth,
                                   float* out_acc, float* out_weights, float early_stop_eps, void* stream) {
  if (int e = validate_field(f)) return e;
  if (int e = validate_rays(rays)) return e;
  if (rays->n_rays == 0) return NRHIP_OK;
  NR_REQUIRE(out_features && out_depth && out_acc, NRHIP_ERR_INVALID_ARG, "render_fwd: NULL output");
  NR_REQUIRE(rays->n_samples >= 1, NRHIP_ERR_INVALID_ARG, "render_fwd: needs >= 1 sample per ray");
  if (int e = check_stop_eps("render_fwd", early_stop_eps)) return e;
  return dispatch_render("render_fwd", f, to_dev(*rays), false, Out::Composite, Src::Static,
                         composite_args(out_features, out_depth, out_acc, out_weights, early_stop_eps, nullptr, stream));
}

extern "C" int nrhip_render_fwd(const nrhip_field* f, const nrhip_rays* rays, float* out_features, float* out_depth,
                                float* out_acc, float* out_weights, void* stream) {
  return nrhip_render_fwd_ex(f, rays, out_features, out_depth, out_acc, out_weights, 0.f, stream);
}

extern "C" int nrhip_render_fwd_packed(const nrhip_field* f, const nrhip_packed_rays* rays, float* out_features,
                                       float* out_depth, float* out_acc, float* out_weights, float early_stop_eps,
                                       void* stream) {
  const char* who = "render_fwd_packed";
  if (int e = validate_field(f)) return e;
  if (int e = validate_packed_rays(who, rays, true)) return e;
  if (rays->n_rays == 0) return NRHIP_OK;
  NR_REQUIRE(out_features && out_depth && out_acc, NRHIP_ERR_INVALID_ARG, "%s: NULL output", who);
  if (int e = check_stop_eps(who, early_stop_eps)) return e;
  if (rays->n_samples == 0) return zero_ray_outputs(who, rays->n_rays, out_features, out_depth, out_acc, (hipStream_t)stream);
  return dispatch_render(who, f, packed_launch_rays(*rays), true, Out::Composite, Src::Static,
                         composite_args(out_features, out_depth, out_acc, out_weights, early_stop_eps, rays->segments, stream));
}

extern "C" int nrhip_field_fwd_train_packed(const nrhip_field* f, const nrhip_packed_rays* rays, float* feature,
                                            float* geo_out, float* head, float* save_enc, float* save_geo_hidden,
                                            float* save_feat_in, float* save_feat_hidden, void* stream) {
  const char* who = "field_fwd_train_packed";
  if (int e = validate_field(f)) return e;
  if (int e = validate_packed_rays(who, rays, true)) return e;
  if (rays->n_rays == 0 || rays->n_samples == 0) return NRHIP_OK;  // nothing per sample to write: no pointer is read
  return field_fwd_train(who, f, packed_launch_rays(*rays), rays->segments, nullptr, feature, geo_out, head,
                         SaveDev{save_enc, save_geo_hidden, save_feat_in, save_feat_hidden}, stream);
}

extern "C" int nrhip_field_fwd_train_packed_ovr(const nrhip_field* f, const nrhip_packed_rays* rays,
                                                const int32_t* ovr_row, const float* ovr_rows, const float* ovr_dirs,
                                                float* feature, float* geo_out, float* head, float* save_enc,
                                                float* save_geo_hidden, float* save_feat_in, float* save_feat_hidden,
                                                void* stream) {
  const char* who = "field_fwd_train_packed_ovr";
  if (int e = validate_field(f)) return e;
  if (int e = validate_packed_rays(who, rays, true)) return e;
  if (rays->n_rays == 0 || rays->n_samples == 0) return NRHIP_OK;  // nothing per sample to write: no pointer is read
  const OverrideLaunch ovr{ovr_row, ovr_rows, ovr_dirs};
  return field_fwd_train(who, f, packed_launch_rays(*rays), rays->segments, &ovr, feature, geo_out, head,
                         SaveDev{save_enc, save_geo_hidden, save_feat_in, save_feat_hidden}, stream);
}

extern "C" int nrhip_render_fwd_actors(const nrhip_field* f, const nrhip_actors* a, const nrhip_rays* rays,
                                       const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                                       float* out_features, float* out_depth, float* out_acc, float* out_weights,
                                       float early_stop_eps, int32_t* workspace, void* stream) {
  const char* who = "render_fwd_actors";
  if (int e = validate_field(f)) return e;
  if (int e = validate_rays(rays)) return e;
  NR_REQUIRE(a, NRHIP_ERR_INVALID_ARG, "%s: actors descriptor is NULL", who);
  if (int e = validate_grid(&a->grid)) return e;
  if (rays->n_rays == 0) return NRHIP_OK;
  NR_REQUIRE(out_features && out_depth && out_acc && actor_inputs_present(a, cand_count, cand_actor, cand_w2b, workspace),
             NRHIP_ERR_INVALID_ARG, "%s: NULL pointer / empty actor set", who);
  NR_REQUIRE(rays->n_samples >= 1, NRHIP_ERR_INVALID_ARG, "%s: needs >= 1 sample per ray", who);
  if (int e = check_stop_eps(who, early_stop_eps)) return e;
  if (int e = check_actor_grid(who, f, a)) return e;
  return render_split_by_candidates(
      who, f, a, to_dev(*rays), false,
      composite_args(out_features, out_depth, out_acc, out_weights, early_stop_eps, nullptr, stream), cand_count,
      cand_actor, cand_w2b, workspace);
}

// The packed counterpart of nrhip_render_fwd_actors: the same three launches on the march's ragged segments.
extern "C" int nrhip_render_fwd_packed_actors(const nrhip_field* f, const nrhip_actors* a, const nrhip_packed_rays* rays,
                                              const int32_t* cand_count, const int32_t* cand_actor, const float* cand_w2b,
                                              float* out_features, float* out_depth, float* out_acc, float* out_weights,
                                              float early_stop_eps, int32_t* workspace, void* stream) {
  const char* who = "render_fwd_packed_actors";
  if (int e = validate_field(f)) return e;
  if (int e = validate_packed_rays(who, rays, true)) return e;
  NR_REQUIRE(a, NRHIP_ERR_INVALID_ARG, "%s: actors descriptor is NULL", who);
  if (int e = validate_grid(&a->grid)) return e;
  if (rays->n_rays == 0) return NRHIP_OK;
  NR_REQUIRE(out_features && out_depth && out_acc, NRHIP_ERR_INVALID_ARG, "%s: NULL output", who);
  if (int e = check_stop_eps(who, early_stop_eps)) return e;
  if (int e = check_actor_grid(who, f, a)) return e;
  if (rays->n_samples == 0) return zero_ray_outputs(who, rays->n_rays, out_features, out_depth, out_acc, (hipStream_t)stream);
  NR_REQUIRE(actor_inputs_present(a, cand_count, cand_actor, cand_w2b, workspace), NRHIP_ERR_INVALID_ARG,
             "%s: NULL pointer / empty actor set", who);
  NR_REQUIRE(rays->n_rays < (INT64_C(1) << 31), NRHIP_ERR_UNSUPPORTED, "%s: n_rays >= 2^31", who);
  return render_split_by_candidates(
      who, f, a, packed_launch_rays(*rays), true,
      composite_args(out_features, out_depth, out_acc, out_weights, early_stop_eps, rays->segments, stream), cand_count,
      cand_actor, cand_w2b, workspace);
}

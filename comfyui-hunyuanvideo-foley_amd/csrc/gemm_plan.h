// GEMM tile planning: which tile, K split, panel-group order and K-origin rotation a launch takes.  Host arithmetic on shapes
// and pointers only - launch_typed (gemm_impl.h) validates and plans through plan_gemm, then dispatches on the tile's family;
// foley_debug_gemm_plan (tests/test_gemm_plan_cpu.py) plans without a device.
#pragma once
#include "gemm_common.h"

namespace {

// Mainloop families: register-staged (gemm_kernel), direct-to-LDS (gemm_glds_kernel), wave-specialised with 8 / 4 consumer waves
// (gemm_ws_impl.h; the 4-consumer tiles have the vector epilogue only), its head-split tiles (fused head split, bf16 weights only), the
// legacy tap-fused conv k=3 (gemm_conv3.hip), the wave-specialised tap-fused conv k=3, and 256x256 on the BK = 32 mainloop (gemm_wide_impl.h)
enum TileFamily : unsigned char { FAM_NONE, FAM_REG, FAM_GLDS, FAM_WS8, FAM_WS4, FAM_HEAD, FAM_CONV3, FAM_WSCONV3, FAM_WIDE };

struct TileInfo {
  short bm, bn;
  TileFamily fam;
  bool fp8;          // serves fp8 weight storage
  bool ldw;          // serves padded weight rows (ldw != K)
  bool head;         // serves the fused head-split epilogue
  bool chunks;       // splits K over the channel chunks of one tap (tap-fused conv)
  bool grouped;      // takes the panel-group tile order on large grids (GemmArgs::n_groups)
  short ks_target;   // split-K: workgroups to aim for (small tiles ~3 per CU; the large, efficient ones split only below one round)
  char per_cu;       // deferred split-K: resident workgroups per CU
  char reg_twin;     // register-staged twin for operands past the 2 GiB buffer-offset range (0: none)
  char scalar_twin;  // twin for problems that need the scalar epilogue (0: none)
};

// indexed by tile id (foley_gemm_desc.tile); ids without an entry do not exist
constexpr TileInfo kTiles[33] = {
    //             bm   bn   family       fp8 ldw head chunks grouped target per_cu reg scalar
    /*  0 */ {},
    /*  1 */ {128, 128, FAM_REG,     0, 0, 1, 0, 0, 192, 1, 0, 0},
    /*  2 */ {64,  128, FAM_REG,     0, 0, 1, 0, 0, 768, 1, 0, 0},
    /*  3 */ {64,  64,  FAM_REG,     0, 0, 0, 0, 0, 768, 3, 0, 0},
    /*  4 */ {128, 64,  FAM_REG,     0, 0, 0, 0, 0, 768, 1, 0, 0},
    /*  5 */ {128, 128, FAM_GLDS,    0, 0, 1, 0, 0, 192, 1, 1, 0},
    /*  6 */ {64,  64,  FAM_GLDS,    0, 0, 0, 0, 0, 768, 3, 3, 0},
    /*  7 */ {128, 128, FAM_GLDS,    0, 0, 1, 0, 0, 192, 1, 1, 0},
    /*  8 */ {64,  128, FAM_GLDS,    0, 0, 1, 0, 0, 768, 1, 2, 0},
    /*  9 */ {256, 128, FAM_GLDS,    0, 0, 1, 0, 0, 192, 1, 1, 0}, {},
    /* 11 */ {128, 128, FAM_CONV3,   0, 0, 0, 1, 0, 192, 1, 0, 0}, {},
    /* 13 */ {64,  64,  FAM_CONV3,   0, 0, 0, 1, 0, 512, 3, 0, 0}, {},
    /* 15 */ {128, 128, FAM_WS8,     1, 1, 1, 0, 1, 192, 1, 1, 0}, {}, {}, {},
    /* 19 */ {256, 128, FAM_WS8,     1, 1, 1, 0, 1, 192, 1, 1, 0}, {},
    /* 21 */ {128, 128, FAM_WSCONV3, 1, 1, 0, 1, 1, 192, 1, 0, 0},
    /* 22 */ {256, 64,  FAM_WSCONV3, 0, 1, 0, 1, 0, 192, 1, 0, 0},
    /* 23 */ {256, 128, FAM_WSCONV3, 1, 1, 0, 1, 1, 192, 1, 0, 0},
    /* 24 */ {192, 128, FAM_WSCONV3, 0, 1, 0, 1, 1, 192, 1, 0, 0},
    /* 25 */ {128, 128, FAM_WS4,     0, 1, 1, 0, 1, 192, 1, 1, 15},
    /* 26 */ {96,  128, FAM_HEAD,    0, 1, 1, 0, 0, 768, 1, 1, 0},
    /* 27 */ {64,  128, FAM_HEAD,    0, 1, 1, 0, 0, 768, 1, 2, 0},
    /* 28 */ {192, 128, FAM_HEAD,    0, 1, 1, 0, 1, 768, 1, 1, 0},
    /* 29 */ {256, 128, FAM_WS4,     0, 1, 1, 0, 1, 192, 1, 1, 19}, {},
    /* 31 */ {256, 256, FAM_WIDE,    1, 1, 0, 1, 1, 192, 1, 0, 0},
    /* 32 */ {256, 256, FAM_WIDE,    1, 1, 1, 0, 1, 192, 1, 0, 0},
};

inline const TileInfo& tile_info(int tile) {
  static constexpr TileInfo none{};
  return tile >= 0 && tile < 33 ? kTiles[tile] : none;
}

struct GemmPlan {
  int tile = 0, ksplit = 1, n_groups = 0, k_rot = 0;
  int vec_out[2] = {0, 0};   // per problem: the LDS-transposed vector epilogue
  bool attn_fused = false;   // EPI_QKV_SPLIT: the cross attention runs in the epilogue (EPI_QKV_ATTN)
  int wt_out = 0;            // write-through output stores (GemmArgs::wt_out): one-round grids of 16-bit operands only
  const char* err = nullptr;
};

// Workgroups of a launch on tile `ti`: both problems, every K range
inline long plan_workgroups(const TileInfo& ti, const GemmArgs& g, const GemmArgs* g1, int epi, int ksplit) {
  auto tiles = [&](const GemmArgs& q) { return (long)((q.M + ti.bm - 1) / ti.bm) * ((q.N + ti.bn - 1) / ti.bn); };
  return (tiles(g) + (g1 ? tiles(*g1) : 0)) * (epi == EPI_GATE_RES ? ksplit : 1);
}

template <typename T>
const char* check_args(const GemmArgs& g) {
  constexpr int BK = 8 * Frag<T>::EPC;
  if (g.K % BK || g.tapC % BK || g.taps * g.tapC != g.K || g.lda % Frag<T>::EPC)
    return "GEMM: K / tap width / lda must be multiples of the 128-byte K-slice";
  if (((uintptr_t)g.A | (uintptr_t)g.W) & 15) return "GEMM: operands must be 16-byte aligned";
  if (g.partial_half && sizeof(T) != 2) return "GEMM: 16-bit partial slabs need 16-bit operands";
  if (g.wfmt && sizeof(T) != 2) return "GEMM: fp8 weight storage needs bf16 operands";
  return nullptr;
}

template <typename T>
const char* check_qkv_split(const GemmArgs& q) {
  const QkvSplitArgs& s = q.qs;
  if (s.nK < 1 || s.nK > 3 || s.H < 1 || q.N != s.nK * s.H * 128 || s.L < 1 || q.M % s.L)
    return "fused head split: N must be nK*H*128 and M a multiple of L";
  if (s.out_dtype != DtCode<T>::v) return "fused head split: output dtype must equal the operand dtype";
  if (s.vt_pitch && (sizeof(T) != 2 || s.vt_pitch % 8 || (s.tok_off + s.L) > s.vt_pitch))
    return "fused head split: bad transposed-V pitch";
  uintptr_t al = (uintptr_t)s.cos_tab | (uintptr_t)s.sin_tab | (uintptr_t)q.bias;
  for (int i = 0; i < s.nK; ++i) {
    if (!s.dst[i]) return "fused head split: null destination";
    al |= (uintptr_t)s.dst[i] | (uintptr_t)s.gain[i] | (uintptr_t)s.rcos[i] | (uintptr_t)s.rsin[i];
    if (s.pos[i] && (!s.cos_tab || !s.sin_tab)) return "fused head split: RoPE tables missing";
    if ((s.rcos[i] != nullptr) != (s.rsin[i] != nullptr) || (s.rcos[i] && !s.pos[i]))
      return "fused head split: gathered rotation rows need both tables and a position table";
  }
  if (al & 15) return "fused head split: operands must be 16-byte aligned";
  return nullptr;
}

// Bytes the A / W operands span from their base pointers (A: every source row the virtual rows touch; W: N rows of ldw
// elements, one byte each in fp8 storage), and whether both fit the 32-bit buffer offsets of the direct-to-LDS loops
template <typename T>
long gemm_a_bytes(const GemmArgs& q) { return (long)((q.M + q.segV - 1) / q.segV) * q.segS * q.lda * (long)sizeof(T); }
template <typename T>
long gemm_w_bytes(const GemmArgs& q) { return (long)q.N * q.ldw * (q.wfmt ? 1L : (long)sizeof(T)); }
template <typename T>
bool gemm_fits_buffer_range(const GemmArgs& q) { return gemm_a_bytes<T>(q) < 0x7fff0000L && gemm_w_bytes<T>(q) < 0x7fff0000L; }

// One problem (g1 null) or the two problems of a pair launch; tile 0 = automatic; krot_ok: the caller's opt-in to K-origin rotation
// (GemmArgs::krot_ok, decided outside the planner).  Reads no globals, writes nothing but the plan.
template <typename T>
GemmPlan plan_gemm(const GemmArgs& g_in, const GemmArgs* g1_in, int epi, int tile, int krot_ok) {
  GemmPlan plan;
  auto fail = [&](const char* msg) { plan.err = msg; return plan; };
  GemmArgs g = g_in, g1s = g1_in ? *g1_in : g_in;
  const GemmArgs* g1 = g1_in ? &g1s : nullptr;
  if (g.ldw <= 0) g.ldw = g.K;
  if (g1s.ldw <= 0) g1s.ldw = g1s.K;
  for (const GemmArgs* q : {(const GemmArgs*)&g, g1})
    if (const char* e = q ? check_args<T>(*q) : nullptr) return fail(e);
  if (g1 && g1s.wfmt != g.wfmt) return fail("GEMM: the two problems of a launch must share the weight format");
  constexpr int BK = 8 * Frag<T>::EPC;
  // tap-fused wave-specialised conv3 (tile 21): bf16 operands (any weight storage), dense k=3 'same' conv
  const bool ws_conv3_ok = sizeof(T) == 2 && !g1 && g.taps == 3 && g.dil == 1 && g.tap0 == -1 && g.rstride <= 1 && g.segV == g.segS &&
                           g.osegV >= g.M && (epi == EPI_STORE_F32 || epi == EPI_GATE_RES || epi == EPI_SILUGATE_T);
  if (tile_info(tile).fam == FAM_WSCONV3 && !ws_conv3_ok) return fail("GEMM: tiles 21 / 22 / 23 / 24 need a bf16 channels-last conv k=3");
  if (tile == 24 && (g.wfmt || epi == EPI_SILUGATE_T)) return fail("GEMM: tile 24 (192x128 conv) serves bf16 weights, gated-residual / fp32-store epilogues");
  if (tile == 22 && g.wfmt) return fail("GEMM: tile 22 serves bf16 weights");
  const bool conv3_ok = !g.wfmt && !g1 && g.taps == 3 && g.dil == 1 && g.tap0 == -1 && g.rstride <= 1 && g.segV == g.segS && g.lda == g.tapC &&
                        g.osegV >= g.M && (epi == EPI_STORE_F32 || epi == EPI_GATE_RES || epi == EPI_SILUGATE_T);
  const bool tile_auto = tile == 0;
  // deferred split-K available (bf16 mode, caller provided partial slabs): reductions are cheap
  // vector stores + a few extra row reads in the next LayerNorm
  const bool deferred = epi == EPI_GATE_RES && g.partials && g.partial_cap > 1 && sizeof(T) == 2 && g.ksplit != 1 &&
                        (!g1 || g1->partials);
  // Measured end to end (xxl, 5 s): the tap-fused kernel wins in fp32 (parity mode, -7 % loop time)
  // and for the small-M gated w1/w3 GEMM; elsewhere the generic tiles (+ split-K / 256x128) are as
  // fast or faster in bf16, so it is only auto-selected there.
  const bool small_grid = (long)((g.M + 127) / 128) * ((g.N + 127) / 128) <= 256;
  if (tile == 0 && conv3_ok && (sizeof(T) == 4 || (deferred && small_grid))) {   // other bf16 cases: the wave-specialised generic tiles win (tools/gemm_timeline.py)
    const long b128 = (long)((g.M + 127) / 128) * ((g.N + 127) / 128);
    tile = (b128 >= 100 || epi == EPI_SILUGATE_T || deferred) ? 11 : 13;   // the gated epilogue needs 64-wide wave tiles
  }
  if (tile == 0) {
    // Tile choice for 256 CUs (measured on the M=500 / M=4000 shapes of the xxl DiT,
    // tools/gemm_bench.py): the 128x128 / 8-wave tile wins whenever it fills the chip without a
    // ragged last wave of workgroups; otherwise many small 64x64 tiles hide latency better.
    auto nblk = [&](int bm, int bn) { return (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn); };
    const long b128 = nblk(128, 128);
    const long rem = b128 % 256;
    // (head-split pairs count both problems: the cross-attention q projection of the 30 s clip - 144 + 24 tiles of 256x128 in ONE round -
    // sat on 336 tiles of 128x128 in two ragged ones: 39.8 us per launch)
    const long pair256 = (epi == EPI_QKV_SPLIT && g1) ? (long)((g1s.M + 255) / 256) * ((g1s.N + 127) / 128) : 0;
    if (sizeof(T) == 2 && g.N > 64 && g.M > 128 && nblk(256, 128) + pair256 >= 160) tile = 9;   // big grids: 64x64 per wave (one M tile: 128 rows
                                                                                         // halve the activation DMA, modulation GEMM at M = 16: 258 -> 227 us)
    else if (deferred && g.N > 64 && b128 <= 256) tile = 5;   // 128x128 tiles, K ranges fill the chip (tools/gemm_timeline.py)
    else if (g.N <= 64 && epi != EPI_SILUGATE_T) tile = nblk(128, 64) >= 192 ? 4 : 3;
    // fp32 (the DAC decoder): a long-K GEMM whose 128x128 tiles cover half the chip or less runs at the pace of ONE workgroup
    // (decoder stage 1: M = 2000, N = 1024, K = 7168 -> 128 workgroups, 470 us at 39 % of the fp32 matrix peak); 64x128 tiles
    // double the workgroups
    else if (sizeof(T) == 4 && b128 >= 100 && b128 <= 160 && nblk(64, 128) <= 320 && g.K >= 1024 && epi != EPI_SILUGATE_T) tile = 8;
    else if (b128 >= 100 && (b128 <= 256 || rem == 0 || rem >= 128 || b128 >= 2048)) tile = 5;
    else if (epi == EPI_SILUGATE_T) tile = nblk(64, 128) >= 192 ? 2 : 5;
    else tile = 3;
  }
  if (sizeof(T) == 2 && tile_auto) {   // bf16: loader / consumer wave specialisation of the same tiles
    // Four consumer waves (64x64 / 128x64 wave tiles, a third less LDS fragment traffic) with the loader waves
    // helping in the epilogue beat the eight-consumer form wherever the grid does not saturate the L2s
    // (M = 500: q/k/v 22.7 -> 19.1 us, fc1 21.1 -> 16.2, cross-q 21.1 -> 16.5; tools/gemm_timeline.py); the
    // big gated-residual GEMMs at large M keep eight consumers.  fp8 weights exist in the eight-consumer form.
    if (tile == 5) tile = g.wfmt ? 15 : 25;
    else if (tile == 9) tile = (g.wfmt || epi == EPI_GATE_RES) ? 19 : 29;
  }
  // channels-last conv k=3 on a 128x128-class grid: the tap-fused wave-specialised kernel stages the activation
  // chunk once for the three taps (a third fewer bytes out of the L2s: lin1 16.4 -> 12.1 us, w2 32.4 -> 23.2 us,
  // w1/w3 49.3 -> 40.0 us at M = 500; tools/gemm_timeline.py).  Large grids use its 256x128 form (tile 23).
  if (tile_auto && ws_conv3_ok && (tile == 15 || tile == 25 || tile == 11 || tile == 13 || tile == 5 || tile == 3 || tile == 2)) tile = 21;
  // split-K convs on a one-round grid: the 256x64 form has the same workgroup count on N = 1536 and moves 12 % fewer operand bytes
  // per workgroup; the same form for w1 / w3 (SiLU gate, M = 500: 2 x 128 workgroups instead of 4 x 64): 39.2 -> 37.7 us
  if (tile_auto && tile == 21 && ((deferred && epi == EPI_GATE_RES) || epi == EPI_SILUGATE_T) && !g.wfmt && g.M > 256 && g.N % 128 == 0 &&
      (long)((g.M + 255) / 256) * (g.N / 64) == (long)((g.M + 127) / 128) * (g.N / 128))
    tile = 22;
  if (tile_auto && ws_conv3_ok && (tile == 19 || tile == 29 || tile == 9)) tile = 23;   // large grids: the 256x128 tap-fused form (w1/w3 at M = 4000: 329 -> 285 us)
  // 256x256 tiles on the BK = 32 mainloop (gemm_wide_impl.h, tiles 31 / 32) for the large grids, wherever their workgroups
  // fill the last round of 256 CUs about as well as the 256x128 tiles' do (tools/wide_bench.py at M = 4000: w1/w3 298 -> 249 us,
  // w2 158 -> 134, linear2 66 -> 59, fc2 92 -> 79; fc1 - 1.5 rounds of 256x256 against exactly 3 of 256x128 - stays).
  // Mid-size grids (M = 3000: the 30 s clip) whose N = 1536 gated-residual GEMMs landed on 128x128 tiles with two K ranges
  // (288 tiles, 1.1 rounds) take the same route: 72 tiles of 256x256 x three K ranges (w2 149 -> 97 us, fc2 99 -> 59 us).
  // (plain layers arrive here on tile 3 / 5 when their 288 tiles of 128x128 fit no rule above - fp8 weights turn that into tile 15 below)
  // (bf16 convs on tile 22, the 256x64 tap-fused form); measured down to M = 2000 (w2 89 -> 70 us, fc2 65 -> 46 with five K ranges)
  const bool mid_split = (tile == 21 || tile == 22 || tile == 15 || tile == 25 || tile == 5 || tile == 3) && g.M >= 1536 && g.N >= 256 &&
                         epi == EPI_GATE_RES && deferred;
  // (round 6) two-problem launches - the audio + visual pair of a two-stream block's gated-residual layers (proj, fc2) - take the same
  // route at mid-size grids: at M = 3000 + 480 they sat on 128x128 tiles (fc2 113 us where the single-problem form of the same shape
  // takes 57 - 59 on 72 tiles x three K ranges)
  // The 256x256 tiles range every load against 32-bit buffer extents and have no register-staged twin: operands past the 2 GiB
  // buffer-offset range (the check after the K split below) keep the tiles that fall back, in the wide route and the short-K rule alike
  const bool fits = gemm_fits_buffer_range<T>(g) && (!g1 || gemm_fits_buffer_range<T>(g1s));
  // ... where their 128x128 tiles do not fit ONE round of 256 workgroups (M = 3000 + 480: 336).  Where they do (bs = 4, M = 2000 + 320:
  // 228 tiles, no K split, no slabs for the next LayerNorm to read) the 256x256 route with four K ranges LOSES 1.1 % of the loop.
  const long pair_b128 = !g1 ? 0 : (long)((g.M + 127) / 128) * ((g.N + 127) / 128) + (long)((g1s.M + 127) / 128) * ((g1s.N + 127) / 128);
  const bool pair_ok = !g1 || (mid_split && pair_b128 > 256 && !ws_conv3_ok && g1s.taps == 1 && g1s.segV >= g1s.M && g1s.rstride <= 1 && g1s.tap0 == 0 &&
                               g1s.tapC % 32 == 0 && g1s.M >= 1 && g1s.N >= 256);
  if (tile_auto && sizeof(T) == 2 && pair_ok && fits && (tile == 23 || tile == 19 || tile == 29 || mid_split)) {
    const bool conv = tile == 23 || tile == 21 || (mid_split && ws_conv3_ok);
    const bool epi_ok = epi == EPI_STORE_F32 || epi == EPI_GATE_RES || epi == EPI_SILUGATE_T || (!conv && epi == EPI_GELU_T);
    // plain layers: long K only - a 256x256 tile pays its two-pass epilogue and 6-slice ring fill once per 24 slices at K = 768
    // (the ViT-B encoders' fc1 at M = 22 000: 223 us on this tile against ~140 on 256x128)
    const bool addr_ok = conv || (g.taps == 1 && g.segV >= g.M && g.rstride <= 1 && g.tap0 == 0 &&
                                  // ... or a weight-streaming panel (the single-block modulation GEMM of a video clip: M = 224 rows against
                                  // N = 331 776 columns - a 256-column tile re-reads the activations half as often: 60.6 -> 51.9 us per eighth)
                                  (g.K >= 2048 || mid_split || (epi == EPI_STORE_F32 && g.N >= 16384 && g.M >= 128)));
    if (epi_ok && addr_ok && g.tapC % 32 == 0) {
      long mt = (g.M + 255) / 256, tw = mt * ((g.N + 255) / 256), tb = mt * ((g.N + 127) / 128);
      if (g1) {
        const long mt1 = (g1s.M + 255) / 256;
        tw += mt1 * ((g1s.N + 255) / 256);
        tb += mt1 * ((g1s.N + 127) / 128);
      }
      const int nk64 = (conv ? g.tapC : g.K) / 64;
      auto ksp = [&](long blocks) -> long {   // the K split the deferred rule below will choose for `blocks` tiles
        if (epi != EPI_GATE_RES) return 1;
        if (g.ksplit > 0) return g.ksplit;
        if (!deferred) return 1;
        long w = 256 / blocks;
        if (w > nk64 / 4) w = nk64 / 4;
        if (w > g.partial_cap) w = g.partial_cap;
        return w < 1 ? 1 : (w > 16 ? 16 : w);
      };
      auto eff = [](long wg) { return (double)wg / (double)(((wg + 255) / 256) * 256); };
      const long kw = ksp(tw);
      const double ew = eff(tw * kw), eb = eff(tb * ksp(tb));
      GemmArgs gt = g;
      gt.ksplit = (int)kw;
      // a K split on top of it pays only where the 256x128 tiles leave the chip half empty (M = 3000, N = 1536: 144 workgroups
      // - w2 143 -> 97 us, fc2 99 -> 59 us with three K ranges); at M = 4000 the two slabs cost the next LayerNorm 12 us per launch
      // (pending form 21.6 vs 9.6 us) for 7 us won in the GEMM
      const bool split_ok = kw == 1 || eb < 0.6 || mid_split;
      bool vec1 = true;
      if (g1) {
        GemmArgs gt1 = g1s;
        gt1.ksplit = (int)kw;
        vec1 = gemm_vec_out_ok<T>(gt1, epi);
      }
      if (ew >= 0.74 && ew >= eb - 0.13 && split_ok && gemm_vec_out_ok<T>(gt, epi) && vec1) tile = conv ? 31 : 32;
    }
  }
  // A large conv grid whose 256-row tiles cover clearly less than one round of 256 CUs while 192-row tiles still fit it (w2 / linear1 at
  // M = 4000: 16 x 12 = 192 workgroups against 21 x 12 = 252) takes the 192x128 form: every CU works, and each workgroup streams
  // (192 + 128) instead of (256 + 128) rows per K-slice.
  if (tile_auto && tile == 23 && !g.wfmt && epi != EPI_SILUGATE_T && g.N % 128 == 0) {
    const long b256 = (long)((g.M + 255) / 256) * (g.N / 128), b192 = (long)((g.M + 191) / 192) * (g.N / 128);
    if (b256 <= 216 && b192 <= 256 && b192 > b256) tile = 24;
  }
  if (g.wfmt && !tile_info(tile).fp8) {   // fp8 weights exist only in the wave-specialised mainloops
    if (!tile_auto) return fail("GEMM: fp8 weights need tile 15, 19 or 21");
    tile = 15;
  }
  if (epi == EPI_QKV_SPLIT) {
    for (const GemmArgs* q : {(const GemmArgs*)&g, g1})
      if (const char* e = q ? check_qkv_split<T>(*q) : nullptr) return fail(e);
    const bool listed = tile_info(tile).head;
    if (tile_auto && tile == 29 && !g.wfmt) {
      // Large grids: workgroups run in ceil(n / 256) rounds of (BM + 128) * 128 bytes per K-slice each - 192-row tiles
      // win when they save bytes without adding a round (M = 4000 q/k/v: 3 rounds either way, 320 instead of 384 rows
      // per workgroup and slice)
      auto cost = [&](int bm) {
        long n = (long)((g.M + bm - 1) / bm) * (g.N / 128);
        if (g1) n += (long)((g1s.M + bm - 1) / bm) * (g1s.N / 128);
        return ((n + 255) / 256) * (bm + 128);
      };
      if (cost(192) < cost(256)) tile = 28;
    }
    if (!listed || (tile_auto && tile == 25)) {
      long b128 = (long)((g.M + 127) / 128) * (g.N / 128);
      if (!listed) tile = b128 >= 24 ? (sizeof(T) == 2 ? (g.wfmt ? 15 : 25) : 5) : 2;
      // few 128-row tiles (the cross-attention q projection: 48 + 12 workgroups on 256 CUs): 64-row tiles double the
      // workgroups and move a quarter fewer bytes per workgroup and K-slice
      if (g1) b128 += (long)((g1s.M + 127) / 128) * (g1s.N / 128);
      if (tile == 25 && b128 <= 100) tile = 27;
      // 96-row tiles when they still fit one round of workgroups (M = 500: 6 x 36 = 216): an eighth fewer bytes per
      // workgroup and K-slice than 128 rows
      long b96 = (long)((g.M + 95) / 96) * (g.N / 128);
      if (g1) b96 += (long)((g1s.M + 95) / 96) * (g1s.N / 128);
      if (tile == 25 && b96 <= 256 && b128 > 100 && (g.M % 128 == 0 ? false : (g.M + 95) / 96 * 96 - g.M < 96)) tile = 26;
    }
  }
  // Short-K plain layers of the large grids whose epilogue rules out a K split (fc1's GELU, the q/k/v head split; K = 1536 / 1408;
  // one problem or the audio + visual pair of a two-stream block): such a launch is whole ROUNDS of 256 workgroups, and per round a
  // 256x256 BK = 32 tile costs ~1.64x a 256x128 tile's round at K = 1536 for twice the area (tools/wide_bench.py, M = 4000 / 3000, bf16
  // and fp8 storage: 45 / 43 us against 27.5 / 26 us; a 192x128 round 23.7 us = 0.86).  The 256x256 tile is taken where that count
  // says it wins by more than 5 %: fc1 of the two-stream blocks at bs = 8 (M = 4000 + 640: 2 rounds against 4), q/k/v of the 30 s
  // clip (M = 3000: 216 / 252 tiles = ONE round against two of 256x128).
  if (tile_auto && sizeof(T) == 2 && fits && (epi == EPI_GELU_T || epi == EPI_QKV_SPLIT) && (tile == 19 || tile == 29 || tile == 28)) {
    auto plain = [&](const GemmArgs& q) {
      return q.taps == 1 && q.segV >= q.M && q.rstride <= 1 && q.tap0 == 0 && q.tapC % 32 == 0 && q.K >= 1024 && q.K < 2048 &&
             (epi == EPI_QKV_SPLIT || gemm_vec_out_ok<T>(q, epi));
    };
    auto tiles = [&](int bm, int bn) {
      long n = (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
      if (g1) n += (long)((g1s.M + bm - 1) / bm) * ((g1s.N + bn - 1) / bn);
      return n;
    };
    if (plain(g) && (!g1 || plain(g1s))) {
      const double cur = (double)((tiles(tile == 28 ? 192 : 256, 128) + 255) / 256) * (tile == 28 ? 0.86 : 1.0);
      const double wide = (double)((tiles(256, 256) + 255) / 256) * 1.64;
      if (wide < 0.95 * cur) tile = 32;
    }
  }
  if (epi != EPI_GATE_RES || g.ksplit == 1 || (g.ksplit == 0 && sizeof(T) == 4)) {
    g.ksplit = 1;   // fp32 (parity) mode keeps a fixed summation order
  } else if (g.ksplit == 0) {
    // fill ~3 workgroups per CU, keep >= 12 K-slices per range
    const TileInfo& ti = tile_info(tile);
    if (ti.bm == 0) return fail("GEMM: unknown tile");
    const long blocks = (long)((g.M + ti.bm - 1) / ti.bm) * ((g.N + ti.bn - 1) / ti.bn);
    const int nk = ti.chunks ? g.tapC / BK : g.K / BK;   // conv3 splits over channel chunks
    long want = (ti.ks_target + blocks - 1) / blocks;
    if (want > nk / 12) want = nk / 12;
    if (deferred) {   // one resident round of workgroups: as many K ranges as fit on 256 CUs (>= 4 slices each)
      long both = blocks;   // a two-problem launch (audio + visual stream) shares the round and the K split
      if (g1) both += (long)((g1->M + ti.bm - 1) / ti.bm) * ((g1->N + ti.bn - 1) / ti.bn);
      want = 256L * ti.per_cu / both;
      if (tile == 21 && both > 256) want = both < 512 ? 2 : 1;   // mid-size grids: two K ranges beat a ragged second round (M = 3000: 68 -> 58 us)
      if (want > nk / 4) want = nk / 4;
    }
    g.ksplit = (int)(want < 1 ? 1 : (want > 16 ? 16 : want));
  }
  if (epi == EPI_GATE_RES && g.partials) {
    int cap = g.partial_cap;
    if (g1 && g1s.partial_cap < cap) cap = g1s.partial_cap;
    if (g1 && !g1s.partials) cap = 1;
    if (g.ksplit > cap) g.ksplit = cap < 1 ? 1 : cap;
  }
  g1s.ksplit = g.ksplit;
  // the direct-to-LDS loop addresses its operands through 32-bit buffer offsets
  if (!fits) {
    if (g.wfmt) return fail("GEMM: fp8-weight operands exceed the 2 GiB buffer-offset range");
    if (tile_info(tile).fam == FAM_WSCONV3) return fail("GEMM: conv3 operands exceed the 2 GiB buffer-offset range");
    if (tile_info(tile).fam == FAM_WIDE) return fail("GEMM: the 256x256 tiles range every load against 32-bit buffer extents: operands exceed the 2 GiB buffer-offset range");
    if (tile_info(tile).reg_twin) tile = tile_info(tile).reg_twin;   // register-staged twins
  }
  const TileInfo& ti = tile_info(tile);
  {
    // Large grids (several rounds of workgroups, activation panel larger than an L2): tile order [panel group][M tile][panel in group]
    // (tile_coords, gemm_ws_impl.h) so that the ~32 workgroups an XCD runs at a time cover a near-square block of tiles - panels
    // per group ~ sqrt(32 BM / BN) minimises the rows + columns the block pulls out of the fabric per K-slice.  Measured at
    // bs = 8 (one box, both orders twice): q/k/v 85 -> 77 us, fc1 115 -> 111, loop 1459 -> 1436 ms (+1.6 %); C5 +1 %.
    if (ti.grouped && g.M >= 1536 && !g1) {
      const long tm_ = (g.M + ti.bm - 1) / ti.bm, tn_ = (g.N + ti.bn - 1) / ti.bn;
      if (tm_ * tn_ * (epi == EPI_GATE_RES ? g.ksplit : 1) > 256 && tn_ >= 2) {
        int pg = 1;
        while ((pg + 1) * (pg + 1) * ti.bn <= 32 * ti.bm) ++pg;   // floor(sqrt(32 BM / BN))
        const int n = (int)((tn_ + pg / 2) / pg);
        plan.n_groups = n < 1 ? 1 : n;
      }
    }
  }
  {
    // Small grids (one round of workgroups), plain layers on the wave-specialised tiles: K-origin rotation per M tile (GemmArgs::k_rot,
    // gemm_ws_impl.h).  All M tiles of a weight panel start together and walk K in step, so every one of them waits for the SAME cold
    // line (one HBM fill, the others queued behind it in the L2) - each holds a slot of its CU's memory queue for the full HBM latency.
    // Started 1 / tiles_m of the range apart they take turns at the miss and find the other lines in the L2.  Only where the caller
    // opted in (GemmArgs::krot_ok: the summation order of a row then depends on its tile).
    const int rbm = (ti.fam == FAM_WS8 || ti.fam == FAM_WS4 || ti.fam == FAM_HEAD) ? ti.bm : 0;
    if (krot_ok && rbm && sizeof(T) == 2 && g.taps == 1 && (!g1 || g1s.taps == 1)) {
      const long ks_ = epi == EPI_GATE_RES ? g.ksplit : 1;
      long n = (long)((g.M + rbm - 1) / rbm) * ((g.N + 127) / 128) * ks_;
      if (g1) n += (long)((g1s.M + rbm - 1) / rbm) * ((g1s.N + 127) / 128) * ks_;
      if (n <= 256 && (g.M + rbm - 1) / rbm >= 2) plan.k_rot = 1;
    }
  }
  plan.vec_out[0] = gemm_vec_out_ok<T>(g, epi) ? 1 : 0;
  if (g1) plan.vec_out[1] = gemm_vec_out_ok<T>(g1s, epi) ? 1 : 0;
  // The four-consumer tiles hold 64 / 128 accumulator registers per wave: only the LDS-transposed vector
  // epilogue is instantiated for them (the scalar one made the compiler keep the 256x128 tile's accumulators
  // in scratch memory - 576 bytes per lane, loads / stores inside the K loop: 0.6 -> 0.37 ms for the
  // single-block modulation GEMM once it was gone).  Problems that need the scalar epilogue take the twins.
  if (ti.scalar_twin && epi != EPI_QKV_SPLIT && !(plan.vec_out[0] && (!g1 || plan.vec_out[1]))) tile = ti.scalar_twin;
  if (ti.fam == FAM_HEAD && (epi != EPI_QKV_SPLIT || g.wfmt)) return fail("GEMM: tile 27 (64x128) serves the fused head split with bf16 weights only");
  if ((g.ldw != g.K || (g1 && g1s.ldw != g1s.K)) && !tile_info(tile).ldw)
    return fail("GEMM: padded weight rows (ldw != K) need a wave-specialised tile");
  if (tile_info(tile).fam == FAM_NONE) return fail("GEMM: bad tile id");
  // Cross-attention q projections may carry the attention in their epilogue (QkvSplitArgs::attn_out): taken when the problem
  // landed on the 64-row head-split tile (small grids, where the attention launch and its boundary cost more than its math);
  // otherwise the plain head split runs and the caller launches the attention (attn_fused tells).
  if (epi == EPI_QKV_SPLIT) {
    auto fuses = [](const GemmArgs& q) {
      const QkvSplitArgs& s = q.qs;
      return s.attn_out && s.attn_k && s.attn_vt && s.nK == 1 && s.vt_pitch == 0 && s.attn_skv >= 1 && s.attn_skv <= 96 &&
             s.attn_pitch >= 96 && s.attn_pitch % 8 == 0 && s.attn_bdiv >= 1 &&
             ((long)s.L * s.attn_bdiv >= 64 || q.M <= 2L * s.L * s.attn_bdiv) &&   // a 64-row tile meets at most two text sets
             !(((uintptr_t)s.attn_k | (uintptr_t)s.attn_vt | (uintptr_t)s.attn_out) & 15);
    };
    plan.attn_fused = sizeof(T) == 2 && tile == 27 && fuses(g) && (!g1 || fuses(g1s));
  }
  plan.tile = tile;
  plan.ksplit = g.ksplit;
  // Write-through output stores (common.h GStore): a launch of ONE round of workgroups (<= 256: the single-clip regime) ends in
  // the write-back of everything its epilogues left dirty in the L2s, with all 256 CUs waiting.  Stored write-through, those
  // bytes leave while the other workgroups are still in their K loops.  Larger problems - more than one round, or the
  // planner's large-M side (M >= 1536: the 256x256 K-range route fits 20 s / 30 s clips into one round too, with outputs
  // beyond the L2s, matrix-pipe bound) - and the fp32 parity mode keep the plain stores.  Served: the deferred split-K slabs
  // of the vector epilogue, which the next launch reads once (the other epilogues' outputs keep the plain stores: DESIGN.md
  // section 4, "Round 8").
  if (sizeof(T) == 2 && g.M + (g1 ? g1s.M : 0) < 1536 && plan_workgroups(tile_info(tile), g, g1, epi, g.ksplit) <= 256) {
    auto slab_ok = [&](const GemmArgs& q, int vec) {
      return vec && q.partials && store_wt_fits((long)q.M * q.N * (g.partial_half ? 2 : 4));   // (the pair shares g's slab type)
    };
    if (epi == EPI_GATE_RES && g.ksplit > 1 && slab_ok(g, plan.vec_out[0]) && (!g1 || slab_ok(g1s, plan.vec_out[1]))) plan.wt_out = 1;
  }
  return plan;
}

}  // namespace

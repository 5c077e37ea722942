// What the reference-keyed loader (weights.hip) and the low-rank merge (lora.hip) share: the scalar conversions between the
// checkpoint / arena dtypes and fp32, and THE table that says where a reference state-dict key of the DiT lands in the packed
// arena - slot name, index extents, checkpoint strides, packed strides and element offset.  The loader stores through that map;
// the merge walks the same map backwards (packed position -> checkpoint row / column) to add a low-rank product in place.
#pragma once
#include "../../include/foley_hip.h"
#include "kernels.h"

#include <cstdlib>
#include <cstring>
#include <string>

enum { DT_F16 = FOLEY_F16 };   // fp16: a checkpoint dtype and (precision=fp16) a compute / arena dtype

__host__ __device__ inline int dt_size(int dt) {
  return (dt == FOLEY_F8E4M3 || dt == FOLEY_F8E5M2) ? 1 : (dt == FOLEY_BF16 || dt == DT_F16) ? 2 : 4;
}

// ---- scalar conversions (device); fp8 follows the OCP formats torch implements, round-to-nearest-even.  NaNs decode to the
// bits torch's casts give (sign kept, payload left-aligned, quiet bit set), so a loaded arena equals the packers' byte for byte.
__device__ inline float f16_to_f32(uint16_t h) {
  const uint32_t s = (uint32_t)(h & 0x8000) << 16, e = (h >> 10) & 31, m = h & 1023;
  if (e == 0) {
    if (m == 0) return __uint_as_float(s);
    float v = (float)m * 5.9604644775390625e-08f;   // 2^-24
    return (h & 0x8000) ? -v : v;
  }
  if (e == 31) return __uint_as_float(s | 0x7f800000u | (m ? 0x00400000u : 0u) | (m << 13));
  return __uint_as_float(s | ((e + 112) << 23) | (m << 13));
}
template <int EB, int MB, bool FN>   // exponent / mantissa bits; FN: no infinities, NaN = all ones (e4m3fn)
__device__ inline float f8_to_f32(uint8_t v) {
  constexpr int BIAS = (1 << (EB - 1)) - 1;
  const uint32_t s = (uint32_t)(v & 0x80) << 24;
  const int e = (v >> MB) & ((1 << EB) - 1), m = v & ((1 << MB) - 1);
  if (FN ? ((v & 0x7f) == 0x7f) : (e == (1 << EB) - 1 && m != 0))
    return __uint_as_float(s | 0x7f800000u | (FN ? 0u : 0x00400000u) | ((uint32_t)m << (23 - MB)));
  if (!FN && e == (1 << EB) - 1) return __uint_as_float(s | 0x7f800000u);
  if (e == 0) {
    float x = (float)m * exp2f((float)(1 - BIAS - MB));
    return s ? -x : x;
  }
  return __uint_as_float(s | ((uint32_t)(e - BIAS + 127) << 23) | ((uint32_t)m << (23 - MB)));
}
template <int EB, int MB, bool FN>
__device__ inline uint8_t f32_to_f8(float f) {
  constexpr int BIAS = (1 << (EB - 1)) - 1;
  const uint32_t u = __float_as_uint(f);
  const uint8_t s = (uint8_t)((u >> 24) & 0x80);
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return s | 0x7f;                                    // NaN
  const float maxv = FN ? 448.0f : 57344.0f;
  const float af = __uint_as_float(a);
  if (FN) {
    if (af > 464.0f) return s | 0x7f;                                      // beyond the rounding range of 448: NaN (torch e4m3fn)
  } else if (af >= 61440.0f) {
    return s | 0x7c;                                                       // rounds to infinity (e5m2)
  }
  (void)maxv;
  const int e = (int)(a >> 23) - 127;                                      // unbiased exponent
  if (e < 1 - BIAS) {                                                      // subnormal of the target: fixed grid 2^(1-BIAS-MB)
    const float q = af * exp2f((float)(BIAS - 1 + MB));
    const float r = rintf(q);                                              // round-to-nearest-even
    return s | (uint8_t)r;                                                 // r == 2^MB lands on the first normal: same bits
  }
  uint32_t m = a & 0x7fffffu;
  const uint32_t drop = 23 - MB, half = 1u << (drop - 1);
  uint32_t keep = m >> drop;
  const uint32_t rem = m & ((1u << drop) - 1);
  int eb = e + BIAS;
  if (rem > half || (rem == half && (keep & 1))) {
    if (++keep == (1u << MB)) {
      keep = 0;
      ++eb;
    }
  }
  const uint8_t out = (uint8_t)((eb << MB) | keep);
  if (FN && (out & 0x7f) == 0x7f) return s | 0x7f;
  return s | out;
}

// one element as its raw bits (low dt_size(dt) bytes of the word) <-> fp32: the one widening and the one rounding every path uses
__device__ inline float bits_to_f32(uint32_t raw, int dt) {
  switch (dt) {
    case FOLEY_F32: return __uint_as_float(raw);
    case FOLEY_BF16: return bf16_to_f32((bf16_t)raw);
    case DT_F16: return f16_to_f32((uint16_t)raw);
    case FOLEY_F8E4M3: return f8_to_f32<4, 3, true>((uint8_t)raw);
    default: return f8_to_f32<5, 2, false>((uint8_t)raw);
  }
}
__device__ inline uint32_t f32_to_bits(float v, int dt) {
  switch (dt) {
    case FOLEY_F32: return __float_as_uint(v);
    case FOLEY_BF16: return f32_to_bf16(v);
    case DT_F16: return __builtin_bit_cast(uint16_t, (f16_t)v);
    case FOLEY_F8E4M3: return f32_to_f8<4, 3, true>(v);
    default: return f32_to_f8<5, 2, false>(v);
  }
}
__device__ inline float load_as_f32(const void* p, long i, int dt) {
  switch (dt_size(dt)) {
    case 4: return bits_to_f32(((const uint32_t*)p)[i], dt);
    case 2: return bits_to_f32(((const uint16_t*)p)[i], dt);
    default: return bits_to_f32(((const uint8_t*)p)[i], dt);
  }
}
__device__ inline void store_from_f32(void* p, long i, int dt, float v) {
  const uint32_t raw = f32_to_bits(v, dt);
  switch (dt_size(dt)) {
    case 4: ((uint32_t*)p)[i] = raw; break;
    case 2: ((uint16_t*)p)[i] = (uint16_t)raw; break;
    default: ((uint8_t*)p)[i] = (uint8_t)raw; break;
  }
}

// ---- reference key -> packed position
// One checkpoint tensor [O, I(, k)] (or a vector of O elements) lands in `slot` at element  out_off + sum_d idx[d] * os[d],
// read from checkpoint element  sum_d idx[d] * is[d],  idx[d] in [0, size[d]).  The first `row_dims` index dimensions walk the
// tensor's rows (dimension 0; their `is` are multiples of I*k, their `os` multiples of the packed row length), the others walk
// the flattened (I, k) of one row; the packed columns of a row are contiguous (the last `os` is 1).
struct KeyMap {
  std::string slot;
  int nd = 0, row_dims = 0;
  long size[4] = {1, 1, 1, 1}, is[4] = {0, 0, 0, 0}, os[4] = {0, 0, 0, 0};
  long out_off = 0;
  int64_t O = 0, I = 1, k = 1;   // the checkpoint shape [O, I, k]
  bool by_numel = false;         // a vector: only the element count is checked
  bool shape_ok = true;          // false: the configuration cannot hold this tensor (a SwiGLU half that is no multiple of 32 rows)
  bool matrix = false;           // a weight matrix (what a low-rank adapter may target); biases, gains and feature rows are not
  int mid_dt = -1;               // >= 0: the value is first rounded through this dtype (fp8 time-embedding quirk)
};

enum { KEY_MAPPED = 0, KEY_FOREIGN = 1, KEY_DEAD = 2, KEY_BAD_BLOCK = -1 };

namespace keymap {
inline void dims(KeyMap& m, int row_dims, std::initializer_list<long> size, std::initializer_list<long> is,
                 std::initializer_list<long> os) {
  m.nd = (int)size.size();
  m.row_dims = row_dims;
  int d = 0;
  auto b = is.begin();
  auto c = os.begin();
  for (auto a = size.begin(); a != size.end(); ++a, ++b, ++c, ++d) { m.size[d] = *a; m.is[d] = *b; m.os[d] = *c; }
}
// [N] vector, or [N, K] matrix stored as it is
inline KeyMap plain(const std::string& slot, int64_t N, int64_t K, int mid_dt = -1) {
  KeyMap m;
  m.slot = slot; m.O = N; m.I = K; m.by_numel = K == 1; m.matrix = K != 1; m.mid_dt = mid_dt;
  dims(m, 1, {N, K}, {K, 1}, {K, 1});
  return m;
}
inline KeyMap vec(const std::string& slot, int64_t N, int mid_dt = -1) { return plain(slot, N, 1, mid_dt); }
// [O, I, k] -> [O, k*I] (K index = tap*I + c)
inline KeyMap conv(const std::string& slot, int64_t O, int64_t I, int64_t k) {
  KeyMap m;
  m.slot = slot; m.O = O; m.I = I; m.k = k; m.matrix = true;
  dims(m, 1, {O, k, I}, {I * k, 1, k}, {k * I, I, 1});
  return m;
}
// SwiGLU half `slot01` (0: w1, 1: w3) of [Hh, I(, k)] into alternating 32-row groups of [2*Hh, k*I]
inline KeyMap gate(const std::string& slot, int slot01, int64_t Hh, int64_t I, int64_t k) {
  KeyMap m;
  m.slot = slot; m.O = Hh; m.I = I; m.k = k; m.matrix = true; m.shape_ok = Hh % 32 == 0;
  const long KI = k * I;
  dims(m, 2, {Hh / 32, 32, k, I}, {32 * I * k, I * k, 1, k}, {64 * KI, KI, I, 1});
  m.out_off = slot01 * 32 * KI;
  return m;
}
}  // namespace keymap

// The DiT's keys.  KEY_MAPPED: *m is filled; KEY_FOREIGN: not a tensor of the DiT's sampling path; KEY_DEAD: accepted and unused
// (final_layer.adaLN_modulation, dead code with 3-D conditioning); KEY_BAD_BLOCK: a block index beyond the depth.
// wfmt: the arena's weight format (0: compute dtype; 1 / 2: fp8 block matrices), which only decides the time-embedding quirk.
inline int dit_key_map(const foley_config& f, int wfmt, const std::string& key, KeyMap* m) {
  using namespace keymap;
  const int64_t D = f.hidden, H = f.heads, hd = D / H;
  auto blk = [&](const char* prefix, int* b, std::string* rest) {
    const size_t n = strlen(prefix);
    if (key.compare(0, n, prefix)) return false;
    const size_t dot = key.find('.', n);
    if (dot == std::string::npos) return false;
    *b = atoi(key.substr(n, dot - n).c_str());
    *rest = key.substr(dot + 1);
    return true;
  };
  int b = 0;
  std::string r;
  if (blk("triple_blocks.", &b, &r)) {
    if (b < 0 || b >= f.depth_triple) return KEY_BAD_BLOCK;
    const std::string p = "t" + std::to_string(b) + ".";
    static const struct { const char* ref; const char* packed; int n_mul; int k_kind; } LIN[] = {
        {"audio_mod.linear", "a_mod", 9, 0}, {"v_cond_mod.linear", "v_mod", 9, 0},
        {"audio_self_attn_qkv", "a_qkv", 3, 0}, {"v_cond_attn_qkv", "v_qkv", 3, 0},
        {"audio_self_proj", "a_proj", 1, 0}, {"v_cond_self_proj", "v_proj", 1, 0},
        {"audio_cross_q", "a_cq", 1, 0}, {"v_cond_cross_q", "v_cq", 1, 0}, {"text_cross_kv", "t_kv", 2, 0},
        {"audio_cross_proj", "a_cproj", 1, 0}, {"v_cond_cross_proj", "v_cproj", 1, 0},
        {"audio_mlp.fc1", "a_fc1", -1, 0}, {"v_cond_mlp.fc1", "v_fc1", -1, 0},
        {"audio_mlp.fc2", "a_fc2", 1, 1}, {"v_cond_mlp.fc2", "v_fc2", 1, 1}};
    for (const auto& L : LIN) {
      const std::string n = L.ref;
      const int64_t N = L.n_mul < 0 ? f.mlp_hidden : L.n_mul * D, K = L.k_kind ? f.mlp_hidden : D;
      if (r == n + ".weight") return *m = plain(p + L.packed + ".w", N, K), KEY_MAPPED;
      if (r == n + ".bias") return *m = vec(p + L.packed + ".b", N), KEY_MAPPED;
    }
    static const struct { const char* ref; const char* packed; } GAIN[] = {
        {"audio_self_q_norm", "a_qn"}, {"audio_self_k_norm", "a_kn"}, {"v_cond_attn_q_norm", "v_qn"},
        {"v_cond_attn_k_norm", "v_kn"}, {"audio_cross_q_norm", "a_cqn"}, {"v_cond_cross_q_norm", "v_cqn"},
        {"text_cross_k_norm", "t_kn"}};
    for (const auto& G : GAIN)
      if (r == std::string(G.ref) + ".weight") return *m = vec(p + G.packed, hd), KEY_MAPPED;
    return KEY_FOREIGN;
  }
  if (blk("single_blocks.", &b, &r)) {
    if (b < 0 || b >= f.depth_single) return KEY_BAD_BLOCK;
    const std::string p = "s" + std::to_string(b) + ".";
    const int64_t Hc = f.conv_hidden;
    if (r == "modulation.linear.weight") {   // block b of the stacked [n_single*6D, D] matrix
      *m = plain("smod_all.w", 6 * D, D);
      m->out_off = (long)b * 6 * D * D;
      return KEY_MAPPED;
    }
    if (r == "modulation.linear.bias") {
      *m = vec("smod_all.b", 6 * D);
      m->out_off = (long)b * 6 * D;
      return KEY_MAPPED;
    }
    if (r == "linear_qkv.weight") {   // rows "(H D K)" -> "(K H D)"  (hifi_foley.py:362)
      *m = plain(p + "qkv.w", 3 * D, D);
      dims(*m, 3, {3, H, hd, D}, {D, hd * 3 * D, 3 * D, 1}, {H * hd * D, hd * D, D, 1});
      return KEY_MAPPED;
    }
    if (r == "linear_qkv.bias") {
      *m = vec(p + "qkv.b", 3 * D);
      dims(*m, 3, {3, H, hd}, {1, hd * 3, 3}, {H * hd, hd, 1});
      return KEY_MAPPED;
    }
    if (r == "q_norm.weight") return *m = vec(p + "qn", hd), KEY_MAPPED;
    if (r == "k_norm.weight") return *m = vec(p + "kn", hd), KEY_MAPPED;
    if (r == "linear1.weight") return *m = conv(p + "lin1.w", D, D, 3), KEY_MAPPED;
    if (r == "linear1.bias") return *m = vec(p + "lin1.b", D), KEY_MAPPED;
    if (r == "linear2.w1.weight") return *m = gate(p + "w13.w", 0, Hc, D, 3), KEY_MAPPED;
    if (r == "linear2.w3.weight") return *m = gate(p + "w13.w", 1, Hc, D, 3), KEY_MAPPED;
    if (r == "linear2.w2.weight") return *m = conv(p + "w2.w", D, Hc, 3), KEY_MAPPED;
    return KEY_FOREIGN;
  }
  const bool f8time = wfmt != 0 && foley_is_half(f.compute_dtype);   // golden g8 "Q14": the first time-embedding bias passes through fp8
  if (key == "audio_embedder.proj.weight") return *m = plain("audio_in.w", D, f.latent_dim), KEY_MAPPED;
  if (key == "audio_embedder.proj.bias") return *m = vec("audio_in.b", D), KEY_MAPPED;
  if (key == "visual_proj.w1.weight") return *m = gate("vis.w13.w", 0, D, f.clip_dim, 1), KEY_MAPPED;
  if (key == "visual_proj.w3.weight") return *m = gate("vis.w13.w", 1, D, f.clip_dim, 1), KEY_MAPPED;
  if (key == "visual_proj.w2.weight") return *m = plain("vis.w2.w", D, D), KEY_MAPPED;
  if (key == "cond_in.linear_1.weight") return *m = plain("cond1.w", D, f.cond_dim), KEY_MAPPED;
  if (key == "cond_in.linear_1.bias") return *m = vec("cond1.b", D), KEY_MAPPED;
  if (key == "cond_in.linear_2.weight") return *m = plain("cond2.w", D, D), KEY_MAPPED;
  if (key == "cond_in.linear_2.bias") return *m = vec("cond2.b", D), KEY_MAPPED;
  if (key == "time_in.mlp.0.weight") return *m = plain("time0.w", D, f.time_freq_dim), KEY_MAPPED;
  if (key == "time_in.mlp.0.bias")
    return *m = vec("time0.b", D, f8time ? (wfmt == 1 ? FOLEY_F8E4M3 : FOLEY_F8E5M2) : -1), KEY_MAPPED;
  if (key == "time_in.mlp.2.weight") return *m = plain("time2.w", D, D), KEY_MAPPED;
  if (key == "time_in.mlp.2.bias") return *m = vec("time2.b", D), KEY_MAPPED;
  if (key == "sync_in.0.weight") return *m = plain("sync0.w", D, f.sync_dim), KEY_MAPPED;
  if (key == "sync_in.0.bias") return *m = vec("sync0.b", D), KEY_MAPPED;
  if (key == "sync_in.2.w1.weight") return *m = gate("sync.w13.w", 0, f.sync_hidden, D, 1), KEY_MAPPED;
  if (key == "sync_in.2.w3.weight") return *m = gate("sync.w13.w", 1, f.sync_hidden, D, 1), KEY_MAPPED;
  if (key == "sync_in.2.w2.weight") return *m = plain("sync.w2.w", D, f.sync_hidden), KEY_MAPPED;
  if (key == "sync_pos_emb") {
    *m = plain("sync_pos", 8, f.sync_dim);
    m->by_numel = true;
    m->matrix = false;
    return KEY_MAPPED;
  }
  if (key == "final_layer.linear.weight") return *m = plain("final.w", f.latent_dim, D), KEY_MAPPED;
  if (key == "final_layer.linear.bias") return *m = vec("final.b", f.latent_dim), KEY_MAPPED;
  if (key == "empty_clip_feat") return *m = vec("empty_clip", f.clip_dim), KEY_MAPPED;
  if (key == "empty_sync_feat") return *m = vec("empty_sync", f.sync_dim), KEY_MAPPED;
  if (key.compare(0, 29, "final_layer.adaLN_modulation.") == 0) return KEY_DEAD;
  return KEY_FOREIGN;
}

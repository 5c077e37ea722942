// Timeline cross-attention for gfx950, head_dim = 128: every query attends the text set of its own time
// (host/prompt_timeline.py; kernels.h AttnTimelineArgs).
//   out[q] = (1 - alpha[q]) * softmax(q K_a^T / sqrt(128)) V_a + alpha[q] * softmax(q K_b^T / sqrt(128)) V_b,   a = set_a[q], b = set_b[q]
// One wavefront owns 32 query rows, with the operand layouts of attention.hip (scores transposed, S^T = K Q^T, so that a lane
// holds 16 keys of ONE query and the exponentiated scores are the B operand of O^T += V^T P^T in place).  The wave makes one full
// pass - its own online softmax over all Skv keys - per set that some row of the tile uses; sets no row uses are skipped by a
// wave-uniform test.  Every pass is computed for all 32 rows alike and a row then takes its one or two weighted, normalised results
// by a per-lane SELECT (never a multiplication by zero: a set the row does not use may hold anything, NaN included), so a row's bits
// do not depend on its tile-mates and, where alpha == 0, the output is the plain attention against set_a: 0 + 1.0f * x.
// The set indices come from a caller's device table: they are clamped to [0, n_sets) before they address anything.
#include "kernels.h"

namespace {

template <typename OutT> __device__ __forceinline__ void tl_store4(OutT* p, const f32x4 v) {
  if constexpr (sizeof(OutT) == 4) {
    *(f32x4*)p = v;
  } else {
    uint2 w;
    w.x = pack_h2<OutT>(v[0], v[1]);
    w.y = pack_h2<OutT>(v[2], v[3]);
    *(uint2*)p = w;
  }
}

// What query column j of this tile reads: its clamped sets and weight.  Rows past the sequence use nothing.
struct TlRow {
  int sa, sb;
  float al;
  bool live;
};
__device__ __forceinline__ TlRow tl_row(const AttnTimelineArgs& a, int b, int tok) {
  TlRow r{0, 0, 0.f, tok < a.Sq};
  if (r.live) {
    const long i = (long)b * a.Sq + tok;
    r.sa = min(max(a.set_a[i], 0), a.n_sets - 1);
    r.sb = min(max(a.set_b[i], 0), a.n_sets - 1);
    r.al = a.alpha[i];
  }
  return r;
}

// acc += w_a * val (rows whose set_a is s) and += w_b * val (rows that blend towards s); other rows keep acc untouched
__device__ __forceinline__ void tl_blend(f32x16 (&acc)[4], const f32x16 (&o)[4], float inv, bool use_a, bool use_b, float al) {
  const float wa = 1.0f - al;
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float val = o[d][e] * inv;
      float r = acc[d][e];
      r = use_a ? r + wa * val : r;
      r = use_b ? r + al * val : r;
      acc[d][e] = r;
    }
}

template <typename OutT> __device__ __forceinline__ void tl_write(const AttnTimelineArgs& a, const f32x16 (&acc)[4], int b, int h, int tok, int kh) {
  if (tok >= a.Sq) return;
  OutT* dst;
  if (tok < a.split) dst = (OutT*)a.outA + ((long)b * a.split + tok) * (a.H * 128);
  else dst = (OutT*)a.outB + ((long)b * (a.Sq - a.split) + (tok - a.split)) * (a.H * 128);
  dst += h * 128;
  // lane (j, kh) holds dims d*32 + 8*g4 + 4*kh + {0..3} of query j: 4 consecutive outputs per store
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const f32x4 v = {acc[d][g4 * 4 + 0], acc[d][g4 * 4 + 1], acc[d][g4 * 4 + 2], acc[d][g4 * 4 + 3]};
      tl_store4<OutT>(dst + d * 32 + 8 * g4 + 4 * kh, v);
    }
}

// fp32 operands (parity mode) on v_mfma_f32_32x32x2_f32: the pass over one set is attn_kernel's loop (attention.hip).
template <typename OutT>
__global__ __launch_bounds__(64) void attn_tl_kernel(const AttnTimelineArgs a) {
  constexpr int HD = 128, HH = 64, NC = 16;
  const int lane = threadIdx.x;
  const int j = lane & 31, kh = lane >> 5;
  const int q0 = blockIdx.x * 32;
  const int h = blockIdx.y, b = blockIdx.z;
  const float* __restrict__ Q = (const float*)a.q + ((long)(b * a.H + h) * a.Sq) * HD;
  const float scale = 0.08838834764831845f;
  const TlRow row = tl_row(a, b, q0 + j);

  float qr[HH];
  {
    const f32x4* p = (const f32x4*)(Q + (long)min(q0 + j, a.Sq - 1) * HD + kh * HH);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const f32x4 v = p[c];
      qr[c * 4 + 0] = v[0]; qr[c * 4 + 1] = v[1]; qr[c * 4 + 2] = v[2]; qr[c * 4 + 3] = v[3];
    }
  }
  f32x16 acc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[d][e] = 0.f;

  for (int s = 0; s < a.n_sets; ++s) {
    const bool use_a = row.live && row.sa == s, use_b = row.live && row.sb == s && row.al != 0.f;
    if (__builtin_amdgcn_ballot_w64(use_a || use_b) == 0) continue;   // wave-uniform: no row of the tile reads this set
    const float* __restrict__ K = (const float*)a.k + ((long)(s * a.H + h) * a.Skv) * HD;
    const float* __restrict__ V = (const float*)a.v + ((long)(s * a.H + h) * a.Skv) * HD;
    f32x16 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[d][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    for (int kt = 0; kt < a.Skv; kt += 32) {
      f32x16 sc;
#pragma unroll
      for (int e = 0; e < 16; ++e) sc[e] = 0.f;
      {
        const f32x4* p = (const f32x4*)(K + (long)min(kt + j, a.Skv - 1) * HD + kh * HH);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const f32x4 v = p[c];
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[0], qr[c * 4 + 0], sc, 0, 0, 0);
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[1], qr[c * 4 + 1], sc, 0, 0, 0);
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[2], qr[c * 4 + 2], sc, 0, 0, 0);
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[3], qr[c * 4 + 3], sc, 0, 0, 0);
        }
      }
      // sc[e] = score(key kt + r(e), query q0 + j), r(e) = (e&3) + 8*(e>>2) + 4*kh
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = kt + (e & 3) + 8 * (e >> 2) + 4 * kh;
        sc[e] = (key < a.Skv) ? sc[e] * scale : -INFINITY;
        mx = fmaxf(mx, sc[e]);
      }
      mx = xhalf_max(mx);
      const float m_new = fmaxf(m_run, mx);     // every tile holds at least one valid key
      const float resc = expf(m_run - m_new);   // exp(-inf) = 0 on the first tile
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        sc[e] = expf(sc[e] - m_new);
        ps += sc[e];
      }
      ps = xhalf_sum(ps);
      l_run = l_run * resc + ps;
      m_run = m_new;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[d][e] *= resc;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int vrow = min(kt + (t & 3) + 8 * (t >> 2) + 4 * kh, a.Skv - 1);
        const float* vp = V + (long)vrow * HD + j;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[d * 32], sc[t], o[d], 0, 0, 0);
      }
    }
    tl_blend(acc, o, 1.0f / l_run, use_a, use_b, row.al);
  }
  tl_write<OutT>(a, acc, b, h, q0 + j, kh);
}

// 16-bit operands (bf16 / fp16) on v_mfma_f32_32x32x16: Skv <= 96, so a set is at most three key tiles and the wave walks them
// itself (no key split across waves, no LDS).  The pass over one set is the tile of attn_bf16_kernel (attention.hip): permuted key
// rows (pi) so that a lane's 16 scores are 16 consecutive keys, log2-domain exponentials, P rounded once to the operand type.
// bf16: a probability travels as TWO bf16 values, its rounding and the rounding's residual, and P V runs over both (PSPLIT, as
// attn_bf16_wide_kernel does at head dim 64).  A text set may be a handful of keys - a short prompt, or the 5-key case of
// tests/test_timeline_ops_gpu.py - and one 8-bit probability then carries a row's whole error, up to 2^-8 of sum p |v|, twice what the
// per-element bound of tests/opcheck.py allows (measured: 1.08 x the bound at 5 keys); with the residual the rounding of P drops to
// 2^-16.  Eight more MFMAs per tile; fp16 (11 bits) does not need it.
template <typename T, typename OutT>
__global__ __launch_bounds__(64) void attn_tl16_kernel(const AttnTimelineArgs a) {
  constexpr int HD = 128;
  constexpr bool PSPLIT = __is_same(T, bf16_t);
  const int lane = threadIdx.x;
  const int j = lane & 31, kh = lane >> 5;
  const int q0 = blockIdx.x * 32;
  const int h = blockIdx.y, b = blockIdx.z;
  const T* __restrict__ Q = (const T*)a.q + ((long)(b * a.H + h) * a.Sq) * HD;
  const float scale2 = 0.08838834764831845f * 1.4426950408889634f;   // log2(e) / sqrt(128)
  const TlRow row = tl_row(a, b, q0 + j);

  bf16x8 qf[8];
  {
    const T* p = Q + (long)min(q0 + j, a.Sq - 1) * HD + 8 * kh;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *(const bf16x8*)(p + 16 * s);
  }
  f32x16 acc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[d][e] = 0.f;
  const int pi = 16 * ((j >> 2) & 1) + (j & 3) + 4 * (j >> 3);  // A-row j carries key kt + pi

  for (int s = 0; s < a.n_sets; ++s) {
    const bool use_a = row.live && row.sa == s, use_b = row.live && row.sb == s && row.al != 0.f;
    if (__builtin_amdgcn_ballot_w64(use_a || use_b) == 0) continue;   // wave-uniform: no row of the tile reads this set
    const T* __restrict__ K = (const T*)a.k + ((long)(s * a.H + h) * a.Skv) * HD;
    const T* __restrict__ VT = (const T*)a.v + ((long)(s * a.H + h) * HD) * a.vt_pitch;
    f32x16 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[d][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    for (int kt = 0; kt < a.Skv; kt += 32) {
      bf16x8 kf[8], vf[2][4];
      {
        const T* p = K + (long)min(kt + pi, a.Skv - 1) * HD + 8 * kh;
#pragma unroll
        for (int st = 0; st < 8; ++st) kf[st] = *(const bf16x8*)(p + 16 * st);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int d = 0; d < 4; ++d) vf[u][d] = *(const bf16x8*)(VT + (long)(d * 32 + j) * a.vt_pitch + kt + 16 * kh + 8 * u);
      f32x16 sc;
#pragma unroll
      for (int e = 0; e < 16; ++e) sc[e] = 0.f;
#pragma unroll
      for (int st = 0; st < 8; ++st) sc = mfma16<T>(kf[st], qf[st], sc);
      // sc[e] = score(key kt + 16*kh + e, query q0 + j), kept in the log2 domain
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        sc[e] = (kt + 16 * kh + e < a.Skv) ? sc[e] * scale2 : -INFINITY;
        mx = fmaxf(mx, sc[e]);
      }
      mx = xhalf_max(mx);
      const float m_new = fmaxf(m_run, mx);
      float ps = 0.f;
      bf16x8 pb[2], pr[PSPLIT ? 2 : 1];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float pv = __builtin_amdgcn_exp2f(sc[e] - m_new);
        ps += pv;
        const __bf16 hi = to_carrier<T>(pv);
        pb[e >> 3][e & 7] = hi;
        if constexpr (PSPLIT) pr[e >> 3][e & 7] = (__bf16)(pv - (float)hi);   // exact difference, rounded once more
      }
      ps = xhalf_sum(ps);
      const float resc = __builtin_amdgcn_exp2f(m_run - m_new);   // exp2(-inf) = 0 on the first tile
      l_run = l_run * resc + ps;
      m_run = m_new;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[d][e] *= resc;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          o[d] = mfma16<T>(vf[u][d], pb[u], o[d]);
          if constexpr (PSPLIT) o[d] = mfma16<T>(vf[u][d], pr[u], o[d]);
        }
    }
    tl_blend(acc, o, 1.0f / l_run, use_a, use_b, row.al);
  }
  tl_write<OutT>(a, acc, b, h, q0 + j, kh);
}

}  // namespace

int launch_attention_timeline(const AttnTimelineArgs& a, int out_dtype, hipStream_t st) {
  if (!a.q || !a.k || !a.v || !a.set_a || !a.set_b || !a.alpha || !a.outA || !a.outB)
    return foley_set_err("timeline attention: null operand", __FILE__, __LINE__);
  if (a.Bq <= 0 || a.H <= 0 || a.Sq <= 0 || a.Skv <= 0 || a.n_sets <= 0)
    return foley_set_err("timeline attention: empty problem", __FILE__, __LINE__);
  if (a.split < 0 || a.split > a.Sq) return foley_set_err("timeline attention: split outside [0, Sq]", __FILE__, __LINE__);
  if (a.Bq > 65535 || a.H > 65535) return foley_set_err("timeline attention: more than 65535 batch rows or heads", __FILE__, __LINE__);
  const dim3 grid((a.Sq + 31) / 32, a.H, a.Bq), block(64);
  if (foley_is_half(a.in_dtype)) {
    if (a.Skv > 96) return foley_set_err("timeline attention: 16-bit operands take at most 96 keys per set", __FILE__, __LINE__);
    if (a.vt_pitch < ((a.Skv + 31) & ~31) || (a.vt_pitch & 7))
      return foley_set_err("timeline attention: V^T pitch must cover Skv rounded up to 32 (multiple of 8)", __FILE__, __LINE__);
    if (out_dtype != a.in_dtype && out_dtype != FOLEY_F32)
      return foley_set_err("timeline attention: 16-bit operands produce the same type or fp32", __FILE__, __LINE__);
    const bool h16 = a.in_dtype == FOLEY_F16, o32 = out_dtype == FOLEY_F32;
    if (h16) {
      if (o32) FOLEY_LAUNCH((attn_tl16_kernel<f16_t, float>), grid, block, 0, st, a);
      else FOLEY_LAUNCH((attn_tl16_kernel<f16_t, f16_t>), grid, block, 0, st, a);
    } else {
      if (o32) FOLEY_LAUNCH((attn_tl16_kernel<bf16_t, float>), grid, block, 0, st, a);
      else FOLEY_LAUNCH((attn_tl16_kernel<bf16_t, bf16_t>), grid, block, 0, st, a);
    }
  } else if (a.in_dtype == FOLEY_F32) {
    if (out_dtype == FOLEY_F32) FOLEY_LAUNCH((attn_tl_kernel<float>), grid, block, 0, st, a);
    else if (out_dtype == FOLEY_BF16) FOLEY_LAUNCH((attn_tl_kernel<bf16_t>), grid, block, 0, st, a);
    else if (out_dtype == FOLEY_F16) FOLEY_LAUNCH((attn_tl_kernel<f16_t>), grid, block, 0, st, a);
    else return foley_set_err("timeline attention: bad output dtype", __FILE__, __LINE__);
  } else {
    return foley_set_err("timeline attention: operands are fp32, bf16 or fp16", __FILE__, __LINE__);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return foley_set_err(hipGetErrorString(e), __FILE__, __LINE__);
  return 0;
}

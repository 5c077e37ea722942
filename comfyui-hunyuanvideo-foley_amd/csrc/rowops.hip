// HBM-bound row kernels of the Foley path: LayerNorm+modulate, RMSNorm+RoPE head split, small
// elementwise helpers, the solver update and the DAC output convolution.  All arithmetic fp32;
// one wavefront per row with 16-byte vector accesses and wave-level (DPP) reductions.
#include <type_traits>

#include "kernels.h"

namespace {

#define FOLEY_LAUNCH_CHECK()                                                             \
  do {                                                                                   \
    hipError_t _e = hipGetLastError();                                                   \
    if (_e != hipSuccess) return foley_set_err(hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// ------------------------------------------------------------------ LayerNorm (+ AdaLN modulate)
// reference: nn.LayerNorm(elementwise_affine=False) + modulate() (modulate_layers.py:19-30) and
// SingleStreamBlock's norm*(1+scale)+shift (hifi_foley.py:368,387)
// store_wt: the same four values write-through, at byte offset `off` behind a wave-uniform base (common.h GStore)
template <typename OutT> struct Pack4;
template <> struct Pack4<float> {
  static __device__ __forceinline__ void store(float* p, const f32x4 v) { *(f32x4*)p = v; }
  static __device__ __forceinline__ void store_wt(void* base, unsigned bytes, unsigned off, const f32x4 v) {
    GStore<ST_WT>::st16(base, bytes, off, __builtin_bit_cast(u32x4, v));
  }
};
template <> struct Pack4<bf16_t> {
  static __device__ __forceinline__ void store(bf16_t* p, const f32x4 v) {
    uint2 w;
    w.x = pack_bf16x2(v[0], v[1]);
    w.y = pack_bf16x2(v[2], v[3]);
    *(uint2*)p = w;
  }
  static __device__ __forceinline__ void store_wt(void* base, unsigned bytes, unsigned off, const f32x4 v) {
    const u32x2 w = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    GStore<ST_WT>::st8(base, bytes, off, w);
  }
};

template <> struct Pack4<f16_t> {
  static __device__ __forceinline__ void store(f16_t* p, const f32x4 v) {
    uint2 w;
    w.x = pack_f16x2(v[0], v[1]);
    w.y = pack_f16x2(v[2], v[3]);
    *(uint2*)p = w;
  }
  static __device__ __forceinline__ void store_wt(void* base, unsigned bytes, unsigned off, const f32x4 v) {
    const u32x2 w = {pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3])};
    GStore<ST_WT>::st8(base, bytes, off, w);
  }
};

// four consecutive partial products of a slab row: fp32, or the 16-bit operand type
template <typename ST> __device__ __forceinline__ f32x4 slab_load4(const void* base, long elem) {
  if constexpr (sizeof(ST) == 4) {
    return *(const f32x4*)((const float*)base + elem);
  } else {
    const uint2 w = *(const uint2*)((const ST*)base + elem);
    const ST* h = (const ST*)&w;
    f32x4 v = {Cvt<ST>::from(h[0]), Cvt<ST>::from(h[1]), Cvt<ST>::from(h[2]), Cvt<ST>::from(h[3])};
    return v;
  }
}

// One wave per row; every global load of the row (x, shift, scale) is issued before the first
// reduction so the kernel pays one memory round trip, results leave as 8/16-byte vector stores.
// LnPair: the two row sets of a launch as the caller describes them (the per-operand kernels read it as it is).
struct LnPair {
  LnArgs a[2];
  int blocks0;
};
static long long* g_ln_dbg = nullptr;
extern "C" void foley_debug_ln_timeline(void* p) { g_ln_dbg = (long long*)p; }
// tests: did this thread's last LayerNorm launch take the write-through kernel (launch_ln_mod_pair)?
static thread_local int g_ln_last_wt = 0;
extern "C" int foley_debug_ln_last_wt() { return g_ln_last_wt; }

// The resolved launch (common.h RowMap): what the kernels read of one row set, packed so that the selected set arrives in two wide
// scalar loads at entry - 120 bytes instead of LnArgs' 288 with their fields fetched where they are first used.
struct LnRes {
  float* x;
  void* out;
  const float *shift, *scale, *gate;   // operand bases (null: absent); the gate belongs to the pending update
  const float *partials, *bias;        // LnPending
  long pstride;
  int M, k;
  RowMap map;                          // of shift, scale and gate alike
};
struct LnResPair {
  const int* step_ptr;   // the launch's one counter; without one, any readable word (every step_stride is then 0)
  int blocks0;
  LnRes a[2];
  long long* dbg;        // DBG instantiations (tools/ln_timeline.py): 4 wall-clock stamps per workgroup of the wide kernel
};

// One batch of SB pending slabs of a row.  The loads (clamped slab index keeps them unconditional) leave the slabs as they are
// stored - a conversion here would wait for them before the operand rows are requested - ...
template <typename ST> struct SlabRaw { using type = f32x4; };
template <> struct SlabRaw<bf16_t> { using type = uint2; };
template <> struct SlabRaw<f16_t> { using type = uint2; };
template <typename ST> __device__ __forceinline__ f32x4 slab_cvt4(const typename SlabRaw<ST>::type& w) {
  if constexpr (sizeof(ST) == 4) {
    return w;
  } else {
    const ST* h = (const ST*)&w;
    f32x4 v = {Cvt<ST>::from(h[0]), Cvt<ST>::from(h[1]), Cvt<ST>::from(h[2]), Cvt<ST>::from(h[3])};
    return v;
  }
}
template <typename ST, int MAXV, int SB, typename ColFn>
__device__ __forceinline__ void slab_batch_load(typename SlabRaw<ST>::type (&t)[SB][MAXV], const void* partials, long pstride, int k, int s0, long row_elem,
                                                ColFn col) {
#pragma unroll
  for (int u = 0; u < SB; ++u) {
    const int s = min(s0 + u, k - 1);
    const long pe = s * pstride + row_elem;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) t[u][i] = *(const typename SlabRaw<ST>::type*)((const ST*)partials + pe + 4L * col(i));
  }
}
// ... and their sum into acc, in slab order (weight 0 drops the repeats of the last slab)
template <typename ST, int MAXV, int SB>
__device__ __forceinline__ void slab_batch_add(f32x4 (&acc)[MAXV], const typename SlabRaw<ST>::type (&t)[SB][MAXV], int k, int s0) {
#pragma unroll
  for (int u = 0; u < SB; ++u) {
    const float w = (s0 + u < k) ? 1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const f32x4 tv = slab_cvt4<ST>(t[u][i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][e] += w * tv[e];
    }
  }
}

// The counter of a resolved launch: one scalar load, issued by ln_step_issue and waited for by ln_step_wait, in the places the
// kernels choose.  Scalar loads return out of order, so any wait for a kernel argument waits for every scalar load in flight -
// and the compiler fetches an argument in the block that first uses it.  Every field of the row set is therefore an input of
// the issuing statement: all are resident (one wait) before the counter's load goes out, and nothing waits for the counter
// until rb_map_off needs its value - the x, bias and slab loads are issued in between.  The compiler does not track the load:
// the value must pass through ln_step_wait before its first use.  step_ptr is never null (the launcher sees to it).
__device__ __forceinline__ int ln_step_issue(const LnRes& A, const int* step_ptr) {
  int v;
  asm volatile("s_load_dword %0, %1, 0x0"
               : "=&s"(v)
               : "s"(step_ptr), "s"(A.x), "s"(A.out), "s"(A.shift), "s"(A.scale), "s"(A.gate), "s"(A.partials), "s"(A.bias), "s"(A.pstride), "s"(A.M), "s"(A.k),
                 "s"(A.map.ld), "s"(A.map.step_stride), "s"(A.map.mode), "s"(A.map.rows_per_cfg), "s"(A.map.L), "s"(A.map.Ls), "s"(A.map.scale),
                 "s"(A.map.per), "s"(A.map.dense_from), "s"(A.map.dense_base));
  return v;
}
__device__ __forceinline__ int ln_step_wait(int v) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v));
  return v;
}

// Resolved one-wave-per-row kernel.  Order of the memory work: the counter (scalar), then everything that does not depend on it
// - x, the bias and the first batch of slabs -, then the row offset (its divisions run under those loads), and only then the
// wait for the counter and the shift / scale / gate rows.  The arithmetic is ln_mod_each_kernel's, operation for operation.
template <typename OutT, int MAXV, bool PEND, bool SLAB16 = false>
__global__ __launch_bounds__(128) void ln_mod_kernel(const LnResPair pr, int D, float eps) {
  using ST = typename std::conditional<SLAB16, OutT, float>::type;   // slab element type
  constexpr int SB = 6;
  const int sel = (int)blockIdx.x >= pr.blocks0 ? 1 : 0;
  const LnRes& A = pr.a[sel];
  const int step_sent = ln_step_issue(A, pr.step_ptr);
  const int M = A.M;
  OutT* __restrict__ out = (OutT*)A.out;
  const int row = ((int)blockIdx.x - (sel ? pr.blocks0 : 0)) * 2 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const int nv = D >> 2;  // float4 per row
  f32x4* xr = (f32x4*)(A.x + (long)row * D);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  const bool pend = PEND && A.partials;
  const auto col = [&](int i) { return min(lane + i * 64, nv - 1); };   // clamped: loads stay unconditional
  f32x4 v[MAXV], hv[MAXV], cv[MAXV], acc[MAXV], gt[MAXV];
  typename SlabRaw<ST>::type t[PEND ? SB : 1][MAXV];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) v[i] = xr[col(i)];
  if (pend) {
    const f32x4* bp = (const f32x4*)A.bias;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) acc[i] = bp ? bp[col(i)] : z4;
    if constexpr (PEND) slab_batch_load<ST, MAXV, SB>(t, A.partials, A.pstride, A.k, 0, (long)row * D, col);
  }
  const long row_off = rb_map_off(A.map, 0, row);   // the divisions of modes 1 and 2 run under the loads above
  const long off = row_off + (long)ln_step_wait(step_sent) * A.map.step_stride;
  const f32x4* sh = A.shift ? (const f32x4*)(A.shift + off) : nullptr;
  const f32x4* sc = A.scale ? (const f32x4*)(A.scale + off) : nullptr;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    hv[i] = sh ? sh[col(i)] : z4;
    cv[i] = sc ? sc[col(i)] : z4;
  }
  if constexpr (PEND) {
    if (pend) {
      // finish the deferred split-K GEMM: x += gate * (sum of partial products + bias), SB slabs in flight at a time
      const f32x4* gp = (const f32x4*)(A.gate + off);
#pragma unroll
      for (int i = 0; i < MAXV; ++i) gt[i] = gp[col(i)];
      for (int s0 = 0; s0 < A.k; s0 += SB) {
        if (s0 > 0) slab_batch_load<ST, MAXV, SB>(t, A.partials, A.pstride, A.k, s0, (long)row * D, col);
        slab_batch_add<ST, MAXV, SB>(acc, t, A.k, s0);
      }
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] += gt[i][e] * acc[i][e];
        if (lane + i * 64 < nv) xr[lane + i * 64] = v[i];
      }
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + i * 64 < nv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + i * 64 < nv) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float d = v[i][u] - mean;
        q += d * d;
      }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  OutT* orow = out + (long)row * D;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      f32x4 y;
#pragma unroll
      for (int u = 0; u < 4; ++u) y[u] = (v[i][u] - mean) * rstd * (1.0f + cv[i][u]) + hv[i][u];
      Pack4<OutT>::store(orow + c * 4, y);
    }
  }
}

// The per-operand path, for a launch whose operands do not share one counter and one row map: every RowBcast resolves itself
// through rb_row.  One launch of run_forward's 126 per iteration is of this kind - the first LayerNorm of the single-stream
// blocks, whose pending gate is still the two-stream blocks' vector while shift and scale are per-token rows.
// SLAB16: the pending slabs hold OutT (a 16-bit type) instead of fp32
template <typename OutT, int MAXV, bool PEND, bool SLAB16 = false>
__global__ __launch_bounds__(128) void ln_mod_each_kernel(const LnPair pr, int D, float eps) {
  using ST = typename std::conditional<SLAB16, OutT, float>::type;   // slab element type
  const int sel = (int)blockIdx.x >= pr.blocks0 ? 1 : 0;
  const LnArgs& A = pr.a[sel];
  float* __restrict__ x = A.x;
  const int M = A.M;
  const RowBcast& shift = A.shift;
  const RowBcast& scale = A.scale;
  OutT* __restrict__ out = (OutT*)A.out;
  const int row = ((int)blockIdx.x - (sel ? pr.blocks0 : 0)) * 2 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const int nv = D >> 2;  // float4 per row
  f32x4* xr = (f32x4*)(x + (long)row * D);
  const f32x4* sh = shift.p ? (const f32x4*)rb_row(shift, row) : nullptr;
  const f32x4* sc = scale.p ? (const f32x4*)rb_row(scale, row) : nullptr;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[MAXV], hv[MAXV], cv[MAXV];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = min(lane + i * 64, nv - 1);  // clamped: loads stay unconditional
    v[i] = xr[c];
    hv[i] = sh ? sh[c] : z4;
    cv[i] = sc ? sc[c] : z4;
  }
  if (PEND && A.pend.partials) {   // (separate instantiation: the slab registers would halve the plain kernel's occupancy)
    // finish the deferred split-K GEMM: x += gate * (sum of partial products + bias), SB slabs in
    // flight at a time (clamped slab index keeps the loads unconditional, weight 0 drops repeats)
    constexpr int SB = 6;
    const LnPending& P = A.pend;
    const f32x4* gp = (const f32x4*)rb_row(P.gate, row);
    const f32x4* bp = (const f32x4*)P.bias;
    f32x4 acc[MAXV], gt[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = min(lane + i * 64, nv - 1);
      gt[i] = gp[c];
      acc[i] = bp ? bp[c] : z4;
    }
    for (int s0 = 0; s0 < P.k; s0 += SB) {
      f32x4 t[SB][MAXV];
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int s = min(s0 + u, P.k - 1);
        const long pe = s * P.stride + (long)row * D;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) t[u][i] = slab_load4<ST>(P.partials, pe + 4L * min(lane + i * 64, nv - 1));
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const float w = (s0 + u < P.k) ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][e] += w * t[u][i][e];
      }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] += gt[i][e] * acc[i][e];
      if (lane + i * 64 < nv) xr[lane + i * 64] = v[i];
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + i * 64 < nv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + i * 64 < nv) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float d = v[i][u] - mean;
        q += d * d;
      }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  OutT* orow = out + (long)row * D;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      f32x4 y;
#pragma unroll
      for (int u = 0; u < 4; ++u) y[u] = (v[i][u] - mean) * rstd * (1.0f + cv[i][u]) + hv[i][u];
      Pack4<OutT>::store(orow + c * 4, y);
    }
  }
}

// Same operation with WPR waves cooperating on one row (D = 64 * WPR * MAXV float4): at M = 500 the
// one-wave-per-row kernel puts 500 waves on 256 CUs, each walking a 6 KiB row (plus up to five partial
// slabs) alone - latency bound, not bandwidth bound.  Splitting a row over WPR waves multiplies the
// loads in flight; the two statistics cross the waves through LDS.
// SEL (which row set of the pair) is a template parameter: argument fields are then loaded at constant
// kernel-argument offsets, in a few wide scalar loads at entry, instead of one dependent dword at a time
// in front of the first global load of this latency-bound kernel (same reason as gemm_ws_body).
#ifndef FOLEY_LN_RPB
#define FOLEY_LN_RPB 1   // rows per workgroup of the multi-wave LayerNorm (A/B builds with -DFOLEY_LN_RPB=2 / 4 through FOLEY_HIP_LIB: 1 row
                         // -0.3 % on the bs=1 loop against 2, 4 rows +0.5 %)
#endif
// Statistics and output of the multi-wave kernels, from the row part v each wave holds (after any pending update): each wave
// reduces its own part to (sum, centred sum of squares) in registers; the parts meet once in LDS and are combined exactly (Chan
// et al.): M2 = sum_w [M2_w + n_w (mean_w - mean)^2] - one barrier instead of two.  STAMP: the timeline probe's stamps 2 and 3.
// WT: the output leaves write-through - wt_base is the (wave-uniform) base of the row set's output, wt_bytes its extent and wt_row
// the byte offset of this row in it; the values and the lane -> address map are those of the plain stores.  The policy is a
// compile-time parameter: the WT = false instances are the code they were.
template <typename OutT, int MAXV, int WPR, bool STAMP, bool WT = false>
__device__ __forceinline__ void ln_wide_finish(const f32x4 (&v)[MAXV], const f32x4 (&hv)[MAXV], const f32x4 (&cv)[MAXV], OutT* orow, int c0, int rb,
                                               int part, int lane, bool live, int D, float eps, long long* stamps, void* wt_base = nullptr,
                                               unsigned wt_bytes = 0, unsigned wt_row = 0) {
  __shared__ float red[FOLEY_LN_RPB][2][WPR];   // [row of the block][statistic][wave of the row]
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  s = wave_sum(s);
  const float nw = (float)(MAXV * 4 * 64);
  const float mean_w = s / nw;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float d = v[i][u] - mean_w;
      q += d * d;
    }
  q = wave_sum(q);
  if (lane == 0) {
    red[rb][0][part] = s;
    red[rb][1][part] = q;
  }
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < WPR; ++w) tot += red[rb][0][w];     // fixed order: every wave of the row gets the same mean
  const float mean = tot / (float)D;
  float qt = 0.f;
#pragma unroll
  for (int w = 0; w < WPR; ++w) {
    const float dm = red[rb][0][w] / nw - mean;
    qt += red[rb][1][w] + nw * dm * dm;
  }
  const float rstd = 1.0f / sqrtf(qt / (float)D + eps);
  if (STAMP && stamps) stamps[2] = wall_clock64();
  if (!live) return;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    f32x4 y;
#pragma unroll
    for (int u = 0; u < 4; ++u) y[u] = (v[i][u] - mean) * rstd * (1.0f + cv[i][u]) + hv[i][u];
    if constexpr (WT) Pack4<OutT>::store_wt(wt_base, wt_bytes, wt_row + (unsigned)((c0 + i * 64) * 4 * sizeof(OutT)), y);
    else Pack4<OutT>::store(orow + (c0 + i * 64) * 4, y);
  }
  if (STAMP && stamps) stamps[3] = wall_clock64();
}

// Resolved multi-wave body; memory work in the order of ln_mod_kernel above: counter, then x / bias / first slab batch, then the
// row offset, then the counter's wait and the three operand rows.  DBG: the instantiations tools/ln_timeline.py launches - the
// product ones carry no stamp, branch or store of the probe.  WT: the launcher's store policy for small grids (ln_mod_wide_wt_kernel):
// the x write-back and the output rows are stored write-through (common.h GStore<ST_WT>) - they leave the L2 while other rows are
// still being read.  A template parameter, so that the launches that do not take it run the code they ran before.
template <typename OutT, int MAXV, bool PEND, int WPR, int SEL, bool SLAB16, bool DBG, bool WT = false>
__device__ __forceinline__ void ln_mod_wide_body(const LnResPair& pr, int D, float eps) {
  using ST = typename std::conditional<SLAB16, OutT, float>::type;   // slab element type
  constexpr int RPB = FOLEY_LN_RPB, SB = 6;
  const LnRes& A = pr.a[SEL];
  const int M = A.M;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rb = wave / WPR, part = wave % WPR;               // row of the block (0/1), column part
  const int row_u = ((int)blockIdx.x - (SEL ? pr.blocks0 : 0)) * RPB + rb;
  const bool live = row_u < M;
  const int row = live ? row_u : M - 1;                       // dead waves shadow the last row (no stores)
  const int c0 = part * (MAXV * 64) + lane;                   // first float4 of this lane; stride 64
  long long* const stamps = (DBG && threadIdx.x == 0) ? pr.dbg + (long)blockIdx.x * 4 : nullptr;
  if (DBG && stamps) stamps[0] = wall_clock64();
  f32x4* xr = (f32x4*)(A.x + (long)row * D);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  const bool pend = PEND && A.partials;
  const auto col = [&](int i) { return c0 + i * 64; };
  f32x4 v[MAXV], hv[MAXV], cv[MAXV], acc[MAXV], gt[MAXV];
  typename SlabRaw<ST>::type t[PEND ? SB : 1][MAXV];
  const int step_sent = ln_step_issue(A, pr.step_ptr);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) v[i] = xr[col(i)];
  if constexpr (PEND) {
    if (pend) {
      const f32x4* bp = (const f32x4*)A.bias;
#pragma unroll
      for (int i = 0; i < MAXV; ++i) acc[i] = bp ? bp[col(i)] : z4;
      slab_batch_load<ST, MAXV, SB>(t, A.partials, A.pstride, A.k, 0, (long)row * D, col);
    }
  }
  const long row_off = rb_map_off(A.map, 0, row);   // the divisions of modes 1 and 2 run under the loads above
  const long off = row_off + (long)ln_step_wait(step_sent) * A.map.step_stride;
  const f32x4* sh = A.shift ? (const f32x4*)(A.shift + off) : nullptr;
  const f32x4* sc = A.scale ? (const f32x4*)(A.scale + off) : nullptr;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    hv[i] = sh ? sh[col(i)] : z4;
    cv[i] = sc ? sc[col(i)] : z4;
  }
  if constexpr (PEND) {
    if (pend) {
      const f32x4* gp = (const f32x4*)(A.gate + off);
#pragma unroll
      for (int i = 0; i < MAXV; ++i) gt[i] = gp[col(i)];
      for (int s0 = 0; s0 < A.k; s0 += SB) {
        if (s0 > 0) slab_batch_load<ST, MAXV, SB>(t, A.partials, A.pstride, A.k, s0, (long)row * D, col);
        slab_batch_add<ST, MAXV, SB>(acc, t, A.k, s0);
      }
      // The residual update reads and writes x in place; the read stays on the default path.  Each 16-byte run of a row is
      // WRITTEN by one lane only, and among the live waves it is read by that lane only: the lanes that share a 128-byte line
      // belong to one wave, whose loads of the line are all behind it when its first store goes out.  One exception, as with
      // the plain stores: with an odd row count the dead wave pair of the last workgroup shadows row M - 1 and loads its x
      // while the live pair stores it.  Harmless: dead waves store nothing, and their statistics go to their own red[rb].
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] += gt[i][e] * acc[i][e];
        if (live) {
          if constexpr (WT) GStore<ST_WT>::st16(A.x, (unsigned)M * (unsigned)D * 4u, (unsigned)row * (unsigned)D * 4u + (unsigned)col(i) * 16u, __builtin_bit_cast(u32x4, v[i]));
          else xr[col(i)] = v[i];
        }
      }
    }
  }
  if (DBG) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (stamps) stamps[1] = wall_clock64();
  }
  if constexpr (WT)
    ln_wide_finish<OutT, MAXV, WPR, DBG, true>(v, hv, cv, (OutT*)A.out + (long)row * D, c0, rb, part, lane, live, D, eps, stamps, A.out,
                                               (unsigned)M * (unsigned)D * (unsigned)sizeof(OutT), (unsigned)row * (unsigned)D * (unsigned)sizeof(OutT));
  else ln_wide_finish<OutT, MAXV, WPR, DBG>(v, hv, cv, (OutT*)A.out + (long)row * D, c0, rb, part, lane, live, D, eps, stamps);
}

template <typename OutT, int MAXV, bool PEND, int WPR, bool SLAB16 = false, bool DBG = false>
__global__ __launch_bounds__(64 * FOLEY_LN_RPB * WPR) void ln_mod_wide_kernel(const LnResPair pr, int D, float eps) {
  if ((int)blockIdx.x >= pr.blocks0) ln_mod_wide_body<OutT, MAXV, PEND, WPR, 1, SLAB16, DBG>(pr, D, eps);   // workgroup-uniform
  else ln_mod_wide_body<OutT, MAXV, PEND, WPR, 0, SLAB16, DBG>(pr, D, eps);
}
// the same kernel with write-through stores (small grids: launch_ln_mod_pair)
template <typename OutT, int MAXV, bool PEND, int WPR, bool SLAB16 = false>
__global__ __launch_bounds__(64 * FOLEY_LN_RPB * WPR) void ln_mod_wide_wt_kernel(const LnResPair pr, int D, float eps) {
  if ((int)blockIdx.x >= pr.blocks0) ln_mod_wide_body<OutT, MAXV, PEND, WPR, 1, SLAB16, false, true>(pr, D, eps);   // workgroup-uniform
  else ln_mod_wide_body<OutT, MAXV, PEND, WPR, 0, SLAB16, false, true>(pr, D, eps);
}

// The per-operand path of the multi-wave kernel (see ln_mod_each_kernel)
template <typename OutT, int MAXV, bool PEND, int WPR, int SEL, bool SLAB16>
__device__ __forceinline__ void ln_mod_wide_each_body(const LnPair& pr, int D, float eps) {
  using ST = typename std::conditional<SLAB16, OutT, float>::type;   // slab element type
  constexpr int RPB = FOLEY_LN_RPB;
  constexpr int sel = SEL;
  const LnArgs& A = pr.a[SEL];
  const int M = A.M;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rb = wave / WPR, part = wave % WPR;               // row of the block (0/1), column part
  const int row_u = ((int)blockIdx.x - (sel ? pr.blocks0 : 0)) * RPB + rb;
  const bool live = row_u < M;
  const int row = live ? row_u : M - 1;                       // dead waves shadow the last row (no stores)
  const int c0 = part * (MAXV * 64) + lane;                   // first float4 of this lane; stride 64
  f32x4* xr = (f32x4*)(A.x + (long)row * D);
  const f32x4* sh = A.shift.p ? (const f32x4*)rb_row(A.shift, row) : nullptr;
  const f32x4* sc = A.scale.p ? (const f32x4*)rb_row(A.scale, row) : nullptr;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[MAXV], hv[MAXV], cv[MAXV];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = c0 + i * 64;
    v[i] = xr[c];
    hv[i] = sh ? sh[c] : z4;
    cv[i] = sc ? sc[c] : z4;
  }
  if (PEND && A.pend.partials) {
    constexpr int SB = 6;
    const LnPending& P = A.pend;
    const f32x4* gp = (const f32x4*)rb_row(P.gate, row);
    const f32x4* bp = (const f32x4*)P.bias;
    f32x4 acc[MAXV], gt[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = c0 + i * 64;
      gt[i] = gp[c];
      acc[i] = bp ? bp[c] : z4;
    }
    for (int s0 = 0; s0 < P.k; s0 += SB) {
      f32x4 t[SB][MAXV];
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int s = min(s0 + u, P.k - 1);
        const long pe = s * P.stride + (long)row * D;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) t[u][i] = slab_load4<ST>(P.partials, pe + 4L * (c0 + i * 64));
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const float w = (s0 + u < P.k) ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][e] += w * t[u][i][e];
      }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] += gt[i][e] * acc[i][e];
      if (live) xr[c0 + i * 64] = v[i];
    }
  }
  ln_wide_finish<OutT, MAXV, WPR, false>(v, hv, cv, (OutT*)A.out + (long)row * D, c0, rb, part, lane, live, D, eps, nullptr);
}

template <typename OutT, int MAXV, bool PEND, int WPR, bool SLAB16 = false>
__global__ __launch_bounds__(64 * FOLEY_LN_RPB * WPR) void ln_mod_wide_each_kernel(const LnPair pr, int D, float eps) {
  if ((int)blockIdx.x >= pr.blocks0) ln_mod_wide_each_body<OutT, MAXV, PEND, WPR, 1, SLAB16>(pr, D, eps);   // workgroup-uniform
  else ln_mod_wide_each_body<OutT, MAXV, PEND, WPR, 0, SLAB16>(pr, D, eps);
}

// ------------------------------------------------------------------ q/k RMSNorm + RoPE + head split
// reference: rearrange "(K H D)", RMSNorm (norm_layers.py:36-52 / nn.RMSNorm), apply_rotary_emb
// (attn_layers.py:112-146).  One wave per (row, head, operand); lane owns the rotation pair
// (2*lane, 2*lane+1).
struct QkvPair {
  QkvSplitArgs a[2];
  int blocks0;
};

// Two workgroup roles in one launch: (1) one wave per (row, head, operand) for every operand that
// keeps the [clip, H, S, 128] layout - RMSNorm / RoPE are per (row, head), lane = rotation pair;
// (2) for a transposed V operand, one workgroup per (clip, head, 32-token tile) moves the tile
// through LDS so that V^T leaves as 64-byte runs instead of 2-byte scatters.
template <typename OutT>
__global__ __launch_bounds__(256) void qkv_split_kernel(const QkvPair pr) {
  __shared__ OutT vt[32][128 + 2];
  const int sel = (int)blockIdx.x >= pr.blocks0 ? 1 : 0;
  const QkvSplitArgs& a = pr.a[sel];
  int bid = (int)blockIdx.x - (sel ? pr.blocks0 : 0);
  const bool vtrans = a.vt_pitch > 0;
  const int nQ = a.nK - (vtrans ? 1 : 0);  // operands handled by role (1)
  const int lane = threadIdx.x & 63;
  constexpr int IPW = 4;  // items per wave: their loads are issued together (memory-level parallelism)
  const long n_items = (long)a.M * a.H * nQ;
  const int bqk = (int)((n_items + 4 * IPW - 1) / (4 * IPW));
  if (bid < bqk) {
    const long it0 = ((long)bid * 4 + (threadIdx.x >> 6)) * IPW;
    if (it0 >= n_items) return;
    float x0[IPW], x1[IPW];
    int wq[IPW], hq[IPW], rq[IPW];
#pragma unroll
    for (int u = 0; u < IPW; ++u) {
      const long it = min(it0 + u, n_items - 1);
      wq[u] = (int)(it % nQ);
      hq[u] = (int)((it / nQ) % a.H);
      rq[u] = (int)(it / ((long)nQ * a.H));
      const float* src = a.qkv + (long)rq[u] * (a.nK * a.H * 128) + (long)wq[u] * a.H * 128 + hq[u] * 128 + 2 * lane;
      x0[u] = src[0];
      x1[u] = src[1];
    }
#pragma unroll
    for (int u = 0; u < IPW; ++u) {
      if (it0 + u >= n_items) break;
      const int w = wq[u], h = hq[u], r = rq[u];
      const int b = r / a.L, l = r - b * a.L;
      float y0 = x0[u], y1 = x1[u];
      if (a.gain[w]) {
        const float ss = wave_sum(y0 * y0 + y1 * y1);
        const float rinv = rsqrtf(ss * (1.0f / 128.0f) + a.eps);
        y0 = y0 * rinv * a.gain[w][2 * lane];
        y1 = y1 * rinv * a.gain[w][2 * lane + 1];
      }
      if (a.pos[w]) {
        const int p = a.pos[w][l];
        const float c = a.cos_tab[(long)p * 64 + lane], sn = a.sin_tab[(long)p * 64 + lane];
        const float z0 = y0 * c - y1 * sn;
        const float z1 = y1 * c + y0 * sn;
        y0 = z0;
        y1 = z1;
      }
      OutT* dst = (OutT*)a.dst[w] + (((long)b * a.H + h) * a.S_tot + a.tok_off + l) * 128 + 2 * lane;
      dst[0] = Cvt<OutT>::to(y0);
      dst[1] = Cvt<OutT>::to(y1);
    }
    return;
  }
  // ---- role (2): V tile -> V^T  (plain copy: V is neither normalised nor rotated)
  bid -= bqk;
  const int tiles = (a.L + 31) >> 5;
  const int tl = bid % tiles;
  bid /= tiles;
  const int h = bid % a.H;
  const int b = bid / a.H;
  const int l0 = tl * 32;
  const int nrows = min(32, a.L - l0);
  const int w = a.nK - 1;
  {
    // 32 rows x 128 fp32 = 1024 float4: 4 per thread, all in flight together
    const int c4 = threadIdx.x & 31, r0 = threadIdx.x >> 5;  // float4 column, row group
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = r0 + i * 8;
      const int l = l0 + min(lr, nrows - 1);
      const f32x4 v = *(const f32x4*)(a.qkv + ((long)b * a.L + l) * (a.nK * a.H * 128) + (long)w * a.H * 128 +
                                      h * 128 + c4 * 4);
      vt[lr][c4 * 4 + 0] = Cvt<OutT>::to(v[0]);
      vt[lr][c4 * 4 + 1] = Cvt<OutT>::to(v[1]);
      vt[lr][c4 * 4 + 2] = Cvt<OutT>::to(v[2]);
      vt[lr][c4 * 4 + 3] = Cvt<OutT>::to(v[3]);
    }
  }
  __syncthreads();
  const int d = threadIdx.x >> 1, half = threadIdx.x & 1;  // channel, half of the tile
  OutT* dst = (OutT*)a.dst[w] + (((long)b * a.H + h) * 128 + d) * a.vt_pitch + a.tok_off + l0 + half * 16;
#pragma unroll
  for (int t = 0; t < 16; ++t)
    if (half * 16 + t < nrows) dst[t] = vt[half * 16 + t][d];
}

// ------------------------------------------------------------------ small elementwise helpers
template <typename OutT>
__global__ void rows_add_act_kernel(const float* __restrict__ a, RowBcast v, int R, int D, int act_silu,
                                    OutT* __restrict__ out) {
  const int step = rb_step_load(v.p ? v.step_ptr : nullptr);   // first memory instruction; the `a` loads do not wait for it
  const long n = (long)R * D;
  const float* vr = v.p ? rb_row_at(v, step, 0) : nullptr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float y = a ? a[i] : 0.f;
    if (vr) y += vr[i % D];
    if (act_silu) y = silu_f(y);
    out[i] = Cvt<OutT>::to(y);
  }
}

template <typename OutT>
__global__ void add_periodic_kernel(const float* __restrict__ x, const float* __restrict__ pos, int R, int D,
                                    int period, OutT* __restrict__ out) {
  const long n = (long)R * D;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / D), c = (int)(i - (long)r * D);
    out[i] = Cvt<OutT>::to(x[i] + pos[(long)(r % period) * D + c]);
  }
}

__global__ void gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ idx, int n_idx,
                                   int groups, int src_rows, int D, float* __restrict__ out) {
  const long n = (long)groups * n_idx * D;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / D;
    const int c = (int)(i - r * D);
    const int g = (int)(r / n_idx), l = (int)(r - (long)g * n_idx);
    out[i] = src[((long)g * src_rows + idx[l]) * D + c];
  }
}

template <typename S, typename Dst>
__global__ void cast_kernel(const S* __restrict__ s, Dst* __restrict__ d, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    d[i] = Cvt<Dst>::to(Cvt<S>::from(s[i]));
}

// latents [clips, C, L] -> token rows [(cfg*clips + b)*L + l, C]  (PatchEmbed1D's transpose,
// embed_layers.py:43-52, and the CFG duplication of utils.py:205)
template <typename OutT>
__global__ __launch_bounds__(256) void latent_rows_kernel(const float* __restrict__ x, int clips, int C, int L,
                                                          int ncfg, OutT* __restrict__ out) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, l = l0 + tx;
    tile[i][tx] = (c < C && l < L) ? x[((long)b * C + c) * L + l] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < L && c < C) {
      const OutT v = Cvt<OutT>::to(tile[tx][i]);
      for (int g = 0; g < ncfg; ++g) out[(((long)g * clips + b) * L + l) * C + c] = v;
    }
  }
}

// ------------------------------------------------------------------ solver update
// CFG combine (utils.py:241-243) + FlowMatchDiscreteScheduler.step (scheduling_flow_match_
// discrete.py:262-297 and the multi-stage bookkeeping :299-373) driven by a per-iteration
// coefficient row {w_new, w_acc, dt, w_store, flags}; then re-stages the next model input rows.
//
// The three forms (plain, edit, windows) are built from the routines below and promise each other's bits: an all-ones mask is the
// plain run, one window is the plain step, a null or constant guidance descriptor gives the plain arithmetic.  So the roundings
// are written out: every routine that computes turns contraction off and names each fused multiply-add, and no form has an
// expression of its own for a value another form computes too.
constexpr int STEP_SAVE_X = 1, STEP_USE_SAVED = 2, STEP_ACC_RESET = 4, STEP_BLEND = 8, STEP_HIST = 16;

// The one place where the prediction halves of a (row, channel) become the velocity the step uses.  r = b*L + l is the row inside
// a half, `it` the loop iteration (*step_ptr).  Two halves: v = u + g (c - u); three (h0 = nothing, h1 = video only, h2 = video
// and prompt): v = p0 + g_video (p1 - p0) + g_text (p2 - p1), left to right.  Without a schedule g = g_video = g_text = the scalar
// `guidance` and the two-half expression is the one the step kernels always had: plain runs keep their bits.  `scale` (the CFG
// rescale factors, or null) multiplies the result by scale[b].  Two halves fuse the product into the sum; three halves round both
// products and add them in order.
// PROJ (projected guidance, foley_set_projected_guidance; two halves): the combine is v = fma(a_c, cnd, rnd(a_w * w)) with
// {a_c, a_w} = a.proj_coef[b] of this iteration (guidance_proj_coef_kernel) and w the momentum plane's element (APG) or, without a
// plane, u (CFG-Zero*).  a_c = 1, a_w = 0 (g == 1) returns cnd itself, both 0 (a dead row) a zero.  Like HIST it is a template
// parameter: the kernels without it are the code they were.
template <bool PROJ = false>
__device__ __forceinline__ float guided_value(const StepArgs& a, int it, int b, long r, int c, const float* __restrict__ scale) {
#pragma clang fp contract(off)
  const long half = (long)a.clips * a.L * a.C;
  const float* p = a.pred + r * a.C + c;
  float v;
  if (PROJ) {
    const float cnd = p[half];
    const float w = a.proj_plane ? a.proj_plane[r * a.C + c] : p[0];
    const float t = a.proj_coef[2 * b + 1] * w;
    return __builtin_fmaf(a.proj_coef[2 * b], cnd, t);
  }
  if (a.ncfg == 2) {
    const float g = a.sched ? a.sched[2 * it] : a.guidance;
    const float u = p[0], cnd = p[half];
    v = __builtin_fmaf(g, cnd - u, u);
  } else if (a.ncfg == 3) {
    const float gv = a.sched ? a.sched[2 * it] : a.guidance, gt = a.sched ? a.sched[2 * it + 1] : a.guidance;
    const float p0 = p[0], p1 = p[half], p2 = p[2 * half];
    v = p0 + gv * (p1 - p0) + gt * (p2 - p1);
  } else {
    v = p[0];
  }
  if (scale) v *= scale[b];
  return v;
}

// Row *step_ptr of the coefficient table.  c1 / c2 (columns 6 and 7, the multistep weights of v_{n-1} and v_{n-2}) are read by the
// history instantiations only.
struct StepCoef {
  float w_new, w_acc, dt, w_store, s_next;
  int flags;
  float c1, c2;
};
template <bool HIST = false>
__device__ __forceinline__ StepCoef step_coef(const StepArgs& a, int it) {
  const float* cf = a.coef + (long)it * 8;
  return StepCoef{cf[0], cf[1], cf[2], cf[3], cf[5], (int)cf[4], HIST ? cf[6] : 0.f, HIST ? cf[7] : 0.f};
}

// phase 1: the guided value of clip b's rows lb .. lb + 31 (lb may be negative; rows outside [0, L) give 0), read [l][c] (coalesced
// over c) into the tile that phase 2 reads transposed
template <bool PROJ = false>
__device__ __forceinline__ void step_guided_tile(float (*tile)[33], const StepArgs& a, int it, int b, int lb, int c0) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int l = lb + i, c = c0 + tx;
    float v = 0.f;
    if (l >= 0 && l < a.L && c < a.C) v = guided_value<PROJ>(a, it, b, (long)b * a.L + l, c, PROJ ? nullptr : a.clip_scale);
    tile[i][tx] = v;
  }
}

// phase 2, one element: the flow-match update of x[xi] from its velocity v.  Stores x_saved as the row's flags say and returns the
// new x, which the caller stores blended or not, and in `acc_new` the new d_acc, which the caller stores after x where a.d_acc is
// set: stored here, ahead of x, it costs the plain kernel 0.3 us of 7.5 (the waits fall differently).
//
// HIST (multistep runs, foley_set_multistep): a.hist is a ring of a.hist_slots (1 or 2) slots [clips, C, L] of earlier velocities.
// On a row flagged STEP_HIST the derivative continues  deriv = fma(c1, h1, deriv), deriv = fma(c2, h2, deriv)  with h_j the slot
// (it - j) mod slots; a term whose weight is 0.0f is not read, so warm-up rows do not depend on what the ring holds and a row with
// both weights zero is the plain row bit for bit.  Every row then stores v - the guided value exactly as this step used it - to
// slot it mod slots, after the reads: with two slots v_{n-2} sits in the slot being written.  One thread owns the element in all
// three forms, so the order inside the thread is the only ordering there is.
template <bool HIST = false>
__device__ __forceinline__ float step_update(const StepArgs& a, const StepCoef& k, int it, long xi, float v, float& acc_new) {
#pragma clang fp contract(off)
  const float xc = a.x[xi];
  float acc = 0.f;
  if (a.d_acc) acc = (k.flags & STEP_ACC_RESET) ? 0.f : a.d_acc[xi];
  const float t = k.w_new * v;
  float deriv = (k.w_acc != 0.f) ? __builtin_fmaf(k.w_acc, acc, t) : t;
  if (HIST) {
    const long n = (long)a.clips * a.C * a.L;
    const int slots = a.hist_slots;
    if (k.flags & STEP_HIST) {
      if (k.c1 != 0.f) deriv = __builtin_fmaf(k.c1, a.hist[(long)((it + 2 * slots - 1) % slots) * n + xi], deriv);
      if (k.c2 != 0.f) deriv = __builtin_fmaf(k.c2, a.hist[(long)((it + 2 * slots - 2) % slots) * n + xi], deriv);
    }
    a.hist[(long)(it % slots) * n + xi] = v;
  }
  const float base = (k.flags & STEP_USE_SAVED) ? a.x_saved[xi] : xc;
  if (k.flags & STEP_SAVE_X) a.x_saved[xi] = xc;
  acc_new = __builtin_fmaf(k.w_store, v, acc);
  return __builtin_fmaf(deriv, k.dt, base);
}

// phase 3: the tile [l][c] as clip b's next model input rows lb .. lb + 31 (cfg-duplicated), coalesced over c; nothing without rows_out
template <typename OutT>
__device__ __forceinline__ void step_stage_rows(const float (*tile)[33], const StepArgs& a, int b, int lb, int c0) {
  if (!a.rows_out) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int l = lb + i, c = c0 + tx;
    if (l >= 0 && l < a.L && c < a.C) {
      const OutT v = Cvt<OutT>::to(tile[i][tx]);
      for (int g = 0; g < a.ncfg; ++g) ((OutT*)a.rows_out)[(((long)g * a.clips + b) * a.L + l) * a.C + c] = v;
    }
  }
}

// Edit form (audio-to-audio / span regeneration): the same step, then - on rows flagged STEP_BLEND, the iterations that end a
// solver step - the kept frames are pulled back onto the source's forward-noised path:
//   x <- m*x + (1-m)*(s*noise + (1-s)*x0),  s = sigma_{k+1} (column 5 of the row), m = mask[clip][l] (1 = regenerate).
// The blend is two rounded products so that m = 1 returns x and m = 0 the target bit for bit: an all-ones mask is a plain run.
// The source's point on the flow-match path at sigma s: one fused multiply-add over a rounded product.  The FlowEdit step stages
// its source branch from the same expression.
__device__ __forceinline__ float edit_target(float s, float noise, float x0) {
#pragma clang fp contract(off)
  return __builtin_fmaf(1.f - s, x0, s * noise);
}
__device__ __forceinline__ float edit_blend(float xn, float m, float s, float noise, float x0) {
#pragma clang fp contract(off)
  const float tgt = edit_target(s, noise, x0);
  return m * xn + (1.f - m) * tgt;
}

template <typename OutT, bool EDIT, bool HIST, bool PROJ = false>
__device__ __forceinline__ void solver_step_body(const StepArgs& a) {
  __shared__ float tile[32][33];
  const int it = *a.step_ptr;
  const StepCoef k = step_coef<HIST>(a, it);
  const int b = blockIdx.z;
  const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  step_guided_tile<PROJ>(tile, a, it, b, l0, c0);
  __syncthreads();
  const float* x0b = EDIT ? a.x0 + (a.x0_clips == 1 ? 0L : (long)b * a.C * a.L) : nullptr;
  const float* mb = EDIT && a.mask ? a.mask + (a.mask_clips == 1 ? 0L : (long)b * a.L) : nullptr;
  // phase 2: update x [b][c][l] (coalesced over l)
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, l = l0 + tx;
    float xn = 0.f;
    if (c < a.C && l < a.L) {
      const long xi = ((long)b * a.C + c) * a.L + l;
      float acc_new;
      xn = step_update<HIST>(a, k, it, xi, tile[tx][i], acc_new);
      if (EDIT && (k.flags & STEP_BLEND)) xn = edit_blend(xn, mb ? mb[l] : 1.f, k.s_next, a.noise[xi], x0b[(long)c * a.L + l]);
      a.x[xi] = xn;
      if (a.d_acc) a.d_acc[xi] = acc_new;
    }
    tile[tx][i] = xn;
  }
  __syncthreads();
  step_stage_rows<OutT>(tile, a, b, l0, c0);
}

// History is a template parameter: the kernels without it are the code they were, the multistep ones have names of their own.
template <typename OutT, bool EDIT>
__global__ __launch_bounds__(256) void solver_step_kernel(const StepArgs a) { solver_step_body<OutT, EDIT, false>(a); }
template <typename OutT, bool EDIT>
__global__ __launch_bounds__(256) void solver_step_hist_kernel(const StepArgs a) { solver_step_body<OutT, EDIT, true>(a); }
// So is the projected combine (a.proj_coef set): the same bodies with guided_value<true>.
template <typename OutT, bool EDIT>
__global__ __launch_bounds__(256) void solver_step_proj_kernel(const StepArgs a) { solver_step_body<OutT, EDIT, false, true>(a); }
template <typename OutT, bool EDIT>
__global__ __launch_bounds__(256) void solver_step_proj_hist_kernel(const StepArgs a) { solver_step_body<OutT, EDIT, true, true>(a); }

// FlowEdit (kernels.h FlowEditArgs): the step integrates the DIFFERENCE of the target-prompt and source-prompt velocities of a
// (source, target) pair of batch clips, so what both prompts agree on cancels.  Kernels of their own, built from the routines of
// the forms above: step_guided_tile / guided_value for the two velocities, edit_target for the source branch's next input.
__device__ __forceinline__ float flowedit_update(float z, float vs, float vt, bool masked, float m, float dt) {
#pragma clang fp contract(off)
  float d = vt - vs;
  if (masked) d = m * d;
  return __builtin_fmaf(d, dt, z);
}
// the pair of next model inputs at sigma s; in this order z == xs gives zt == zs bit for bit
__device__ __forceinline__ void flowedit_pair(float z, float xs, float n, float s, float& zs, float& zt) {
#pragma clang fp contract(off)
  zs = edit_target(s, n, xs);
  zt = (z - xs) + zs;
}

// phase 2 of variation v's tile, coalesced over l.  UPDATE: z takes the step from the velocity tiles ts / tt (read transposed).
// Then both tiles receive the inputs of the next model call at sigma s from noise row nr: ts the source branch, tt the target.
template <bool UPDATE>
__device__ __forceinline__ void flowedit_phase2(float (*ts)[33], float (*tt)[33], const FlowEditArgs& a, int v, int l0, int c0, float dt,
                                                float s, int nr) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long plane = (long)a.C * a.L;
  const float* xs = a.x_src + (a.src_clips == 1 ? 0L : (long)v * plane);
  const float* mb = a.mask ? a.mask + (a.mask_clips == 1 ? 0L : (long)v * a.L) : nullptr;
  const float* nz = a.noise + ((long)nr * a.V + v) * plane;
  float* zv = a.z + (long)v * plane;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, l = l0 + tx;
    float zs = 0.f, zt = 0.f;
    if (c < a.C && l < a.L) {
      const long ci = (long)c * a.L + l;
      float z = zv[ci];
      if (UPDATE) {
        z = flowedit_update(z, ts[tx][i], tt[tx][i], mb != nullptr, mb ? mb[l] : 1.f, dt);
        zv[ci] = z;
      }
      flowedit_pair(z, xs[ci], nz[ci], s, zs, zt);
    }
    ts[tx][i] = zs;
    tt[tx][i] = zt;
  }
}

// phase 3: the tiles [l][c] as the next model input rows of source clip v and target clip V + v, both cfg halves, coalesced over c
template <typename OutT>
__device__ __forceinline__ void flowedit_stage_rows(const float (*ts)[33], const float (*tt)[33], const FlowEditArgs& a, int v, int l0, int c0) {
  if (!a.rows_out) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int clips = 2 * a.V;
  OutT* out = (OutT*)a.rows_out;
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < a.L && c < a.C) {
      const OutT s = Cvt<OutT>::to(ts[i][tx]), t = Cvt<OutT>::to(tt[i][tx]);
      for (int g = 0; g < 2; ++g) {
        out[(((long)g * clips + v) * a.L + l) * a.C + c] = s;
        out[(((long)g * clips + a.V + v) * a.L + l) * a.C + c] = t;
      }
    }
  }
}

// one workgroup per (32-frame tile, 32-channel tile, variation), like solver_step_body
template <typename OutT>
__global__ __launch_bounds__(256) void flowedit_step_kernel(const FlowEditArgs a) {
  __shared__ float ts[32][33], tt[32][33];
  const int it = *a.step_ptr;
  const float* cf = a.coef + (long)it * 8;
  const float dt = cf[2], s_next = cf[5];
  const int v = blockIdx.z;
  const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  // phase 1: the guided velocities of the pair's clips, each with its own scale
  const StepArgs gs{a.pred, nullptr, nullptr, nullptr, 2 * a.V, a.C, a.L, 2, a.g_src, nullptr, nullptr, nullptr, FOLEY_F32};
  const StepArgs gt{a.pred, nullptr, nullptr, nullptr, 2 * a.V, a.C, a.L, 2, a.g_tar, nullptr, nullptr, nullptr, FOLEY_F32};
  step_guided_tile(ts, gs, it, v, l0, c0);
  step_guided_tile(tt, gt, it, a.V + v, l0, c0);
  __syncthreads();
  const int nr = a.noise_rows == 1 ? 0 : (it + 1 < a.noise_rows ? it + 1 : a.noise_rows - 1);
  flowedit_phase2<true>(ts, tt, a, v, l0, c0, dt, s_next, nr);
  __syncthreads();
  flowedit_stage_rows<OutT>(ts, tt, a, v, l0, c0);
}

// the staging half alone: the rows of the first model call from (z, x_src, noise row nr, sigma)
template <typename OutT>
__global__ __launch_bounds__(256) void flowedit_stage_kernel(const FlowEditArgs a, float sigma, int nr) {
  __shared__ float ts[32][33], tt[32][33];
  const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  flowedit_phase2<false>(ts, tt, a, blockIdx.z, l0, c0, 0.f, sigma, nr);
  __syncthreads();
  flowedit_stage_rows<OutT>(ts, tt, a, blockIdx.z, l0, c0);
}

// Windows form (long clips): the clips of one variation are overlapping windows of ONE long clip - clip v*n_win + k covers the
// global frames [starts[k], starts[k] + L) of variation v - and the step is indexed by GLOBAL frame: a thread owns (g, c) and
// does, for every window that covers g, that element's update.  On rows flagged
// STEP_BLEND (the iterations that end a solver step) the covering windows' new values are replaced in all of them by
//   xb = sum_k weights[k][g - starts[k]] * xn_k      (fp32, in window order; the weights of a frame sum to 1)
// and the next model input rows of every covering window are staged from xb.  A frame that one window covers has weight 1.0f
// and a single term: it keeps its xn bit for bit.  Rows without the flag (intermediate stages) leave every window its own xn.
// Every (clip, c, l) element belongs to exactly one thread, so no window reads what another thread wrote.  Any table of starts is
// memory-safe: all accesses are indexed by (clip < clips, c < C, 0 <= l < L).
__device__ __forceinline__ float windows_accumulate(bool first, float wk, float xn, float xb) {
#pragma clang fp contract(off)
  return first ? wk * xn : __builtin_fmaf(wk, xn, xb);
}

template <typename OutT, bool HIST, bool PROJ = false>
__device__ __forceinline__ void solver_step_windows_body(const StepArgs& a) {
  __shared__ float tile[32][33];
  const int it = *a.step_ptr;
  const StepCoef kf = step_coef<HIST>(a, it);
  const bool blend = (kf.flags & STEP_BLEND) != 0;
  const int b0 = blockIdx.z * a.n_win;
  const int g0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float xb[4] = {0.f, 0.f, 0.f, 0.f};
  int ncov = 0;
  for (int k = 0; k < a.n_win; ++k) {
    const int s0 = a.starts[k];
    if (s0 >= g0 + 32 || s0 + a.L <= g0) continue;   // the window misses this tile (uniform over the block)
    const int b = b0 + k;
    step_guided_tile<PROJ>(tile, a, it, b, g0 - s0, c0);
    __syncthreads();
    // phase 2: update x [b][c][l] (coalesced over l)
    const int l = g0 + tx - s0;
    const bool in = l >= 0 && l < a.L;
    const float wk = (in && blend) ? a.weights[(long)k * a.L + l] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = ty + 8 * j;
      const int c = c0 + i;
      float xn = 0.f;
      if (c < a.C && in) {
        const long xi = ((long)b * a.C + c) * a.L + l;
        float acc_new;
        xn = step_update<HIST>(a, kf, it, xi, tile[tx][i], acc_new);
        if (blend) xb[j] = windows_accumulate(ncov == 0, wk, xn, xb[j]);
        else a.x[xi] = xn;
        if (a.d_acc) a.d_acc[xi] = acc_new;
      }
      if (!blend) tile[tx][i] = xn;
    }
    if (in) ++ncov;
    __syncthreads();
    // phase 3 (no blend): this window's next model input rows from its own xn
    if (!blend) {
      step_stage_rows<OutT>(tile, a, b, g0 - s0, c0);
      __syncthreads();
    }
  }
  if (!blend) return;
  // blend rows: the agreed value goes to x and to the rows of every covering window
#pragma unroll
  for (int j = 0; j < 4; ++j) tile[tx][ty + 8 * j] = xb[j];
  __syncthreads();
  for (int k = 0; k < a.n_win; ++k) {
    const int s0 = a.starts[k];
    if (s0 >= g0 + 32 || s0 + a.L <= g0) continue;
    const int b = b0 + k;
    const int l = g0 + tx - s0;
    if (l >= 0 && l < a.L) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + ty + 8 * j;
        if (c < a.C) a.x[((long)b * a.C + c) * a.L + l] = xb[j];
      }
    }
    step_stage_rows<OutT>(tile, a, b, g0 - s0, c0);
  }
}

template <typename OutT>
__global__ __launch_bounds__(256) void solver_step_windows_kernel(const StepArgs a) { solver_step_windows_body<OutT, false>(a); }
template <typename OutT>
__global__ __launch_bounds__(256) void solver_step_windows_hist_kernel(const StepArgs a) { solver_step_windows_body<OutT, true>(a); }
template <typename OutT>
__global__ __launch_bounds__(256) void solver_step_windows_proj_kernel(const StepArgs a) { solver_step_windows_body<OutT, false, true>(a); }
template <typename OutT>
__global__ __launch_bounds__(256) void solver_step_windows_proj_hist_kernel(const StepArgs a) { solver_step_windows_body<OutT, true, true>(a); }

// Stitch the windows of every variation into one long clip: G[v][c][g] = sum_k weights[k][g - starts[k]] * x[v*n_win + k][c][g - starts[k]]
// over the covering windows, in window order.  Where the covering windows hold the identical bits (after a blend row: under euler
// always) the mean of equal values is that value, and it is copied as it is.
__global__ __launch_bounds__(256) void windows_stitch_kernel(const float* __restrict__ x, int n_win, int C, int L, int Ltot,
                                                             const int* __restrict__ starts, const float* __restrict__ weights,
                                                             float* __restrict__ out) {
  const int g = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, v = blockIdx.z;
  if (g >= Ltot) return;
  float sum = 0.f, first = 0.f;
  int ncov = 0;
  bool same = true;
  for (int k = 0; k < n_win; ++k) {
    const int l = g - starts[k];
    if (l < 0 || l >= L) continue;
    const float xv = x[(((long)v * n_win + k) * C + c) * L + l];
    const float wk = weights[(long)k * L + l];
    if (ncov == 0) { first = xv; sum = wk * xv; }
    else { same = same && (__float_as_uint(xv) == __float_as_uint(first)); sum = sum + wk * xv; }
    ++ncov;
  }
  out[((long)v * C + c) * Ltot + g] = same ? first : sum;
}

__global__ __launch_bounds__(256) void flow_mix_kernel(const float* __restrict__ noise, const float* __restrict__ x0,
                                                       long plane, long n, int x0_per_clip, float sigma,
                                                       float* __restrict__ out) {
  // grid-stride: launch_flow_mix sizes the grid with grid1d, which stops at 4096 workgroups
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float src = x0[x0_per_clip ? i : i % plane];
    out[i] = sigma * noise[i] + (1.f - sigma) * src;
  }
}

// ------------------------------------------------------------------ CFG rescale: per-clip statistics of the guided velocity
// clip_scale[b] = phi * s_pos / s_cfg + (1 - phi): s_pos the standard deviation (about the mean) of the last, fully conditioned
// half over clip b's C x L elements, s_cfg that of the guided v (guided_value without a factor); 1.0f when s_cfg is 0.
// Launch 1: a workgroup takes GS_ROWS rows of one clip, a wave GS_RW of them - a lane reads channels lane, lane + 64, ... of a
// row, so every load of the wave is one contiguous run of the pred row - and keeps its elements in registers: the wave's sum (about
// its first element) gives its provisional centre, the second pass over the registers the squares about it (never E[x^2] - E[x]^2).  The four waves meet
// in LDS, thread 0 merges them in wave order with the exact pairwise formula (Chan et al., as ln_mod_wide_body does) and stores
// the workgroup's {n, mean_v, M2_v, mean_p, M2_p}.  Launch 2: one wave per clip; lane j merges records j, j + 64, ... in
// ascending order, lane 0 then the 64 lanes' results in lane order.  Every order is fixed and nothing is atomic: the same input
// gives the same bits.  128 x 50 elements per clip: 2 workgroups per clip; 128 x 3000: 94.
constexpr int GS_ROWS = 32, GS_RW = 8, GS_REC = 5;

// (n, mean, M2) <- merged with (nb, mb, m2b): M2 = M2_a + M2_b + d^2 n_a n_b / n, d = mean_b - mean_a; an empty part changes nothing
__device__ __forceinline__ void moments_merge(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
  if (nb == 0.f) return;
  if (n == 0.f) {
    n = nb; mean = mb; m2 = m2b;
    return;
  }
  const float nt = n + nb, d = mb - mean;
  mean += d * (nb / nt);
  m2 += m2b + d * d * (n * (nb / nt));
  n = nt;
}
// the same for the pair of statistics that share their count (v and the last half)
__device__ __forceinline__ void moments_merge2(float* acc, const float* rec) {
  float n2 = acc[0];
  moments_merge(n2, acc[3], acc[4], rec[0], rec[3], rec[4]);
  moments_merge(acc[0], acc[1], acc[2], rec[0], rec[1], rec[2]);
}

template <int JC>
__global__ __launch_bounds__(256) void guidance_stats_kernel(const StepArgs a, float* __restrict__ part) {
  __shared__ float red[4][GS_REC];
  const int it = *a.step_ptr;
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l0 = blockIdx.x * GS_ROWS + wave * GS_RW;
  const long last = (long)(a.ncfg - 1) * a.clips * a.L * a.C;
  float v[GS_RW][JC], p[GS_RW][JC];
#pragma unroll
  for (int i = 0; i < GS_RW; ++i)
#pragma unroll
    for (int j = 0; j < JC; ++j) {
      const int l = l0 + i, c = lane + 64 * j;
      const bool ok = l < a.L && c < a.C;
      const long r = (long)b * a.L + l;
      v[i][j] = ok ? guided_value(a, it, b, r, c, nullptr) : 0.f;
      p[i][j] = ok ? a.pred[last + r * a.C + c] : 0.f;
    }
  // the sums are taken about the wave's first element: constant data then has every difference 0, its mean and M2 exact
  const float cv = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v[0][0])));
  const float cp = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p[0][0])));
  float sv = 0.f, sp = 0.f;
#pragma unroll
  for (int i = 0; i < GS_RW; ++i)
#pragma unroll
    for (int j = 0; j < JC; ++j) {
      const bool ok = l0 + i < a.L && lane + 64 * j < a.C;
      sv += ok ? v[i][j] - cv : 0.f;
      sp += ok ? p[i][j] - cp : 0.f;
    }
  const int nrow = min(max(a.L - l0, 0), GS_RW);
  const float n = (float)(nrow * a.C);   // exact in fp32
  sv = wave_sum(sv);
  sp = wave_sum(sp);
  const float mv = nrow ? cv + sv / n : 0.f, mp = nrow ? cp + sp / n : 0.f;
  float qv = 0.f, qp = 0.f;
#pragma unroll
  for (int i = 0; i < GS_RW; ++i)
#pragma unroll
    for (int j = 0; j < JC; ++j) {
      const bool ok = l0 + i < a.L && lane + 64 * j < a.C;
      const float dv = ok ? v[i][j] - mv : 0.f, dp = ok ? p[i][j] - mp : 0.f;
      qv += dv * dv;
      qp += dp * dp;
    }
  qv = wave_sum(qv);
  qp = wave_sum(qp);
  if (lane == 0) {
    red[wave][0] = n; red[wave][1] = mv; red[wave][2] = qv; red[wave][3] = mp; red[wave][4] = qp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc[GS_REC] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < 4; ++w) moments_merge2(acc, red[w]);
    float* o = part + ((long)b * gridDim.x + blockIdx.x) * GS_REC;
    for (int k = 0; k < GS_REC; ++k) o[k] = acc[k];
  }
}

__global__ __launch_bounds__(64) void guidance_scale_kernel(const float* __restrict__ part, int nblk, const float* __restrict__ phi_ptr,
                                                            float phi, float* __restrict__ clip_scale) {
  __shared__ float red[64][GS_REC];
  const int b = blockIdx.x, lane = threadIdx.x;
  float acc[GS_REC] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = lane; k < nblk; k += 64) moments_merge2(acc, part + ((long)b * nblk + k) * GS_REC);
  for (int k = 0; k < GS_REC; ++k) red[lane][k] = acc[k];
  __syncthreads();
  if (lane != 0) return;
  for (int j = 1; j < 64; ++j) moments_merge2(acc, red[j]);
  const float ph = phi_ptr ? *phi_ptr : phi;
  float f = 1.0f;
  if (acc[2] > 0.f) f = ph * sqrtf(acc[4] / acc[2]) + (1.0f - ph);   // the counts cancel in the ratio of the deviations
  clip_scale[b] = f;
}

// ------------------------------------------------------------------ projected guidance: per-clip inner products, then two coefficients
// APG (Sadat et al. 2024) and CFG-Zero* (Fan et al. 2025) over two halves u = pred half 0, c = pred half 1; <a,b> is the sum over
// a clip's C x L elements, g the iteration's scale and {eta, beta, R, live} = rows[*step_ptr].  Every line below is one fp32
// operation as written (contraction off, the fused ones named):
//   launch 1, per element (APG)   d = c - u;  m = beta != 0 ? fma(beta, m_prev, d) : d;  plane <- m  (beta == 0.0f reads no plane)
//   launch 1, per lane            over its rows i ascending, inside a row its channels lane + 64 j ascending:
//                                   APG    s0 = fma(m, c, s0)  s1 = fma(c, c, s1)  s2 = fma(m, m, s2)
//                                   Zero*  s0 = fma(c, u, s0)  s1 = fma(u, u, s1)
//                                 then wave_sum of each, the four waves through LDS added in wave order by thread 0:
//                                 one record {s0, s1, s2} per workgroup (PJ_REC floats; Zero* leaves s2 = 0)
//   launch 2, one wave per clip   lane j adds records j, j + 64, ... ascending; lane 0 adds the 64 lanes' sums in lane order
//     APG    n = sqrtf(s2);  r = (R > 0 && n > R) ? R / n : 1;  rho = s1 > 0 ? s0 / s1 : 0;  t = (g - 1) * r;
//            a_w = live * t;  a_c = live * fma(t, (eta - 1) * rho, 1)
//     Zero*  s = s1 > 0 ? s0 / s1 : 0;  a_c = live * g;  a_w = live * ((1 - g) * s)
// and the step's v = fma(a_c, c, rnd(a_w * w)), w = m (APG; the plane keeps the unclipped m) or u (Zero*): guided_value<true>.
// g == 1 gives t = 0, a_w = 0 and a_c = live exactly; live == 0 gives two zeros.  APG with eta = 1, beta = 0, R = 0 has a_c = 1,
// a_w = g - 1: plain CFG to rounding (v = c + (g - 1)(c - u), not the step's fma(g, c - u, u)), not bit-equal to it.
// The geometry is guidance_stats_kernel's (GS_ROWS rows per workgroup, GS_RW per wave, a lane takes channels lane + 64 j, every
// load issued before the first sum), every order is fixed and nothing is atomic: the same input gives the same bits.  Every access
// is guarded by (l < L, c < C); masked elements enter the sums as fma(0, 0, s) = s.
constexpr int PJ_REC = 3;

template <int JC, int MODE>
__global__ __launch_bounds__(256) void guidance_proj_stats_kernel(const float* __restrict__ pred, float* plane,
                                                                  const float* __restrict__ rows, const int* __restrict__ step_ptr,
                                                                  int clips, int C, int L, float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float red[4][PJ_REC];
  constexpr bool APG = MODE == PROJ_APG;
  const int it = *step_ptr;
  const float beta = APG ? rows[4 * it + 1] : 0.f;
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l0 = blockIdx.x * GS_ROWS + wave * GS_RW;
  const long half = (long)clips * L * C;
  float u[GS_RW][JC], cn[GS_RW][JC], mp[GS_RW][JC];
#pragma unroll
  for (int i = 0; i < GS_RW; ++i)
#pragma unroll
    for (int j = 0; j < JC; ++j) {
      const int l = l0 + i, c = lane + 64 * j;
      const bool ok = l < L && c < C;
      const long e = ((long)b * L + l) * C + c;
      u[i][j] = ok ? pred[e] : 0.f;
      cn[i][j] = ok ? pred[half + e] : 0.f;
      mp[i][j] = (APG && ok && beta != 0.f) ? plane[e] : 0.f;
    }
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < GS_RW; ++i)
#pragma unroll
    for (int j = 0; j < JC; ++j) {
      if (APG) {
        const int l = l0 + i, c = lane + 64 * j;
        const float d = cn[i][j] - u[i][j];
        const float m = (beta != 0.f) ? __builtin_fmaf(beta, mp[i][j], d) : d;
        if (l < L && c < C) plane[((long)b * L + l) * C + c] = m;
        s0 = __builtin_fmaf(m, cn[i][j], s0);
        s1 = __builtin_fmaf(cn[i][j], cn[i][j], s1);
        s2 = __builtin_fmaf(m, m, s2);
      } else {
        s0 = __builtin_fmaf(cn[i][j], u[i][j], s0);
        s1 = __builtin_fmaf(u[i][j], u[i][j], s1);
      }
    }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (APG) s2 = wave_sum(s2);
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = part + ((long)b * gridDim.x + blockIdx.x) * PJ_REC;
    for (int k = 0; k < PJ_REC; ++k) {
      float acc = red[0][k];
      for (int w = 1; w < 4; ++w) acc = acc + red[w][k];
      o[k] = acc;
    }
  }
}

__global__ __launch_bounds__(64) void guidance_proj_coef_kernel(const float* __restrict__ part, int nblk, int mode,
                                                                const float* __restrict__ rows, const float* __restrict__ sched,
                                                                float guidance, const int* __restrict__ step_ptr,
                                                                float* __restrict__ coef) {
#pragma clang fp contract(off)
  __shared__ float red[64][PJ_REC];
  const int b = blockIdx.x, lane = threadIdx.x;
  float acc[PJ_REC] = {0.f, 0.f, 0.f};
  for (int k = lane; k < nblk; k += 64) {
    const float* rec = part + ((long)b * nblk + k) * PJ_REC;
    for (int q = 0; q < PJ_REC; ++q) acc[q] = acc[q] + rec[q];
  }
  for (int q = 0; q < PJ_REC; ++q) red[lane][q] = acc[q];
  __syncthreads();
  if (lane != 0) return;
  for (int j = 1; j < 64; ++j)
    for (int q = 0; q < PJ_REC; ++q) acc[q] = acc[q] + red[j][q];
  const int it = *step_ptr;
  const float g = sched ? sched[2 * it] : guidance;
  const float eta = rows[4 * it], R = rows[4 * it + 2], live = rows[4 * it + 3];
  float a_c, a_w;
  if (mode == PROJ_APG) {
    const float n = sqrtf(acc[2]);
    const float r = (R > 0.f && n > R) ? R / n : 1.0f;
    const float rho = acc[1] > 0.f ? acc[0] / acc[1] : 0.f;
    const float t = (g - 1.0f) * r;
    const float q = (eta - 1.0f) * rho;
    a_w = live * t;
    a_c = live * __builtin_fmaf(t, q, 1.0f);
  } else {
    const float s = acc[1] > 0.f ? acc[0] / acc[1] : 0.f;
    const float t = (1.0f - g) * s;
    a_c = live * g;
    a_w = live * t;
  }
  coef[2 * b] = a_c;
  coef[2 * b + 1] = a_w;
}

__global__ void step_increment_kernel(int* p) { *p = *p + 1; }

// ------------------------------------------------------------------ step cache: probe, residual, re-entry
// The step cache (foley_set_step_cache) reuses the blocks' residual aN - a0 of the last full iteration while the first block's
// modulated input m = LayerNorm(a0; eps) * (1 + scale) + shift barely moves.  cache_probe_kernel computes m of one stream row per
// wave exactly as ln_mod_kernel does (every load of the row - a0, shift, scale and the previous m - issued before the first
// reduction; mean, then the squares about it: never E[x^2] - E[x]^2), adds up |m - m_prev| and |m_prev| and writes m over m_prev (the
// lane that read an element writes it: no hazard).  It does not copy a0: the residual buffer still holds the delta a skipped
// iteration needs when the probe runs, so the full body takes its own copy of the stream first.  The four waves of a workgroup meet in LDS and
// thread 0 adds them in wave order into the workgroup's record {sum|m - m_prev|, sum|m_prev|}; the grid is (ceil(La / 4), Bc), so a
// record never mixes two batch rows.  cache_rel_kernel: one wave per batch row; lane j adds records j, j + 64, ... in ascending
// order, lane 0 the 64 lanes' sums in lane order, rel_b = sum|m - m_prev| / sum|m_prev| (0 when that is 0).  Every order is fixed
// and nothing is atomic: the same input gives the same bits.
constexpr int CP_ROWS = 4;   // rows (= waves) per workgroup of the probe

template <int MAXV>
__global__ __launch_bounds__(64 * CP_ROWS) void cache_probe_kernel(const float* __restrict__ a0, int La, int D, float eps,
                                                                   const RowBcast shift, const RowBcast scale,
                                                                   float* __restrict__ m_prev, float* __restrict__ part) {
  __shared__ float red[CP_ROWS][2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.y, l_u = blockIdx.x * CP_ROWS + wave;
  const bool live = l_u < La;
  const long row = (long)b * La + (live ? l_u : La - 1);   // dead waves shadow the batch row's last row (no stores, no sums)
  const int nv = D >> 2;
  const f32x4* xr = (const f32x4*)(a0 + row * D);
  const f32x4* sh = shift.p ? (const f32x4*)rb_row(shift, (int)row) : nullptr;
  const f32x4* sc = scale.p ? (const f32x4*)rb_row(scale, (int)row) : nullptr;
  f32x4* mp = (f32x4*)(m_prev + row * D);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[MAXV], hv[MAXV], cv[MAXV], ov[MAXV];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = min(lane + i * 64, nv - 1);   // clamped: loads stay unconditional
    v[i] = xr[c];
    hv[i] = sh ? sh[c] : z4;
    cv[i] = sc ? sc[c] : z4;
    ov[i] = mp[c];
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + i * 64 < nv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + i * 64 < nv) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float d = v[i][u] - mean;
        q += d * d;
      }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  float sd = 0.f, so = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (live && c < nv) {
      f32x4 y;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        y[u] = (v[i][u] - mean) * rstd * (1.0f + cv[i][u]) + hv[i][u];
        sd += fabsf(y[u] - ov[i][u]);
        so += fabsf(ov[i][u]);
      }
      mp[c] = y;
    }
  }
  sd = wave_sum(sd);
  so = wave_sum(so);
  if (lane == 0) {
    red[wave][0] = sd;
    red[wave][1] = so;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float td = 0.f, to = 0.f;
    for (int w = 0; w < CP_ROWS; ++w) {
      td += red[w][0];
      to += red[w][1];
    }
    float* o = part + ((long)b * gridDim.x + blockIdx.x) * 2;
    o[0] = td;
    o[1] = to;
  }
}

__global__ __launch_bounds__(64) void cache_rel_kernel(const float* __restrict__ part, int nblk, float* __restrict__ rel) {
  __shared__ float red[64][2];
  const int b = blockIdx.x, lane = threadIdx.x;
  float td = 0.f, to = 0.f;
  for (int k = lane; k < nblk; k += 64) {
    td += part[((long)b * nblk + k) * 2];
    to += part[((long)b * nblk + k) * 2 + 1];
  }
  red[lane][0] = td;
  red[lane][1] = to;
  __syncthreads();
  if (lane != 0) return;
  for (int j = 1; j < 64; ++j) {
    td += red[j][0];
    to += red[j][1];
  }
  rel[b] = to > 0.f ? td / to : 0.f;
}

// delta = aN - a0 in place over a copy of a0 (SUB), audio += delta (!SUB): plain fp32, 16-byte accesses where both pointers
// allow them (vec), the tail (and unaligned operands) one element at a time
template <bool SUB>
__global__ __launch_bounds__(256) void cache_axpy_kernel(const float* __restrict__ src, float* __restrict__ dst, long n, int vec) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  const long n4 = vec ? n >> 2 : 0;
  for (long i = tid; i < n4; i += nth) {
    const f32x4 a = ((const f32x4*)src)[i], d = ((f32x4*)dst)[i];
    ((f32x4*)dst)[i] = SUB ? a - d : d + a;
  }
  for (long i = n4 * 4 + tid; i < n; i += nth) dst[i] = SUB ? src[i] - dst[i] : dst[i] + src[i];
}

// ------------------------------------------------------------------ DAC output conv (64 -> 1, k=7) + tanh
// reference: decoder.model[-2:] = WNConv1d(C, 1, 7, padding=3), nn.Tanh() (dac.py:141-146).
// A block handles 64 consecutive samples; the (64+6) x C snake-activated rows are staged in LDS.
__global__ __launch_bounds__(256) void dac_out_kernel(const float* __restrict__ s, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int T, int C,
                                                      float* __restrict__ out) {
  extern __shared__ float sm[];  // (70 rows) * (C + 1) + 7 * C weights
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * 64;
  const int pitch = C + 1;
  float* rows = sm;
  float* wl = sm + 70 * pitch;
  for (int i = threadIdx.x; i < 7 * C; i += 256) wl[i] = w[i];
  for (int i = threadIdx.x; i < 70 * C; i += 256) {
    const int rr = i / C, c = i - rr * C;
    const int t = t0 + rr - 3;
    rows[rr * pitch + c] = (t >= 0 && t < T) ? s[((long)b * T + t) * C + c] : 0.f;
  }
  __syncthreads();
  // 4 lanes per output sample, each covering a quarter of the channels
  const int ti = threadIdx.x >> 2, part = threadIdx.x & 3;
  const int cq = C >> 2;
  float acc = 0.f;
  for (int j = 0; j < 7; ++j) {
    const float* rp = rows + (ti + j) * pitch + part * cq;
    const float* wp = wl + j * C + part * cq;
    for (int c = 0; c < cq; ++c) acc += rp[c] * wp[c];
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  const int t = t0 + ti;
  if (part == 0 && t < T) out[(long)b * T + t] = tanhf(acc + bias[0]);
}

// ------------------------------------------------------------------ DAC encoder input conv (1 -> C, k=7)
// reference: Encoder.block[0] = WNConv1d(1, d_model, 7, padding=3) (dac.py:86); the first residual
// unit needs both y (trunk) and snake(y) (its conv input), so both are written.
__global__ __launch_bounds__(256) void dac_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ alpha,
                                                     int B, int T, int C, float* __restrict__ out0,
                                                     float* __restrict__ out1) {
  const int c4n = C >> 2;
  const long n = (long)B * T * c4n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4n) * 4;
    const long bt = i / c4n;
    const int t = (int)(bt % T);
    const float* xr = x + (bt - t);
    f32x4 acc = *(const f32x4*)(bias + c);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const int tt = t + j - 3;
      const float xv = (tt >= 0 && tt < T) ? xr[tt] : 0.f;
      const f32x4 wv = *(const f32x4*)(w + j * C + c);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += xv * wv[u];
    }
    *(f32x4*)(out0 + bt * C + c) = acc;
    const f32x4 al = *(const f32x4*)(alpha + c);
    f32x4 sn;
#pragma unroll
    for (int u = 0; u < 4; ++u) sn[u] = snake_f(acc[u], al[u], 1.0f / (al[u] + 1e-9f));
    *(f32x4*)(out1 + bt * C + c) = sn;
  }
}

// rows [B*T, C] -> planes [B, C, T] (the [B, 2*latent, T'] layout DAC.encode returns)
__global__ void rows_to_planes_kernel(const float* __restrict__ rows, int B, int T, int C, float* __restrict__ out) {
  const long n = (long)B * T * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const long bc = i / T;
    const int c = (int)(bc % C);
    const long b = bc / C;
    out[i] = rows[(b * T + t) * C + c];
  }
}

inline int grid1d(long n, int block) {
  long g = (n + block - 1) / block;
  return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

int launch_ln_mod_pair(const LnArgs& a0, const LnArgs& a1, int D, float eps, int out_dtype, hipStream_t st) {
  if (D % 4 || D > 8 * 256) return foley_set_err("ln_mod: D must be a multiple of 4 and <= 2048", __FILE__, __LINE__);
  for (const LnArgs* a : {&a0, &a1})
    if (a->M > 0 && a->pend.partials &&
        (a->pend.k < 1 || a->pend.stride % 4 || ((uintptr_t)a->pend.partials & 15) || ((uintptr_t)a->pend.bias & 15) ||
         !a->pend.gate.p || ((uintptr_t)a->pend.gate.p & 15) || a->pend.gate.ld % 4 || a->pend.gate.step_stride % 4))
      return foley_set_err("ln_mod: bad pending split-K descriptor", __FILE__, __LINE__);
  g_ln_last_wt = 0;
  LnPair pr;
  pr.a[0] = a0;
  pr.a[1] = a1;
  pr.blocks0 = (a0.M + 1) / 2;
  // One counter and one row map per row set (and the one counter for both sets): the resolved kernels; else every operand for itself
  LnResPair rp{};
  bool resolved = true;
  for (int i = 0; i < 2; ++i) {
    const LnArgs& a = pr.a[i];
    const bool pd = a.M > 0 && a.pend.partials;
    LnRes& r = rp.a[i];
    r = LnRes{a.x, a.out, a.shift.p, a.scale.p, pd ? a.pend.gate.p : nullptr, pd ? a.pend.partials : nullptr, pd ? a.pend.bias : nullptr,
              pd ? a.pend.stride : 0, a.M, pd ? a.pend.k : 0, RowMap{}};
    const RowBcast none{};
    const RowBcast* ops[3] = {&a.shift, &a.scale, pd ? &a.pend.gate : &none};
    if (a.M > 0 && !rb_resolvable(ops, 3, &rp.step_ptr, &r.map)) resolved = false;
  }
  // no counter: the kernels' unconditional load reads a word of x instead, and every step_stride is 0
  if (!rp.step_ptr) rp.step_ptr = (const int*)(a0.M > 0 ? a0.x : a1.x);
  rp.blocks0 = pr.blocks0;
  rp.dbg = g_ln_dbg;
  dim3 grid(pr.blocks0 + (a1.M + 1) / 2), block(128);
  const int need = (D / 4 + 63) / 64;   // float4 per lane
  if (out_dtype != FOLEY_F32 && !foley_is_half(out_dtype)) return foley_set_err("ln_mod: bad dtype", __FILE__, __LINE__);
  const bool f32o = out_dtype == FOLEY_F32, f16o = out_dtype == FOLEY_F16;
  const bool pend = (a0.M > 0 && a0.pend.partials) || (a1.M > 0 && a1.pend.partials);
  // 16-bit slabs (LnPending::half): both row sets of a launch agree, and the slab type is the output type
  const int h0 = (a0.M > 0 && a0.pend.partials) ? a0.pend.half : -1, h1 = (a1.M > 0 && a1.pend.partials) ? a1.pend.half : -1;
  const int slab_dt = h0 >= 0 ? h0 : (h1 >= 0 ? h1 : 0);
  if ((h0 >= 0 && h1 >= 0 && h0 != h1) || (slab_dt != 0 && slab_dt != out_dtype))
    return foley_set_err("ln_mod: 16-bit pending slabs must have the output dtype (and agree between the two row sets)", __FILE__, __LINE__);
  const bool s16 = slab_dt != 0;
  // K: the kernel family (resolved or per operand), P: its argument
#define FOLEY_LN_PEND(K, P, G, B, ...)                                                         \
  {                                                                                            \
    if (f32o) FOLEY_LAUNCH((K<float, __VA_ARGS__>), G, B, 0, st, P, D, eps);                   \
    else if (f16o && s16) FOLEY_LAUNCH((K<f16_t, __VA_ARGS__, true>), G, B, 0, st, P, D, eps); \
    else if (f16o) FOLEY_LAUNCH((K<f16_t, __VA_ARGS__>), G, B, 0, st, P, D, eps);              \
    else if (s16) FOLEY_LAUNCH((K<bf16_t, __VA_ARGS__, true>), G, B, 0, st, P, D, eps);        \
    else FOLEY_LAUNCH((K<bf16_t, __VA_ARGS__>), G, B, 0, st, P, D, eps);                       \
  }
#define FOLEY_LN_PLAIN(K, P, G, B, ...)                                                          \
  {                                                                                              \
    if (f32o) FOLEY_LAUNCH((K<float, __VA_ARGS__>), G, B, 0, st, P, D, eps);                     \
    else if (f16o) FOLEY_LAUNCH((K<f16_t, __VA_ARGS__>), G, B, 0, st, P, D, eps);                \
    else FOLEY_LAUNCH((K<bf16_t, __VA_ARGS__>), G, B, 0, st, P, D, eps);                         \
  }
#define FOLEY_LN_ANY(K, P, G, B, V, ...)                           \
  {                                                                \
    if (pend) FOLEY_LN_PEND(K, P, G, B, V, true, ##__VA_ARGS__)    \
    else FOLEY_LN_PLAIN(K, P, G, B, V, false, ##__VA_ARGS__)       \
  }
  // rows that split evenly over 2 waves (D = 1536: 2 waves x 3 float4 per lane; 1408 / 256: one wave).  Two waves per row since
  // the slabs are 16-bit (round 3, one box: bs=1 loop 347.4 -> 345.8 ms, bs=8 1525.7 -> 1520.2, 30 s 1488.7 -> 1478.6 against three
  // waves, which were better with fp32 slabs in round 2)
  const int total_rows = a0.M + a1.M;
  const bool wide = total_rows <= 4096 && D % (4 * 64 * 2) == 0 && D / (4 * 64 * 2) <= 4;
  if (rp.dbg) {   // tools/ln_timeline.py: the probe's instantiations
    if (!(resolved && wide && out_dtype == FOLEY_BF16 && D == 1536))
      return foley_set_err("ln_mod: the timeline probe is built for the resolved two-wave kernel, bf16 output, D = 1536", __FILE__, __LINE__);
    rp.blocks0 = (a0.M + FOLEY_LN_RPB - 1) / FOLEY_LN_RPB;
    const dim3 gridw(rp.blocks0 + (a1.M + FOLEY_LN_RPB - 1) / FOLEY_LN_RPB), blk(64 * FOLEY_LN_RPB * 2);
    if (pend && s16) FOLEY_LAUNCH((ln_mod_wide_kernel<bf16_t, 3, true, 2, true, true>), gridw, blk, 0, st, rp, D, eps);
    else if (pend) FOLEY_LAUNCH((ln_mod_wide_kernel<bf16_t, 3, true, 2, false, true>), gridw, blk, 0, st, rp, D, eps);
    else FOLEY_LAUNCH((ln_mod_wide_kernel<bf16_t, 3, false, 2, false, true>), gridw, blk, 0, st, rp, D, eps);
    FOLEY_LAUNCH_CHECK();
    return 0;
  }
  if (wide) {
    LnPair prw = pr;   // the two-wave kernel takes FOLEY_LN_RPB rows per workgroup
    prw.blocks0 = rp.blocks0 = (a0.M + FOLEY_LN_RPB - 1) / FOLEY_LN_RPB;
    const dim3 gridw(prw.blocks0 + (a1.M + FOLEY_LN_RPB - 1) / FOLEY_LN_RPB), blk(64 * FOLEY_LN_RPB * 2);
    // Small grids (the single-clip regime: every workgroup resident at once, at most four two-wave workgroups per CU) store x and
    // the output rows write-through; larger ones, whose rows exceed the L2s anyway, keep the plain stores.
    const bool wt = resolved && !g_foley_store_default && gridw.x <= 4 * 256 && store_wt_fits((long)(a0.M > a1.M ? a0.M : a1.M) * D * 4);
    g_ln_last_wt = wt ? 1 : 0;
#define FOLEY_LNW(V)                                                          \
    {                                                                            \
      if (wt) FOLEY_LN_ANY(ln_mod_wide_wt_kernel, rp, gridw, blk, V, 2)          \
      else if (resolved) FOLEY_LN_ANY(ln_mod_wide_kernel, rp, gridw, blk, V, 2)  \
      else FOLEY_LN_ANY(ln_mod_wide_each_kernel, prw, gridw, blk, V, 2)          \
    }
    const int v2 = D / (4 * 64 * 2);
    if (v2 == 1) FOLEY_LNW(1)
    else if (v2 == 2) FOLEY_LNW(2)
    else if (v2 == 3) FOLEY_LNW(3)
    else FOLEY_LNW(4)
#undef FOLEY_LNW
    FOLEY_LAUNCH_CHECK();
    return 0;
  }
#define FOLEY_LNN(V)                                                             \
  {                                                                              \
    if (resolved) FOLEY_LN_ANY(ln_mod_kernel, rp, grid, block, V)                \
    else FOLEY_LN_ANY(ln_mod_each_kernel, pr, grid, block, V)                    \
  }
  if (need <= 2) FOLEY_LNN(2)
  else if (need <= 4) FOLEY_LNN(4)
  else if (need <= 6) FOLEY_LNN(6)
  else FOLEY_LNN(8)
#undef FOLEY_LNN
#undef FOLEY_LN_ANY
#undef FOLEY_LN_PLAIN
#undef FOLEY_LN_PEND
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_ln_mod(const float* x, int M, int D, float eps, const RowBcast& shift, const RowBcast& scale,
                  void* out, int out_dtype, hipStream_t st) {
  LnArgs a0{const_cast<float*>(x), M, shift, scale, out, LnPending{}};
  LnArgs a1 = a0;
  a1.M = 0;
  return launch_ln_mod_pair(a0, a1, D, eps, out_dtype, st);
}

int launch_ln_mod_pending(float* x, int M, int D, float eps, const RowBcast& shift, const RowBcast& scale,
                          void* out, int out_dtype, const LnPending& pend, hipStream_t st) {
  LnArgs a0{x, M, shift, scale, out, pend};
  LnArgs a1 = a0;
  a1.M = 0;
  return launch_ln_mod_pair(a0, a1, D, eps, out_dtype, st);
}

int launch_qkv_split_pair(const QkvSplitArgs& a0, const QkvSplitArgs& a1, hipStream_t st) {
  if (a0.out_dtype != a1.out_dtype) return foley_set_err("qkv_split pair: dtype mismatch", __FILE__, __LINE__);
  QkvPair pr;
  pr.a[0] = a0;
  pr.a[1] = a1;
  auto nblk = [](const QkvSplitArgs& q) {
    if (q.M <= 0) return 0;
    const int nQ = q.nK - (q.vt_pitch > 0 ? 1 : 0);
    const int bqk = (int)(((long)q.M * q.H * nQ + 15) / 16);
    const int bv = q.vt_pitch > 0 ? (q.M / q.L) * q.H * ((q.L + 31) / 32) : 0;   // rows are [clip][l]
    return bqk + bv;
  };
  if ((a0.M > 0 && a0.M % a0.L) || (a1.M > 0 && a1.M % a1.L))
    return foley_set_err("qkv_split: M must be a multiple of L", __FILE__, __LINE__);
  pr.blocks0 = nblk(a0);
  dim3 grid((unsigned)(pr.blocks0 + nblk(a1))), block(256);
  if (grid.x == 0) return 0;
  if (a0.out_dtype == FOLEY_BF16) FOLEY_LAUNCH(qkv_split_kernel<bf16_t>, grid, block, 0, st, pr);
  else if (a0.out_dtype == FOLEY_F16) FOLEY_LAUNCH(qkv_split_kernel<f16_t>, grid, block, 0, st, pr);
  else FOLEY_LAUNCH(qkv_split_kernel<float>, grid, block, 0, st, pr);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_qkv_split(const QkvSplitArgs& a, hipStream_t st) {
  QkvSplitArgs none = a;
  none.M = 0;
  return launch_qkv_split_pair(a, none, st);
}

// flag |= 1 when some row s >= period of a group differs (bit pattern) from row s - period
__global__ void rows_periodic_check_kernel(const unsigned* __restrict__ x, int groups, int rows, int period, int D, int* flag) {
  const long per_g = (long)(rows - period) * D, n = (long)groups * per_g;
  unsigned diff = 0;   // bit g: group g (<= 32 groups) has a row that differs from the one `period` rows above it -> flag[g] = 1
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long g = i / per_g, r = i - g * per_g;
    const long at = (g * rows + period) * D + r;
    if (x[at] != x[at - (long)period * D]) diff |= 1u << g;
  }
  for (int g = 0; g < groups; ++g)
    if (diff >> g & 1u) atomicOr(flag + g, 1);
}

int launch_rows_periodic_check(const float* x, int groups, int rows, int period, int D, int* flag, hipStream_t st) {
  if (rows <= period) return 0;
  if (groups > 32) return foley_set_err("rows_periodic_check: at most 32 groups", __FILE__, __LINE__);
  const long n = (long)groups * (rows - period) * D;
  FOLEY_LAUNCH(rows_periodic_check_kernel, dim3(grid1d(n, 256)), dim3(256), 0, st, (const unsigned*)x, groups, rows, period, D, flag);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_rows_add_act(const float* a, const RowBcast& v, int R, int D, int act_silu, void* out, int out_dtype,
                        hipStream_t st) {
  const long n = (long)R * D;
  if (out_dtype == FOLEY_F32)
    FOLEY_LAUNCH(rows_add_act_kernel<float>, dim3(grid1d(n, 256)), dim3(256), 0, st, a, v, R, D, act_silu, (float*)out);
  else if (out_dtype == FOLEY_BF16)
    FOLEY_LAUNCH(rows_add_act_kernel<bf16_t>, dim3(grid1d(n, 256)), dim3(256), 0, st, a, v, R, D, act_silu, (bf16_t*)out);
  else if (out_dtype == FOLEY_F16)
    FOLEY_LAUNCH(rows_add_act_kernel<f16_t>, dim3(grid1d(n, 256)), dim3(256), 0, st, a, v, R, D, act_silu, (f16_t*)out);
  else return foley_set_err("rows_add_act: bad dtype", __FILE__, __LINE__);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_add_periodic(const float* x, const float* pos, int R, int D, int period, void* out, int out_dtype,
                        hipStream_t st) {
  const long n = (long)R * D;
  if (out_dtype == FOLEY_F32)
    FOLEY_LAUNCH(add_periodic_kernel<float>, dim3(grid1d(n, 256)), dim3(256), 0, st, x, pos, R, D, period, (float*)out);
  else if (out_dtype == FOLEY_BF16)
    FOLEY_LAUNCH(add_periodic_kernel<bf16_t>, dim3(grid1d(n, 256)), dim3(256), 0, st, x, pos, R, D, period, (bf16_t*)out);
  else if (out_dtype == FOLEY_F16)
    FOLEY_LAUNCH(add_periodic_kernel<f16_t>, dim3(grid1d(n, 256)), dim3(256), 0, st, x, pos, R, D, period, (f16_t*)out);
  else return foley_set_err("add_periodic: bad dtype", __FILE__, __LINE__);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_gather_rows(const float* src, const int* idx, int n_idx, int groups, int src_rows, int D, float* out,
                       hipStream_t st) {
  const long n = (long)groups * n_idx * D;
  FOLEY_LAUNCH(gather_rows_kernel, dim3(grid1d(n, 256)), dim3(256), 0, st, src, idx, n_idx, groups, src_rows, D, out);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_cast(const void* src, int sd, void* dst, int dd, long n, hipStream_t st) {
  dim3 g(grid1d(n, 256)), b(256);
  if (sd == FOLEY_F32 && dd == FOLEY_BF16)
    FOLEY_LAUNCH((cast_kernel<float, bf16_t>), g, b, 0, st, (const float*)src, (bf16_t*)dst, n);
  else if (sd == FOLEY_BF16 && dd == FOLEY_F32)
    FOLEY_LAUNCH((cast_kernel<bf16_t, float>), g, b, 0, st, (const bf16_t*)src, (float*)dst, n);
  else if (sd == FOLEY_F32 && dd == FOLEY_F16)
    FOLEY_LAUNCH((cast_kernel<float, f16_t>), g, b, 0, st, (const float*)src, (f16_t*)dst, n);
  else if (sd == FOLEY_F16 && dd == FOLEY_F32)
    FOLEY_LAUNCH((cast_kernel<f16_t, float>), g, b, 0, st, (const f16_t*)src, (float*)dst, n);
  else if (sd == FOLEY_F32 && dd == FOLEY_F32)
    FOLEY_LAUNCH((cast_kernel<float, float>), g, b, 0, st, (const float*)src, (float*)dst, n);
  else return foley_set_err("cast: unsupported dtype pair", __FILE__, __LINE__);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_latent_rows(const float* x, int clips, int C, int L, int ncfg, void* out, int out_dtype, hipStream_t st) {
  dim3 grid((L + 31) / 32, (C + 31) / 32, clips), block(256);
  if (out_dtype == FOLEY_F32)
    FOLEY_LAUNCH(latent_rows_kernel<float>, grid, block, 0, st, x, clips, C, L, ncfg, (float*)out);
  else if (out_dtype == FOLEY_BF16)
    FOLEY_LAUNCH(latent_rows_kernel<bf16_t>, grid, block, 0, st, x, clips, C, L, ncfg, (bf16_t*)out);
  else if (out_dtype == FOLEY_F16)
    FOLEY_LAUNCH(latent_rows_kernel<f16_t>, grid, block, 0, st, x, clips, C, L, ncfg, (f16_t*)out);
  else return foley_set_err("latent_rows: bad dtype", __FILE__, __LINE__);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

static int windows_args_ok(int clips, int n_win, int L, int Ltot, const int* starts, const float* weights) {
  return n_win >= 1 && clips >= n_win && clips % n_win == 0 && starts && weights && Ltot >= L && (long)Ltot <= (long)n_win * L;
}

// the kernel of a.form for one rows dtype; the windows form's grid runs over global frames and variations
template <typename OutT>
static void launch_step_form(const StepArgs& a, hipStream_t st) {
  const bool win = a.form == STEP_FORM_WINDOWS;
  const dim3 grid(((win ? a.Ltot : a.L) + 31) / 32, (a.C + 31) / 32, win ? a.clips / a.n_win : a.clips), block(256);
  if (a.proj_coef) {   // projected guidance: the instantiations of the same forms with the projected combine
    if (a.hist) {
      if (win) FOLEY_LAUNCH(solver_step_windows_proj_hist_kernel<OutT>, grid, block, 0, st, a);
      else if (a.form == STEP_FORM_EDIT) FOLEY_LAUNCH((solver_step_proj_hist_kernel<OutT, true>), grid, block, 0, st, a);
      else FOLEY_LAUNCH((solver_step_proj_hist_kernel<OutT, false>), grid, block, 0, st, a);
    } else {
      if (win) FOLEY_LAUNCH(solver_step_windows_proj_kernel<OutT>, grid, block, 0, st, a);
      else if (a.form == STEP_FORM_EDIT) FOLEY_LAUNCH((solver_step_proj_kernel<OutT, true>), grid, block, 0, st, a);
      else FOLEY_LAUNCH((solver_step_proj_kernel<OutT, false>), grid, block, 0, st, a);
    }
    return;
  }
  if (a.hist) {   // a multistep run: the history instantiation of the same form
    if (win) FOLEY_LAUNCH(solver_step_windows_hist_kernel<OutT>, grid, block, 0, st, a);
    else if (a.form == STEP_FORM_EDIT) FOLEY_LAUNCH((solver_step_hist_kernel<OutT, true>), grid, block, 0, st, a);
    else FOLEY_LAUNCH((solver_step_hist_kernel<OutT, false>), grid, block, 0, st, a);
    return;
  }
  if (win) FOLEY_LAUNCH(solver_step_windows_kernel<OutT>, grid, block, 0, st, a);
  else if (a.form == STEP_FORM_EDIT) FOLEY_LAUNCH((solver_step_kernel<OutT, true>), grid, block, 0, st, a);
  else FOLEY_LAUNCH((solver_step_kernel<OutT, false>), grid, block, 0, st, a);
}

int launch_solver_step(const StepArgs& a, hipStream_t st) {
  if (a.form == STEP_FORM_EDIT) {
    if (!a.x0 || !a.noise) return foley_set_err("solver_step_edit: x0 and noise are required", __FILE__, __LINE__);
    if ((a.x0_clips != 1 && a.x0_clips != a.clips) || (a.mask && a.mask_clips != 1 && a.mask_clips != a.clips))
      return foley_set_err("solver_step_edit: x0 / mask clip count must be 1 or clips", __FILE__, __LINE__);
  } else if (a.form == STEP_FORM_WINDOWS) {
    if (!windows_args_ok(a.clips, a.n_win, a.L, a.Ltot, a.starts, a.weights))
      return foley_set_err("solver_step_windows: clips must be a multiple of n_win, La <= Ltot <= n_win*La, tables required", __FILE__, __LINE__);
  }
  if ((a.hist || a.hist_slots) && (!a.hist || a.hist_slots < 1 || a.hist_slots > 2))
    return foley_set_err("solver_step: a history ring needs its buffer and 1 or 2 slots", __FILE__, __LINE__);
  if (a.proj_plane && !a.proj_coef) return foley_set_err("solver_step: a projection plane needs its coefficients", __FILE__, __LINE__);
  if (a.proj_coef && (a.ncfg != 2 || a.clip_scale))
    return foley_set_err("solver_step: projected guidance takes two halves (ncfg 2) and no rescale factors", __FILE__, __LINE__);
  if (a.rows_dtype == FOLEY_BF16) launch_step_form<bf16_t>(a, st);
  else if (a.rows_dtype == FOLEY_F16) launch_step_form<f16_t>(a, st);
  else launch_step_form<float>(a, st);
  FOLEY_LAUNCH_CHECK();
  FOLEY_LAUNCH(step_increment_kernel, dim3(1), dim3(1), 0, st, a.step_ptr);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

static int flowedit_args_ok(const FlowEditArgs& a) {
  if (!a.z || !a.x_src || !a.noise) return foley_set_err("flowedit: z, x_src and noise are required", __FILE__, __LINE__);
  if (a.V < 1 || a.V > 32767 || a.C < 1 || a.L < 1 || a.n_iter < 1)
    return foley_set_err("flowedit: 1 <= V <= 32767, C, L, n_iter >= 1", __FILE__, __LINE__);
  if ((a.src_clips != 1 && a.src_clips != a.V) || (a.mask && a.mask_clips != 1 && a.mask_clips != a.V))
    return foley_set_err("flowedit: src_clips / mask_clips must be 1 or V", __FILE__, __LINE__);
  if (a.noise_rows != 1 && a.noise_rows != a.n_iter)
    return foley_set_err("flowedit: noise_rows must be 1 or n_iter", __FILE__, __LINE__);
  if (a.rows_out && a.rows_dtype != FOLEY_F32 && a.rows_dtype != FOLEY_BF16 && a.rows_dtype != FOLEY_F16)
    return foley_set_err("flowedit: rows_dtype must be fp32, bf16 or fp16", __FILE__, __LINE__);
  return 0;
}

int launch_flowedit_step(const FlowEditArgs& a, hipStream_t st) {
  if (!a.pred || !a.coef || !a.step_ptr) return foley_set_err("flowedit_step: pred, coef and step_ptr are required", __FILE__, __LINE__);
  if (int rc = flowedit_args_ok(a)) return rc;
  const dim3 grid((a.L + 31) / 32, (a.C + 31) / 32, a.V), block(256);
  if (a.rows_dtype == FOLEY_BF16) FOLEY_LAUNCH(flowedit_step_kernel<bf16_t>, grid, block, 0, st, a);
  else if (a.rows_dtype == FOLEY_F16) FOLEY_LAUNCH(flowedit_step_kernel<f16_t>, grid, block, 0, st, a);
  else FOLEY_LAUNCH(flowedit_step_kernel<float>, grid, block, 0, st, a);
  FOLEY_LAUNCH_CHECK();
  FOLEY_LAUNCH(step_increment_kernel, dim3(1), dim3(1), 0, st, a.step_ptr);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_flowedit_stage(const FlowEditArgs& a, float sigma, int noise_row, hipStream_t st) {
  if (!a.rows_out) return foley_set_err("flowedit_stage: rows_out is required", __FILE__, __LINE__);
  if (int rc = flowedit_args_ok(a)) return rc;
  if (noise_row < 0 || noise_row >= a.noise_rows) return foley_set_err("flowedit_stage: noise_row outside [0, noise_rows)", __FILE__, __LINE__);
  if (!(sigma >= 0.f && sigma <= 1.f)) return foley_set_err("flowedit_stage: sigma must lie in [0, 1]", __FILE__, __LINE__);
  const dim3 grid((a.L + 31) / 32, (a.C + 31) / 32, a.V), block(256);
  if (a.rows_dtype == FOLEY_BF16) FOLEY_LAUNCH(flowedit_stage_kernel<bf16_t>, grid, block, 0, st, a, sigma, noise_row);
  else if (a.rows_dtype == FOLEY_F16) FOLEY_LAUNCH(flowedit_stage_kernel<f16_t>, grid, block, 0, st, a, sigma, noise_row);
  else FOLEY_LAUNCH(flowedit_stage_kernel<float>, grid, block, 0, st, a, sigma, noise_row);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

long guidance_stats_floats(int clips, int L) { return (long)clips * ((L + GS_ROWS - 1) / GS_ROWS) * GS_REC; }

int launch_guidance_stats(const StepArgs& a, float* part, const float* phi_ptr, float phi, float* clip_scale, hipStream_t st) {
  if (!a.pred || !a.step_ptr || !part || !clip_scale || a.clips < 1 || a.clips > 65535 || a.C < 1 || a.L < 1 || a.ncfg < 1 || a.ncfg > 3)
    return foley_set_err("guidance_stats: pred, step_ptr, work and output buffers required; 1 <= clips <= 65535, ncfg in [1, 3]", __FILE__, __LINE__);
  if (a.C > 256) return foley_set_err("guidance_stats: at most 256 channels", __FILE__, __LINE__);
  if ((long)a.clips * a.C * a.L >= (1L << 31) || (long)a.C * a.L >= (1L << 24))
    return foley_set_err("guidance_stats: clip too large (C*L < 2^24 elements per clip)", __FILE__, __LINE__);
  const int nblk = (a.L + GS_ROWS - 1) / GS_ROWS;
  dim3 grid(nblk, a.clips), block(256);
  if (a.C <= 64) FOLEY_LAUNCH(guidance_stats_kernel<1>, grid, block, 0, st, a, part);
  else if (a.C <= 128) FOLEY_LAUNCH(guidance_stats_kernel<2>, grid, block, 0, st, a, part);
  else FOLEY_LAUNCH(guidance_stats_kernel<4>, grid, block, 0, st, a, part);
  FOLEY_LAUNCH_CHECK();
  FOLEY_LAUNCH(guidance_scale_kernel, dim3(a.clips), dim3(64), 0, st, (const float*)part, nblk, phi_ptr, phi, clip_scale);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

long guidance_project_floats(int clips, int L) { return (long)clips * ((L + GS_ROWS - 1) / GS_ROWS) * PJ_REC; }

template <int MODE>
static void launch_proj_stats(const StepArgs& a, const float* rows, float* part, float* plane, dim3 grid, hipStream_t st) {
  const dim3 block(256);
  if (a.C <= 64) FOLEY_LAUNCH((guidance_proj_stats_kernel<1, MODE>), grid, block, 0, st, a.pred, plane, rows, (const int*)a.step_ptr, a.clips, a.C, a.L, part);
  else if (a.C <= 128) FOLEY_LAUNCH((guidance_proj_stats_kernel<2, MODE>), grid, block, 0, st, a.pred, plane, rows, (const int*)a.step_ptr, a.clips, a.C, a.L, part);
  else FOLEY_LAUNCH((guidance_proj_stats_kernel<4, MODE>), grid, block, 0, st, a.pred, plane, rows, (const int*)a.step_ptr, a.clips, a.C, a.L, part);
}

int launch_guidance_project(const StepArgs& a, int mode, const float* rows, float* part, float* coef, float* plane, hipStream_t st) {
  if (mode != PROJ_APG && mode != PROJ_ZERO_STAR) return foley_set_err("guidance_project: unknown mode (1 APG, 2 CFG-Zero*)", __FILE__, __LINE__);
  if (a.ncfg != 2) return foley_set_err("guidance_project: projected guidance takes two halves (ncfg 2)", __FILE__, __LINE__);
  if (!a.pred || !a.step_ptr || !rows || !part || !coef || a.clips < 1 || a.clips > 65535 || a.C < 1 || a.L < 1)
    return foley_set_err("guidance_project: pred, step_ptr, rows, work and coefficient buffers required; 1 <= clips <= 65535", __FILE__, __LINE__);
  if (mode == PROJ_APG && !plane) return foley_set_err("guidance_project: APG needs its momentum plane", __FILE__, __LINE__);
  if (a.C > 256) return foley_set_err("guidance_project: at most 256 channels", __FILE__, __LINE__);
  if ((long)a.clips * a.C * a.L >= (1L << 31) || (long)a.C * a.L >= (1L << 24))
    return foley_set_err("guidance_project: clip too large (C*L < 2^24 elements per clip)", __FILE__, __LINE__);
  const int nblk = (a.L + GS_ROWS - 1) / GS_ROWS;
  const dim3 grid(nblk, a.clips);
  if (mode == PROJ_APG) launch_proj_stats<PROJ_APG>(a, rows, part, plane, grid, st);
  else launch_proj_stats<PROJ_ZERO_STAR>(a, rows, part, nullptr, grid, st);
  FOLEY_LAUNCH_CHECK();
  FOLEY_LAUNCH(guidance_proj_coef_kernel, dim3(a.clips), dim3(64), 0, st, (const float*)part, nblk, mode, rows, a.sched, a.guidance,
               (const int*)a.step_ptr, coef);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

long cache_probe_floats(int Bc, int La) { return (long)Bc * ((La + CP_ROWS - 1) / CP_ROWS) * 2; }

int launch_cache_probe(const float* a0, int Bc, int La, int D, float eps, const RowBcast& shift, const RowBcast& scale, float* m_prev,
                       float* part, float* rel, hipStream_t st) {
  if (Bc < 1 || La < 1 || D < 4 || D % 4 || D > 8 * 256) return foley_set_err("cache_probe: D must be a multiple of 4 in [4, 2048], Bc and La >= 1", __FILE__, __LINE__);
  if (!a0 || !m_prev || !part || !rel) return foley_set_err("cache_probe: null operand", __FILE__, __LINE__);
  for (const void* p : {(const void*)a0, (const void*)m_prev, (const void*)shift.p, (const void*)scale.p})
    if ((uintptr_t)p & 15) return foley_set_err("cache_probe: operands must be 16-byte aligned", __FILE__, __LINE__);
  if ((shift.p && (shift.ld % 4 || shift.step_stride % 4)) || (scale.p && (scale.ld % 4 || scale.step_stride % 4)))
    return foley_set_err("cache_probe: shift / scale row pitch must be a multiple of 4", __FILE__, __LINE__);
  const dim3 grid((La + CP_ROWS - 1) / CP_ROWS, Bc), block(64 * CP_ROWS);
  const int need = (D / 4 + 63) / 64;   // float4 per lane
  if (need <= 1) FOLEY_LAUNCH((cache_probe_kernel<1>), grid, block, 0, st, a0, La, D, eps, shift, scale, m_prev, part);
  else if (need <= 6) FOLEY_LAUNCH((cache_probe_kernel<6>), grid, block, 0, st, a0, La, D, eps, shift, scale, m_prev, part);
  else FOLEY_LAUNCH((cache_probe_kernel<8>), grid, block, 0, st, a0, La, D, eps, shift, scale, m_prev, part);
  FOLEY_LAUNCH_CHECK();
  hipLaunchKernelGGL(cache_rel_kernel, dim3(Bc), dim3(64), 0, st, part, (int)grid.x, rel);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

static int launch_cache_axpy(bool sub, const float* src, float* dst, long n, hipStream_t st) {
  if (n < 0 || (n > 0 && (!src || !dst))) return foley_set_err("cache_delta / cache_apply: bad operands", __FILE__, __LINE__);
  if (n == 0) return 0;
  const int vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const dim3 grid(grid1d((n + 3) / 4, 256)), block(256);
  if (sub) FOLEY_LAUNCH((cache_axpy_kernel<true>), grid, block, 0, st, src, dst, n, vec);
  else FOLEY_LAUNCH((cache_axpy_kernel<false>), grid, block, 0, st, src, dst, n, vec);
  FOLEY_LAUNCH_CHECK();
  return 0;
}
int launch_cache_delta(const float* aN, float* delta, long n, hipStream_t st) { return launch_cache_axpy(true, aN, delta, n, st); }
int launch_cache_apply(float* audio, const float* delta, long n, hipStream_t st) { return launch_cache_axpy(false, delta, audio, n, st); }

int launch_windows_stitch(const float* x, int clips, int n_win, int C, int L, int Ltot, const int* starts, const float* weights,
                          float* out, hipStream_t st) {
  if (!x || !out || C < 1 || L < 1 || !windows_args_ok(clips, n_win, L, Ltot, starts, weights))
    return foley_set_err("windows_stitch: clips must be a multiple of n_win, La <= Ltot <= n_win*La, tables required", __FILE__, __LINE__);
  dim3 grid((Ltot + 255) / 256, C, clips / n_win), block(256);
  FOLEY_LAUNCH(windows_stitch_kernel, grid, block, 0, st, x, n_win, C, L, Ltot, starts, weights, out);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_flow_mix(const float* noise, const float* x0, int x0_clips, int clips, int C, int L, float sigma, float* out,
                    hipStream_t st) {
  if (!noise || !x0 || !out || clips < 1 || C < 1 || L < 1 || (x0_clips != 1 && x0_clips != clips))
    return foley_set_err("flow_mix: bad arguments (x0 clip count must be 1 or clips)", __FILE__, __LINE__);
  const long plane = (long)C * L, n = plane * clips;
  FOLEY_LAUNCH(flow_mix_kernel, dim3(grid1d(n, 256)), dim3(256), 0, st, noise, x0, plane, n, x0_clips != 1 || clips == 1 ? 1 : 0,
               sigma, out);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_dac_in(const float* x, const float* w, const float* bias, const float* alpha, int B, int T, int C,
                  float* out0, float* out1, hipStream_t st) {
  if (C % 4) return foley_set_err("dac_in: channel count must be a multiple of 4", __FILE__, __LINE__);
  FOLEY_LAUNCH(dac_in_kernel, dim3(grid1d((long)B * T * (C / 4), 256)), dim3(256), 0, st, x, w, bias, alpha, B, T, C,
                     out0, out1);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Token regrouping between a fused q / k / v projection and the attention of the conditioning encoders (round 5): the
// divided space-time attention of the Synchformer (reference models/synchformer/vit_helper.py:37-105: patch tokens attend over
// the frames of their location or the locations of their frame, the CLS key / value prepended to every group) and the plain
// ViT attention of SigLIP2 / CLAP.  qkv [rows, 3*H*64] ('(K H D)' packing of nn.Linear(dim, 3 dim)); group g takes source rows
// idx_q[g][0..Sq) as queries and idx_kv[g][0..Skv) as keys / values, written head-major as foley_op_attention_hd reads them:
// q [G,H,Sq,64], k [G,H,Skv,64], v [G,H,Skv,64] or - 16-bit operands - v^T [G,H,64,pitch] (zeros beyond Skv) through a 64x64 LDS
// transpose.  One launch replaces ~10 full-tensor torch copies (permute / cat / contiguous / the transposed-V staging).
template <typename E>   // E = the element's storage type (uint16_t: bf16 / fp16, uint32_t: fp32)
__global__ __launch_bounds__(256) void qkv_regroup_kernel(const E* __restrict__ qkv, int H, const int* __restrict__ idx_q, int Sq,
                                                          const int* __restrict__ idx_kv, int Skv, E* __restrict__ q, E* __restrict__ k,
                                                          E* __restrict__ v, int vt_pitch, int n_rows) {
  constexpr int HD = 64, CPR = HD * sizeof(E) / 16;   // 16-byte chunks per head row
  __shared__ __attribute__((aligned(16))) E tile[64][HD + 16 / sizeof(E)];
  const int t0 = blockIdx.x * 64, h = blockIdx.y, g = blockIdx.z;
  const long ld = 3L * H * HD;
  const int tid = threadIdx.x;
  for (int c = tid; c < 64 * CPR; c += 256) {
    const int t = t0 + c / CPR, ch = c % CPR;
    if (t < Sq) {
      const long r = min(max(idx_q[(long)g * Sq + t], 0), n_rows - 1);   // caller-supplied table: never read outside qkv [n_rows, 3*H*64]
      *(u32x4*)(q + (((long)g * H + h) * Sq + t) * HD + ch * (16 / sizeof(E))) = *(const u32x4*)(qkv + r * ld + (long)h * HD + ch * (16 / sizeof(E)));
    }
    if (t < Skv) {
      const long r = min(max(idx_kv[(long)g * Skv + t], 0), n_rows - 1);
      const E* src = qkv + r * ld + (long)(H + h) * HD + ch * (16 / sizeof(E));
      *(u32x4*)(k + (((long)g * H + h) * Skv + t) * HD + ch * (16 / sizeof(E))) = *(const u32x4*)src;
      const u32x4 vv = *(const u32x4*)(src + (long)H * HD);
      if (vt_pitch == 0) *(u32x4*)(v + (((long)g * H + h) * Skv + t) * HD + ch * (16 / sizeof(E))) = vv;
      else *(u32x4*)&tile[c / CPR][ch * (16 / sizeof(E))] = vv;
    } else if (vt_pitch != 0) {
      *(u32x4*)&tile[c / CPR][ch * (16 / sizeof(E))] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  if (vt_pitch == 0) return;   // grid-uniform
  __syncthreads();
  // v^T rows: d-major, 8 tokens (16-bit) per 16-byte store
  constexpr int TPS = 16 / sizeof(E);   // tokens per store
  for (int c = tid; c < HD * (64 / TPS); c += 256) {
    const int d = c / (64 / TPS), tb = (c % (64 / TPS)) * TPS;
    if (t0 + tb >= vt_pitch) continue;
    E tmp[TPS];
#pragma unroll
    for (int u = 0; u < TPS; ++u) tmp[u] = tile[tb + u][d];
    *(u32x4*)(v + (((long)g * H + h) * HD + d) * vt_pitch + t0 + tb) = *(const u32x4*)tmp;
  }
}

int launch_qkv_regroup(const void* qkv, int n_rows, int dtype, int H, const int* idx_q, int G, int Sq, const int* idx_kv, int Skv, void* q, void* k,
                       void* v, int vt_pitch, hipStream_t st) {
  if (G < 1 || H < 1 || Sq < 1 || Skv < 1 || n_rows < 1) return foley_set_err("qkv_regroup: empty problem", __FILE__, __LINE__);
  if (vt_pitch && (vt_pitch % 8 || vt_pitch < Skv || vt_pitch > (Skv + 63) / 64 * 64))
    return foley_set_err("qkv_regroup: the transposed-V pitch must be a multiple of 8 in [Skv, ceil64(Skv)]", __FILE__, __LINE__);
  if (((uintptr_t)qkv | (uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return foley_set_err("qkv_regroup: operands must be 16-byte aligned", __FILE__, __LINE__);
  const int S = Sq > Skv ? Sq : Skv;
  const dim3 grid((S + 63) / 64, H, G);
  if (dtype == FOLEY_F32) {
    if (vt_pitch) return foley_set_err("qkv_regroup: fp32 operands keep V untransposed", __FILE__, __LINE__);
    FOLEY_LAUNCH(qkv_regroup_kernel<uint32_t>, grid, dim3(256), 0, st, (const uint32_t*)qkv, H, idx_q, Sq, idx_kv, Skv, (uint32_t*)q, (uint32_t*)k, (uint32_t*)v, 0, n_rows);
  } else if (foley_is_half(dtype)) {
    FOLEY_LAUNCH(qkv_regroup_kernel<uint16_t>, grid, dim3(256), 0, st, (const uint16_t*)qkv, H, idx_q, Sq, idx_kv, Skv, (uint16_t*)q, (uint16_t*)k, (uint16_t*)v, vt_pitch, n_rows);
  } else {
    return foley_set_err("qkv_regroup: fp32, bf16 or fp16 operands", __FILE__, __LINE__);
  }
  FOLEY_LAUNCH_CHECK();
  return 0;
}

// One pass of the separable antialiased uint8 resize the reference pre-processes its frames with (torchvision v2.Resize(bicubic,
// antialias=True) on uint8 CPU tensors, nodes.py:184-196 / utils.py:262-283 - ATen's native uint8 kernel, PIL's scheme): along the
// resized axis every output sample is a fixed-point weighted sum of `xsize` input bytes starting at `xmin`, int16 weights scaled by
// 2^prec, accumulator preset to 2^(prec-1), arithmetic shift, saturate to a byte.  The horizontal pass runs first and its rounded
// uint8 image feeds the vertical pass - integer arithmetic end to end, so the result is the reference's bit for bit
// (tests/test_encoders_gpu.py; the tables are built by host/encoders.py::aa_tables and pinned in tests/test_oracle_golden.py).
// Layout [outer, len, inner]: inner = 1 is the horizontal pass (threads along the output row), inner = W the vertical one
// (threads along x, V bytes each - one 32-bit load per tap when the row pitch allows).  HBM-bound byte work: 37 MB in, 31 MB out
// for the 40 SigLIP2 frames of a 5 s clip; the taps of neighbouring outputs overlap in the L1 / L2.
template <int V>
__global__ __launch_bounds__(256) void resize_aa_u8_kernel(const uint8_t* __restrict__ in, long outer, int len_in, long inner, int len_out,
                                                           const int* __restrict__ xmin, const int* __restrict__ xsize,
                                                           const short* __restrict__ w, int kmax, int prec, uint8_t* __restrict__ out) {
  const long inner_v = inner / V;
  const long total = outer * len_out * inner_v;
  for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256L) {
    const long iv = idx % inner_v, t = idx / inner_v;
    const int xo = (int)(t % len_out);
    const long o = t / len_out;
    int x0 = xmin[xo], n = xsize[xo];   // clamped: a bad table must not read outside the image
    x0 = x0 < 0 ? 0 : (x0 > len_in ? len_in : x0);
    n = n > kmax ? kmax : n;
    n = n > len_in - x0 ? len_in - x0 : n;
    const short* wr = w + (long)xo * kmax;
    const uint8_t* src = in + (o * len_in + x0) * inner + iv * V;
    int acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 1 << (prec - 1);
    for (int j = 0; j < n; ++j) {
      const int wj = wr[j];
      if constexpr (V == 4) {
        const uint32_t px = *(const uint32_t*)(src + (long)j * inner);
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[v] += (int)((px >> (8 * v)) & 255u) * wj;
      } else if constexpr (V == 2) {
        const uint32_t px = *(const uint16_t*)(src + (long)j * inner);
        acc[0] += (int)(px & 255u) * wj;
        acc[1] += (int)(px >> 8) * wj;
      } else {
        acc[0] += (int)src[(long)j * inner] * wj;
      }
    }
    uint32_t packed = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      int r = acc[v] >> prec;
      r = r < 0 ? 0 : (r > 255 ? 255 : r);
      packed |= (uint32_t)r << (8 * v);
    }
    uint8_t* dst = out + (o * len_out + xo) * inner + iv * V;
    if constexpr (V == 4) *(uint32_t*)dst = packed;
    else if constexpr (V == 2) *(uint16_t*)dst = (uint16_t)packed;
    else *dst = (uint8_t)packed;
  }
}

int launch_resize_aa_u8(const uint8_t* in, long outer, int len_in, long inner, int len_out, const int* xmin, const int* xsize,
                        const short* w, int kmax, int prec, uint8_t* out, hipStream_t st) {
  if (outer < 1 || inner < 1 || len_in < 1 || len_out < 1 || kmax < 1) return foley_set_err("resize_aa_u8: empty problem", __FILE__, __LINE__);
  if (prec < 1 || prec > 22) return foley_set_err("resize_aa_u8: weight precision must be in [1, 22] bits", __FILE__, __LINE__);
  const int V = (inner % 4 == 0 && !(((uintptr_t)in | (uintptr_t)out) & 3)) ? 4 : (inner % 2 == 0 && !(((uintptr_t)in | (uintptr_t)out) & 1)) ? 2 : 1;
  const long total = outer * len_out * (inner / V);
  const long blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < 65536L * 16 ? blocks : 65536L * 16));
  if (V == 4) FOLEY_LAUNCH(resize_aa_u8_kernel<4>, grid, dim3(256), 0, st, in, outer, len_in, inner, len_out, xmin, xsize, w, kmax, prec, out);
  else if (V == 2) FOLEY_LAUNCH(resize_aa_u8_kernel<2>, grid, dim3(256), 0, st, in, outer, len_in, inner, len_out, xmin, xsize, w, kmax, prec, out);
  else FOLEY_LAUNCH(resize_aa_u8_kernel<1>, grid, dim3(256), 0, st, in, outer, len_in, inner, len_out, xmin, xsize, w, kmax, prec, out);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_rows_to_planes(const float* rows, int B, int T, int C, float* out, hipStream_t st) {
  FOLEY_LAUNCH(rows_to_planes_kernel, dim3(grid1d((long)B * T * C, 256)), dim3(256), 0, st, rows, B, T, C, out);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

int launch_dac_out(const float* s, const float* w, const float* bias, int B, int T, int C, float* out,
                   hipStream_t st) {
  if (C % 4 || C > 256) return foley_set_err("dac_out: unsupported channel count", __FILE__, __LINE__);
  const size_t sh = (70 * (C + 1) + 7 * C) * sizeof(float);
  FOLEY_LAUNCH(dac_out_kernel, dim3((T + 63) / 64, B), dim3(256), sh, st, s, w, bias, T, C, out);
  FOLEY_LAUNCH_CHECK();
  return 0;
}

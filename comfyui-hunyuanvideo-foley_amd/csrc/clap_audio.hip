// The CLAP audio tower's own kernels (host/clap_score.py): transformers' ClapFeatureExtractor + ClapAudioModel (HTSAT, a Swin
// transformer over a log-mel image) restated for the engine.  Everything else of the tower is foley_op_gemm / foley_op_ln_mod /
// foley_op_gather_rows.
//
//   melspec_db_kernel         ten-second windows of a 48 kHz waveform (the extractor's repeatpad, or a crop of a longer clip)
//                             -> centred reflect-padded STFT (n_fft 1024, periodic Hann, hop 480) -> power -> 64 Slaney mel
//                             triangles -> 10 log10(max(mel, 1e-10)):  [windows, 1001, 64] fp32.
//   spec_patches_kernel       BatchNorm2d (eval: one affine per mel bin) -> bicubic resize along time (a 4-tap table) ->
//                             reshape_mel2img's fold -> the im2col matrix of the 4x4 / stride 4 patch embedding.
//   window_attention_kernel   Swin's windowed attention for 64-token windows of head dim 32, straight from the fused q/k/v
//                             projection through a table of source rows (roll + partition), with the relative-position bias and
//                             the shift mask added to the scores; every query is written back to the row it came from.
#include "kernels.h"

namespace {

// ---- dB-mel spectrogram
constexpr int MS_NFFT = 1024, MS_HOP = 480, MS_PAD = 512, MS_WIN = 480000, MS_FRAMES = 1001;
constexpr int MS_BINS = 513, MS_BINP = 544, MS_MELS = 64;
constexpr int MS_SPAN = 31 * MS_HOP + MS_NFFT;                 // samples the 32 frames of a tile cover: 15 904
// sample i of the span lives at LDS word i + i / 480: frame j starts at word 481 j, so the 32 rows of an MFMA operand (one tap,
// 32 frames) fall into 32 distinct banks (481 = 33 mod 64, odd) instead of the two that a pitch of 480 words leaves
constexpr int MS_SPANW = MS_SPAN + MS_SPAN / MS_HOP + 4;       // 15 941 words
constexpr int MS_PWP = 552;                                    // pitch of a power row (rows 4 apart sit 32 banks apart)
constexpr int MS_LDS = (MS_SPANW + 3 + 32 * MS_PWP) / 4 * 16;  // 134 432 bytes

// One workgroup = 32 frames of one window (frame tile ft: frames 32 ft ..; the last tile of the 1001 holds 9).
//   1. the tile's span of the padded signal is staged once (the frames overlap: hop 480 < 1024).  Padded sample p of a window is
//      x[start + p % seg] for p < n_rep * seg and 0 beyond (seg = min(N, 480000), n_rep = 480000 / seg: the extractor's
//      repeatpad; seg = 480000, n_rep = 1 is a plain crop), and the STFT's reflect padding maps p = -1, -2, .. to 1, 2, ..
//      and p = 480000 + d to 479998 - d;
//   2. real DFT on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation), C / S [1024][544] = Hann * cos / sin built
//      on the host; the 1024 taps run as two halves with accumulators of their own (four independent MFMA chains);
//   3. mel[f][c] = sum_{k < mel_len[c]} power[f][mel_lo[c] + k] * mel_w[c][k] (every Slaney triangle covers contiguous bins);
//   4. 10 log10(max(mel, 1e-10)); a value at the floor is written as -100 exactly.
__global__ __launch_bounds__(256) void melspec_db_kernel(const float* __restrict__ x, int N, int n_win, const int* __restrict__ starts,
                                                         int seg, int n_rep, const float* __restrict__ basis,
                                                         const int* __restrict__ mel_lo, const int* __restrict__ mel_len,
                                                         const float* __restrict__ mel_w, int mel_wp, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float ms_lds[];
  float* sp = ms_lds;                               // [MS_SPANW]
  float* pw = ms_lds + (MS_SPANW + 3) / 4 * 4;      // [32][MS_PWP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ft = blockIdx.x, gw = blockIdx.y;       // gw = clip * n_win + window
  const int b = gw / n_win;
  const int start = min(max(starts[gw - b * n_win], 0), N - seg);      // caller-supplied table: kept inside the clip
  const float* xb = x + (long)b * N + start;
  const int f0 = ft * 32;
  const int nf = min(32, MS_FRAMES - f0);
  const int live = n_rep * seg;
  for (int i = tid; i < MS_SPAN; i += 256) {
    int p = f0 * MS_HOP + i - MS_PAD;
    p = p < 0 ? -p : (p >= MS_WIN ? 2 * (MS_WIN - 1) - p : p);
    p = min(max(p, 0), MS_WIN - 1);                 // frames past the 1001st (last tile): any in-range sample, never stored
    sp[i + i / MS_HOP] = p < live ? xb[p % seg] : 0.f;
  }
  __syncthreads();
  const int j = lane & 31, kh = lane >> 5;
  const float* a0 = sp + j * (MS_HOP + 1) + kh;
  for (int bt = w; bt < MS_BINP / 32; bt += 4) {
    f32x16 re0, im0, re1, im1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { re0[e] = 0.f; im0[e] = 0.f; re1[e] = 0.f; im1[e] = 0.f; }
    const float* bc = basis + (long)kh * MS_BINP + bt * 32 + j;
    const float* bs = bc + (long)MS_NFFT * MS_BINP;
    // taps k + kh and k + kh + 512; o0 / o1 = the skew (tap / 480) of either half, constant over [k_lo, k_hi)
    auto run = [&](int k_lo, int k_hi, int o0, int o1) {
#pragma unroll 4
      for (int k = k_lo; k < k_hi; k += 2) {
        const float av0 = a0[k + o0], av1 = a0[k + 512 + o1];
        re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bc[(long)k * MS_BINP], re0, 0, 0, 0);
        im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bs[(long)k * MS_BINP], im0, 0, 0, 0);
        re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bc[(long)(k + 512) * MS_BINP], re1, 0, 0, 0);
        im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bs[(long)(k + 512) * MS_BINP], im1, 0, 0, 0);
      }
    };
    run(0, 448, 0, 1);       // taps [0, 448) and [512, 960)
    run(448, 480, 0, 2);     // taps [448, 480) and [960, 992)
    run(480, 512, 1, 2);     // taps [480, 512) and [992, 1024)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = (e & 3) + 8 * (e >> 2) + 4 * kh;
      const float re = re0[e] + re1[e], im = im0[e] + im1[e];
      pw[row * MS_PWP + bt * 32 + j] = re * re + im * im;
    }
  }
  __syncthreads();
  for (int e = tid; e < nf * MS_MELS; e += 256) {
    const int f = e / MS_MELS, c = e - f * MS_MELS;
    const int lo = min(max(mel_lo[c], 0), MS_BINS);       // caller-supplied tables: clamped to the staged bins
    const int n = min(min(mel_len[c], mel_wp), MS_BINS - lo);
    const float* p = pw + f * MS_PWP + lo;
    const float* wc = mel_w + (long)c * mel_wp;
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc = __builtin_fmaf(p[k], wc[k], acc);
    out[((long)gw * MS_FRAMES + f0 + f) * MS_MELS + c] = acc > 1e-10f ? 10.0f * log10f(acc) : -100.0f;
  }
}

// ---- image layout
// One workgroup = the 4 resized time steps of patch column w in fold r of one spectrogram: values (f, kw) for every mel bin f,
// read along f (coalesced), transposed through LDS into the F / 4 patch rows (h = r F / 4 + f / 4; K index (f % 4) * 4 + kw).
template <typename OutT>
__global__ __launch_bounds__(256) void spec_patches_kernel(const float* __restrict__ spec, int T, int F, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const int* __restrict__ ridx,
                                                           const float* __restrict__ rw, int Tq, int ratio, OutT* __restrict__ out,
                                                           int Kp) {
  __shared__ float tile[256 * 4];
  const int tid = threadIdx.x;
  const int w = blockIdx.x, r = blockIdx.y, g = blockIdx.z;
  const float* sg = spec + (long)g * T * F;
  for (int e = tid; e < 4 * F; e += 256) {
    const int kw = e / F, f = e - kw * F;
    const int to = r * Tq + 4 * w + kw;
    const float sc = scale[f], sh = shift[f];
    float v;
    if (ridx) {
      v = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ti = min(max(ridx[to * 4 + t], 0), T - 1);
        v = __builtin_fmaf(rw[to * 4 + t], __builtin_fmaf(sg[(long)ti * F + f], sc, sh), v);
      }
    } else {
      v = to < T ? __builtin_fmaf(sg[(long)to * F + f], sc, sh) : 0.f;
    }
    tile[f * 4 + kw] = v;
  }
  __syncthreads();
  const int nh = F / 4, gh = ratio * nh, gwid = Tq / 4;
  for (int e = tid; e < nh * Kp; e += 256) {
    const int hl = e / Kp, c = e - hl * Kp;
    const float v = c < 16 ? tile[hl * 16 + c] : 0.f;
    out[(((long)g * gh + r * nh + hl) * gwid + w) * Kp + c] = Cvt<OutT>::to(v);
  }
}

// ---- windowed attention
constexpr int WA_TOK = 64, WA_HD = 32, WA_PAIRS = 4;     // tokens per window, head dim, (window, head) pairs per workgroup
constexpr int WA_VP = 72;                                // pitch (16-bit elements) of a transposed V row in LDS: 144 bytes
constexpr float WA_SCALE = 0.17677669529663687f;         // 1 / sqrt(32)

template <typename T> struct Pack4 {
  static __device__ __forceinline__ void store(T* p, const f32x4 v) {
    uint2 u;
    u.x = pack_h2<T>(v[0], v[1]);
    u.y = pack_h2<T>(v[2], v[3]);
    *(uint2*)p = u;
  }
};
template <> struct Pack4<float> {
  static __device__ __forceinline__ void store(float* p, const f32x4 v) { *(f32x4*)p = v; }
};

struct WinAttnArgs {
  const void* qkv;      // [rows, 3 * H * 32]
  int rows, H;
  const int* table;     // [n_win, 64] source row of every window token
  int n_win;
  const float* bias;    // [H, 64, 64]
  const float* mask;    // [n_mask, 64, 64] or null
  int n_mask;
  void* out;            // [rows, out_pitch]
  int out_pitch;
};

// One wave = one (window, head) pair.  Scores are S^T[key][query] (A = K rows, B = Q rows), so a lane owns ONE query column of
// each of the two 32-query tiles and 2 x 16 of its 64 keys: the row maximum / sum are 32 register operations and one exchange
// with lane ^ 32; all 64 keys are in registers at once, so the softmax is the plain two-pass one (maximum, then exponentials and
// their sum) in a fixed order.  A pair past the end (n_win * H not a multiple of 4) computes the last pair again and stores nothing.
//
// 16-bit form: v_mfma_f32_32x32x16, two k-steps per score tile.  A-row j carries key 32 kt + pi(j), pi chosen so that the 16
// scores of a lane are 16 CONSECUTIVE keys (32 kt + 16 kh + e): bias and mask rows are read as float4, and the probabilities
// form, in place, the key-contiguous B operand of the P V product (O^T[d][query], A = V^T from LDS, four k-steps per query tile).
template <typename T>
__global__ __launch_bounds__(256) void window_attention_kernel(const WinAttnArgs a) {
  __shared__ __attribute__((aligned(16))) T vt[WA_PAIRS][WA_HD * WA_VP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 31, kh = lane >> 5;
  const int n_pairs = a.n_win * a.H;
  const int pr_raw = blockIdx.x * WA_PAIRS + wv;
  const bool live = pr_raw < n_pairs;
  const int pr = live ? pr_raw : n_pairs - 1;
  const int g = pr / a.H, h = pr - g * a.H;
  const int ld = 3 * a.H * WA_HD;
  const int* tab = a.table + (long)g * WA_TOK;
  const T* base = (const T*)a.qkv;
  auto row_of = [&](int t) { return min(max(tab[t], 0), a.rows - 1); };   // caller-supplied table: loads stay inside qkv

  // V of the pair, transposed into LDS: chunk c = (key, 8 head dims), 256 chunks of 16 bytes
  T* vw = vt[wv];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i, key = c >> 2, dc = c & 3;
    const bf16x8 v = *(const bf16x8*)(base + (long)row_of(key) * ld + 2 * a.H * WA_HD + h * WA_HD + 8 * dc);
    const u32x4 u = __builtin_bit_cast(u32x4, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned short bits = (unsigned short)(u[e >> 1] >> (16 * (e & 1)));
      vw[(8 * dc + e) * WA_VP + key] = __builtin_bit_cast(T, bits);
    }
  }
  const int pi = 16 * ((j >> 2) & 1) + (j & 3) + 4 * (j >> 3);
  bf16x8 qf[2][2], kf[2][2];
  int qrow[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    qrow[t] = tab[32 * t + j];
    const T* qp = base + (long)min(max(qrow[t], 0), a.rows - 1) * ld + h * WA_HD + 8 * kh;
    const T* kp = base + (long)row_of(32 * t + pi) * ld + a.H * WA_HD + h * WA_HD + 8 * kh;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qf[t][s] = *(const bf16x8*)(qp + 16 * s);
      kf[t][s] = *(const bf16x8*)(kp + 16 * s);
    }
  }
  const float* bias = a.bias + (long)h * WA_TOK * WA_TOK;
  const float* mask = a.mask ? a.mask + (long)(g % a.n_mask) * WA_TOK * WA_TOK : nullptr;
  __syncthreads();
  f32x16 o[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    f32x16 s[2];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[kt][e] = 0.f;
      s[kt] = mfma16<T>(kf[kt][0], qf[qt][0], s[kt]);
      s[kt] = mfma16<T>(kf[kt][1], qf[qt][1], s[kt]);
      const long off = (long)(32 * qt + j) * WA_TOK + 32 * kt + 16 * kh;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 bv = *(const f32x4*)(bias + off + 4 * c);
        f32x4 mv = {0.f, 0.f, 0.f, 0.f};
        if (mask) mv = *(const f32x4*)(mask + off + 4 * c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float v = s[kt][4 * c + u] * WA_SCALE + bv[u] + mv[u];
          s[kt][4 * c + u] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = xhalf_max(mx);
    float ps = 0.f;
    bf16x8 pb[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float pv = expf(s[kt][e] - mx);
        ps += pv;
        pb[kt][e >> 3][e & 7] = to_carrier<T>(pv);
      }
    ps = xhalf_sum(ps);
#pragma unroll
    for (int e = 0; e < 16; ++e) o[qt][e] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16x8 vf = *(const bf16x8*)(vw + j * WA_VP + 32 * kt + 16 * kh + 8 * u);
        o[qt] = mfma16<T>(vf, pb[kt][u], o[qt]);
      }
    const float inv = 1.0f / ps;
    if (live && (unsigned)qrow[qt] < (unsigned)a.rows) {
      T* dst = (T*)a.out + (long)qrow[qt] * a.out_pitch + h * WA_HD;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 v = {o[qt][g4 * 4] * inv, o[qt][g4 * 4 + 1] * inv, o[qt][g4 * 4 + 2] * inv, o[qt][g4 * 4 + 3] * inv};
        Pack4<T>::store(dst + 8 * g4 + 4 * kh, v);
      }
    }
  }
}

// fp32 form (parity mode): v_mfma_f32_32x32x2_f32 as attention.hip's fp32 kernel.  Lane (j, kh) holds half kh of the 32 head dims
// of its query / key rows; s[e] is key 32 kt + r(e), r(e) = (e & 3) + 8 (e >> 2) + 4 kh, so bias / mask come as four float4 per
// tile, and the P V product takes V rows in that same order straight from global memory (32 lanes read one 128-byte row).
__global__ __launch_bounds__(256) void window_attention_f32_kernel(const WinAttnArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 31, kh = lane >> 5;
  const int n_pairs = a.n_win * a.H;
  const int pr_raw = blockIdx.x * WA_PAIRS + wv;
  const bool live = pr_raw < n_pairs;
  const int pr = live ? pr_raw : n_pairs - 1;
  const int g = pr / a.H, h = pr - g * a.H;
  const int ld = 3 * a.H * WA_HD;
  const int* tab = a.table + (long)g * WA_TOK;
  const float* base = (const float*)a.qkv;
  auto row_of = [&](int t) { return min(max(tab[t], 0), a.rows - 1); };
  constexpr int HH = WA_HD / 2;
  float qr[2][HH], kr[2][HH];
  int qrow[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    qrow[t] = tab[32 * t + j];
    const f32x4* qp = (const f32x4*)(base + (long)min(max(qrow[t], 0), a.rows - 1) * ld + h * WA_HD + kh * HH);
    const f32x4* kp = (const f32x4*)(base + (long)row_of(32 * t + j) * ld + a.H * WA_HD + h * WA_HD + kh * HH);
#pragma unroll
    for (int c = 0; c < HH / 4; ++c) {
      const f32x4 qv = qp[c], kv = kp[c];
#pragma unroll
      for (int u = 0; u < 4; ++u) { qr[t][4 * c + u] = qv[u]; kr[t][4 * c + u] = kv[u]; }
    }
  }
  const float* bias = a.bias + (long)h * WA_TOK * WA_TOK;
  const float* mask = a.mask ? a.mask + (long)(g % a.n_mask) * WA_TOK * WA_TOK : nullptr;
  const float* vbase = base + 2 * a.H * WA_HD + h * WA_HD + j;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    f32x16 s[2];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[kt][e] = 0.f;
#pragma unroll
      for (int c = 0; c < HH; ++c) s[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[kt][c], qr[qt][c], s[kt], 0, 0, 0);
      const long off = (long)(32 * qt + j) * WA_TOK + 32 * kt + 4 * kh;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 bv = *(const f32x4*)(bias + off + 8 * c);
        f32x4 mv = {0.f, 0.f, 0.f, 0.f};
        if (mask) mv = *(const f32x4*)(mask + off + 8 * c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float v = s[kt][4 * c + u] * WA_SCALE + bv[u] + mv[u];
          s[kt][4 * c + u] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = xhalf_max(mx);
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        s[kt][e] = expf(s[kt][e] - mx);
        ps += s[kt][e];
      }
    ps = xhalf_sum(ps);
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int key = 32 * kt + (t & 3) + 8 * (t >> 2) + 4 * kh;
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(vbase[(long)row_of(key) * ld], s[kt][t], o, 0, 0, 0);
      }
    const float inv = 1.0f / ps;
    if (live && (unsigned)qrow[qt] < (unsigned)a.rows) {
      float* dst = (float*)a.out + (long)qrow[qt] * a.out_pitch + h * WA_HD;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 v = {o[g4 * 4] * inv, o[g4 * 4 + 1] * inv, o[g4 * 4 + 2] * inv, o[g4 * 4 + 3] * inv};
        *(f32x4*)(dst + 8 * g4 + 4 * kh) = v;
      }
    }
  }
}

}  // namespace

int launch_melspec_db(const float* x, int B, int N, const int* starts, int n_win, const float* basis, const int* mel_lo,
                      const int* mel_len, const float* mel_w, int mel_wp, float* out, hipStream_t st) {
  if (B < 1 || n_win < 1 || N < MS_NFFT) return foley_set_err("melspec_db: needs at least one 1024-sample frame", __FILE__, __LINE__);
  if (mel_wp < 1) return foley_set_err("melspec_db: bad mel table pitch", __FILE__, __LINE__);
  if ((long)B * n_win > 65535) return foley_set_err("melspec_db: more than 65535 windows in one call", __FILE__, __LINE__);
  const int seg = N < MS_WIN ? N : MS_WIN;
  if (n_win > 1 && N < MS_WIN) return foley_set_err("melspec_db: a clip below ten seconds has one window", __FILE__, __LINE__);
  static std::atomic<unsigned long long> raised{0};
  const hipError_t e = foley_raise_lds((const void*)melspec_db_kernel, MS_LDS, raised);
  if (e != hipSuccess) return foley_set_err(hipGetErrorString(e), __FILE__, __LINE__);
  FOLEY_LAUNCH(melspec_db_kernel, dim3((MS_FRAMES + 31) / 32, B * n_win), dim3(256), MS_LDS, st, x, N, n_win, starts, seg,
               MS_WIN / seg, basis, mel_lo, mel_len, mel_w, mel_wp, out);
  return 0;
}

int launch_spec_patches(const float* spec, int G, int T, int F, const float* scale, const float* shift, const int* ridx,
                        const float* rw, int Tq, int ratio, void* out, int out_dtype, int Kp, hipStream_t st) {
  if (G < 1 || T < 1 || F < 4 || F > 256 || F % 4 || Tq < 4 || Tq % 4 || ratio < 1 || ratio > 65535 || G > 65535)
    return foley_set_err("spec_patches: needs F a multiple of 4 up to 256, Tq a multiple of 4, ratio >= 1", __FILE__, __LINE__);
  if (Kp < 16) return foley_set_err("spec_patches: the patch matrix needs at least the 16 columns of a 4x4 patch", __FILE__, __LINE__);
  if (!ridx && (long)ratio * Tq != T) return foley_set_err("spec_patches: without a resize table T must equal ratio * Tq", __FILE__, __LINE__);
  const dim3 grid(Tq / 4, ratio, G);
  if (out_dtype == FOLEY_F32)
    FOLEY_LAUNCH(spec_patches_kernel<float>, grid, dim3(256), 0, st, spec, T, F, scale, shift, ridx, rw, Tq, ratio, (float*)out, Kp);
  else if (out_dtype == FOLEY_BF16)
    FOLEY_LAUNCH(spec_patches_kernel<bf16_t>, grid, dim3(256), 0, st, spec, T, F, scale, shift, ridx, rw, Tq, ratio, (bf16_t*)out, Kp);
  else if (out_dtype == FOLEY_F16)
    FOLEY_LAUNCH(spec_patches_kernel<f16_t>, grid, dim3(256), 0, st, spec, T, F, scale, shift, ridx, rw, Tq, ratio, (f16_t*)out, Kp);
  else return foley_set_err("spec_patches: bad output dtype", __FILE__, __LINE__);
  return 0;
}

int launch_window_attention(const void* qkv, int dtype, int rows, int H, const int* table, int n_win, const float* bias,
                            const float* mask, int n_mask, void* out, int out_pitch, hipStream_t st) {
  if (rows < 1 || H < 1 || n_win < 1 || out_pitch < H * WA_HD || (mask && n_mask < 1))
    return foley_set_err("window_attention: empty problem or an output pitch below H * 32", __FILE__, __LINE__);
  if ((((uintptr_t)qkv | (uintptr_t)bias | (uintptr_t)mask | (uintptr_t)out) & 15) || out_pitch % 8)
    return foley_set_err("window_attention: operands must be 16-byte aligned, the output pitch a multiple of 8", __FILE__, __LINE__);
  const WinAttnArgs a{qkv, rows, H, table, n_win, bias, mask, mask ? n_mask : 1, out, out_pitch};
  const dim3 grid((unsigned)(((long)n_win * H + WA_PAIRS - 1) / WA_PAIRS));
  if (dtype == FOLEY_F32) FOLEY_LAUNCH(window_attention_f32_kernel, grid, dim3(256), 0, st, a);
  else if (dtype == FOLEY_BF16) FOLEY_LAUNCH(window_attention_kernel<bf16_t>, grid, dim3(256), 0, st, a);
  else if (dtype == FOLEY_F16) FOLEY_LAUNCH(window_attention_kernel<f16_t>, grid, dim3(256), 0, st, a);
  else return foley_set_err("window_attention: bad dtype", __FILE__, __LINE__);
  return 0;
}

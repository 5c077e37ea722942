// Audio front end of the sync scorer (host/sync_score.py): the rational windowed-sinc resampler and the fused log-mel
// spectrogram that feeds the Synchformer audio branch.
//
//   resample_sinc_kernel   torchaudio.functional.resample's polyphase convolution (taps built on the host, host/sync_score.py
//                          ::sinc_resample_taps): out[b, j*new + p] = sum_t x[j*orig + t - width] * taps[p][t], zero outside x.
//   logmel_kernel          encode_audio_with_sync (reference models/synchformer/synchformer.py:294-317): 0.64 s segments at a
//                          0.32 s stride -> torch.stft(n_fft 1024, hop 160, win 400, center, reflect) -> |X|^2 -> 128 HTK mel
//                          triangles -> log(x + 1e-6) -> time pad 65 -> 66 with 0 -> AST normalisation, written as the im2col
//                          matrix of the AST patch embedding (Conv2d(1, 768, 16, stride 10) over [128 F, 66 T]).
#include "kernels.h"

namespace {

__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* __restrict__ x, int N, int orig, int nnew,
                                                            const float* __restrict__ taps, int ntaps, int width,
                                                            float* __restrict__ out, int Nout) {
  const int b = blockIdx.y;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= Nout) return;
  const int j = o / nnew, p = o - j * nnew;
  const float* xb = x + (long)b * N;
  const float* k = taps + (long)p * ntaps;
  const int i0 = j * orig - width;
  float acc = 0.f;
  for (int t = 0; t < ntaps; ++t) {
    const int i = i0 + t;
    if (i >= 0 && i < N) acc = __builtin_fmaf(xb[i], k[t], acc);
  }
  out[(long)b * Nout + o] = acc;
}

// ---- log-mel
constexpr int LM_SEG = 10240, LM_STEP = 5120, LM_HOP = 160, LM_WIN = 400, LM_OFF = 200;   // window taps m read sample f*160 + m - 200
constexpr int LM_FRAMES = 65, LM_T = 66, LM_BINS = 513, LM_BINP = 544, LM_MELS = 128;
constexpr int LM_FP = LM_WIN + 1;                // LDS pitch of a staged frame (odd: the 32 frames of an MFMA operand hit distinct banks)
constexpr int LM_LDS = (32 * LM_FP + 32 * LM_BINP) * 4;   // 51 328 + 69 632 bytes

// One workgroup = 32 frames of one segment (frame tile ft: frames 32*ft ..; the third tile holds frame 64 only).
//   1. the tile's frames are staged in LDS (reflect padding at the segment's edges, as torch.stft pads the segment), 400
//      samples each - the taps outside the 400-sample Hann window (offset 312 of the 1024) are zero;
//   2. the real DFT: power[f][k] = (sum_m s[f][m] C[m][k])^2 + (sum_m s[f][m] S[m][k])^2 on v_mfma_f32_32x32x2_f32 (exact
//      fp32 products, fp32 accumulation); C / S [400][544] = window * cos / sin of the 1024-point transform, built on the host;
//   3. mel: mel[f][c] = sum_{k < mel_len[c]} power[f][mel_lo[c] + k] * mel_w[c][k] (every HTK triangle covers contiguous bins);
//   4. v = (log(mel + 1e-6) + 4.2677393) / (2 * 4.5689974), scattered into every 16x16 patch (stride 10) that contains (c, f).
template <typename OutT>
__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ w16, int N16, int S, const float* __restrict__ basis,
                                                     const int* __restrict__ mel_lo, const int* __restrict__ mel_len,
                                                     const float* __restrict__ mel_w, int mel_wp, OutT* __restrict__ patches,
                                                     float* __restrict__ mel_out) {
  extern __shared__ __attribute__((aligned(16))) float lm_lds[];
  float* fr = lm_lds;                  // [32][LM_FP]
  float* pw = lm_lds + 32 * LM_FP;     // [32][LM_BINP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ft = blockIdx.x, seg = blockIdx.y;          // seg = b * S + s
  const int b = seg / S, s = seg - b * S;
  const float* x = w16 + (long)b * N16 + (long)s * LM_STEP;
  const int f0 = ft * 32;
  const int nf = min(32, LM_FRAMES - f0);
  for (int e = tid; e < 32 * LM_WIN; e += 256) {
    const int f = e / LM_WIN, m = e - f * LM_WIN;
    float v = 0.f;
    if (f < nf) {
      int i = (f0 + f) * LM_HOP + m - LM_OFF;
      i = i < 0 ? -i : (i >= LM_SEG ? 2 * (LM_SEG - 1) - i : i);    // reflect (no edge repeat)
      v = x[i];
    }
    fr[f * LM_FP + m] = v;
  }
  __syncthreads();
  // DFT: 17 bin tiles of 32, wave w takes tiles w, w+4, ...; D[frame i][bin j], A = frames (row i = lane&31), B = basis
  const int j = lane & 31, kh = lane >> 5;
  for (int bt = w; bt < LM_BINP / 32; bt += 4) {
    f32x16 re, im;
#pragma unroll
    for (int e = 0; e < 16; ++e) { re[e] = 0.f; im[e] = 0.f; }
    const float* a = fr + j * LM_FP + kh;
    const float* bc = basis + (long)kh * LM_BINP + bt * 32 + j;
    const float* bs = bc + (long)LM_WIN * LM_BINP;
#pragma unroll 4
    for (int k = 0; k < LM_WIN; k += 2) {
      const float av = a[k];
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bc[(long)k * LM_BINP], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bs[(long)k * LM_BINP], im, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = (e & 3) + 8 * (e >> 2) + 4 * kh;
      pw[row * LM_BINP + bt * 32 + j] = re[e] * re[e] + im[e] * im[e];
    }
  }
  __syncthreads();
  const float lo_norm = 4.2677393f, inv2std = 1.0f / (2.0f * 4.5689974f);
  const long pbase = (long)seg * 72;
  // the patch (fi, ti) holds (c, t) at column (c - 10 fi) * 16 + (t - 10 ti) for 0 <= c - 10 fi < 16, 0 <= t - 10 ti < 16
  auto emit = [&](int c, int t, float v) {
    if (mel_out) mel_out[((long)seg * LM_MELS + c) * LM_T + t] = v;
    const int fa = c / 10, ta = t / 10;
#pragma unroll
    for (int df = 0; df < 2; ++df) {
      const int fi = fa - df, kf = c - 10 * fi;
      if (fi < 0 || fi >= 12 || kf >= 16) continue;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int ti = ta - dt, kt = t - 10 * ti;
        if (ti < 0 || ti >= 6 || kt >= 16) continue;
        patches[(pbase + fi * 6 + ti) * 256 + kf * 16 + kt] = Cvt<OutT>::to(v);
      }
    }
  };
  for (int e = tid; e < nf * LM_MELS; e += 256) {
    const int f = e / LM_MELS, c = e - f * LM_MELS;
    const int lo = min(max(mel_lo[c], 0), LM_BINS);       // caller-supplied tables: clamped to the staged bins
    const int n = min(min(mel_len[c], mel_wp), LM_BINS - lo);
    const float* p = pw + f * LM_BINP + lo;
    const float* wc = mel_w + (long)c * mel_wp;
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc = __builtin_fmaf(p[k], wc[k], acc);
    emit(c, f0 + f, (logf(acc + 1e-6f) + lo_norm) * inv2std);
  }
  if (f0 + nf == LM_FRAMES)       // pad_or_truncate: the 66th column is 0 after the log
    for (int c = tid; c < LM_MELS; c += 256) emit(c, LM_FRAMES, lo_norm * inv2std);
}

}  // namespace

int launch_resample_sinc(const float* x, int B, int N, int orig, int nnew, const float* taps, int ntaps, int width, float* out,
                         int Nout, hipStream_t st) {
  if (B < 1 || N < 1 || orig < 1 || nnew < 1 || ntaps < 1 || width < 0 || Nout < 1)
    return foley_set_err("resample_sinc: empty problem", __FILE__, __LINE__);
  if ((long)Nout > ((long)N * nnew + orig - 1) / orig)       // ceil(N * new / orig): torchaudio's length, the last output x can reach
    return foley_set_err("resample_sinc: Nout exceeds the resampled length", __FILE__, __LINE__);
  FOLEY_LAUNCH(resample_sinc_kernel, dim3((Nout + 255) / 256, B), dim3(256), 0, st, x, N, orig, nnew, taps, ntaps, width, out, Nout);
  return 0;
}

int launch_logmel(const float* w16, int B, int N16, const float* basis, const int* mel_lo, const int* mel_len, const float* mel_w,
                  int mel_wp, void* patches, int out_dtype, float* mel_out, hipStream_t st) {
  if (B < 1 || N16 < LM_SEG) return foley_set_err("logmel: needs at least one 10240-sample segment", __FILE__, __LINE__);
  if (mel_wp < 1) return foley_set_err("logmel: bad mel table pitch", __FILE__, __LINE__);
  const int S = (N16 - LM_SEG) / LM_STEP + 1;
  const dim3 grid((LM_FRAMES + 31) / 32, B * S);
  hipError_t e = hipSuccess;
#define FOLEY_LOGMEL(O)                                                                                                       \
  do {                                                                                                                        \
    static std::atomic<unsigned long long> raised{0};                                                                         \
    e = foley_raise_lds((const void*)logmel_kernel<O>, LM_LDS, raised);                                                       \
    if (e == hipSuccess)                                                                                                      \
      FOLEY_LAUNCH(logmel_kernel<O>, grid, dim3(256), LM_LDS, st, w16, N16, S, basis, mel_lo, mel_len, mel_w, mel_wp,         \
                   (O*)patches, mel_out);                                                                                     \
  } while (0)
  if (out_dtype == FOLEY_F32) FOLEY_LOGMEL(float);
  else if (out_dtype == FOLEY_BF16) FOLEY_LOGMEL(bf16_t);
  else if (out_dtype == FOLEY_F16) FOLEY_LOGMEL(f16_t);
  else return foley_set_err("logmel: bad output dtype", __FILE__, __LINE__);
#undef FOLEY_LOGMEL
  if (e != hipSuccess) return foley_set_err(hipGetErrorString(e), __FILE__, __LINE__);
  return 0;
}

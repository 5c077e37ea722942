// Low-rank adapters merged into the packed weights, in place:
//
//   stored'[o, c] = rnd_store( f32(pristine[o, c]) + sum_j s_j * sum_q up_j[o, q] * down_j[q, c] )      c over the flattened (I, k)
//
// for one reference state-dict key per call (foley_lora_merge).  The destination is whatever tensor the context has registered
// under the key's packed name - the host packers' arena (foley_set_tensor) or the ctx-owned one (foley_weights_begin) - at the
// position weight_map.h gives the key: the same size / stride / offset tuples the loader stores through, walked backwards here
// (packed row -> checkpoint row of `up`, packed column -> flattened (I, k) column of `down`).  One pass over the slot: read the
// pristine value, add the rank-R product, round with the loader's own rounding, store; no fp32 delta tensor exists in HBM.
// `pristine` is a library-owned copy of the packed tensor taken the first time an adapter touches it, so every merge starts from
// the loaded values with one rounding and foley_lora_begin / foley_lora_clear give the loaded bytes back.  Addresses never
// change: a captured loop iteration stays valid, and an fp8 arena stays fp8.
//
// Summation order (fixed, so a merge repeats bit for bit): adapters in list order, rank chunks of 16 ascending, q ascending
// within a chunk, one fp32 FMA chain per element starting from 0 with s_j folded into the `up` operand; then one addition to
// the widened pristine value and one rounding.
#include "../../include/foley_hip.h"
#include "kernels.h"
#include "weight_map.h"

#include <cmath>
#include <map>
#include <set>
#include <string>
#include <vector>

// internal hooks of foley_rt.hip (not part of the C ABI)
void** foley_ctx_lora_slot(foley_ctx* c);
void foley_ctx_set_lora_free(foley_ctx* c, void (*fn)(void*));
bool foley_ctx_tensor(foley_ctx* c, const char* name, void** p, int* dtype, std::vector<int64_t>* shape);
void foley_ctx_weights_changed(foley_ctx* c);
const foley_config* foley_ctx_config(foley_ctx* c);
int foley_ctx_device(foley_ctx* c);

namespace {

#define L_FAIL(code, msg) (foley_set_err(msg, __FILE__, __LINE__), (code))
#define L_HIP(expr)                                              \
  do {                                                           \
    hipError_t _e = (expr);                                      \
    if (_e != hipSuccess) {                                      \
      foley_set_err(hipGetErrorString(_e), __FILE__, __LINE__);  \
      return FOLEY_ERR_HIP;                                      \
    }                                                            \
  } while (0)

constexpr int MAX_ADAPTERS = 8, MAX_RANK = 256;
constexpr int TR = 64;    // packed rows of a tile: 16 thread rows x 4
constexpr int RPT = 4;    // rows per thread
constexpr int RC = 16;    // rank chunk staged in LDS

struct MergeOp {
  const void* down;   // [rank, I*k] in the checkpoint's own (I, k) order
  const void* up;     // [O, rank]
  int dt, rank;
  float scale;
};
struct MergeDesc {
  const void* pristine;   // copy of the packed tensor as loaded
  void* out;              // the packed tensor
  int dt;                 // its dtype
  int n;
  MergeOp op[MAX_ADAPTERS];
  int O, Kp;              // targeted rows; packed row length I*k
  int row_dims;           // rows: t in [0, O) enumerates the map's row index space in packed order
  int rsize[3], r_in[3], r_out[3], out_row0;   // -> checkpoint row sum idx*r_in, packed row out_row0 + sum idx*r_out
  int csize1, c_in0, c_in1;                    // packed column pc -> flattened (I, k) column (pc / csize1)*c_in0 + (pc % csize1)*c_in1
  int vec_ok;             // rows are whole 16-byte pieces at 16-byte aligned addresses
};

template <int ES> __device__ __forceinline__ uint32_t piece_get(const uint4& w, int v) {   // v is a compile-time constant after unrolling
  const uint32_t a[4] = {w.x, w.y, w.z, w.w};
  if constexpr (ES == 4) return a[v];
  else if constexpr (ES == 2) return (a[v >> 1] >> ((v & 1) * 16)) & 0xffffu;
  else return (a[v >> 2] >> ((v & 3) * 8)) & 0xffu;
}

// One thread's piece of one packed row: pristine + delta, rounded with the loader's rounding, as one 16-byte store where the rows
// are whole aligned pieces and element by element otherwise (the embedders' odd widths).
template <int ES, int DT>
__device__ __forceinline__ void merge_row(const MergeDesc& d, const float (&delta)[16 / ES], int orow, int col) {
  constexpr int VEC = 16 / ES;
  if (orow < 0) return;
  const size_t at = (size_t)orow * d.Kp + col;   // element offset inside the packed tensor
  if (d.vec_ok) {                                // col + VEC <= Kp: Kp is a multiple of VEC
    const uint4 w = *(const uint4*)((const char*)d.pristine + at * ES);
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const uint32_t raw = f32_to_bits(bits_to_f32(piece_get<ES>(w, v), DT) + delta[v], DT);
      if constexpr (ES == 4) o[v] = raw;
      else if constexpr (ES == 2) o[v >> 1] |= (raw & 0xffffu) << ((v & 1) * 16);
      else o[v >> 2] |= (raw & 0xffu) << ((v & 3) * 8);
    }
    *(uint4*)((char*)d.out + at * ES) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (col + v < d.Kp) store_from_f32(d.out, (long)(at + v), DT, load_as_f32(d.pristine, (long)(at + v), DT) + delta[v]);
  }
}

// One tile of TR packed rows x 16*VEC packed columns per block of 256 threads; thread (ty, tx) owns rows ty*4 .. ty*4+3 and the
// 16-byte piece tx of each (VEC = 16 / ES elements).  Per rank chunk the tile's `up` rows (times s_j) and `down` columns are
// gathered into LDS through the inverse of the key's stride map, then every thread runs its FMA chain from LDS.
template <int ES>
__global__ __launch_bounds__(256) void lora_merge_kernel(const MergeDesc d) {
  constexpr int VEC = 16 / ES, TC = 16 * VEC;
  __shared__ float up_s[TR * RC];
  __shared__ float down_s[RC * TC];
  __shared__ int in_row_s[TR], out_row_s[TR], in_col_s[TC];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.y * TR, col0 = blockIdx.x * TC;
  if (tid < TR) {   // row t of the map's row index space, last dimension fastest (= ascending packed rows within a group)
    int t = row0 + tid, ir = -1, orow = -1;
    if (t < d.O) {
      ir = 0;
      orow = d.out_row0;
      for (int k = d.row_dims - 1; k >= 0; --k) {
        const int i = t % d.rsize[k];
        t /= d.rsize[k];
        ir += i * d.r_in[k];
        orow += i * d.r_out[k];
      }
    }
    in_row_s[tid] = ir;
    out_row_s[tid] = orow;
  }
  for (int e = tid; e < TC; e += 256) {
    const int pc = col0 + e;
    in_col_s[e] = pc < d.Kp ? (pc / d.csize1) * d.c_in0 + (pc % d.csize1) * d.c_in1 : -1;
  }
  __syncthreads();

  float acc[RPT][VEC];
#pragma unroll
  for (int r = 0; r < RPT; ++r)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[r][v] = 0.f;

  for (int j = 0; j < d.n; ++j) {
    const MergeOp op = d.op[j];
    for (int q0 = 0; q0 < op.rank; q0 += RC) {
      const int rc = min(RC, op.rank - q0);
      for (int e = tid; e < TR * RC; e += 256) {
        const int row = e / RC, q = e % RC, ir = in_row_s[row];
        up_s[e] = (ir >= 0 && q < rc) ? op.scale * load_as_f32(op.up, (long)ir * op.rank + q0 + q, op.dt) : 0.f;
      }
      for (int e = tid; e < RC * TC; e += 256) {
        const int q = e / TC, ic = in_col_s[e % TC];
        down_s[e] = (ic >= 0 && q < rc) ? load_as_f32(op.down, (long)(q0 + q) * d.Kp + ic, op.dt) : 0.f;
      }
      __syncthreads();
      for (int q = 0; q < rc; ++q) {
        float dn[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) dn[v] = down_s[q * TC + tx * VEC + v];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          const float u = up_s[(ty * RPT + r) * RC + q];
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[r][v] = fmaf(u, dn[v], acc[r][v]);
        }
      }
      __syncthreads();
    }
  }

  const int col = col0 + tx * VEC;
  if (col >= d.Kp) return;
  static_assert(RPT == 4, "the epilogue names its four rows");
  // the tensor's dtype is uniform over the launch: branch once, so that every conversion below is straight-line code
  constexpr int DT_A = ES == 4 ? (int)FOLEY_F32 : ES == 2 ? (int)FOLEY_BF16 : (int)FOLEY_F8E4M3;
  if (d.dt == DT_A) {
    merge_row<ES, DT_A>(d, acc[0], out_row_s[ty * RPT + 0], col);
    merge_row<ES, DT_A>(d, acc[1], out_row_s[ty * RPT + 1], col);
    merge_row<ES, DT_A>(d, acc[2], out_row_s[ty * RPT + 2], col);
    merge_row<ES, DT_A>(d, acc[3], out_row_s[ty * RPT + 3], col);
  } else if constexpr (ES != 4) {
    constexpr int DT_B = ES == 2 ? (int)DT_F16 : (int)FOLEY_F8E5M2;
    merge_row<ES, DT_B>(d, acc[0], out_row_s[ty * RPT + 0], col);
    merge_row<ES, DT_B>(d, acc[1], out_row_s[ty * RPT + 1], col);
    merge_row<ES, DT_B>(d, acc[2], out_row_s[ty * RPT + 2], col);
    merge_row<ES, DT_B>(d, acc[3], out_row_s[ty * RPT + 3], col);
  }
}

// ---- host state: pristine copies of the touched packed tensors
struct Backup {
  void* dst = nullptr;    // the registered tensor it was taken from
  void* copy = nullptr;
  size_t bytes = 0;
};
struct LoraState {
  int device = 0;
  std::map<std::string, Backup> backups;   // by packed name
  std::set<std::string> merged;            // reference keys merged since foley_lora_begin
  bool open = false;
};

void lora_free(void* p) {
  LoraState* s = (LoraState*)p;
  if (!s) return;
  hipSetDevice(s->device);
  for (auto& kv : s->backups) hipFree(kv.second.copy);
  delete s;
}

LoraState* state_of(foley_ctx* c, bool create) {
  void** slot = foley_ctx_lora_slot(c);
  if (!*slot && create) {
    LoraState* s = new LoraState();
    s->device = foley_ctx_device(c);
    *slot = s;
    foley_ctx_set_lora_free(c, lora_free);
  }
  return (LoraState*)*slot;
}

// every touched tensor back to its loaded bytes; a copy whose tensor has been registered elsewhere since is dropped unused
int restore_all(foley_ctx* c, LoraState& s, hipStream_t st) {
  for (auto it = s.backups.begin(); it != s.backups.end();) {
    void* p = nullptr;
    int dt = 0;
    std::vector<int64_t> shape;
    if (foley_ctx_tensor(c, it->first.c_str(), &p, &dt, &shape) && p == it->second.dst) {
      L_HIP(hipMemcpyAsync(it->second.dst, it->second.copy, it->second.bytes, hipMemcpyDeviceToDevice, st));
      ++it;
    } else {
      L_HIP(hipStreamSynchronize(st));
      hipFree(it->second.copy);
      it = s.backups.erase(it);
    }
  }
  s.merged.clear();
  return 0;
}

bool trimmed_is(const int64_t* shape, int ndim, std::initializer_list<int64_t> want) {   // trailing singleton dims are ignored
  std::vector<int64_t> a(shape, shape + ndim), b(want);
  while (a.size() > 1 && a.back() == 1) a.pop_back();
  while (b.size() > 1 && b.back() == 1) b.pop_back();
  return a == b;
}

int refuse(const std::string& key, const std::string& why) {
  return L_FAIL(FOLEY_ERR_INVALID, ("lora: '" + key + "': " + why).c_str());
}

}  // namespace

// the ctx-owned arena is about to be replaced (foley_weights_begin): its pristine copies describe memory that no longer exists
void foley_lora_forget(foley_ctx* c) {
  void** slot = foley_ctx_lora_slot(c);
  if (*slot) lora_free(*slot);
  *slot = nullptr;
}

// --------------------------------------------------------------------------- C ABI
extern "C" int foley_lora_begin(foley_ctx* c, void* stream) {
  if (!c) return L_FAIL(FOLEY_ERR_INVALID, "bad argument");
  LoraState* s = state_of(c, true);
  L_HIP(hipSetDevice(s->device));
  const int rc = restore_all(c, *s, (hipStream_t)stream);
  if (rc != 0) return rc;
  s->open = true;
  return 0;
}

extern "C" int foley_lora_merge(foley_ctx* c, const char* ref_key, int n, const foley_lora_pair* pairs, void* stream) {
  if (!c || !ref_key) return L_FAIL(FOLEY_ERR_INVALID, "bad argument");
  LoraState* s = state_of(c, false);
  if (!s || !s->open) return L_FAIL(FOLEY_ERR_STATE, "foley_lora_begin has not been called");
  const std::string key(ref_key);
  const foley_config& f = *foley_ctx_config(c);
  // ---- everything that can be refused is refused before the device is touched
  KeyMap m;
  const int kind = dit_key_map(f, 0, key, &m);
  if (kind != KEY_MAPPED) {
    for (const char* p : {"decoder.", "encoder.", "post_quant_conv.", "quant_conv.", "quantizer."})
      if (key.compare(0, strlen(p), p) == 0) return refuse(key, "not targetable: the DAC takes no adapters");
    return refuse(key, kind == KEY_BAD_BLOCK ? "unknown key (block index out of range)" : "unknown key (no such tensor in the DiT)");
  }
  if (!m.matrix) return refuse(key, "not targetable: only weight matrices take adapters (no biases, norm gains or feature rows)");
  if (!m.shape_ok) return refuse(key, "the configuration cannot hold this tensor");
  if (n < 1 || !pairs) return refuse(key, "no adapters given");
  if (n > MAX_ADAPTERS) return refuse(key, "more than 8 adapters on one key");
  if (s->merged.count(key)) return refuse(key, "merged twice between foley_lora_begin and foley_lora_end (pass all adapters of a key in one call)");
  const int64_t Kp = m.I * m.k;
  MergeDesc d{};
  for (int j = 0; j < n; ++j) {
    const foley_lora_pair& p = pairs[j];
    const std::string aj = "adapter " + std::to_string(j) + ": ";
    if (!(p.dtype == FOLEY_DT_F32 || p.dtype == FOLEY_DT_BF16 || p.dtype == FOLEY_DT_F16))
      return refuse(key, aj + "operand dtype must be f32, bf16 or f16");
    if (p.rank < 1 || p.rank > MAX_RANK) return refuse(key, aj + "rank must be in [1, 256], got " + std::to_string(p.rank));
    if (!std::isfinite(p.scale)) return refuse(key, aj + "non-finite scale");
    if (!p.down || !p.up || p.down_ndim < 2 || p.down_ndim > 3 || p.up_ndim < 2 || p.up_ndim > 3)
      return refuse(key, aj + "shape does not match (down is [rank, in(, k)], up is [out, rank(, 1)])");
    if (p.up_ndim == 3 && p.up_shape[2] > 1) return refuse(key, aj + "up has a kernel > 1");
    if (!trimmed_is(p.down_shape, p.down_ndim, {p.rank, m.I, m.k}) || !trimmed_is(p.up_shape, p.up_ndim, {m.O, p.rank}))
      return refuse(key, aj + "shape does not match: the weight is [" + std::to_string(m.O) + ", " + std::to_string(m.I) +
                             (m.k > 1 ? ", " + std::to_string(m.k) : "") + "], rank " + std::to_string(p.rank));
    d.op[j] = MergeOp{p.down, p.up, p.dtype, p.rank, p.scale};
  }
  void* dst = nullptr;
  int dt = 0;
  std::vector<int64_t> shape;
  if (!foley_ctx_tensor(c, m.slot.c_str(), &dst, &dt, &shape))
    return L_FAIL(FOLEY_ERR_MISSING, ("lora: '" + key + "': packed tensor '" + m.slot + "' is not registered").c_str());
  // rows of the key inside the packed tensor: strides in whole packed rows, extent checked against the registered shape
  d.row_dims = m.row_dims;
  d.out_row0 = (int)(m.out_off / Kp);
  int64_t last_row = d.out_row0, rows = 1;
  bool ok = m.out_off % Kp == 0 && m.row_dims >= 1 && m.row_dims <= 3 && m.nd - m.row_dims >= 1 && m.nd - m.row_dims <= 2;
  for (int k = 0; ok && k < m.row_dims; ++k) {
    ok = m.is[k] % Kp == 0 && m.os[k] % Kp == 0;
    d.rsize[k] = (int)m.size[k];
    d.r_in[k] = (int)(m.is[k] / Kp);
    d.r_out[k] = (int)(m.os[k] / Kp);
    last_row += (m.size[k] - 1) * (m.os[k] / Kp);
    rows *= m.size[k];
  }
  if (ok && m.nd - m.row_dims == 1) {   // [.., K]: packed column = checkpoint column
    ok = m.size[m.nd - 1] == Kp && m.is[m.nd - 1] == 1 && m.os[m.nd - 1] == 1;
    d.csize1 = (int)Kp; d.c_in0 = 0; d.c_in1 = 1;
  } else if (ok) {                      // [.., k, I]: tap-major packed columns
    const int a = m.nd - 2, b = m.nd - 1;
    ok = m.size[a] * m.size[b] == Kp && m.os[b] == 1 && m.os[a] == m.size[b];
    d.csize1 = (int)m.size[b]; d.c_in0 = (int)m.is[a]; d.c_in1 = (int)m.is[b];
  }
  if (!ok || rows != m.O) return L_FAIL(FOLEY_ERR_INVALID, ("lora: '" + key + "': internal: the key's map is not row / column separable").c_str());
  const bool dt_ok = dt == FOLEY_F32 || dt == FOLEY_BF16 || dt == DT_F16 || dt == FOLEY_F8E4M3 || dt == FOLEY_F8E5M2;
  if (!dt_ok || shape.size() != 2 || shape[1] != Kp || last_row >= shape[0] || shape[0] * Kp >= ((int64_t)1 << 31))
    return refuse(key, "the registered packed tensor '" + m.slot + "' does not have the layout of this configuration");
  const int es = dt_size(dt);
  const size_t bytes = (size_t)shape[0] * (size_t)Kp * es;
  // ---- device work
  L_HIP(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  auto bk = s->backups.find(m.slot);
  if (bk != s->backups.end() && (bk->second.dst != dst || bk->second.bytes != bytes)) {   // registered elsewhere since: a stale copy
    L_HIP(hipStreamSynchronize(st));
    hipFree(bk->second.copy);
    s->backups.erase(bk);
    bk = s->backups.end();
  }
  if (bk == s->backups.end()) {   // first touch: the tensor as loaded
    Backup b;
    b.dst = dst;
    b.bytes = bytes;
    L_HIP(hipMalloc(&b.copy, bytes));
    hipError_t e = hipMemcpyAsync(b.copy, dst, bytes, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      hipFree(b.copy);
      return L_FAIL(FOLEY_ERR_HIP, hipGetErrorString(e));
    }
    bk = s->backups.emplace(m.slot, b).first;
  }
  d.pristine = bk->second.copy;
  d.out = dst;
  d.dt = dt;
  d.n = n;
  d.O = (int)m.O;
  d.Kp = (int)Kp;
  const int vec = 16 / es;
  d.vec_ok = Kp % vec == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)d.pristine & 15) == 0;
  const dim3 grid((unsigned)((Kp + 16 * vec - 1) / (16 * vec)), (unsigned)((m.O + TR - 1) / TR));
  if (es == 4) FOLEY_LAUNCH(lora_merge_kernel<4>, grid, dim3(256), 0, st, d);
  else if (es == 2) FOLEY_LAUNCH(lora_merge_kernel<2>, grid, dim3(256), 0, st, d);
  else FOLEY_LAUNCH(lora_merge_kernel<1>, grid, dim3(256), 0, st, d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return L_FAIL(FOLEY_ERR_HIP, hipGetErrorString(e));
  s->merged.insert(key);
  return 0;
}

extern "C" int foley_lora_end(foley_ctx* c, void* stream) {
  LoraState* s = c ? state_of(c, false) : nullptr;
  if (!s || !s->open) return L_FAIL(FOLEY_ERR_STATE, "foley_lora_begin has not been called");
  L_HIP(hipSetDevice(s->device));
  L_HIP(hipStreamSynchronize((hipStream_t)stream));   // the adapters' operands were only borrowed until here
  s->open = false;
  foley_ctx_weights_changed(c);
  return 0;
}

extern "C" int foley_lora_clear(foley_ctx* c, void* stream) {
  if (!c) return L_FAIL(FOLEY_ERR_INVALID, "bad argument");
  LoraState* s = state_of(c, false);
  if (!s) return 0;   // nothing was ever merged
  L_HIP(hipSetDevice(s->device));
  const int rc = restore_all(c, *s, (hipStream_t)stream);
  if (rc != 0) return rc;
  L_HIP(hipStreamSynchronize((hipStream_t)stream));
  foley_lora_forget(c);
  foley_ctx_weights_changed(c);
  return 0;
}

extern "C" int foley_lora_backup_bytes(foley_ctx* c, uint64_t* bytes) {
  if (!c || !bytes) return L_FAIL(FOLEY_ERR_INVALID, "bad argument");
  LoraState* s = state_of(c, false);
  *bytes = 0;
  if (s)
    for (auto& kv : s->backups) *bytes += kv.second.bytes;
  return 0;
}

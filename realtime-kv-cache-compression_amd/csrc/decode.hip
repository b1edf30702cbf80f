// decode.hip — decode attention over packed KV: the launch geometry of the split
// kernels, the merge of a decode step's splits (the packed rows' and, for decode_tail.hip, the dense
// tail's behind them) and rtkv_decode_attention_packed; the split kernel and its design notes are
// in decode_kernel.h (fp16 instantiations: decode_f16.hip).
#include "decode_kernel.h"

namespace rtkv {

namespace {

struct MergeArgs {
  const float* part_m;  // [B][G][n][Hkv]
  const float* part_l;
  const float* part_acc;  // [B][G][n][F]
  int n;
  int Hkv, D, G;
  float* out;           // [B, Hq, D] fp32
};

// out[b, hq, d] = Σ_s e^{m_s - m*} acc_s / Σ_s e^{m_s - m*} l_s over the n splits of the list.
// Workgroup of 16 features × 64 split phases (phase p takes splits ≡ p mod 64, in order), combined
// through LDS.  A split without rows (m = -inf, l = acc = 0) adds exact zeros, so a step with an
// empty tail has the bits of the step without one.
constexpr int kMF = 16, kMP = 64;
__global__ __launch_bounds__(kMF * kMP) void decode_merge_kernel(MergeArgs a) {
  __shared__ float red[3][kMP][kMF];
  const int F = a.Hkv * a.D;
  const int fl = threadIdx.x % kMF, ph = threadIdx.x / kMF;
  const int f = blockIdx.x * kMF + fl;
  const int g = blockIdx.y, b = blockIdx.z;
  const bool ok = f < F;
  const int hk = ok ? f / a.D : 0, d = f - hk * a.D;
  const int64_t base = ((int64_t)b * a.G + g) * a.n;
  float mm = -INFINITY;
  for (int s = ph; s < a.n; s += kMP) mm = fmaxf(mm, a.part_m[(base + s) * a.Hkv + hk]);
  red[0][ph][fl] = mm;
  __syncthreads();
  mm = red[0][0][fl];
#pragma unroll
  for (int p = 1; p < kMP; ++p) mm = fmaxf(mm, red[0][p][fl]);
  float num = 0.f, den = 0.f;
  if (mm != -INFINITY && ok) {
#pragma unroll 4
    for (int s = ph; s < a.n; s += kMP) {
      const float ms = a.part_m[(base + s) * a.Hkv + hk];
      const float fct = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - mm);
      num += fct * a.part_acc[(base + s) * F + f];
      den += fct * a.part_l[(base + s) * a.Hkv + hk];
    }
  }
  red[1][ph][fl] = num;
  red[2][ph][fl] = den;
  __syncthreads();
  if (ph != 0 || !ok) return;
#pragma unroll
  for (int p = 1; p < kMP; ++p) {
    num += red[1][p][fl];
    den += red[2][p][fl];
  }
  const int Hq = a.Hkv * a.G;
  a.out[((int64_t)b * Hq + (int64_t)hk * a.G + g) * a.D + d] = den > 0.f ? num / den : 0.f;
}

}  // namespace

size_t decode_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t D, int64_t cap) {
  const int64_t G = Hkv > 0 ? Hq / Hkv : 1;
  const int64_t s = decode_splits(B, G, Hkv * D, cap);
  return (size_t)(B * G * s) * (size_t)(2 * Hkv + Hkv * D) * sizeof(float) + 256;
}

int launch_decode_splits(const PackedLayer& p, const void* q, int64_t Hq, float scale, const DecodeParts& parts,
                         hipStream_t st) {
  const int64_t B = p.B, F = p.Hkv * p.D, G = Hq / p.Hkv;
  const DecodeShape sh = decode_shape(F, G);
  DecodeArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pk = p.r;
  a.Hkv = (int)p.Hkv; a.D = (int)p.D; a.G = (int)G;
  a.HG = sh.hg;
  a.GS = sh.gs;
  a.q = q; a.scale = scale * 1.4426950408889634f;
  a.splits = decode_splits(B, G, F, p.r.cap);
  a.n = parts.n;
  a.part_m = parts.m; a.part_l = parts.l; a.part_acc = parts.acc;
  a.nrest = (int)((int64_t)a.splits * a.HG * B);
  const int64_t nblk = ((int64_t)a.nrest + 7) / 8 * 8 * a.GS;
  RTKV_REQUIRE(nblk < (1ll << 31), "decode: grid too large");
  const dim3 grid((unsigned)nblk);
  const size_t lds = (size_t)kDW * 64 * sh.nch * sh.gq * 10 * sizeof(float);
  if (p.dt == RTKV_F16) return launch_decode_split_f16(a, sh.nch, sh.gq, (int)p.D, grid, lds, st);
  if (p.dt == RTKV_BF16) return launch_decode_split<RTKV_BF16>(a, sh.nch, sh.gq, (int)p.D, grid, lds, st);
  return launch_decode_split<RTKV_F32>(a, sh.nch, sh.gq, (int)p.D, grid, lds, st);
}

int launch_decode_merge(const DecodeParts& parts, int64_t B, int64_t Hq, int64_t Hkv, int64_t D, float* out,
                        hipStream_t st) {
  const int64_t F = Hkv * D, G = Hq / Hkv;
  const MergeArgs a = {parts.m, parts.l, parts.acc, parts.n, (int)Hkv, (int)D, (int)G, out};
  hipLaunchKernelGGL(decode_merge_kernel, dim3((unsigned)((F + kMF - 1) / kMF), (unsigned)G, (unsigned)B),
                     dim3(kMF * kMP), 0, st, a);
  RTKV_HIP_CHECK(hipGetLastError());
  return RTKV_OK;
}

int launch_decode(PackedLayer& p, const void* q, int64_t Hq, float scale, float* out, void* ws, size_t ws_bytes,
                  hipStream_t st) {
  // this entry point checks neither the dtype value (anything but fp16 / bf16 is read as fp32) nor the
  // workspace's alignment
  const AttnChecks c = {"decode: ", RTKV_ERR_INVALID, 0u, 0, 65535, true, 1};
  int rc;
  if ((rc = check_attn_query(c, p, q, Hq, out)) != RTKV_OK) return rc;
  if ((rc = check_attn_shape(c, p)) != RTKV_OK) return rc;
  if ((rc = check_packed_layer(c, p)) != RTKV_OK) return rc;
  if ((rc = check_workspace(c, ws, ws_bytes, decode_workspace_bytes(p.B, Hq, p.Hkv, p.D, p.r.cap))) != RTKV_OK) return rc;
  const int64_t G = Hq / p.Hkv;
  const DecodeParts parts = decode_parts(ws, p.B, G, p.Hkv, decode_splits(p.B, G, p.Hkv * p.D, p.r.cap));
  if ((rc = launch_decode_splits(p, q, Hq, scale, parts, st)) != RTKV_OK) return rc;
  return launch_decode_merge(parts, p.B, Hq, p.Hkv, p.D, out, st);
}

}  // namespace rtkv

// decode_tail.hip — one decode step of attention over a layer's PACKED rows followed by a DENSE
// tail of new tokens (rtkv_decode_attention_packed_tail).
//
// Reference: a decode step (q_len == 1) does not compress; it concatenates the new token's K/V onto
// the cache and attends over all of it (modified_llama.py:83-94, 152): at step t the keys are the
// kept, dequantized prefill rows followed by the t dense rows generated so far.  Here the packed
// rows go through the split kernel of decode_kernel.h unchanged, the tail rows through
// decode_tail_kernel below as further splits, and one merge pass takes both sets of (m, l, acc)
// partials: one softmax over the concatenation.
//
// Tail kernel: the decomposition of the packed kernel without the decoding.  One workgroup of 4
// waves per (tail split s, head group hg, batch row b, query-head group gs); wave v takes tail rows
// r0 + v + 4t.  Lane l owns the 8-element chunks c = (hg·NCH + k)·64 + l of a row, so one wave
// instruction reads 64 contiguous 16-byte chunks (fp16/bf16; two such instructions for fp32).  The
// GQ query heads of a kv head share the loaded chunk, the D/8 lanes of a head reduce q·k with the
// DPP group_sum, and the online softmax runs in the exp2 domain with the lazily raised reference.
// fp16 and bf16 keep the packed dot products (v_dot2_f32_f16, v_dot2_f32_bf16) on the stored
// pairs; the values are the stored values, accumulated in fp32.  PD rows of loads stay in flight
// per wave.  Rows at or past the (clamped) count are never read.
#include "decode_kernel.h"

namespace rtkv {

namespace {

struct TailArgs {
  const void* k;              // element (b, t, h, d) at b·stride_b + t·stride_s + h·D + d
  const void* v;
  const int64_t* rows;        // [B] tail rows in use
  int64_t cap, stride_b, stride_s;
  int Hkv, D, G;
  int HG, GS, nrest;          // as DecodeArgs, nrest = splits · HG · B
  const void* q;              // [B, Hq, D] (dtype)
  float scale;                // · log2(e)
  int splits;                 // tail splits
  float* part_m;              // [B][G][splits][Hkv]
  float* part_l;
  float* part_acc;            // [B][G][splits][F]
};

template <int DT, int NCH, int GQ, int LPH>
__global__ __launch_bounds__(64 * kDW) void decode_tail_kernel(TailArgs a) {
  using S_ = typename Dt<DT>::S;
  constexpr bool kH = DT == RTKV_F16;
  constexpr bool kB = DT == RTKV_BF16;
  constexpr int kU = GQ * NCH;    // (query head, chunk) units per lane
  constexpr int PD = DT == RTKV_F32 ? 2 : 4;  // rows in flight (≤ 32 VGPRs of K and V at NCH 2)
  extern __shared__ float lds[];  // [kDW][64][kU][10]: m, l, acc[8] per unit
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int id = blockIdx.x, hi = id >> 3;
  const int gs = hi % a.GS;
  const int rest = (id & 7) + 8 * (hi / a.GS);
  if (rest >= a.nrest) return;
  const int s = rest % a.splits, t1 = rest / a.splits, hg = t1 % a.HG, b = t1 / a.HG;
  const int F = a.HG * NCH * 512, D = a.D, lph = D / 8;
  const int c0 = hg * NCH * 64;
  const int64_t nrows = a.rows[b] < a.cap ? (a.rows[b] > 0 ? a.rows[b] : 0) : a.cap;
  const int64_t per = (nrows + a.splits - 1) / a.splits;
  const int64_t r0 = (int64_t)s * per, r1 = r0 + per < nrows ? r0 + per : nrows;
  const int Hq = a.Hkv * a.G;
  H2 qh[GQ][NCH][4];
  B2 qb[GQ][NCH][4];
  float qf[GQ][NCH][8], acc[GQ][NCH][8], m[GQ][NCH], l[GQ][NCH];
#pragma unroll
  for (int j = 0; j < GQ; ++j) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int f0 = (c0 + k * 64 + lane) * 8, hk = f0 / D, d0 = f0 - hk * D;
      const int g = gs * GQ + j;
      const S_* qp = static_cast<const S_*>(a.q) + ((int64_t)b * Hq + (int64_t)hk * a.G + g) * D + d0;
      const Chunk<DT> qc = *reinterpret_cast<const Chunk<DT>*>(qp);
      if constexpr (kH || kB) {
        const uint32_t w4[4] = {qc.a.x, qc.a.y, qc.a.z, qc.a.w};  // element pairs (2p, 2p + 1)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          if constexpr (kH) qh[j][k][p] = __builtin_bit_cast(H2, w4[p]);
          else qb[j][k][p] = __builtin_bit_cast(B2, w4[p]);
        }
      } else {
        chunk_to_f32<DT>(qc, qf[j][k]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][k][e] = 0.f;
      m[j][k] = -INFINITY;
      l[j][k] = 0.f;
    }
  }
  const float qscale = a.scale;
  // one row of the chunk columns this lane owns: dots → online softmax → accumulators
  auto row = [&](const Chunk<DT> (&xk)[NCH], const Chunk<DT> (&xv)[NCH]) {
    float sc[NCH][GQ];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      if constexpr (kH || kB) {
        const uint32_t w4[4] = {xk[k].a.x, xk[k].a.y, xk[k].a.z, xk[k].a.w};
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
          float d = 0.f;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            if constexpr (kH) d = __builtin_amdgcn_fdot2(qh[j][k][p], __builtin_bit_cast(H2, w4[p]), d, false);
            else d = __builtin_amdgcn_fdot2_f32_bf16(qb[j][k][p], __builtin_bit_cast(B2, w4[p]), d, false);
          }
          sc[k][j] = d;
        }
      } else {
        float kf[8];
        chunk_to_f32<DT>(xk[k], kf);
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) d = __builtin_fmaf(qf[j][k][e], kf[e], d);
          sc[k][j] = d;
        }
      }
    }
    bool up = false;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int j = 0; j < GQ; ++j) {
        sc[k][j] = group_sum<LPH>(sc[k][j], lph) * qscale;
        up |= sc[k][j] > m[j][k] + kSlack;
      }
    // lazily raised reference m, as in the packed kernel: weights stay ≤ 2^kSlack
    if (__ballot(up)) {
#pragma unroll
      for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
          const float mn = sc[k][j] > m[j][k] + kSlack ? sc[k][j] : m[j][k];
          const float cr = __builtin_amdgcn_exp2f(m[j][k] - mn);
          l[j][k] *= cr;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j][k][e] *= cr;
          m[j][k] = mn;
        }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      float pw[GQ];
#pragma unroll
      for (int j = 0; j < GQ; ++j) {
        pw[j] = __builtin_amdgcn_exp2f(sc[k][j] - m[j][k]);
        l[j][k] += pw[j];
      }
      if constexpr (kH) {
        const uint32_t w4[4] = {xv[k].a.x, xv[k].a.y, xv[k].a.z, xv[k].a.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const H2 vh = __builtin_bit_cast(H2, w4[p]);
#pragma unroll
          for (int j = 0; j < GQ; ++j) {
            acc[j][k][2 * p] = __builtin_fmaf(pw[j], (float)vh.x, acc[j][k][2 * p]);
            acc[j][k][2 * p + 1] = __builtin_fmaf(pw[j], (float)vh.y, acc[j][k][2 * p + 1]);
          }
        }
      } else {
        float vf[8];
        chunk_to_f32<DT>(xv[k], vf);
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j][k][e] = __builtin_fmaf(pw[j], vf[e], acc[j][k][e]);
        }
      }
    }
  };
  // Rows of this wave: r0 + wave + kDW·t for t < nt.  PD rows are loaded ahead; a slot is refilled
  // as soon as its row is consumed.  Every branch is wave-uniform (nt is scalar).
  const int64_t nt = r0 + wave < r1 ? (r1 - r0 - wave + kDW - 1) / kDW : 0;
  const int64_t lane_off = (int64_t)b * a.stride_b + (int64_t)(c0 + lane) * 8;
  const S_* kbase = static_cast<const S_*>(a.k) + lane_off;
  const S_* vbase = static_cast<const S_*>(a.v) + lane_off;
  Chunk<DT> bk[PD][NCH], bv[PD][NCH];
  auto issue = [&](int i, int64_t t) {
    if (t >= nt) return;  // never read at or past the count
    const int64_t ro = (r0 + wave + (int64_t)kDW * t) * a.stride_s;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      bk[i][k] = *reinterpret_cast<const Chunk<DT>*>(kbase + ro + k * 512);
      bv[i][k] = *reinterpret_cast<const Chunk<DT>*>(vbase + ro + k * 512);
    }
  };
#pragma unroll
  for (int i = 0; i < PD; ++i) issue(i, i);
  for (int64_t t = 0; t < nt; t += PD) {
#pragma unroll
    for (int i = 0; i < PD; ++i) {
      if (t + i < nt) {
        row(bk[i], bv[i]);
        issue(i, t + i + PD);
      }
    }
  }
  // ---- merge the kDW waves in LDS, then write this split's partial (decode_kernel.h's layout)
  float* mine = lds + ((size_t)wave * 64 + lane) * kU * 10;
#pragma unroll
  for (int j = 0; j < GQ; ++j) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      float* u = mine + (j * NCH + k) * 10;
      u[0] = m[j][k];
      u[1] = l[j][k];
#pragma unroll
      for (int e = 0; e < 8; ++e) u[2 + e] = acc[j][k][e];
    }
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int j = 0; j < GQ; ++j) {
    const int g = gs * GQ + j;
    const int64_t pbase = ((int64_t)b * a.G + g) * a.splits + s;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int un = j * NCH + k;
      float mm = -INFINITY;
      for (int v = 0; v < kDW; ++v) mm = fmaxf(mm, lds[(((size_t)v * 64 + lane) * kU + un) * 10]);
      float ll = 0.f, aa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int v = 0; v < kDW; ++v) {
        const float* src = lds + (((size_t)v * 64 + lane) * kU + un) * 10;
        const float f = src[0] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(src[0] - mm);
        ll += f * src[1];
#pragma unroll
        for (int e = 0; e < 8; ++e) aa[e] += f * src[2 + e];
      }
      const int f0 = (c0 + k * 64 + lane) * 8, hk = f0 / D;
      if ((lane % lph) == 0) {
        a.part_m[pbase * a.Hkv + hk] = mm;
        a.part_l[pbase * a.Hkv + hk] = ll;
      }
      float* pa = a.part_acc + pbase * F + f0;
#pragma unroll
      for (int e = 0; e < 8; ++e) pa[e] = aa[e];
    }
  }
}

template <int DT>
int launch_tail_split(const TailArgs& a, int nch, int gq, int D, dim3 grid, size_t lds, hipStream_t st) {
#define RTKV_D(N, Q)                                                                                  \
  if (nch == N && gq == Q) {                                                                          \
    if (D == 128)                                                                                     \
      hipLaunchKernelGGL((decode_tail_kernel<DT, N, Q, 16>), grid, dim3(64 * kDW), lds, st, a);      \
    else                                                                                              \
      hipLaunchKernelGGL((decode_tail_kernel<DT, N, Q, 0>), grid, dim3(64 * kDW), lds, st, a);       \
    RTKV_HIP_CHECK(hipGetLastError());                                                                \
    return RTKV_OK;                                                                                   \
  }
  RTKV_D(1, 1) RTKV_D(2, 1) RTKV_D(1, 2) RTKV_D(1, 4)
#undef RTKV_D
  RTKV_REQUIRE(false, "decode: unsupported lane shape");
}

// decode_merge_kernel (decode.hip) over two sets of partials: the sp packed splits, then the st
// tail splits, as one list of sp + st splits.  Same geometry and the same arithmetic per split, so
// with an empty tail (every tail partial m = -inf, l = acc = 0) the result has the bits of the
// packed-only merge.
struct TailMergeArgs {
  const float* pm;  // packed partials [B][G][sp][Hkv], [B][G][sp][F]
  const float* pl;
  const float* pa;
  const float* tm;  // tail partials [B][G][st][Hkv], [B][G][st][F]
  const float* tl;
  const float* ta;
  int sp, st;
  int Hkv, D, G;
  float* out;       // [B, Hq, D] fp32
};
constexpr int kMF = 16, kMP = 64;
__global__ __launch_bounds__(kMF * kMP) void decode_tail_merge_kernel(TailMergeArgs a) {
  __shared__ float red[3][kMP][kMF];
  const int F = a.Hkv * a.D;
  const int fl = threadIdx.x % kMF, ph = threadIdx.x / kMF;
  const int f = blockIdx.x * kMF + fl;
  const int g = blockIdx.y, b = blockIdx.z;
  const bool ok = f < F;
  const int hk = ok ? f / a.D : 0, d = f - hk * a.D;
  const int64_t bg = (int64_t)b * a.G + g;
  const int n = a.sp + a.st;
  // split s of the list: its m and l entry, and its acc entry
  auto ml = [&](int s) { return s < a.sp ? (bg * a.sp + s) * a.Hkv + hk : (bg * a.st + (s - a.sp)) * a.Hkv + hk; };
  auto ac = [&](int s) { return s < a.sp ? (bg * a.sp + s) * F + f : (bg * a.st + (s - a.sp)) * F + f; };
  float mm = -INFINITY;
  for (int s = ph; s < n; s += kMP) mm = fmaxf(mm, (s < a.sp ? a.pm : a.tm)[ml(s)]);
  red[0][ph][fl] = mm;
  __syncthreads();
  mm = red[0][0][fl];
#pragma unroll
  for (int p = 1; p < kMP; ++p) mm = fmaxf(mm, red[0][p][fl]);
  float num = 0.f, den = 0.f;
  if (mm != -INFINITY && ok) {
    for (int s = ph; s < n; s += kMP) {
      const bool pk = s < a.sp;
      const float ms = (pk ? a.pm : a.tm)[ml(s)];
      const float fct = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - mm);
      num += fct * (pk ? a.pa : a.ta)[ac(s)];
      den += fct * (pk ? a.pl : a.tl)[ml(s)];
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

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// bytes of the tail partials: B·G·splits·(2·Hkv + F) floats
size_t tail_part_bytes(int64_t B, int64_t G, int64_t Hkv, int64_t D, int splits) {
  return (size_t)(B * G * splits) * (size_t)(2 * Hkv + Hkv * D) * sizeof(float);
}

}  // namespace

size_t decode_tail_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t D, int64_t cap, int64_t tail_cap) {
  const int64_t G = Hkv > 0 ? Hq / Hkv : 1;
  const size_t packed = cap >= 1 ? align256(decode_workspace_bytes(B, Hq, Hkv, D, cap)) : 0;
  return packed + tail_part_bytes(B, G, Hkv, D, decode_splits(B, G, Hkv * D, tail_cap)) + 256;
}

int launch_decode_tail(const uint8_t* codes_k, const uint8_t* codes_v, int64_t codes_bytes, const int64_t* row_offset,
                       const float* scale_zp, const int32_t* kept_index, const uint8_t* labels, int64_t B, int64_t S,
                       int64_t cap, const int64_t* rows, int64_t Hkv, int64_t D, int dt, const int32_t bits[3],
                       const void* q, int64_t Hq, float scale, const rtkv_dense_tail* tail, float* out, void* ws,
                       size_t ws_bytes, hipStream_t st) {
  RTKV_REQUIRE(tail && q && out, "decode: null pointer");
  RTKV_REQUIRE(B >= 1 && Hkv >= 1 && D >= 1 && Hq >= Hkv && Hq % Hkv == 0 && cap >= 0, "decode: bad shape");
  RTKV_REQUIRE(B <= 65535, "decode: grid too large");
  RTKV_REQUIRE(dt == RTKV_F32 || dt == RTKV_F16 || dt == RTKV_BF16, "decode: unsupported dtype");
  const int64_t F = Hkv * D, G = Hq / Hkv;
  RTKV_REQUIRE(F % 512 == 0, "decode: Hkv*D must be a multiple of 512");
  RTKV_REQUIRE(D % 8 == 0 && 64 % (D / 8) == 0, "decode: head_dim must be 8·2^k with 8 <= head_dim <= 512");
  RTKV_REQUIRE(((uintptr_t)q & 15) == 0, "decode: q must be 16-byte aligned");
  RTKV_REQUIRE(tail->capacity >= 0, "decode: negative tail capacity");
  RTKV_REQUIRE(tail->rows_dev != nullptr, "decode: null tail rows_dev");
  const int64_t e = dtype_bytes(dt);
  if (tail->capacity > 0) {
    RTKV_REQUIRE(tail->k_dev && tail->v_dev, "decode: null tail pointer");
    RTKV_REQUIRE(((uintptr_t)tail->k_dev & 15) == 0 && ((uintptr_t)tail->v_dev & 15) == 0,
                 "decode: tail k_dev and v_dev must be 16-byte aligned");
    RTKV_REQUIRE(tail->stride_b >= 0 && tail->stride_s >= F, "decode: tail stride_s below Hkv*D or negative stride_b");
    RTKV_REQUIRE((tail->stride_b * e) % 16 == 0 && (tail->stride_s * e) % 16 == 0,
                 "decode: tail strides must keep rows 16-byte aligned");
  }
  RTKV_REQUIRE(ws && ((uintptr_t)ws & 3) == 0 && ws_bytes >= decode_tail_workspace_bytes(B, Hq, Hkv, D, cap, tail->capacity),
               "decode: workspace too small");
  TailMergeArgs mg;
  std::memset(&mg, 0, sizeof(mg));
  size_t used = 0;
  if (cap >= 1) {  // the packed rows: the split kernels of rtkv_decode_attention_packed, same arguments
    DecodeArgs pa;
    used = align256(decode_workspace_bytes(B, Hq, Hkv, D, cap));
    const int rc = launch_decode_splits(codes_k, codes_v, codes_bytes, row_offset, scale_zp, kept_index, labels, B, S, cap,
                                        rows, Hkv, D, dt, bits, q, Hq, scale, out, ws, used, st, pa);
    if (rc != RTKV_OK) return rc;
    mg.pm = pa.part_m; mg.pl = pa.part_l; mg.pa = pa.part_acc; mg.sp = pa.splits;
  }
  const DecodeShape sh = decode_shape(F, G);
  TailArgs a;
  std::memset(&a, 0, sizeof(a));
  a.k = tail->k_dev; a.v = tail->v_dev; a.rows = tail->rows_dev;
  a.cap = tail->capacity; a.stride_b = tail->stride_b; a.stride_s = tail->stride_s;
  a.Hkv = (int)Hkv; a.D = (int)D; a.G = (int)G;
  a.HG = sh.hg; a.GS = sh.gs;
  a.q = q; a.scale = scale * 1.4426950408889634f;
  a.splits = decode_splits(B, G, F, tail->capacity);
  a.nrest = (int)((int64_t)a.splits * a.HG * B);
  float* p = reinterpret_cast<float*>(static_cast<char*>(ws) + used);
  a.part_m = p;
  p += B * G * a.splits * Hkv;
  a.part_l = p;
  p += B * G * a.splits * Hkv;
  a.part_acc = p;
  const int64_t nblk = ((int64_t)a.nrest + 7) / 8 * 8 * a.GS;
  RTKV_REQUIRE(nblk < (1ll << 31), "decode: grid too large");
  const dim3 grid((unsigned)nblk);
  const size_t lds = (size_t)kDW * 64 * sh.nch * sh.gq * 10 * sizeof(float);
  int rc;
  if (dt == RTKV_F16) rc = launch_tail_split<RTKV_F16>(a, sh.nch, sh.gq, (int)D, grid, lds, st);
  else if (dt == RTKV_BF16) rc = launch_tail_split<RTKV_BF16>(a, sh.nch, sh.gq, (int)D, grid, lds, st);
  else rc = launch_tail_split<RTKV_F32>(a, sh.nch, sh.gq, (int)D, grid, lds, st);
  if (rc != RTKV_OK) return rc;
  mg.tm = a.part_m; mg.tl = a.part_l; mg.ta = a.part_acc; mg.st = a.splits;
  mg.Hkv = (int)Hkv; mg.D = (int)D; mg.G = (int)G; mg.out = out;
  hipLaunchKernelGGL(decode_tail_merge_kernel, dim3((unsigned)((F + kMF - 1) / kMF), (unsigned)G, (unsigned)B),
                     dim3(kMF * kMP), 0, st, mg);
  RTKV_HIP_CHECK(hipGetLastError());
  return RTKV_OK;
}

}  // namespace rtkv

// decode_tail.hip — one decode step of attention over a layer's PACKED rows followed by a DENSE
// tail of new tokens (rtkv_decode_attention_packed_tail).
//
// Reference: a decode step (q_len == 1) does not compress; it concatenates the new token's K/V onto
// the cache and attends over all of it (modified_llama.py:83-94, 152): at step t the keys are the
// kept, dequantized prefill rows followed by the t dense rows generated so far.  Here the packed
// rows go through the split kernel of decode_kernel.h unchanged, the tail rows through
// decode_tail_kernel below as further splits of the same list of (m, l, acc) partials, and the merge
// of decode.hip takes the whole list: one softmax over the concatenation.
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
  int n;                      // splits in the step's list of partials
  float* part_m;              // [B][G][n][Hkv], from the first tail split on
  float* part_l;
  float* part_acc;            // [B][G][n][F], likewise
};

template <int DT, int NCH, int GQ, int LPH>
__global__ __launch_bounds__(64 * kDW) void decode_tail_kernel(TailArgs a) {
  using S_ = typename Dt<DT>::S;
  constexpr bool kH = DT == RTKV_F16;
  constexpr bool kB = DT == RTKV_BF16;
  constexpr int PD = DT == RTKV_F32 ? 2 : 4;  // rows in flight (≤ 32 VGPRs of K and V at NCH 2)
  extern __shared__ float lds[];  // [kDW][64][GQ·NCH][10]: m, l, acc[8] per (query head, chunk) unit
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
  // ---- the kDW waves meet in LDS; wave 0 merges them and writes this split's partial
  float* mine = lds + ((size_t)wave * 64 + lane) * (GQ * NCH) * 10;
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
  merge_waves_write_partial<RTKV_F32, NCH, GQ>(a, lds, lane, gs, b, s, c0, F, D, lph);  // acc in element order
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

}  // namespace

// The partials are one list of n = sp + st splits per (b, g): B·G·(sp + st)·(2·Hkv + F) floats.  The size
// below is that of two separate lists, the packed one rounded up to 256 bytes, and so never smaller:
//   align256(4·B·G·sp·(2·Hkv + F) + 256) + 4·B·G·st·(2·Hkv + F) + 256 >= 4·B·G·(sp + st)·(2·Hkv + F).
size_t decode_tail_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t D, int64_t cap, int64_t tail_cap) {
  const int64_t G = Hkv > 0 ? Hq / Hkv : 1;
  const size_t packed = cap >= 1 ? (decode_workspace_bytes(B, Hq, Hkv, D, cap) + 255) / 256 * 256 : 0;
  const size_t st = decode_splits(B, G, Hkv * D, tail_cap);
  return packed + (size_t)(B * G) * st * (size_t)(2 * Hkv + Hkv * D) * sizeof(float) + 256;
}

// The tail half of a decode step: the tail's decode_splits(tail->capacity) splits are written as splits
// first .. of `parts` (the list of the whole step; the caller has checked the tail and sized the list).
int launch_tail_splits(const rtkv_dense_tail* tail, int dt, int64_t B, int64_t Hkv, int64_t D, const void* q, int64_t Hq,
                       float scale, const DecodeParts& parts, int first, hipStream_t st) {
  const int64_t F = Hkv * D, G = Hq / Hkv;
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
  a.n = parts.n;  // the tail's splits follow the `first` ones before them
  a.part_m = parts.m + (int64_t)first * Hkv;
  a.part_l = parts.l + (int64_t)first * Hkv;
  a.part_acc = parts.acc + (int64_t)first * F;
  const int64_t nblk = ((int64_t)a.nrest + 7) / 8 * 8 * a.GS;
  RTKV_REQUIRE(nblk < (1ll << 31), "decode: grid too large");
  const dim3 grid((unsigned)nblk);
  const size_t lds = (size_t)kDW * 64 * sh.nch * sh.gq * 10 * sizeof(float);
  if (dt == RTKV_F16) return launch_tail_split<RTKV_F16>(a, sh.nch, sh.gq, (int)D, grid, lds, st);
  if (dt == RTKV_BF16) return launch_tail_split<RTKV_BF16>(a, sh.nch, sh.gq, (int)D, grid, lds, st);
  return launch_tail_split<RTKV_F32>(a, sh.nch, sh.gq, (int)D, grid, lds, st);
}

int launch_decode_tail(PackedLayer& p, const void* q, int64_t Hq, float scale, const rtkv_dense_tail* tail, float* out,
                       void* ws, size_t ws_bytes, hipStream_t st) {
  const AttnChecks c = {"decode: ", RTKV_ERR_INVALID, 1u << RTKV_F32 | 1u << RTKV_F16 | 1u << RTKV_BF16, 0, 65535,
                        false, 4};
  int rc;
  if ((rc = check_attn_query(c, p, q, Hq, out)) != RTKV_OK) return rc;
  if ((rc = check_attn_shape(c, p)) != RTKV_OK) return rc;
  const int64_t B = p.B, Hkv = p.Hkv, D = p.D, F = Hkv * D, G = Hq / Hkv;
  if ((rc = check_dense_tail(c, tail, F, dtype_bytes(p.dt))) != RTKV_OK) return rc;
  if ((rc = check_workspace(c, ws, ws_bytes, decode_tail_workspace_bytes(B, Hq, Hkv, D, p.r.cap, tail->capacity))) != RTKV_OK)
    return rc;
  if ((rc = check_packed_layer(c, p)) != RTKV_OK) return rc;
  const int sp = p.r.cap >= 1 ? decode_splits(B, G, F, p.r.cap) : 0;
  const DecodeParts parts = decode_parts(ws, B, G, Hkv, sp + decode_splits(B, G, F, tail->capacity));
  if (sp > 0 && (rc = launch_decode_splits(p, q, Hq, scale, parts, st)) != RTKV_OK) return rc;
  if ((rc = launch_tail_splits(tail, p.dt, B, Hkv, D, q, Hq, scale, parts, sp, st)) != RTKV_OK) return rc;
  return launch_decode_merge(parts, B, Hq, Hkv, D, out, st);
}

}  // namespace rtkv

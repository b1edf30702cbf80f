// gq_decode.hip — one decode step of attention over a layer in the "rtkv-gq/1" format (outlier.hip)
// followed by a DENSE tail of new tokens (rtkv_gq_decode_attention_tail).
//
// NO REFERENCE COUNTERPART for the format (the reference keeps one scale/zero-point per token,
// dynamic_quantization.py:181-194).  The step itself is the reference's decode step
// (modified_llama.py:83-94, 152): it concatenates the new token's K/V onto the cache and attends over
// all of it — here the cache is the gq layer, whose keys and values are decoded on the fly to exactly
// the values rtkv_gq_unpack writes, and the tail is rtkv_dense_tail as decode_tail.hip reads it.
//
// gq_split_kernel has the decomposition of decode_split_kernel (decode_kernel.h): one workgroup of
// kDW waves per (split, head group, query-head group), B = 1; wave v takes rows r0 + v + 4t; lane l
// owns the 8-element chunks c = (hg·NCH + k)·64 + l, so a wave's code load is 64·w contiguous bytes
// of the row, through a buffer descriptor bounded to the row; the rows of one width are taken
// together and several stay in flight; head_dim is 128, so a head is 16 lanes (one DPP row) and
// group_sum<16> reduces q·k; exp2-domain online softmax with the lazily raised maximum; the waves
// meet in merge_waves_write_partial.  Its partial is therefore one more entry of the step's list
// of (m, l, acc) splits: the tail's splits (decode_tail.hip) follow in the same list and the merge
// of decode.hip takes all of it — one softmax over the concatenation.
//
// What the gq format adds per row:
//   parameters  {scale, zero_point} per (row, tensor, head) in the K/V dtype, meta[r][t][h][2]: the 16
//               lanes of a head load the same element (one 4-byte load per lane, tensor and chunk column
//               for the 16-bit dtypes, 8 bytes for fp32), through a descriptor bounded to the row's block.
//   outliers    outlier_idx[2][H][n_outlier] is constant for the layer: before the row loop the 16 lanes
//               of a head hold the head's 16 slots, one each, and every lane collects from them (16
//               lane-to-lane reads per tensor and column) the mask of its 8 elements that are outlier
//               channels and their slots.  Per row the first outlier value of a chunk is loaded with the
//               codes (a bounded descriptor over raw[r]; lanes without an outlier address past its end
//               and read nothing) and replaces the dequantized element bit for bit; a chunk with more
//               than one outlier channel (rare: n_outlier channels over a head's 16 chunks) loads the
//               others on demand.
//   row class   labels[kept_index[r]] → bits[]; a row whose kept index is outside [0, S), whose offset is
//               negative or whose codes would pass codes_capacity is skipped, not read.
#include "decode_kernel.h"

#include <type_traits>

namespace rtkv {

namespace {

constexpr int kGqD = 128;       // head_dim (one group per head)
constexpr int kGqMaxOut = 16;   // outlier slots per head (4-bit slot ids)
constexpr int kNoRaw = 0x40000000;  // byte offset past every raw block: the bounded load returns 0, reads nothing

struct GqSplitArgs {
  const int32_t* kept_index;    // [row_cap] token of each kept row
  const uint8_t* labels;        // [S] class of each token
  const rtkv_layer_stats* stats;
  const int64_t* row_offset;    // [row_cap]
  const uint8_t* codes_k;
  const uint8_t* codes_v;
  int64_t codes_capacity;
  const void* meta;             // [rows][2][H][2] dtype
  const void* raw;              // [rows][2][H][n_out] dtype
  const int16_t* idx;           // [2][H][n_out]
  int64_t S, row_cap;
  int bits[3];
  int n_out;
  int Hkv, G;                   // G = Hq / Hkv
  int HG, GS, nrest;            // as DecodeArgs, nrest = splits · HG
  const void* q;                // [Hq, 128] (dtype)
  float scale;                  // · log2(e)
  int splits;                   // splits of the gq rows
  int n;                        // splits in the step's list of partials
  float* part_m;                // [G][n][Hkv]
  float* part_l;
  float* part_acc;              // [G][n][F]
};

// {scale, zero_point} of one head as loaded: the two 16-bit values in one word, or two floats
template <int DT> using GqMeta = std::conditional_t<DT == RTKV_F32, float2, uint32_t>;

template <int DT> __device__ __forceinline__ GqMeta<DT> load_meta(__amdgpu_buffer_rsrc_t rs, int off) {
  if constexpr (DT == RTKV_F32) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
    return make_float2(__uint_as_float(v[0]), __uint_as_float(v[1]));
  } else {
    return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
  }
}
template <int DT> __device__ __forceinline__ uint32_t load_raw(__amdgpu_buffer_rsrc_t rs, int off) {
  if constexpr (DT == RTKV_F32) return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
  else return __builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0);
}
template <int DT> __device__ __forceinline__ uint32_t load_raw_at(const void* p, int64_t i) {
  if constexpr (DT == RTKV_F32) return static_cast<const uint32_t*>(p)[i];
  else return static_cast<const uint16_t*>(p)[i];
}

// The register pair (16-bit dtypes) that holds element e of a chunk and its half: fp16 keeps the pairs
// (p, p + 4) of slot_elem, bf16 the pairs (2p, 2p + 1).
template <int DT> __device__ __forceinline__ constexpr int pair_of(int e) { return DT == RTKV_F16 ? (e & 3) : (e >> 1); }
template <int DT> __device__ __forceinline__ constexpr bool high_of(int e) { return DT == RTKV_F16 ? (e >> 2) : (e & 1); }

// What a lane keeps about the outlier channels among the 8 elements of one of its chunks.
template <int DT> struct GqPatch {
  int off0;          // byte offset of the first one's value inside a row's raw block, or kNoRaw
  bool multi;        // more than one
  uint32_t sel[DT == RTKV_F32 ? 1 : 4];  // 16-bit dtypes: the halves of each register pair that are outlier
                                         // channels; fp32: bit e set for element e
};

// The further outlier channels of a chunk with more than one (rare): the head's list again, slot by slot
// (idx_h = outlier_idx[t][h], raw_h = raw[r][t][h]); put(e, v) sets element e.
template <int DT, typename Put>
__device__ __forceinline__ void patch_more(const int16_t* idx_h, const void* raw, int64_t hbase, int n_out, int sub, Put put) {
  for (int sn = 0; sn < n_out; ++sn) {
    const int ch = idx_h[sn];
    if (ch >= 0 && ch < kGqD && (ch >> 3) == sub) put(ch & 7, load_raw_at<DT>(raw, hbase + sn));
  }
}

// dequantized chunk (16-bit dtypes: 4 register pairs) with its outlier channels' raw values in place
template <int DT>
__device__ __forceinline__ void patch16(uint32_t (&x)[4], const GqPatch<DT>& p, uint32_t raw0, const int16_t* idx_h,
                                        const void* raw, int64_t hbase, int n_out, int sub) {
  const uint32_t ins = raw0 | (raw0 << 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = (x[i] & ~p.sel[i]) | (ins & p.sel[i]);
  if (p.multi)
    patch_more<DT>(idx_h, raw, hbase, n_out, sub, [&](int e, uint32_t v) {
#pragma unroll
      for (int ee = 0; ee < 8; ++ee)
        if (ee == e) {
          uint32_t& w = x[pair_of<DT>(ee)];
          w = high_of<DT>(ee) ? ((w & 0xffffu) | (v << 16)) : ((w & 0xffff0000u) | v);
        }
    });
}
__device__ __forceinline__ void patch32(float (&x)[8], const GqPatch<RTKV_F32>& p, uint32_t raw0, const int16_t* idx_h,
                                        const void* raw, int64_t hbase, int n_out, int sub) {
  const float r0 = __uint_as_float(raw0);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = ((p.sel[0] >> e) & 1u) ? r0 : x[e];
  if (p.multi)
    patch_more<RTKV_F32>(idx_h, raw, hbase, n_out, sub, [&](int e, uint32_t v) {
#pragma unroll
      for (int ee = 0; ee < 8; ++ee) x[ee] = ee == e ? __uint_as_float(v) : x[ee];
    });
}

template <int DT, int NCH, int GQ>
__global__ __launch_bounds__(64 * kDW) void gq_split_kernel(GqSplitArgs a) {
  using S_ = typename Dt<DT>::S;
  constexpr bool kH = DT == RTKV_F16;
  constexpr bool kB = DT == RTKV_BF16;
  constexpr int kE = Dt<DT>::kBytes;
  constexpr int D = kGqD, lph = D / 8;
  extern __shared__ float lds[];  // [kDW][64][GQ·NCH][10]: m, l, acc[8] per (query head, chunk) unit
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int id = blockIdx.x, hi = id >> 3;
  const int gs = hi % a.GS;
  const int rest = (id & 7) + 8 * (hi / a.GS);
  if (rest >= a.nrest) return;
  const int s = rest % a.splits, hg = rest / a.splits;
  const int H = a.Hkv, F = H * D;
  const int c0 = hg * NCH * 64;  // first chunk of this head group
  int64_t nrows = reinterpret_cast<const rtkv_batch_stats*>(a.stats + 1)[0].kept;
  nrows = nrows < 0 ? 0 : (nrows < a.row_cap ? nrows : a.row_cap);
  const int64_t per = (nrows + a.splits - 1) / a.splits;
  const int64_t r0 = (int64_t)s * per, r1 = r0 + per < nrows ? r0 + per : nrows;
  // q (fp16: half2 pairs in slot order; bf16: pairs; fp32: floats), accumulators in slot order, m / l
  H2 qh[GQ][NCH][4];
  B2 qb[GQ][NCH][4];
  float qf[GQ][NCH][8], acc[GQ][NCH][8], m[GQ][NCH], l[GQ][NCH];
#pragma unroll
  for (int j = 0; j < GQ; ++j) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int f0 = (c0 + k * 64 + lane) * 8, hk = f0 / D, d0 = f0 - hk * D;
      const int g = gs * GQ + j;
      const S_* qp = static_cast<const S_*>(a.q) + ((int64_t)hk * a.G + g) * D + d0;
      const Chunk<DT> qc = *reinterpret_cast<const Chunk<DT>*>(qp);
      if constexpr (kH) {
        const uint32_t w4[4] = {qc.a.x, qc.a.y, qc.a.z, qc.a.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const uint32_t lo = (w4[p >> 1] >> (16 * (p & 1))) & 0xffffu, hi2 = (w4[2 + (p >> 1)] >> (16 * (p & 1))) & 0xffffu;
          qh[j][k][p] = __builtin_bit_cast(H2, lo | (hi2 << 16));
        }
      } else if constexpr (kB) {
        const uint32_t w4[4] = {qc.a.x, qc.a.y, qc.a.z, qc.a.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) qb[j][k][p] = __builtin_bit_cast(B2, w4[p]);  // elements (2p, 2p+1)
      } else {
        chunk_to_f32<DT>(qc, qf[j][k]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][k][e] = 0.f;
      m[j][k] = -INFINITY;
      l[j][k] = 0.f;
    }
  }
  // ---- the layer's outlier channels among this lane's elements, per tensor and chunk column.  Lane j of
  // a head's 16 lanes loads slot j of the head's list; every lane then reads the 16 slots of its head.
  GqPatch<DT> pt[2][NCH];
  int hl[NCH];  // the head of each chunk column
#pragma unroll
  for (int k = 0; k < NCH; ++k) hl[k] = (c0 + k * 64 + lane) >> 4;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int sub = lane & 15;
      int mine = -1;
      if (sub < a.n_out) mine = a.idx[((int64_t)t * H + hl[k]) * a.n_out + sub];
      uint32_t mk = 0, sl = 0;
#pragma unroll
      for (int sn = 0; sn < kGqMaxOut; ++sn) {
        const int ch = __shfl(mine, (lane & 48) + sn, kWave);
        if (ch >= 0 && ch < D && (ch >> 3) == sub) {
          mk |= 1u << (ch & 7);
          sl = (sl & ~(15u << (4 * (ch & 7)))) | ((uint32_t)sn << (4 * (ch & 7)));
        }
      }
      GqPatch<DT>& p = pt[t][k];
      const int e0 = mk ? __ffs(mk) - 1 : 0;
      p.off0 = mk ? (((t * H + hl[k]) * a.n_out + (int)((sl >> (4 * e0)) & 15u)) * kE) : kNoRaw;
      p.multi = (mk & (mk - 1)) != 0u;
      if constexpr (DT == RTKV_F32) {
        p.sel[0] = mk;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) p.sel[i] = 0u;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if ((mk >> e) & 1u) p.sel[pair_of<DT>(e)] |= high_of<DT>(e) ? 0xffff0000u : 0x0000ffffu;
      }
    }
  }
  const float qscale = a.scale;  // 1/sqrt(D) · log2(e): scores in the exp2 domain
  // one row of the chunk columns this lane owns: K' → dots → online softmax → V' → accumulators.
  // jr: the row (scalar), for the raw values a chunk with several outlier channels loads on demand.
  auto row = [&](auto wtag, const ChunkCodes<decltype(wtag)::value> (&xk)[NCH],
                 const ChunkCodes<decltype(wtag)::value> (&xv)[NCH], const GqMeta<DT> (&pk)[NCH],
                 const GqMeta<DT> (&pv)[NCH], const uint32_t (&wk)[NCH], const uint32_t (&wv)[NCH], int64_t jr) {
    constexpr int W = decltype(wtag)::value;
    float sc[NCH][GQ];
    const int64_t rbase = jr * 2 * H * a.n_out;  // raw[jr][0][0][0]
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int64_t hbase = rbase + (int64_t)hl[k] * a.n_out;
      if constexpr (kH) {
        const H2 ms = __builtin_bit_cast(H2, pk[k]);  // {scale, zero_point}
        const H2 sc2 = __builtin_shufflevector(ms, ms, 0, 0), zp2 = __builtin_shufflevector(ms, ms, 1, 1);
        H2 kh[4];
        codes_h2<W>(xk[k], kh);
        uint32_t u[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) u[p] = __builtin_bit_cast(uint32_t, (kh[p] - zp2) * sc2);
        patch16<DT>(u, pt[0][k], wk[k], a.idx + hl[k] * a.n_out, a.raw, hbase, a.n_out, lane & 15);
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
          float d = 0.f;
#pragma unroll
          for (int p = 0; p < 4; ++p) d = __builtin_amdgcn_fdot2(qh[j][k][p], __builtin_bit_cast(H2, u[p]), d, false);
          sc[k][j] = d;
        }
      } else if constexpr (kB) {
        RowParams rk;
        rk.scale = __uint_as_float(pk[k] << 16);
        rk.zp = __uint_as_float(pk[k] & 0xffff0000u);
        float kc[8];
        unpack8<W>(xk[k], kc);
        uint32_t u[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) u[p] = __builtin_bit_cast(uint32_t, dequant_bf2(kc[2 * p], kc[2 * p + 1], rk));
        patch16<DT>(u, pt[0][k], wk[k], a.idx + hl[k] * a.n_out, a.raw, hbase, a.n_out, lane & 15);
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
          float d = 0.f;
#pragma unroll
          for (int p = 0; p < 4; ++p)
            d = __builtin_amdgcn_fdot2_f32_bf16(qb[j][k][p], __builtin_bit_cast(B2, u[p]), d, false);
          sc[k][j] = d;
        }
      } else {
        RowParams rk;
        rk.scale = pk[k].x;
        rk.zp = pk[k].y;
        float kf[8];
        unpack8<W>(xk[k], kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) kf[e] = dequant<DT>(kf[e], rk);
        patch32(kf, pt[0][k], wk[k], a.idx + hl[k] * a.n_out, a.raw, hbase, a.n_out, lane & 15);
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) d = __builtin_fmaf(qf[j][k][e], kf[e], d);
          sc[k][j] = d;
        }
      }
    }
    // head sums (independent DPP chains side by side), scores in the exp2 domain
    bool up = false;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int j = 0; j < GQ; ++j) {
        sc[k][j] = group_sum<lph>(sc[k][j], lph) * qscale;
        up |= sc[k][j] > m[j][k] + kSlack;
      }
    // online softmax with the lazily raised reference m, as in decode_split_kernel
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
      const int64_t hbase = rbase + ((int64_t)H + hl[k]) * a.n_out;  // raw[jr][1][h][0]
      float pw[GQ];
#pragma unroll
      for (int j = 0; j < GQ; ++j) {
        pw[j] = __builtin_amdgcn_exp2f(sc[k][j] - m[j][k]);
        l[j][k] += pw[j];
      }
      // V' and the accumulators
      if constexpr (kH) {
        const H2 ms = __builtin_bit_cast(H2, pv[k]);
        const H2 sc2 = __builtin_shufflevector(ms, ms, 0, 0), zp2 = __builtin_shufflevector(ms, ms, 1, 1);
        H2 vh[4];
        codes_h2<W>(xv[k], vh);
        uint32_t u[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) u[p] = __builtin_bit_cast(uint32_t, (vh[p] - zp2) * sc2);
        patch16<DT>(u, pt[1][k], wv[k], a.idx + (H + hl[k]) * a.n_out, a.raw, hbase, a.n_out, lane & 15);
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const H2 v2 = __builtin_bit_cast(H2, u[p]);
            acc[j][k][2 * p] = __builtin_fmaf(pw[j], (float)v2.x, acc[j][k][2 * p]);
            acc[j][k][2 * p + 1] = __builtin_fmaf(pw[j], (float)v2.y, acc[j][k][2 * p + 1]);
          }
        }
      } else if constexpr (kB) {
        RowParams rv;
        rv.scale = __uint_as_float(pv[k] << 16);
        rv.zp = __uint_as_float(pv[k] & 0xffff0000u);
        float vc[8];
        unpack8<W>(xv[k], vc);
        uint32_t u[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) u[p] = __builtin_bit_cast(uint32_t, dequant_bf2(vc[2 * p], vc[2 * p + 1], rv));
        patch16<DT>(u, pt[1][k], wv[k], a.idx + (H + hl[k]) * a.n_out, a.raw, hbase, a.n_out, lane & 15);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const B2 vb = __builtin_bit_cast(B2, u[p]);
          const float v0 = bf_lo(vb), v1 = bf_hi(vb);
#pragma unroll
          for (int j = 0; j < GQ; ++j) {
            acc[j][k][2 * p] = __builtin_fmaf(pw[j], v0, acc[j][k][2 * p]);
            acc[j][k][2 * p + 1] = __builtin_fmaf(pw[j], v1, acc[j][k][2 * p + 1]);
          }
        }
      } else {
        RowParams rv;
        rv.scale = pv[k].x;
        rv.zp = pv[k].y;
        float vf[8];
        unpack8<W>(xv[k], vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) vf[e] = dequant<DT>(vf[e], rv);
        patch32(vf, pt[1][k], wv[k], a.idx + (H + hl[k]) * a.n_out, a.raw, hbase, a.n_out, lane & 15);
#pragma unroll
        for (int j = 0; j < GQ; ++j) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j][k][e] = __builtin_fmaf(pw[j], vf[e], acc[j][k][e]);
        }
      }
    }
  };
  // Rows of this wave: r0 + wave + kDW·t.  Metadata of 64 rows at a time, one row per lane (kept index
  // and byte offset, then the token's class → width); the rows of each width are then taken together
  // (ballot), so the code loads have the width's exact size and PD rows stay in flight.
  for (int64_t jb = r0 + wave; jb < r1; jb += 64 * kDW) {
    const int64_t jrl = jb + (int64_t)kDW * lane;
    const bool ok = jrl < r1;
    const int ki = ok ? a.kept_index[jrl] : -1;
    const int64_t off = ok ? a.row_offset[jrl] : -1;
    const bool inS = ki >= 0 && (int64_t)ki < a.S;
    const int lab = inS ? (int)a.labels[ki] : 0;
    const int w = lab == 1 ? a.bits[1] : (lab == 2 ? a.bits[2] : a.bits[0]);
    // a row outside the token range or the code buffer is skipped, not read
    const int wl = (inS && off >= 0 && off + (int64_t)(F / 8) * w <= a.codes_capacity) ? w : 0;
    const uint32_t off_lo = (uint32_t)off, off_hi = (uint32_t)((uint64_t)off >> 32);
    auto by_width = [&](auto wtag) {
      constexpr int W = decltype(wtag)::value;
      // rows in flight: a row holds NCH·(W/2 + 4) VGPRs of codes, parameters and outlier values (16-bit
      // dtypes).  Measured at Hkv = Hq = 32 fp16 (NCH 2): 4 rows instead of 2 cost a wave per SIMD (185 VGPRs)
      // and 6 us per step; one chunk column per lane with 8 rows in flight (4 waves per SIMD) changed nothing.
      constexpr int PD = NCH == 1 ? (W <= 4 && GQ < 4 ? 8 : 4) : 2;
      uint64_t mask = __ballot(wl == W);
      const int n = __builtin_popcountll(mask);
      if (n == 0) return;
      int last = 0;
      auto next = [&]() {  // lane index of the next row of this width (the last one again at the end)
        if (mask) {
          last = __builtin_ctzll(mask);
          mask &= mask - 1;
        }
        return last;
      };
      // row t's codes, head parameters and first outlier values, through descriptors bounded to the row
      auto issue = [&](int t, ChunkCodes<W> (&xk)[NCH], ChunkCodes<W> (&xv)[NCH], GqMeta<DT> (&pk)[NCH],
                       GqMeta<DT> (&pv)[NCH], uint32_t (&wk)[NCH], uint32_t (&wv)[NCH]) {
        const int64_t o = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_hi, t) << 32) |
                                    (uint32_t)__builtin_amdgcn_readlane((int)off_lo, t));
        const int64_t jr = jb + (int64_t)kDW * t;
        const int nb = (F / 8) * W;
        const auto sk = __builtin_amdgcn_make_buffer_rsrc((void*)(a.codes_k + o), (short)0, nb, 0x00020000);
        const auto sv = __builtin_amdgcn_make_buffer_rsrc((void*)(a.codes_v + o), (short)0, nb, 0x00020000);
        const int mb = 2 * H * 2 * kE, rb = 2 * H * a.n_out * kE;
        const auto sm = __builtin_amdgcn_make_buffer_rsrc((void*)(static_cast<const uint8_t*>(a.meta) + jr * mb), (short)0,
                                                          mb, 0x00020000);
        const auto sr = __builtin_amdgcn_make_buffer_rsrc((void*)(static_cast<const uint8_t*>(a.raw) + jr * rb), (short)0,
                                                          rb, 0x00020000);
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
          const int vo = (c0 + k * 64 + lane) * W;
          xk[k] = load_codes<W>(sk, vo);
          xv[k] = load_codes<W>(sv, vo);
          pk[k] = load_meta<DT>(sm, hl[k] * 2 * kE);
          pv[k] = load_meta<DT>(sm, (H + hl[k]) * 2 * kE);
          wk[k] = load_raw<DT>(sr, pt[0][k].off0);
          wv[k] = load_raw<DT>(sr, pt[1][k].off0);
        }
      };
      ChunkCodes<W> bk[PD][NCH], bv[PD][NCH];
      GqMeta<DT> pk[PD][NCH], pv[PD][NCH];
      uint32_t wk[PD][NCH], wv[PD][NCH];
      int tl[PD];
#pragma unroll
      for (int i = 0; i < PD; ++i) {
        tl[i] = next();
        issue(tl[i], bk[i], bv[i], pk[i], pv[i], wk[i], wv[i]);
      }
      auto compute = [&](int i) { row(wtag, bk[i], bv[i], pk[i], pv[i], wk[i], wv[i], jb + (int64_t)kDW * tl[i]); };
      int base = 0;
      for (; base + PD <= n; base += PD) {  // full rounds: straight-line, each slot refilled
#pragma unroll
        for (int i = 0; i < PD; ++i) {
          compute(i);
          tl[i] = next();
          issue(tl[i], bk[i], bv[i], pk[i], pv[i], wk[i], wv[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < PD; ++i)  // the rest (< PD rows), already loaded
        if (base + i < n) compute(i);
    };
    by_width(std::integral_constant<int, 2>{});
    by_width(std::integral_constant<int, 4>{});
    by_width(std::integral_constant<int, 8>{});
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
  merge_waves_write_partial<DT, NCH, GQ>(a, lds, lane, gs, 0, s, c0, F, D, lph);
}

template <int DT>
int launch_gq_split(const GqSplitArgs& a, int nch, int gq, dim3 grid, size_t lds, hipStream_t st) {
#define RTKV_D(N, Q)                                                                           \
  if (nch == N && gq == Q) {                                                                   \
    hipLaunchKernelGGL((gq_split_kernel<DT, N, Q>), grid, dim3(64 * kDW), lds, st, a);        \
    RTKV_HIP_CHECK(hipGetLastError());                                                         \
    return RTKV_OK;                                                                            \
  }
  RTKV_D(1, 1) RTKV_D(2, 1) RTKV_D(1, 2) RTKV_D(1, 4)
#undef RTKV_D
  RTKV_REQUIRE(false, "gq decode: unsupported lane shape");
}

size_t gq_tail_workspace_bytes(int64_t Hq, int64_t Hkv, int64_t row_cap, int64_t tail_cap) {
  if (Hkv < 1 || Hq < Hkv) return 256;
  const int64_t G = Hq / Hkv, F = Hkv * kGqD;
  const int64_t sp = row_cap >= 1 ? decode_splits(1, G, F, row_cap) : 0;
  const int64_t stl = decode_splits(1, G, F, tail_cap);
  return (size_t)(G * (sp + stl)) * (size_t)(2 * Hkv + F) * sizeof(float) + 256;
}

}  // namespace

}  // namespace rtkv

using namespace rtkv;

extern "C" {

size_t rtkv_gq_decode_tail_workspace_size(int64_t Hq, int64_t Hkv, int64_t row_capacity, int64_t tail_capacity) {
  return gq_tail_workspace_bytes(Hq, Hkv, row_capacity, tail_capacity);
}

#define RTKV_GQD_REQUIRE(cond, msg) RTKV_REQUIRE(cond, "gq decode: " msg)

int rtkv_gq_decode_attention_tail(const rtkv_kv_desc* kv, const int32_t* kept_index_dev, const uint8_t* labels_dev,
                                  const rtkv_layer_stats* stats_dev, const int32_t bits[3], const rtkv_gq_params* g,
                                  const int16_t* outlier_idx_dev, const int64_t* row_offset_dev,
                                  const uint8_t* codes_k_dev, const uint8_t* codes_v_dev, int64_t codes_capacity,
                                  const void* meta_dev, const void* raw_dev, int64_t row_capacity, const void* q_dev,
                                  int64_t Hq, float scale, const rtkv_dense_tail* tail, float* out_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream) {
  // ---- everything is checked here, before any launch
  RTKV_GQD_REQUIRE(kv && g && bits, "null argument");
  RTKV_GQD_REQUIRE(kv->B == 1, "one batch row (B = 1)");
  RTKV_GQD_REQUIRE(kv->D == kGqD, "head_dim 128 (one group per head)");
  RTKV_GQD_REQUIRE(kv->stride_h == kv->D, "heads contiguous within a row ([B, S, H*D] layout)");
  RTKV_GQD_REQUIRE(kv->H >= 4 && kv->H % 4 == 0 && kv->H <= 64, "H a multiple of 4 up to 64");
  RTKV_GQD_REQUIRE(kv->dtype == RTKV_F32 || kv->dtype == RTKV_F16 || kv->dtype == RTKV_BF16, "unsupported dtype");
  RTKV_GQD_REQUIRE(kv->S >= 1, "S >= 1");
  RTKV_GQD_REQUIRE(g->n_outlier >= 0 && g->n_outlier <= kGqMaxOut, "n_outlier in [0, 16]");
  for (int c = 0; c < 3; ++c) RTKV_GQD_REQUIRE(bits[c] == 2 || bits[c] == 4 || bits[c] == 8, "class widths 2, 4 or 8 bits");
  const int64_t H = kv->H, F = H * kGqD;
  RTKV_GQD_REQUIRE(Hq >= H && Hq % H == 0, "Hq a multiple of Hkv");
  const int64_t G = Hq / H;
  const DecodeShape sh = decode_shape(F, G);
  RTKV_GQD_REQUIRE(sh.hg >= 1 && sh.gs >= 1 && sh.gq * sh.gs == G && (sh.gq == 1 || sh.nch == 1),
                   "GQA group size outside the lane shapes");
  RTKV_GQD_REQUIRE(q_dev && out_dev, "null q or out");
  RTKV_GQD_REQUIRE(((uintptr_t)q_dev & 15) == 0 && ((uintptr_t)out_dev & 3) == 0, "q must be 16-byte aligned, out 4-byte");
  RTKV_GQD_REQUIRE(row_capacity >= 0 && codes_capacity >= 0, "negative row or codes capacity");
  RTKV_GQD_REQUIRE(row_capacity * 2 * H * (g->n_outlier > 2 ? g->n_outlier : 2) < ((int64_t)1 << 29),
                   "meta / raw-value buffers beyond 2^31 bytes");
  if (row_capacity >= 1) {
    RTKV_GQD_REQUIRE(kept_index_dev && labels_dev && stats_dev && row_offset_dev && codes_k_dev && codes_v_dev && meta_dev,
                     "null layer pointer");
    RTKV_GQD_REQUIRE(g->n_outlier == 0 || (outlier_idx_dev && raw_dev), "null outlier index or raw-value buffer");
    RTKV_GQD_REQUIRE(((uintptr_t)meta_dev & 7) == 0 && ((uintptr_t)raw_dev & 3) == 0, "meta must be 8-byte aligned, raw 4-byte");
  }
  const int e = dtype_bytes(kv->dtype);
  const AttnChecks c = {"gq decode: ", RTKV_ERR_INVALID, 0u, 0, 1, false, 4};
  int rc;
  if ((rc = check_dense_tail(c, tail, F, e)) != RTKV_OK) return rc;
  if ((rc = check_workspace(c, workspace_dev, workspace_bytes,
                            gq_tail_workspace_bytes(Hq, H, row_capacity, tail->capacity))) != RTKV_OK)
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int sp = row_capacity >= 1 ? decode_splits(1, G, F, row_capacity) : 0;
  const int stl = decode_splits(1, G, F, tail->capacity);
  const DecodeParts parts = decode_parts(workspace_dev, 1, G, H, sp + stl);
  if (sp > 0) {
    GqSplitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.kept_index = kept_index_dev; a.labels = labels_dev; a.stats = stats_dev; a.row_offset = row_offset_dev;
    a.codes_k = codes_k_dev; a.codes_v = codes_v_dev; a.codes_capacity = codes_capacity;
    a.meta = meta_dev; a.raw = raw_dev; a.idx = outlier_idx_dev;
    a.S = kv->S; a.row_cap = row_capacity;
    for (int k = 0; k < 3; ++k) a.bits[k] = bits[k];
    a.n_out = g->n_outlier;
    a.Hkv = (int)H; a.G = (int)G;
    a.HG = sh.hg; a.GS = sh.gs;
    a.q = q_dev; a.scale = scale * 1.4426950408889634f;
    a.splits = sp;
    a.nrest = sp * a.HG;
    a.n = parts.n;
    a.part_m = parts.m; a.part_l = parts.l; a.part_acc = parts.acc;
    const int64_t nblk = ((int64_t)a.nrest + 7) / 8 * 8 * a.GS;
    RTKV_GQD_REQUIRE(nblk < (1ll << 31), "grid too large");
    const dim3 grid((unsigned)nblk);
    const size_t lds = (size_t)kDW * 64 * sh.nch * sh.gq * 10 * sizeof(float);
    if (kv->dtype == RTKV_F16) rc = launch_gq_split<RTKV_F16>(a, sh.nch, sh.gq, grid, lds, st);
    else if (kv->dtype == RTKV_BF16) rc = launch_gq_split<RTKV_BF16>(a, sh.nch, sh.gq, grid, lds, st);
    else rc = launch_gq_split<RTKV_F32>(a, sh.nch, sh.gq, grid, lds, st);
    if (rc != RTKV_OK) return rc;
  }
  if ((rc = launch_tail_splits(tail, kv->dtype, 1, H, kGqD, q_dev, Hq, scale, parts, sp, st)) != RTKV_OK) return rc;
  return launch_decode_merge(parts, 1, Hq, H, kGqD, out_dev, st);
}

#undef RTKV_GQD_REQUIRE

}  // extern "C"

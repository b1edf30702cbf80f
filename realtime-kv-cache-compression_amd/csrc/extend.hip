// extend.hip — attention of T new tokens per batch row over a layer's PACKED rows followed by the
// DENSE tail (rtkv_extend_attention_packed_tail): the multi-token form of decode_tail.hip.
//
// Reference: none that works (modified_llama.py:83-102 concatenates and then compresses again with a
// non-square attention matrix).  This is the plain causal attention a model computes over
// cat(cache, new tokens): the tail already holds the T new tokens as its last T rows, query t sees
// every packed row and the tail rows u < vis(b, t) = max(0, n_b − (T − 1 − t)).
//
// Work decomposition: one workgroup of 4 waves per (split, pass of ≤ 16·NQT query rows, kv head,
// batch row).  The G·T query rows of a kv head are ordered (g, t) and cut into passes, so every GQA
// head and every new token shares each decoded key tile.  The splits are one list: first the sp
// splits of the packed rows, then the st splits of the tail rows.  Each wave owns a contiguous
// quarter of its split's rows and keeps its own (m, l, Oᵀ); there is no workgroup barrier in the
// main loop.  A wave fills a private LDS image of 32 keys — K rows and V rows, row-major, 128
// elements each — and then runs one MFMA step over it:
//   Sᵀ = K·Qᵀ   v_mfma_f32_16x16x32: A = 16 keys × 32 d from the K image (ds_read_b128), B = 8
//               contiguous elements of a query row, loaded once from global.  Lane (g4, c16) then
//               holds the logits of keys 4·g4 + r of each 16-key tile for query column c16.
//   Oᵀ += Vᵀ·Pᵀ the two 16-key tiles of P, rounded to the dtype, are the B fragment as they stand
//               (k index 8·g4 + e ↔ key 4·g4 + e of tile 0 for e < 4, of tile 1 for e ≥ 4); Vᵀ in
//               the same k order comes from the row-major V image with two ds_read_b64_tr_b16.
// Packed rows are decoded with the helpers of decode_kernel.h, element for element dequant<DT>.
// Their order inside a tile does not matter (all are visible to every query), so the rows of one
// field width are taken together, four rows per wave instruction (one per 16-lane group, a lane per
// 8-element chunk of the kv head).  Tail rows are copied as stored, in order; the causal limit is a
// compare on the slot index.  The row sum l stays fp32 from the unrounded exponentials; the running
// max is raised lazily (slack 8).  The 4 waves merge through LDS at the end, one query tile at a
// time, and write (m, l, acc[D]) per (b, query head, t, split); extend_merge_kernel combines the
// splits with the arithmetic of decode_merge_kernel (decode.hip).
//
// Bounds: B·Hkv·passes·splits < 2^31 workgroups and B·Hq·T < 2^29 query rows.
#include "decode_kernel.h"

namespace rtkv {

namespace {

typedef _Float16 xf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 xbf16x8 __attribute__((ext_vector_type(8)));
typedef short xs16x4 __attribute__((ext_vector_type(4)));
typedef float xf32x4 __attribute__((ext_vector_type(4)));

template <int DT> struct XFrag;
template <> struct XFrag<RTKV_F16> {
  using T = xf16x8;
  __device__ __forceinline__ static xf32x4 mfma(T a, T b, xf32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  __device__ __forceinline__ static T round8(const float (&p)[8]) {
    T r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (_Float16)p[e];
    return r;
  }
};
template <> struct XFrag<RTKV_BF16> {
  using T = xbf16x8;
  __device__ __forceinline__ static xf32x4 mfma(T a, T b, xf32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  __device__ __forceinline__ static T round8(const float (&p)[8]) {
    T r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (__bf16)p[e];
    return r;
  }
};

constexpr int kXD = 128;         // head_dim
constexpr int kXKeys = 32;       // keys per wave step
constexpr int kXKPitch = 272;    // bytes per K image row: 16 rows of one ds_read_b128 fall on distinct banks
constexpr int kXVPitch = 288;    // bytes per V image row: the 8 rows × 4 pieces of a transposed read likewise
constexpr int kXWaveLds = kXKeys * (kXKPitch + kXVPitch);  // 17920 bytes per wave
constexpr int kXMergeFloats = 32 + 32 * 64;                // m[16], l[16], O[8][4][64] of one query tile
static_assert(kXMergeFloats * 4 <= kXWaveLds, "the merge image lives in the wave's key image");
constexpr float kXFloor = -1e30f;  // initial running max (finite: exp2(-inf − m) stays 0, never NaN)
constexpr int kXTargetWgs = 1024;
constexpr int kXMinRows = 128;     // rows per split at least: one 32-key tile per wave
constexpr int kXPassMax = 32;      // query rows per pass at most (NQT = 2: 252 VGPRs; NQT = 4 spills)

struct ExtendArgs {
  PackedRows pk;
  const void* tk;             // tail: element (b, u, h, d) at b·tsb + u·tss + h·D + d
  const void* tv;
  const int64_t* trows;       // [B]
  int64_t tcap, tsb, tss;
  int Hkv, G, T;
  int npass, sp, st;          // passes of 16·NQT query rows; packed splits, then tail splits
  const void* q;              // element (b, h, t, d) at b·qsb + h·qsh + t·qst + d
  int64_t qsb, qsh, qst;
  float scale;                // · log2(e)
  float* part_ml;             // [B·Hq·T][sp + st][2]
  float* part_acc;            // [B·Hq·T][sp + st][D]
  float* out;                 // [B, Hq, T, D]
};

// one decoded chunk (8 elements of the dtype, in element order)
template <int DT, int W>
__device__ __forceinline__ uint4 decode_chunk(const ChunkCodes<W>& x, float scale, float zp) {
  uint32_t o[4];
  if constexpr (DT == RTKV_F16) {
    const H2 zp2 = {(_Float16)zp, (_Float16)zp}, sc2 = {(_Float16)scale, (_Float16)scale};
    H2 h[4];
    codes_h2<W>(x, h);
    uint32_t u[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) u[p] = __builtin_bit_cast(uint32_t, (h[p] - zp2) * sc2);  // elements (p, p + 4)
    o[0] = (u[0] & 0xffffu) | (u[1] << 16);
    o[1] = (u[2] & 0xffffu) | (u[3] << 16);
    o[2] = (u[0] >> 16) | (u[1] & 0xffff0000u);
    o[3] = (u[2] >> 16) | (u[3] & 0xffff0000u);
  } else {
    RowParams rp;
    rp.scale = scale;
    rp.zp = zp;
    float c[8];
    unpack8<W>(x, c);
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = __builtin_bit_cast(uint32_t, dequant_bf2(c[2 * p], c[2 * p + 1], rp));
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// the W code bytes of one chunk with plain loads (W-byte aligned: rows start at multiples of 128 bytes)
template <int W>
__device__ __forceinline__ ChunkCodes<W> load_codes_global(const uint8_t* p) {
  ChunkCodes<W> c;
  if constexpr (W == 2) {
    c.r[0] = *reinterpret_cast<const uint16_t*>(p);
  } else if constexpr (W == 4) {
    c.r[0] = *reinterpret_cast<const uint32_t*>(p);
  } else if constexpr (W == 8) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    c.r[0] = v.x; c.r[1] = v.y;
  } else {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    c.r[0] = v.x; c.r[1] = v.y; c.r[2] = v.z; c.r[3] = v.w;
  }
  return c;
}

template <int DT, int NQT>
__global__ __launch_bounds__(64 * kDW, 2) void extend_split_kernel(ExtendArgs a) {
  using Fr = XFrag<DT>;
  using FT = typename Fr::T;
  extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g4 = lane >> 4, c16 = lane & 15;
  unsigned char* kimg = xlds + (size_t)wave * kXWaveLds;
  unsigned char* vimg = kimg + kXKeys * kXKPitch;
  const int nsplit = a.sp + a.st;
  int id = blockIdx.x;
  const int s = id % nsplit;
  id /= nsplit;
  const int pass = id % a.npass;
  id /= a.npass;
  const int hk = id % a.Hkv, b = id / a.Hkv;
  const int T = a.T, GT = a.G * T;
  const int qr0 = pass * 16 * NQT;
  const int Hq = a.Hkv * a.G;
  const int64_t n_b = a.trows[b] < a.tcap ? (a.trows[b] > 0 ? a.trows[b] : 0) : a.tcap;

  // ---- the query fragments (B operand of Sᵀ = K·Qᵀ) and each column's tail visibility
  FT qf[NQT][4];
  int vis[NQT];       // tail rows this lane's query column sees
  int64_t prow[NQT];  // (b, hq, t) row of the partials, −1 for a column past G·T
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    const int qr = qr0 + qt * 16 + c16;
    const bool ok = qr < GT;
    const int g = ok ? qr / T : 0, t = ok ? qr - g * T : 0;
    const int hq = hk * a.G + g;
    const uint16_t* qp = static_cast<const uint16_t*>(a.q) + (int64_t)b * a.qsb + (int64_t)hq * a.qsh + (int64_t)t * a.qst;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (ok) v = *reinterpret_cast<const uint4*>(qp + kk * 32 + g4 * 8);
      qf[qt][kk] = __builtin_bit_cast(FT, v);
    }
    const int64_t vv = n_b - (T - 1 - t);
    vis[qt] = ok ? (int)(vv > 0 ? vv : 0) : 0;
    prow[qt] = ok ? ((int64_t)b * Hq + hq) * T + t : -1;
  }
  // the largest t of this pass (wave-uniform): tail rows at or past its visibility are skipped
  const int qlast = (qr0 + 16 * NQT < GT ? qr0 + 16 * NQT : GT) - 1;
  const int tmax = qr0 / T != qlast / T ? T - 1 : qlast % T;
  const int64_t vmax0 = n_b - (T - 1 - tmax);
  const int64_t vismax = vmax0 > 0 ? vmax0 : 0;

  xf32x4 O[NQT][8];
  float m[NQT], l[NQT];
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) O[qt][dt] = xf32x4{0.f, 0.f, 0.f, 0.f};
    m[qt] = kXFloor;
    l[qt] = 0.f;
  }
  const float qscale = a.scale;

  // this lane's addresses in the images: its 16-byte chunk of key slot g4 (+ 4 per round), its row
  // read of the K operand, its piece of the transposed V read
  unsigned char* kst = kimg + g4 * kXKPitch + c16 * 16;
  unsigned char* vst = vimg + g4 * kXVPitch + c16 * 16;
  const unsigned char* krd = kimg + c16 * kXKPitch + g4 * 16;
  const unsigned char* vrd = vimg + (4 * g4 + (c16 >> 2)) * kXVPitch + (c16 & 3) * 8;
  auto store_slot = [&](int slot0, uint4 k8, uint4 v8) {  // key slot slot0 + g4
    *reinterpret_cast<uint4*>(kst + slot0 * kXKPitch) = k8;
    *reinterpret_cast<uint4*>(vst + slot0 * kXVPitch) = v8;
  };

  // One MFMA step over the wave's 32-key image; lim[qt] = key slots this lane's query column sees.
  // Every lane takes part (the transposed reads need EXEC all ones).
  auto step = [&](const int (&lim)[NQT]) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    FT ka[2][4];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        ka[kt][kk] = *reinterpret_cast<const FT*>(krd + kt * 16 * kXKPitch + kk * 64);
    float sc[NQT][8];
    bool up = false;
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        xf32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = Fr::mfma(ka[kt][kk], qf[qt][kk], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int slot = kt * 16 + 4 * g4 + r;
          const float v = slot < lim[qt] ? acc[r] * qscale : -INFINITY;
          sc[qt][kt * 4 + r] = v;
          up |= v > m[qt] + kSlack;
        }
      }
    }
    if (__ballot(up)) {  // lazily raised reference: weights stay ≤ 2^kSlack
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        float cm = sc[qt][0];
#pragma unroll
        for (int e = 1; e < 8; ++e) cm = fmaxf(cm, sc[qt][e]);
        cm = fmaxf(cm, __shfl_xor(cm, 16, kWave));
        cm = fmaxf(cm, __shfl_xor(cm, 32, kWave));
        const float mn = cm > m[qt] + kSlack ? cm : m[qt];
        const float cr = __builtin_amdgcn_exp2f(m[qt] - mn);
        l[qt] *= cr;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) O[qt][dt] *= cr;
        m[qt] = mn;
      }
    }
    FT pb[NQT];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      float p[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        p[e] = __builtin_amdgcn_exp2f(sc[qt][e] - m[qt]);
        l[qt] += p[e];
      }
      pb[qt] = Fr::round8(p);
    }
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      typedef __attribute__((address_space(3))) xs16x4 lds_s16x4;
      const xs16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vrd + dt * 32));
      const xs16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vrd + 16 * kXVPitch + dt * 32));
      const uint4 vw = make_uint4(__builtin_bit_cast(uint2, v0).x, __builtin_bit_cast(uint2, v0).y,
                                  __builtin_bit_cast(uint2, v1).x, __builtin_bit_cast(uint2, v1).y);
      const FT va = __builtin_bit_cast(FT, vw);
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) O[qt][dt] = Fr::mfma(va, pb[qt], O[qt][dt]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

  if (s < a.sp) {
    // ---------------------------------------------------------------- packed rows of split s
    const int64_t nrows = a.pk.rows[b] < a.pk.cap ? (a.pk.rows[b] > 0 ? a.pk.rows[b] : 0) : a.pk.cap;
    const int64_t per = (nrows + a.sp - 1) / a.sp;
    const int64_t r0 = (int64_t)s * per, r1 = r0 + per < nrows ? r0 + per : nrows;
    const int64_t pw = r1 > r0 ? (r1 - r0 + kDW - 1) / kDW : 0;
    const int64_t w0 = r0 + wave * pw, w1 = w0 + pw < r1 ? w0 + pw : r1;
    const int64_t bcap = (int64_t)b * a.pk.cap;
    const int F = a.Hkv * kXD;
    int fill = 0;  // key slots of the image in use (wave-uniform)
    for (int64_t jb = w0; jb < w1; jb += 64) {
      const int64_t jr = jb + lane;
      const bool ok = jr < w1;
      const int64_t rj = bcap + (ok ? jr : jb);
      const int64_t off = a.pk.row_offset[rj];
      const int64_t offn = (ok && jr + 1 < nrows) ? a.pk.row_offset[rj + 1] : -1;
      const float4 sz = *reinterpret_cast<const float4*>(a.pk.scale_zp + rj * 4);
      // a row's width from its byte span (rows are back to back); the list's last row from its class
      int wl = 0;
      {
        const int64_t span = offn - off;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (span == (int64_t)(F / 8) * a.pk.w[c]) wl = a.pk.w[c];
        if (ok && jr + 1 == nrows) {
          const int ki0 = a.pk.kept_index[rj];
          const int ki = ki0 < 0 ? 0 : (ki0 >= a.pk.S ? (int)a.pk.S - 1 : ki0);
          const int lab = a.pk.labels[(int64_t)b * a.pk.S + ki];
          wl = lab == 2 ? a.pk.w[2] : (lab == 1 ? a.pk.w[1] : a.pk.w[0]);
        }
      }
      const uint32_t off_lo = (uint32_t)off, off_hi = (uint32_t)(off >> 32);
      auto by_width = [&](auto wtag) {
        constexpr int W = decltype(wtag)::value;
        constexpr int PD = W == 16 ? 4 : 8;  // rounds of 4 rows whose codes are in flight together
        uint64_t mask = __ballot(ok && wl == W);
        while (mask) {
          ChunkCodes<W> xk[PD], xv[PD];
          float ksc[PD], kzp[PD], vsc[PD], vzp[PD];
          bool mine[PD];
          int slot0[PD];
          int f = fill;
#pragma unroll
          for (int i = 0; i < PD; ++i) {
            int cnt = __builtin_popcountll(mask);
            cnt = cnt < 4 ? cnt : 4;
            cnt = cnt < kXKeys - f ? cnt : kXKeys - f;
            int src = 0;  // the lane that holds this 16-lane group's row
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              if (g < cnt) {
                const int t = __builtin_ctzll(mask);
                mask &= mask - 1;
                if (g4 == g) src = t;
              }
            }
            mine[i] = g4 < cnt;
            slot0[i] = f;
            f += cnt;
            const uint32_t lo = (uint32_t)__shfl((int)off_lo, src, kWave), hi = (uint32_t)__shfl((int)off_hi, src, kWave);
            ksc[i] = __shfl(sz.x, src, kWave);
            kzp[i] = __shfl(sz.y, src, kWave);
            vsc[i] = __shfl(sz.z, src, kWave);
            vzp[i] = __shfl(sz.w, src, kWave);
            const int64_t o = (int64_t)(((uint64_t)hi << 32) | lo);
            const int64_t nbr = (int64_t)(F / 8) * W;
            const bool inb = mine[i] && o >= 0 && o + nbr <= a.pk.codes_bytes;  // out of range: zero codes
            xk[i] = ChunkCodes<W>{};
            xv[i] = ChunkCodes<W>{};
            if (inb) {
              const int64_t bo = o + (int64_t)(hk * 16 + c16) * W;
              xk[i] = load_codes_global<W>(a.pk.codes_k + bo);
              xv[i] = load_codes_global<W>(a.pk.codes_v + bo);
            }
          }
#pragma unroll
          for (int i = 0; i < PD; ++i) {
            if (mine[i])
              store_slot(slot0[i], decode_chunk<DT, W>(xk[i], ksc[i], kzp[i]), decode_chunk<DT, W>(xv[i], vsc[i], vzp[i]));
          }
          fill = f;
          if (fill == kXKeys) {
            int lim[NQT];
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) lim[qt] = kXKeys;
            step(lim);
            fill = 0;
          }
        }
      };
      by_width(std::integral_constant<int, 2>{});
      by_width(std::integral_constant<int, 4>{});
      by_width(std::integral_constant<int, 8>{});
      by_width(std::integral_constant<int, 16>{});
    }
    if (fill > 0) {  // the last, partial image: zero rows behind the filled slots
#pragma unroll
      for (int i = 0; i < kXKeys / 4; ++i)
        if (i * 4 + g4 >= fill) store_slot(i * 4, zero4, zero4);
      int lim[NQT];
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) lim[qt] = fill;
      step(lim);
    }
  } else {
    // ---------------------------------------------------------------- tail rows of split s − sp
    const int ts = s - a.sp;
    const int64_t per = (n_b + a.st - 1) / a.st;
    const int64_t r0 = (int64_t)ts * per, r1 = r0 + per < n_b ? r0 + per : n_b;
    const int64_t pw0 = r1 > r0 ? (r1 - r0 + kDW - 1) / kDW : 0;
    const int64_t pw = (pw0 + kXKeys - 1) / kXKeys * kXKeys;  // whole images per wave
    const int64_t w0 = r0 + wave * pw;
    int64_t w1 = w0 + pw < r1 ? w0 + pw : r1;
    if (w1 > vismax) w1 = vismax;  // no query of this pass sees further
    const uint16_t* tk = static_cast<const uint16_t*>(a.tk) + (int64_t)b * a.tsb + hk * kXD + c16 * 8;
    const uint16_t* tv = static_cast<const uint16_t*>(a.tv) + (int64_t)b * a.tsb + hk * kXD + c16 * 8;
    for (int64_t u0 = w0; u0 < w1; u0 += kXKeys) {
      uint4 k8[kXKeys / 4], v8[kXKeys / 4];
#pragma unroll
      for (int i = 0; i < kXKeys / 4; ++i) {
        const int64_t u = u0 + i * 4 + g4;
        k8[i] = zero4;
        v8[i] = zero4;
        if (u < w1) {  // never read at or past the count
          k8[i] = *reinterpret_cast<const uint4*>(tk + u * a.tss);
          v8[i] = *reinterpret_cast<const uint4*>(tv + u * a.tss);
        }
      }
#pragma unroll
      for (int i = 0; i < kXKeys / 4; ++i) store_slot(i * 4, k8[i], v8[i]);
      int lim[NQT];
      const int64_t have = w1 - u0;  // rows of this image (the rest are zeros)
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        const int64_t lv = (int64_t)vis[qt] - u0;
        const int64_t lm = lv < have ? lv : have;
        lim[qt] = (int)(lm < 0 ? 0 : (lm > kXKeys ? kXKeys : lm));
      }
      step(lim);
    }
  }

  // ---- merge the 4 waves in LDS, one query tile at a time, and write this split's partials.
  // Wave w reads the images of all 4 waves for the d tiles 2w and 2w + 1.
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    float lt = l[qt];
    lt += __shfl_xor(lt, 16, kWave);
    lt += __shfl_xor(lt, 32, kWave);
    __syncthreads();  // every wave is past its last step (or the previous tile's reads)
    float* mine_f = reinterpret_cast<float*>(kimg);
    if (g4 == 0) {
      mine_f[c16] = m[qt];
      mine_f[16 + c16] = lt;
    }
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mine_f[32 + (dt * 4 + r) * 64 + lane] = O[qt][dt][r];
    __syncthreads();
    float mm = kXFloor;
    for (int v = 0; v < kDW; ++v) mm = fmaxf(mm, reinterpret_cast<const float*>(xlds + (size_t)v * kXWaveLds)[c16]);
    float ll = 0.f;
    xf32x4 aa[2] = {xf32x4{0.f, 0.f, 0.f, 0.f}, xf32x4{0.f, 0.f, 0.f, 0.f}};
    for (int v = 0; v < kDW; ++v) {
      const float* src = reinterpret_cast<const float*>(xlds + (size_t)v * kXWaveLds);
      const float f = __builtin_amdgcn_exp2f(src[c16] - mm);  // both at the floor (no key yet): 1 · zeros
      ll += f * src[16 + c16];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) aa[h][r] += f * src[32 + ((2 * wave + h) * 4 + r) * 64 + lane];
    }
    if (prow[qt] >= 0) {
      const bool none = mm <= kXFloor;
      const int64_t pi = prow[qt] * nsplit + s;
      if (wave == 0 && g4 == 0) {
        a.part_ml[pi * 2] = none ? -INFINITY : mm;
        a.part_ml[pi * 2 + 1] = none ? 0.f : ll;
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 o4 = none ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(aa[h][0], aa[h][1], aa[h][2], aa[h][3]);
        *reinterpret_cast<float4*>(a.part_acc + pi * kXD + (2 * wave + h) * 16 + 4 * g4) = o4;
      }
    }
  }
}

// One workgroup of D threads per (b, query head, t): the splits' (m, l, acc) into out, with the
// arithmetic of decode_merge_kernel (max, exp2 factors, num / den, zeros for no key).  The
// factors are computed once, a split per thread, and kept in LDS; thread d then sums its column.
__global__ __launch_bounds__(kXD) void extend_merge_kernel(ExtendArgs a) {
  __shared__ float w[kXTargetWgs + 1];
  __shared__ float rm[kXD / 64], rd[kXD / 64];
  const int64_t row = blockIdx.x;
  const int d = threadIdx.x, n = a.sp + a.st;
  const float* ml = a.part_ml + row * n * 2;
  const float* ac = a.part_acc + row * n * kXD + d;
  float mm = -INFINITY;
  for (int s = d; s < n; s += kXD) mm = fmaxf(mm, ml[2 * s]);
  mm = wave_max(mm);
  if ((d & 63) == 0) rm[d >> 6] = mm;
  __syncthreads();
  mm = fmaxf(rm[0], rm[1]);
  float den = 0.f;
  for (int s = d; s < n; s += kXD) {
    const float ms = ml[2 * s];
    const float fct = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - mm);
    w[s] = fct;
    den += fct * ml[2 * s + 1];
  }
  den = wave_sum(den);
  if ((d & 63) == 0) rd[d >> 6] = den;
  __syncthreads();
  den = rd[0] + rd[1];
  float num = 0.f;
#pragma unroll 8
  for (int s = 0; s < n; ++s) num += w[s] * ac[(int64_t)s * kXD];
  a.out[row * kXD + d] = den > 0.f ? num / den : 0.f;
}

template <int DT, int NQT>
int launch_extend_split(const ExtendArgs& a, dim3 grid, hipStream_t st) {
  constexpr size_t lds = (size_t)kDW * kXWaveLds;  // 71680 bytes: above the 64 KiB a kernel gets unasked
  static bool attr = false;                        // per instantiation
  if (!attr) {
    RTKV_HIP_CHECK(hipFuncSetAttribute((const void*)extend_split_kernel<DT, NQT>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL((extend_split_kernel<DT, NQT>), grid, dim3(64 * kDW), lds, st, a);
  RTKV_HIP_CHECK(hipGetLastError());
  return RTKV_OK;
}

struct ExtendPlan {
  int nqt, npass, sp, st;
};

// Splits from the capacities alone (no host synchronisation): at least kXMinRows rows per split, at most
// kXTargetWgs workgroups, shared between the packed rows and the tail in proportion to their capacities.
ExtendPlan extend_plan(int64_t B, int64_t Hkv, int64_t G, int64_t T, int64_t cap, int64_t tcap) {
  ExtendPlan p;
  const int64_t gt = G * T;
  p.nqt = gt <= 16 ? 1 : 2;
  p.npass = (int)((gt + 16 * p.nqt - 1) / (16 * p.nqt));
  int64_t sp = (cap + kXMinRows - 1) / kXMinRows, st = (tcap + kXMinRows - 1) / kXMinRows;
  int64_t target = kXTargetWgs / (B * Hkv * p.npass);
  if (target < 1) target = 1;
  if (sp + st > target) {
    if (sp == 0) st = target;
    else if (st == 0) sp = target;
    else if (target < 2) { sp = 1; st = 1; }  // one of each: the two kinds of rows never share a split
    else {
      int64_t t2 = target * st / (sp + st);
      t2 = t2 < 1 ? 1 : (t2 > target - 1 ? target - 1 : t2);
      st = st < t2 ? st : t2;
      sp = sp < target - st ? sp : target - st;
    }
  }
  p.sp = (int)sp;
  p.st = (int)st;
  return p;
}

}  // namespace

// B·Hq·T·min(natural splits, max(1, target·32 / (Hq·T·B)) + 1) partials of 2 + D floats: an upper bound of
// what extend_plan uses that never decreases in T or in either capacity.
size_t extend_workspace_bytes(int64_t B, int64_t Hq, int64_t Hkv, int64_t D, int64_t T, int64_t cap, int64_t tcap) {
  const int64_t nq = B * Hq * T;
  const int64_t nat = (cap + kXMinRows - 1) / kXMinRows + (tcap + kXMinRows - 1) / kXMinRows;
  int64_t lim = nq > (int64_t)kXTargetWgs * kXPassMax ? nq : (int64_t)kXTargetWgs * kXPassMax;
  lim += nq;  // the "one of each" case of extend_plan
  const int64_t parts = nq * nat < lim ? nq * nat : lim;
  return (size_t)parts * (size_t)(2 + D) * sizeof(float) + 256;
}

int launch_extend(PackedLayer& p, const void* q, int64_t qsb, int64_t qsh, int64_t qst, int64_t Hq, int64_t T,
                  float scale, const rtkv_dense_tail* tail, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
  // refusals of the kernel's envelope are RTKV_ERR_UNSUPPORTED, and come after every RTKV_ERR_INVALID
  // check of the query, the tail and the workspace
  const AttnChecks c = {"extend: ", RTKV_ERR_UNSUPPORTED, 1u << RTKV_F16 | 1u << RTKV_BF16, kXD, INT64_MAX, false, 16};
  int rc;
  if ((rc = check_attn_query(c, p, q, Hq, out)) != RTKV_OK) return rc;
  RTKV_REQUIRE(T >= 1, "extend: T must be at least 1");
  RTKV_REQUIRE(qsb % 8 == 0 && qsh % 8 == 0 && qst % 8 == 0 && qsb >= 0 && qsh >= 0 && qst >= 0,
               "extend: q and its strides must keep rows 16-byte aligned");
  const int64_t B = p.B, Hkv = p.Hkv, D = p.D, G = Hq / Hkv;
  if ((rc = check_dense_tail(c, tail, Hkv * D, 2)) != RTKV_OK) return rc;
  RTKV_REQUIRE(B * Hq * T < (1ll << 31) / 4, "extend: too many query rows");
  if ((rc = check_workspace(c, ws, ws_bytes, extend_workspace_bytes(B, Hq, Hkv, D, T, p.r.cap, tail->capacity))) != RTKV_OK)
    return rc;
  if ((rc = check_attn_shape(c, p)) != RTKV_OK) return rc;
  if ((rc = check_packed_layer(c, p)) != RTKV_OK) return rc;
  const ExtendPlan pl = extend_plan(B, Hkv, G, T, p.r.cap, tail->capacity);
  const int64_t nq = B * Hq * T;
  ExtendArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pk = p.r;
  a.tk = tail->k_dev; a.tv = tail->v_dev; a.trows = tail->rows_dev;
  a.tcap = tail->capacity; a.tsb = tail->stride_b; a.tss = tail->stride_s;
  a.Hkv = (int)Hkv; a.G = (int)G; a.T = (int)T;
  a.npass = pl.npass; a.sp = pl.sp; a.st = pl.st;
  a.q = q; a.qsb = qsb; a.qsh = qsh; a.qst = qst;
  a.scale = scale * 1.4426950408889634f;
  a.part_ml = static_cast<float*>(ws);
  a.part_acc = a.part_ml + (nq * (pl.sp + pl.st) * 2 + 3) / 4 * 4;
  a.out = out;
  const int nsplit = pl.sp + pl.st;
  RTKV_REQUIRE(nsplit <= kXTargetWgs, "extend: too many splits");
  if (nsplit > 0) {
    const int64_t nblk = B * Hkv * pl.npass * nsplit;
    RTKV_REQUIRE(nblk < (1ll << 31), "extend: grid too large");
    const dim3 grid((unsigned)nblk);
    if (p.dt == RTKV_F16) rc = pl.nqt == 1 ? launch_extend_split<RTKV_F16, 1>(a, grid, st) : launch_extend_split<RTKV_F16, 2>(a, grid, st);
    else rc = pl.nqt == 1 ? launch_extend_split<RTKV_BF16, 1>(a, grid, st) : launch_extend_split<RTKV_BF16, 2>(a, grid, st);
    if (rc != RTKV_OK) return rc;
  }
  hipLaunchKernelGGL(extend_merge_kernel, dim3((unsigned)nq), dim3(kXD), 0, st, a);
  RTKV_HIP_CHECK(hipGetLastError());
  return RTKV_OK;
}

}  // namespace rtkv

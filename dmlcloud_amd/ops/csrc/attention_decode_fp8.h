// FP8 (OCP e4m3, torch.float8_e4m3fn) K/V cache for ops.fused_attn.sdpa_kvcache
// and kvcache_append. Part of attention.hip (included at its end, inside
// namespace dmlamd, after attention_decode_d128.h and
// attention_kvcache_append.h); it uses the tiled decode kernels' helpers
// (thread_coords, vt_idx, read_tr_frag, Strides, StridesPaged, PageWalk,
// page_seek, PageTable, decode_len, decode_shfl, decode_barrier, the D = 64 and
// D = 128 combine / store functions and BOTH existing merge kernels).
//   attn_decode_fp8_kernel<kD, kPaged>  split-KV forward, any R = (H/Hkv)*Nq >= 1
//   kvcache_append_fp8_kernel<kD>       quantising append, dense or paged
//
// Semantics. k_cache / v_cache hold e4m3 bytes, dense [B, Hkv, Nmax, D] or page
// pools [num_pages, Hkv, page_size, D], D = 64 or 128; q and the appended rows
// are bf16. k_scale / v_scale are fp32 [Hkv] in device memory (a null pointer
// is all ones), read by the kernels: no host sync, capturable, and they may
// change between replays. Key row j of K/V head h IS
// float(k_cache[.., h, j, :]) * k_scale[h] (V alike). Everything else is the
// contract of attention_decode_d128.h: decode_len() clamps kv_len, causal
// masking is bottom-right aligned, rows >= len are never LOADED (0x7F and 0xFF
// are NaN, and P = 0 times NaN is NaN in the MFMA), no atomics, bitwise
// repeatable per (shape, S), forward only. An appended element x is stored as
//   e4m3_rne(clamp(float(x) / scale[h], -448, 448)),
// a true fp32 division and an fp32 clamp in front of the conversion, so the
// result saturates whatever the conversion's overflow mode is.
//
// Why the bf16 MFMAs stay. Every finite e4m3 value is a bf16 value, so
// dequantising a byte to bf16 is exact, and a kernel that does it in registers
// and keeps the bf16 MFMAs, the fp32 softmax and the fp32 accumulators has the
// bf16 kernels' error against an oracle over the dequantised cache. The scales
// never touch a K or V element: k_scale[kvh] is wave-uniform and is folded
// into the softmax scale, v_scale[kvh] multiplies the wave's fp32 O once,
// after the key loop (linear, so block epilogue and merge are unchanged).
//
// The attention kernel keeps, word for word, the tiled kernels' role scheme
// (T in {1, 2, 4} column tiles x P = 4 / T key phases), the lim_max causal
// skip, the per-wave (m, l, O), the barrier-free key loop, the block epilogue
// and the partial layout; see attention_decode_d128.h for those arguments,
// which are not repeated here. New is how 8-bit rows move:
//   * K. A key row is kD bytes, and a lane's 16-byte load holds 16 consecutive
//     d: TWO bf16 A fragments, two MFMA k-steps from one load. Per 16-key half
//     a lane loads K[key][64l + 16(lane/16) .. +15] for l < kD / 64 (one load
//     at D = 64, two at D = 128) and converts its low 8 bytes to the fragment
//     of step j = 0, its high 8 bytes to that of j = 1. The contraction over d
//     may visit d in any order as long as both operands agree, so Q's B
//     fragments are loaded once per block in the same order: qf[l][j] =
//     Q[col][64l + 16(lane/16) + 8j .. +7]. No LDS, no shuffles.
//   * V. A 32-key tile is 32 x kD bytes: kD / 32 16-byte pieces per lane, kD /
//     16 lanes per row. A piece is 16 consecutive d of one row, which is one
//     contiguous 32-byte run of a vt_idx image (col & 15 is the index's lowest
//     term), so the piece is converted in registers and written as two b128
//     stores into the SAME bf16 images the bf16 kernels build; read_tr_frag and
//     the P V loop stand as they are. The alternative, byte images and an
//     8-bit transposed LDS read, would halve the LDS but needs a new image
//     layout and a conversion behind every transposed read, i.e. once per
//     (tile, D chunk) fragment in the MFMA's operand path; converting once in
//     front of LDS keeps the proven read side and the conversion off it.
//   * Conversion: v_cvt_pk_f32_fp8 gives two f32 per 16 bits; the bf16 is the
//     f32's high half (exact, no rounding code), packed pairwise.
//   * Prefetch, K before V, as in the bf16 kernels: the next tile's raw bytes
//     stay in flight through this tile's math. Per lane that is four 16-byte
//     loads at D = 64 and eight at D = 128, half of the bf16 kernels'.
//   * Paged: as in the bf16 kernels (page_size % 32 == 0, one tile in one page,
//     the entry read through the constant address space a round ahead, clamped
//     to the pool). Every key row a lane reads is clamped to len - 1.
//
// Register and LDS budget, counted before the loop was written. D = 128: raw K
// of the current and the next tile 2 x 16 VGPRs, raw V pieces 16, O 32, Q 16,
// one converted K fragment pair 8 and one converted V piece 8 at a time: ~100
// with scores, addresses and softmax state, well under the bf16 D = 128
// kernel's 170..190. D = 64: 2 x 8 + 8 + 16 + 8 + 8: ~70. LDS is what the bf16
// kernels use (the images are bf16): 37888 B per block at D = 64, 70656 B at
// D = 128. Occupancy is left to the compiler; its verdict (D = 64: 94 VGPRs +
// 16 AGPRs, 4 waves/SIMD; D = 128: 138 + 32, 2 waves/SIMD, the LDS bound) and
// the absence of scratch are recorded in profiles/attention_decode_fp8.txt.
#pragma once

typedef int fp8_i32x4 __attribute__((ext_vector_type(4)));
typedef int fp8_i32x2 __attribute__((ext_vector_type(2)));
typedef float fp8_f32x2 __attribute__((ext_vector_type(2)));

// The per-head-dim pieces the kernel borrows from the bf16 kernels.
template <int kD>
struct DecodeFp8Types;
template <>
struct DecodeFp8Types<kAttnD> {
  using WaveLds = DecodeWaveLds;
  using Acc = DecodeAcc;
};
template <>
struct DecodeFp8Types<kAttnD128> {
  using WaveLds = Decode128WaveLds;
  using Acc = Decode128Acc;
};

// Eight e4m3 bytes (w0 holds the first four) as eight bf16, exactly.
kDecodeFn __device__ __forceinline__ bf16x8 fp8x8_to_bf16(int w0, int w1) {
  unsigned r[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int w = i == 0 ? w0 : w1;
    const fp8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false); // bytes 0, 1
    const fp8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true); // bytes 2, 3
    // The elements go through named floats: __builtin_bit_cast applied to a
    // vector ELEMENT reads element 0 whatever the index (clang at hand).
    // v_perm_b32: bytes 2, 3 of the first f32 (selectors 2, 3: the second
    // operand) below bytes 2, 3 of the second f32 (selectors 6, 7: the first)
    const float f0 = lo[0], f1 = lo[1], f2 = hi[0], f3 = hi[1];
    r[2 * i] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, f1),
                                     __builtin_bit_cast(unsigned, f0), 0x07060302u);
    r[2 * i + 1] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, f3),
                                         __builtin_bit_cast(unsigned, f2), 0x07060302u);
  }
  bf16x8 f;
  __builtin_memcpy(&f, r, 16);
  return f;
}

// page_bases() of attention.hip for byte pools.
kDecodeFn __device__ __forceinline__ void page_bases_fp8(int entry, int key_lo, int kvh,
                                                         const uint8_t* k, const uint8_t* v,
                                                         const StridesPaged<true>& sk,
                                                         const Strides& sv, const uint8_t*& kt,
                                                         const uint8_t*& vt) {
  const int64_t page = min(max(entry, 0), sk.num_pages - 1);
  kt = k + page * sk.b + (int64_t)kvh * sk.h - (int64_t)key_lo * sk.r;
  vt = v + page * sv.b + (int64_t)kvh * sv.h - (int64_t)key_lo * sv.r;
}

template <int kD, bool kPaged>
kDecodeFn __global__ void __launch_bounds__(kAttnThreads) attn_decode_fp8_kernel(
    const __hip_bfloat16* __restrict__ q, const uint8_t* __restrict__ k,
    const uint8_t* __restrict__ v, const int* __restrict__ kv_len,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    __hip_bfloat16* __restrict__ o, float* __restrict__ lse, float* __restrict__ ws_o,
    float* __restrict__ ws_ml, int H, int G, int Nq, int Nmax, int S, int chunk, float scale,
    bool causal, Strides sq, StridesPaged<kPaged> sk, Strides sv) {
  static_assert(kD == kAttnD || kD == kAttnD128);
  constexpr int kHalves = kD / 64; // 64-wide d blocks: K loads per key row, V images per tile
  constexpr int kDChunks = kD / 16; // 16-wide O chunks
  constexpr int kVLanes = kD / 16; // lanes (16-byte pieces) of one V row
  constexpr int kVRows = kWave / kVLanes; // V rows one pass of the wave covers: 16 or 8
  constexpr int kVPieces = kKT / kVRows; // pieces per lane: 2 or 4
  constexpr int kPartO = kDecCols * kD, kPartML = kDecCols * 2;
  using WaveLds = typename DecodeFp8Types<kD>::WaveLds;
  constexpr int kWaveLdsFloats = sizeof(WaveLds) / sizeof(float);
  static_assert(sizeof(WaveLds) >= 2 * kHalves * kImgElems * sizeof(__bf16));
  __shared__ WaveLds wave_lds[kWavesPerBlock];
  __shared__ __hip_bfloat16 p_lds_all[kWavesPerBlock][kQT][kPStride];

  // plain ints, not a structured binding: the tile lambdas capture them
  const Coords tc = thread_coords();
  const int lane = tc.lane, row16 = tc.row16, grp = tc.grp;
  const int wave = __builtin_amdgcn_readfirstlane(tc.wave);
  __hip_bfloat16(*p_lds)[kPStride] = p_lds_all[wave];
  // image (kHalves * buffer + D half) of the wave at + that * kImgElems: the
  // `v` member of either union starts the union
  __hip_bfloat16* v_img = (__hip_bfloat16*)&wave_lds[wave];
  // V staging: lane l holds rows l / kVLanes + kVRows * x, d 16 * (l % kVLanes)..+15
  const int st_row = lane / kVLanes;
  const int st_col = (lane % kVLanes) * 16; // 0..kD-16
  const int st_half = st_col >> 6;

  // grid: (b, K/V head, tile group, split), split fastest
  const int Hkv = H / G;
  const int R = G * Nq;
  const int nt = (R + kDecCols - 1) / kDecCols;
  const int groups = (nt + kTileGroup - 1) / kTileGroup;
  const int s = blockIdx.x % S;
  const int tg = (blockIdx.x / S) % groups;
  const int kvh = (blockIdx.x / S / groups) % Hkv;
  const int b = blockIdx.x / S / groups / Hkv;
  const int len = decode_len(kv_len, b, Nq, Nmax, causal);

  // roles
  const int live = min(kTileGroup, nt - tg * kTileGroup); // 1..4
  const int T = live == 1 ? 1 : live == 2 ? 2 : 4;
  const int P = kWavesPerBlock / T;
  const int tile_in_group = wave % T, phase = wave / T;
  const int tile = tg * kTileGroup + tile_in_group; // >= nt: the idle role of live == 3

  // Which keys are walked: attention_decode_d128.h, word for word (split s
  // owns [s * chunk, (s + 1) * chunk); a dead split returns before the
  // barrier, block-uniform; lim_max; exactly-once; the wipe; the empty partial).
  const int k_begin = s * chunk;
  if (k_begin >= len) return;
  const int c0 = tile * kDecCols, c1 = min(c0 + kDecCols - 1, R - 1);
  int lim_max = len - 1;
  if (causal && (c1 + 1) / Nq == c0 / Nq) lim_max = len - Nq + (c1 - c0 / Nq * Nq);
  const int k_stop = tile < nt ? min(k_begin + chunk, lim_max + 1) : k_begin;

  // this lane's query column: Q B-fragments in K's d order, and the last key
  // it attends (the idle role's tile >= nt reads column R - 1 and walks nothing)
  const int col_q = min(c0 + row16, R - 1);
  const int g_q = col_q / Nq;
  const int i_q = col_q - g_q * Nq;
  const int lim = causal ? len - Nq + i_q : len - 1;
  const __hip_bfloat16* qp =
      q + (int64_t)b * sq.b + (int64_t)(kvh * G + g_q) * sq.h + (int64_t)i_q * sq.r;
  bf16x8 qf[kHalves][2];
#pragma unroll
  for (int l = 0; l < kHalves; ++l) {
#pragma unroll
    for (int j = 0; j < 2; ++j) qf[l][j] = *(const bf16x8*)(qp + 64 * l + 16 * grp + 8 * j);
  }

  const uint8_t* kp = k + (int64_t)b * sk.b + (int64_t)kvh * sk.h;
  const uint8_t* vp = v + (int64_t)b * sv.b + (int64_t)kvh * sv.h;
  // Raw K bytes [16-key half h][64-wide block l] and raw V pieces of the tile
  // at key0, every row clamped to len - 1; K before V, pinned (loads return in
  // order, so the wait in front of the V image writes also covers K). kt / vt:
  // the tile's page_bases_fp8() (paged); the dense code reads kp / vp.
  auto load_tile = [&](int key0, const uint8_t* kt, const uint8_t* vt,
                       fp8_i32x4(&kraw)[2][kHalves],
                       fp8_i32x4(&vpc)[kVPieces]) kDecodeFn __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t kr = min(key0 + 16 * h + row16, len - 1);
#pragma unroll
      for (int l = 0; l < kHalves; ++l) {
        kraw[h][l] = *(const fp8_i32x4*)((kPaged ? kt : kp) + kr * sk.r + 64 * l + 16 * grp);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int x = 0; x < kVPieces; ++x) {
      const int64_t vr = min(key0 + st_row + kVRows * x, len - 1);
      vpc[x] = *(const fp8_i32x4*)((kPaged ? vt : vp) + vr * sv.r + st_col);
    }
  };
  // convert a tile's pieces and write them into the images of buffer `buf`
  auto stage_v = [&](int buf, const fp8_i32x4(&vpc)[kVPieces]) kDecodeFn
      __attribute__((always_inline)) {
#pragma unroll
    for (int x = 0; x < kVPieces; ++x) {
      __hip_bfloat16* dst = v_img + (kHalves * buf + st_half) * kImgElems +
                            vt_idx(st_row + kVRows * x, st_col & 63);
      *(bf16x8*)dst = fp8x8_to_bf16(vpc[x][0], vpc[x][1]);
      *(bf16x8*)(dst + 8) = fp8x8_to_bf16(vpc[x][2], vpc[x][3]);
    }
  };

  // fold log2(e) (exp -> v_exp_f32) and the K head's scale into the scores
  const float scale2 = scale * kLog2e * (k_scale != nullptr ? k_scale[kvh] : 1.0f);
  float m_run = -1e30f, l_run = 0.0f;
  f32x4 o_acc[kDChunks];
#pragma unroll
  for (int db = 0; db < kDChunks; ++db) o_acc[db] = f32x4{0, 0, 0, 0};

  const int key_step = P * kKT;
  int key0 = k_begin + phase * kKT;
  bool have = key0 < k_stop;
  fp8_i32x4 kraw[2][kHalves], vpc[kVPieces];
  // Paged: a walked tile key0 < k_stop <= len lies in an allocated page, index
  // key0 / page_size <= (len - 1) / page_size < max_pages (len <= capacity),
  // so only table entries < ceil(len / page_size) are read. Its clamped rows
  // min(key0 + x, len - 1), x < 32, stay in [key0, key0 + 31]: the same
  // 32-aligned tile, hence the same page (page_size % 32 == 0), rows
  // 0..page_size-1 of a page id clamped into the pool. `walk` only ever
  // seeks to a tile that exists, so the entry it names is one of those.
  const uint8_t *kt = kp, *vt = vp; // paged: the current tile's bases
  [[maybe_unused]] PageWalk walk = {0, 0};
  [[maybe_unused]] int ent_next = 0, lo_next = 0; // the NEXT tile's entry and page start
  [[maybe_unused]] PageTable tbl = nullptr; // block_table[b]
  if constexpr (kPaged) {
    if (have) {
      tbl = (PageTable)(sk.table + (int64_t)b * sk.max_pages);
      walk.pg = key0 / sk.page_size;
      walk.key_lo = walk.pg * sk.page_size;
      page_bases_fp8(tbl[walk.pg], walk.key_lo, kvh, k, v, sk, sv, kt, vt);
      if (key0 + key_step < k_stop) page_seek(walk, key0 + key_step, sk.page_size);
      ent_next = tbl[walk.pg];
      lo_next = walk.key_lo;
    }
  }
  if (have) {
    load_tile(key0, kt, vt, kraw, vpc);
    stage_v(0, vpc);
  }
  int buf = 0;
  while (have) {
    // the next tile's loads stay in flight through this tile's math
    const int key_next = key0 + key_step;
    const bool has_next = key_next < k_stop;
    fp8_i32x4 kraw_next[2][kHalves];
    if constexpr (kPaged) page_bases_fp8(ent_next, lo_next, kvh, k, v, sk, sv, kt, vt);
    if (has_next) load_tile(key_next, kt, vt, kraw_next, vpc);
    if constexpr (kPaged) {
      // the entry of the tile after next, behind the loads just issued
      if (key_next + key_step < k_stop) page_seek(walk, key_next + key_step, sk.page_size);
      ent_next = tbl[walk.pg];
      lo_next = walk.key_lo;
    }

    // ---- S^T = K Q^T: rows = key (16h + 4grp + r), col = row16; each raw
    // load is two k-steps, d order [l][grp][j] on both operands ----
    float sc[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int l = 0; l < kHalves; ++l) {
        const bf16x8 k0 = fp8x8_to_bf16(kraw[h][l][0], kraw[h][l][1]);
        const bf16x8 k1 = fp8x8_to_bf16(kraw[h][l][2], kraw[h][l][3]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[l][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[l][1], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = acc[r] * scale2; // log2-domain score of the dequantised key
        // one compare against the lane's OWN lim: causal end, cache end and
        // clamped duplicates alike
        if (key0 + 16 * h + 4 * grp + r > lim) x = -1e30f;
        sc[4 * h + r] = x;
      }
    }

    // ---- online softmax (per column row16; reduce across the grp groups) ----
    float mt = sc[0];
#pragma unroll
    for (int x = 1; x < 8; ++x) mt = fmaxf(mt, sc[x]);
    mt = fmaxf(mt, decode_shfl(mt, lane ^ 16));
    mt = fmaxf(mt, decode_shfl(mt, lane ^ 32));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new); // -1e30 -> 0
    float ps = 0.0f;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      sc[x] = __builtin_amdgcn_exp2f(sc[x] - m_new);
      ps += sc[x];
    }
    ps += decode_shfl(ps, lane ^ 16);
    ps += decode_shfl(ps, lane ^ 32);
    l_run = l_run * alpha + ps;
    m_run = m_new;

    // ---- P^T -> the wave's LDS slice, back as the A operand ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bf16x4 pw;
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[r] = (__bf16)sc[4 * h + r];
      *(bf16x4*)(&p_lds[row16][16 * h + 4 * grp]) = pw;
    }
    float a_o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a_o[r] = decode_shfl(alpha, 4 * grp + r);
    const bf16x8 pf = *(const bf16x8*)(&p_lds[row16][8 * grp]);

    // ---- O = alpha O + P V: rows = column (4grp + r), cols = 16db + row16;
    // chunk db lies in the image of D half db / 4, there at db % 4 ----
#pragma unroll
    for (int db = 0; db < kDChunks; ++db) {
      const bf16x8 vf =
          read_tr_frag(v_img + (kHalves * buf + (db >> 2)) * kImgElems, db & 3, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[db][r] *= a_o[r];
      o_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o_acc[db], 0, 0, 0);
    }

    if (has_next) {
      stage_v(buf ^ 1, vpc); // the images this tile did not read
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int l = 0; l < kHalves; ++l) kraw[h][l] = kraw_next[h][l];
    }
    key0 = key_next;
    buf ^= 1;
    have = has_next;
  }

  // ---- block epilogue: the waves' (m, l, O) through LDS, one barrier ----
  // (a wave overwrites its OWN images, after its own last read of them). The V
  // head's scale goes onto the wave's O here, once; l is a sum of weights and
  // keeps none.
  const float vs = v_scale != nullptr ? v_scale[kvh] : 1.0f;
#pragma unroll
  for (int db = 0; db < kDChunks; ++db) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      wave_lds[wave].part.o[4 * grp + r][16 * db + row16] = o_acc[db][r] * vs;
    }
  }
  if (lane < kDecCols) {
    wave_lds[wave].part.ml[row16][0] = m_run;
    wave_lds[wave].part.ml[row16][1] = l_run;
  }
  decode_barrier();

  // tile t of the group: the partials of waves t, t + T, ... in ascending
  // phase, by the bf16 kernels' combine / store and into their partial layout
  const int col = threadIdx.x >> 4, d4 = (threadIdx.x & 15) * 4;
  for (int t = 0; t < live; ++t) {
    const float* o_parts = &wave_lds[t].part.o[0][0];
    const float* ml_parts = &wave_lds[t].part.ml[0][0];
    const int gt = tg * kTileGroup + t; // < nt
    const int c = gt * kDecCols + col;
    // all 16 columns of a partial: the duplicates of column R - 1 are finite and unread
    const int64_t part = (((int64_t)b * Hkv + kvh) * nt + gt) * S + s;
    if constexpr (kD == kAttnD) {
      const DecodeAcc a = decode_combine(o_parts, ml_parts, P, T * kWaveLdsFloats,
                                         T * kWaveLdsFloats, col, d4);
      if (S == 1) {
        if (c < R) decode_store(a, o, lse, b, kvh, H, G, Nq, c, d4);
      } else {
        *(f32x4*)(ws_o + part * kPartO + col * kD + d4) = a.o;
        if (d4 == 0) {
          ws_ml[part * kPartML + 2 * col] = a.m;
          ws_ml[part * kPartML + 2 * col + 1] = a.l;
        }
      }
    } else {
      const Decode128Acc a = decode128_combine(o_parts, ml_parts, P, T * kWaveLdsFloats,
                                               T * kWaveLdsFloats, col, d4);
      if (S == 1) {
        if (c < R) decode128_store(a, o, lse, b, kvh, H, G, Nq, c, d4);
      } else {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          *(f32x4*)(ws_o + part * kPartO + col * kD + 64 * half + d4) = a.o[half];
        }
        if (d4 == 0) {
          ws_ml[part * kPartML + 2 * col] = a.m;
          ws_ml[part * kPartML + 2 * col + 1] = a.l;
        }
      }
    }
  }
}

// fp32 [Hkv] scales on `like`'s device, or none (all ones): the pointer the
// kernels take.
static const float* checked_fp8_scale(const c10::optional<at::Tensor>& scale, const char* name,
                                      const at::Tensor& like, int64_t Hkv) {
  if (!scale.has_value()) return nullptr;
  TORCH_CHECK(scale->scalar_type() == at::kFloat && scale->device() == like.device() &&
                  scale->dim() == 1 && scale->size(0) == Hkv && scale->is_contiguous(),
              name, " must be fp32 [Hkv] = [", Hkv, "], contiguous, on the other tensors' device");
  return scale->data_ptr<float>();
}

// An e4m3 cache the kernels can address: the dtype, the device, rows of
// contiguous bytes, and base and strides multiples of `align` bytes (16 for the
// attention's loads, 8 for the append's stores; an element is a byte).
static void check_fp8_cache(const at::Tensor& t, const char* name, const at::Tensor& like,
                            int64_t align) {
  TORCH_CHECK(t.scalar_type() == at::kFloat8_e4m3fn && t.device() == like.device() &&
                  t.stride(3) == 1,
              name, " must be float8_e4m3fn on the other tensors' device with a contiguous last dim");
  TORCH_CHECK((uintptr_t)t.data_ptr() % align == 0 && t.stride(0) % align == 0 &&
                  t.stride(1) % align == 0 && t.stride(2) % align == 0,
              name, " must be ", align, "-byte aligned with batch/head/row strides that are "
              "multiples of ", align, " elements (bytes)");
}

// sdpa_kvcache over an e4m3 cache. The arguments of attn_decode_tiled plus the
// two optional scale tensors; attn_decode_tiled_splits and
// attn_decode_tiled_workspace_floats size the call. Everything is checked
// before the first launch.
void attn_decode_fp8(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor kv_len, at::Tensor o,
                     at::Tensor lse, at::Tensor ws, double scale, bool causal, int64_t num_splits,
                     c10::optional<at::Tensor> k_scale, c10::optional<at::Tensor> v_scale,
                     c10::optional<at::Tensor> block_table) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && (q.size(3) == kAttnD || q.size(3) == kAttnD128) &&
                  q.size(2) >= 1 && q.size(0) >= 1 && q.scalar_type() == at::kBFloat16,
              "q must be a bf16 device tensor [B,H,Nq,D] with B, Nq >= 1 and head dim D = 64 or 128");
  const int64_t B = q.size(0), H = q.size(1), Nq = q.size(2), D = q.size(3);
  const bool paged = block_table.has_value();
  TORCH_CHECK(k.dim() == 4 && (paged ? k.size(0) >= 1 : k.size(0) == B) && k.size(3) == D &&
                  k.size(1) >= 1 && H % k.size(1) == 0 && H >= 1,
              "k_cache must be [B,Hkv,Nmax,D] (with a block_table: [num_pages,Hkv,page_size,D]) "
              "with q's B and head dim D and a head count Hkv that divides q's: got ",
              k.sizes(), " for q ", q.sizes());
  const int64_t Hkv = k.size(1), G = H / Hkv;
  TORCH_CHECK(v.dim() == 4 && v.sizes() == k.sizes(), "v_cache must be shaped like k_cache");
  int64_t Nmax = k.size(2);
  if (paged) {
    check_block_table(*block_table, q, B, "attn_decode_fp8");
    TORCH_CHECK(k.size(2) >= kKT && k.size(2) % kKT == 0,
                "attn_decode_fp8: page_size must be a positive multiple of ", kKT, ", got ",
                k.size(2));
    TORCH_CHECK(k.size(0) <= INT32_MAX && block_table->size(1) <= INT32_MAX / k.size(2),
                "attn_decode_fp8: num_pages or max_pages * page_size too large");
    Nmax = block_table->size(1) * k.size(2);
  }
  TORCH_CHECK(Nmax >= Nq, "the cache must hold the Nq new rows: Nmax ", Nmax, " < Nq ", Nq);
  TORCH_CHECK(Nmax <= INT32_MAX - 2 * kDecChunkAlign && B * H * Nq <= INT32_MAX / D,
              "attn_decode_fp8: Nmax or B*H*Nq too large");
  const int64_t R = G * Nq;
  TORCH_CHECK(q.stride(3) == 1 && (uintptr_t)q.data_ptr() % 16 == 0 && q.stride(0) % 8 == 0 &&
                  q.stride(1) % 8 == 0 && q.stride(2) % 8 == 0,
              "q must have a contiguous last dim and be 16-byte aligned with batch/head/row "
              "strides that are multiples of 8 elements");
  // rows are read as 16-byte vectors: 16 elements
  check_fp8_cache(k, "k_cache", q, 16);
  check_fp8_cache(v, "v_cache", q, 16);
  const float* ks = checked_fp8_scale(k_scale, "k_scale", q, Hkv);
  const float* vs = checked_fp8_scale(v_scale, "v_scale", q, Hkv);
  TORCH_CHECK(kv_len.scalar_type() == at::kInt && kv_len.device() == q.device() &&
                  kv_len.dim() == 1 && kv_len.size(0) == B && kv_len.is_contiguous(),
              "kv_len must be int32 [B], contiguous, on q's device");
  TORCH_CHECK(o.scalar_type() == at::kBFloat16 && o.device() == q.device() &&
                  o.sizes() == q.sizes() && o.is_contiguous(),
              "o must be bf16, shaped like q, contiguous, on q's device");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.device() == q.device() &&
                  lse.numel() == B * H * Nq && lse.is_contiguous(),
              "lse must be fp32 [B,H,Nq], contiguous, on q's device");
  const int64_t S = attn_decode_tiled_splits(B, Hkv, R, Nmax, num_splits, q.get_device());
  const int64_t ws_floats = attn_decode_tiled_workspace_floats(B, Hkv, R, S, D);
  TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.device() == q.device() && ws.is_contiguous() &&
                  ws.numel() >= ws_floats && (ws.numel() == 0 || (uintptr_t)ws.data_ptr() % 16 == 0),
              "the workspace must be fp32, contiguous, 16-byte aligned, on q's device, with >= ",
              ws_floats, " elements for ", S, " splits of ", tiled_tiles(R), " column tiles");
  const int64_t groups = tiled_groups(R);
  // chunk: ceil(Nmax / S) rounded up to whole 128-key rounds, so S * chunk >= Nmax
  const int64_t chunk = ceil_div(ceil_div(Nmax, S), kDecChunkAlign) * kDecChunkAlign;
  TORCH_CHECK(B * Hkv * groups * S <= INT32_MAX && S * chunk <= INT32_MAX,
              "attn_decode_fp8: too many blocks or keys");

  auto stream = c10::hip::getCurrentHIPStream();
  float* ws_o = S > 1 ? ws.data_ptr<float>() : nullptr;
  float* ws_ml = S > 1 ? ws_o + B * Hkv * tiled_tiles(R) * S * kDecCols * D : nullptr;
  auto launch = [&](auto kernel, auto sk) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * Hkv * groups * S)), dim3(kAttnThreads), 0,
                       stream, (const __hip_bfloat16*)q.data_ptr(), (const uint8_t*)k.data_ptr(),
                       (const uint8_t*)v.data_ptr(), kv_len.data_ptr<int>(), ks, vs,
                       (__hip_bfloat16*)o.data_ptr(), lse.data_ptr<float>(), ws_o, ws_ml, (int)H,
                       (int)G, (int)Nq, (int)Nmax, (int)S, (int)chunk, (float)scale, causal,
                       strides_of(q), sk, strides_of(v));
  };
  if (D == kAttnD128) {
    if (paged) launch(attn_decode_fp8_kernel<kAttnD128, true>, paged_strides_of(k, *block_table));
    else launch(attn_decode_fp8_kernel<kAttnD128, false>, StridesPaged<false>{strides_of(k)});
  } else {
    if (paged) launch(attn_decode_fp8_kernel<kAttnD, true>, paged_strides_of(k, *block_table));
    else launch(attn_decode_fp8_kernel<kAttnD, false>, StridesPaged<false>{strides_of(k)});
  }
  if (S > 1) {
    // the partials have the bf16 kernels' layout: their merge kernels, as they are
    auto merge = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)(B * Hkv * groups)), dim3(kAttnThreads), 0, stream,
                         (const float*)ws_o, (const float*)ws_ml, kv_len.data_ptr<int>(),
                         (__hip_bfloat16*)o.data_ptr(), lse.data_ptr<float>(), (int)H, (int)G,
                         (int)Nq, (int)Nmax, (int)S, (int)chunk, causal);
    };
    if (D == kAttnD128) merge(attn_decode_d128_merge_kernel);
    else merge(attn_decode_tiled_merge_kernel);
  }
}

// ---------------------------------------------------------------------------
// kvcache_append_fp8: kvcache_append_kernel's contract and work split (see
// attention_kvcache_append.h: rows numbered (b, i, kvh), positions from
// decode_len(), the table entry clamped, nothing but the target rows written),
// with a quantising store: a lane reads one 16-byte bf16 piece of a K row and
// the same piece of the V row, divides its eight elements by the head's scale,
// clamps to +-448 in fp32, converts with four v_cvt_pk_fp8_f32 (round to
// nearest even) and writes 8 bytes. kD / 8 lanes per row as before.
// ---------------------------------------------------------------------------

// e4m3_rne(clamp(float(x[e]) / s, -448, 448)) for the eight elements of a
// piece. A NaN stays a NaN through the clamp and is stored as a NaN byte.
kDecodeFn __device__ __forceinline__ fp8_i32x2 quantise_fp8x8(const bf16x8& x, float s) {
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float y = (float)x[e] / s; // correctly rounded fp32 division
    f[e] = y != y ? y : fminf(fmaxf(y, -448.0f), 448.0f);
  }
  fp8_i32x2 w = {0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i], f[4 * i + 1], w[i], false);
    w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i + 2], f[4 * i + 3], w[i], true);
  }
  return w;
}

template <int kD>
kDecodeFn __global__ void __launch_bounds__(kAttnThreads) kvcache_append_fp8_kernel(
    const __hip_bfloat16* __restrict__ k_new, const __hip_bfloat16* __restrict__ v_new,
    uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache, const int* __restrict__ kv_len,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    const int* __restrict__ table, int Hkv, int Nq, int rows, int capacity, int max_pages,
    int page_size, int num_pages, Strides skn, Strides svn, Strides skc, Strides svc) {
  constexpr int kLanes = kD / 8; // 16-byte source pieces of one row
  constexpr int kRows = kAttnThreads / kLanes; // rows of one block
  const int piece = threadIdx.x % kLanes;
  const int row = blockIdx.x * kRows + threadIdx.x / kLanes; // < rows + kRows <= INT32_MAX
  if (row >= rows) return;
  const int kvh = row % Hkv;
  const int i = (row / Hkv) % Nq;
  const int b = row / Hkv / Nq;
  const int pos = decode_len(kv_len, b, Nq, capacity, true) - Nq + i; // [0, capacity)
  int64_t page = b; // dense: one "page" of Nmax rows per batch row
  int r = pos;
  if (table != nullptr) {
    const int pg = pos / page_size; // < max_pages
    page = min(max(table[(int64_t)b * max_pages + pg], 0), num_pages - 1);
    r = pos - pg * page_size;
  }
  const int64_t src_k = (int64_t)b * skn.b + (int64_t)kvh * skn.h + (int64_t)i * skn.r + 8 * piece;
  const int64_t src_v = (int64_t)b * svn.b + (int64_t)kvh * svn.h + (int64_t)i * svn.r + 8 * piece;
  const bf16x8 kx = *(const bf16x8*)(k_new + src_k);
  const bf16x8 vx = *(const bf16x8*)(v_new + src_v);
  const float ks = k_scale != nullptr ? k_scale[kvh] : 1.0f;
  const float vs = v_scale != nullptr ? v_scale[kvh] : 1.0f;
  *(fp8_i32x2*)(k_cache + page * skc.b + (int64_t)kvh * skc.h + (int64_t)r * skc.r + 8 * piece) =
      quantise_fp8x8(kx, ks);
  *(fp8_i32x2*)(v_cache + page * svc.b + (int64_t)kvh * svc.h + (int64_t)r * svc.r + 8 * piece) =
      quantise_fp8x8(vx, vs);
}

void kvcache_append_fp8(at::Tensor k_new, at::Tensor v_new, at::Tensor k_cache, at::Tensor v_cache,
                        at::Tensor kv_len, c10::optional<at::Tensor> k_scale,
                        c10::optional<at::Tensor> v_scale, c10::optional<at::Tensor> block_table) {
  TORCH_CHECK(k_new.is_cuda() && k_new.dim() == 4 && k_new.scalar_type() == at::kBFloat16 &&
                  (k_new.size(3) == kAttnD || k_new.size(3) == kAttnD128) && k_new.size(0) >= 1 &&
                  k_new.size(1) >= 1 && k_new.size(2) >= 1,
              "k_new must be a bf16 device tensor [B,Hkv,Nq,D] with B, Hkv, Nq >= 1 and D = 64 or 128");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), Nq = k_new.size(2), D = k_new.size(3);
  TORCH_CHECK(v_new.sizes() == k_new.sizes(), "v_new must be shaped like k_new");
  const bool paged = block_table.has_value();
  TORCH_CHECK(k_cache.dim() == 4 && (paged ? k_cache.size(0) >= 1 : k_cache.size(0) == B) &&
                  k_cache.size(1) == Hkv && k_cache.size(2) >= 1 && k_cache.size(3) == D,
              "k_cache must be [B,Hkv,Nmax,D] (with a block_table: [num_pages,Hkv,page_size,D]) "
              "with k_new's Hkv and D: got ", k_cache.sizes(), " for k_new ", k_new.sizes());
  TORCH_CHECK(v_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes(),
              "v_cache must be shaped like k_cache");
  int64_t capacity = k_cache.size(2), max_pages = 1;
  if (paged) {
    check_block_table(*block_table, k_new, B, "kvcache_append_fp8");
    max_pages = block_table->size(1);
    TORCH_CHECK(k_cache.size(0) <= INT32_MAX && max_pages <= INT32_MAX / k_cache.size(2),
                "kvcache_append_fp8: num_pages or max_pages * page_size too large");
    capacity = max_pages * k_cache.size(2);
  }
  TORCH_CHECK(capacity >= Nq, "the cache must hold the Nq new rows: capacity ", capacity, " < Nq ",
              Nq);
  TORCH_CHECK(capacity <= INT32_MAX && B * Nq * Hkv <= INT32_MAX - kAttnThreads,
              "kvcache_append_fp8: capacity or B*Nq*Hkv too large");
  for (const NamedTensor& a : {NamedTensor{"k_new", k_new}, {"v_new", v_new}}) {
    const at::Tensor& t = a.second;
    TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.device() == k_new.device() &&
                    t.stride(3) == 1,
                a.first, " must be bf16 on k_new's device with a contiguous last dim");
    // source rows are read as 16-byte vectors
    TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0 && t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                    t.stride(2) % 8 == 0,
                a.first, " must be 16-byte aligned with batch/head/row strides that are multiples "
                         "of 8 elements");
  }
  // a lane stores 8 bytes: base and strides multiples of 8 bytes
  check_fp8_cache(k_cache, "k_cache", k_new, 8);
  check_fp8_cache(v_cache, "v_cache", k_new, 8);
  const float* ks = checked_fp8_scale(k_scale, "k_scale", k_new, Hkv);
  const float* vs = checked_fp8_scale(v_scale, "v_scale", k_new, Hkv);
  TORCH_CHECK(kv_len.scalar_type() == at::kInt && kv_len.device() == k_new.device() &&
                  kv_len.dim() == 1 && kv_len.size(0) == B && kv_len.is_contiguous(),
              "kv_len must be int32 [B], contiguous, on k_new's device");

  const int64_t rows = B * Nq * Hkv;
  const int64_t rows_per_block = kAttnThreads / (D / 8);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(rows, rows_per_block)), dim3(kAttnThreads),
                       0, c10::hip::getCurrentHIPStream(),
                       (const __hip_bfloat16*)k_new.data_ptr(),
                       (const __hip_bfloat16*)v_new.data_ptr(), (uint8_t*)k_cache.data_ptr(),
                       (uint8_t*)v_cache.data_ptr(), kv_len.data_ptr<int>(), ks, vs,
                       paged ? block_table->data_ptr<int>() : (const int*)nullptr, (int)Hkv,
                       (int)Nq, (int)rows, (int)capacity, (int)max_pages, (int)k_cache.size(2),
                       (int)k_cache.size(0), strides_of(k_new), strides_of(v_new),
                       strides_of(k_cache), strides_of(v_cache));
  };
  if (D == kAttnD128) launch(kvcache_append_fp8_kernel<kAttnD128>);
  else launch(kvcache_append_fp8_kernel<kAttnD>);
}

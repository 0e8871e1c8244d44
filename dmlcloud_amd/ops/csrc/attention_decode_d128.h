// Head dim 128 form of the KV-cache attention kernels (ops.fused_attn.
// sdpa_kvcache). Part of attention.hip (included at its end, inside namespace
// dmlamd, after attention_d128.h); it uses that file's thread_coords, vt_idx,
// read_tr_frag, Strides, decode_len, decode_shfl, decode_barrier and
// kTileGroup. ONE kernel pair serves every R = (H / Hkv) * Nq >= 1:
//   attn_decode_d128_kernel        split-KV forward over column tiles
//   attn_decode_d128_merge_kernel  combines the splits' partials
//
// Contract. q [B, H, Nq, 128] holds NEW rows, k/v [B, Hkv, Nmax, 128] a cache
// of which batch row b has kv_len[b] valid rows (the new tokens' included), an
// int32 read from device memory. len = decode_len(): kv_len[b] clamped so that
// every row keeps a key and no index leaves the cache, whatever the tensor
// holds. Query row i sits at position p = len - Nq + i and attends keys 0..p
// (causal, bottom-right aligned) or 0..len-1. Cache rows >= len are never
// LOADED: they are uninitialised by contract, and P = 0 times a NaN V row is
// NaN inside the MFMA, so every key-row index is clamped to len - 1 and the
// duplicates are masked by the score compare. No atomics: results are bitwise
// repeatable for a (shape, S). The grid depends on shapes and the device only.
// Forward only. attn_decode_d128_kernel<true> reads k/v as page pools
// [num_pages, Hkv, page_size, 128] through a block table, with the capacity
// max_pages * page_size for Nmax (StridesPaged in attention.hip); <false> is
// the dense code.
//
// Work split (decode does ~1 flop per byte, so it is made for bytes in flight):
//   * the R columns c = g * Nq + i (query head kvh * G + g, row i) of one K/V
//     head are cut into nt = ceil(R / 16) MFMA column tiles; tile t owns
//     columns 16t..16t+15, columns >= R re-read column R - 1 and are never
//     stored;
//   * a block serves one (b, K/V head, tile GROUP, split); a group is up to
//     kTileGroup = 4 consecutive tiles of which `live` exist; the keys are
//     split over S blocks, each a contiguous chunk (a multiple of 128 keys);
//   * the four waves take ROLES from live: T = 1, 2 or 4 column tiles side by
//     side (three live tiles run as T = 4 with one role idle). Wave w owns
//     column tile w % T of the group and key phase w / T of P = 4 / T, and
//     walks the 32-key tiles k_begin + 32 * (phase + P * t) of the split on
//     its own, with no barrier in the key loop. T = 1 (R <= 16) is plain
//     split-KV decoding: the four waves share out the split's key tiles. T = 4
//     makes every wave walk all keys of the split for its own 16 columns; the
//     T waves that share a key tile read it through L1/L2, not through LDS;
//   * causal skip: a wave passes over key tiles beyond the largest key any of
//     its columns attends (lim_max below);
//   * the waves' (m, l, O) meet once, in LDS, behind one barrier; for each
//     live tile its P phase partials are combined in ascending phase. S == 1
//     normalises and stores. S > 1 writes one fp32 partial per (tile, split)
//     to the workspace, O [B, Hkv, nt, S, 16, 128] then (m, l)
//     [B, Hkv, nt, S, 16, 2], and the merge kernel combines the LIVE splits in
//     ascending order.
//
// What D = 128 means per wave and 32-key tile:
//   * S^T = K Q^T contracts over four 32-wide chunks: Q is four B fragments
//     qf[4], K eight A fragments kf[2][4] (16-key half h, chunk c), each a
//     16-byte global load K[key0 + 16h + l%16][32c + 8(l/16)..+7]: no LDS;
//   * a V tile is TWO vt_idx images (D columns 0..63 and 64..127). The wave
//     stages it as eight bf16x8 pieces per lane: 16 lanes cover one 256-byte
//     row, lane l holds rows l/16 + 4x (x = 0..7), columns 8(l%16)..+7;
//   * P V writes eight 16-wide D chunks: O is eight f32x4 accumulators;
//   * the block epilogue has 16 x 32 (column, d4) slots for 256 threads: a
//     thread owns column tid / 16 and the elements 4(tid % 16).. of BOTH
//     64-wide D halves.
//
// Register and LDS budget, counted from the code before the loop was written:
// the key loop holds the current and the next tile's K fragments (2 x 32
// VGPRs), the V pieces in flight (32), O (32) and Q (16), 144 registers, with
// scores, addresses and the softmax state about 170..190: a 2 waves/SIMD
// kernel. LDS per wave is the double-buffered pair of images (2 x 2 x 4 KB =
// 16 KB), overlaid after the loop by the wave's o[16][128] fp32 (8 KB) + ml,
// plus a 1280-byte P slice: 70656 B per block, two blocks per CU, the same 2
// waves/SIMD. Bytes in flight per CU: 8 waves x 16 KB (K 8 KB + V 8 KB per
// prefetched tile), what 16 waves x 8 KB give at D = 64. Occupancy is left to
// the compiler (no amdgpu_waves_per_eu); its verdict and the absence of scratch
// are recorded in profiles/attention_decode_d128.txt.
#pragma once

constexpr int kDec128Cols = 16; // query columns of one MFMA tile
constexpr int kDec128ChunkAlign = kWavesPerBlock * kKT; // 128: every phase gets whole tiles
constexpr int kDec128PartO = kDec128Cols * kAttnD128; // floats of one O partial
constexpr int kDec128PartML = kDec128Cols * 2; // floats of one (m, l) partial
constexpr int kDec128VPieces = kKT * kAttnD128 / 8 / kWave; // 8 bf16x8 pieces per lane

// A wave's LDS: its two V tiles (two images each) during the key loop, its
// (m, l, O) for the block epilogue after it (only the wave itself writes either).
union alignas(16) Decode128WaveLds {
  __bf16 v[2][2][kImgElems]; // [buffer][D half]
  struct {
    float o[kDec128Cols][kAttnD128];
    float ml[kDec128Cols][2];
  } part;
};
constexpr int kDec128WaveLdsFloats = sizeof(Decode128WaveLds) / sizeof(float);

// Thread tid of a 256-thread block owns column tid / 16 and, in each 64-wide
// D half, the four elements 4 * (tid % 16).. of the combined result.
struct Decode128Acc {
  float m, l; // log2-domain running max, sum of exp2
  f32x4 o[2]; // unnormalised, [D half]
};

// Combine `n` partials (O at o_parts + s * o_stride, (m, l) at ml_parts +
// s * ml_stride) in ascending s. A partial whose column saw only masked keys
// has m = -1e30 and finite garbage in l and O (the wipe, see the key loop);
// beside a partial with a real maximum M its weight exp2(-1e30 - M) is
// exactly 0. An empty partial (a wave that walked nothing) is m = -1e30,
// l = O = 0.
kDecodeFn __device__ __forceinline__ Decode128Acc decode128_combine(const float* o_parts,
                                                                    const float* ml_parts, int n,
                                                                    int o_stride, int ml_stride,
                                                                    int col, int d4) {
  Decode128Acc a = {-1e30f, 0.0f, {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}}};
  for (int s = 0; s < n; ++s) a.m = fmaxf(a.m, ml_parts[(int64_t)s * ml_stride + 2 * col]);
  for (int s = 0; s < n; ++s) {
    const float* ml = ml_parts + (int64_t)s * ml_stride + 2 * col;
    const float w = __builtin_amdgcn_exp2f(ml[0] - a.m);
    a.l += w * ml[1];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const f32x4 po =
          *(const f32x4*)(o_parts + (int64_t)s * o_stride + col * kAttnD128 + 64 * half + d4);
#pragma unroll
      for (int r = 0; r < 4; ++r) a.o[half][r] += w * po[r];
    }
  }
  return a;
}

// Normalise and store column `col` (< R) of K/V head kvh: o bf16, lse fp32.
kDecodeFn __device__ __forceinline__ void decode128_store(const Decode128Acc& a,
                                                          __hip_bfloat16* __restrict__ o,
                                                          float* __restrict__ lse, int b, int kvh,
                                                          int H, int G, int Nq, int col, int d4) {
  const int g = col / Nq;
  const int64_t row = ((int64_t)b * H + kvh * G + g) * Nq + (col - g * Nq);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    bf16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = (__bf16)(a.o[half][r] / a.l);
    *(bf16x4*)(o + row * kAttnD128 + 64 * half + d4) = ov;
  }
  if (d4 == 0) lse[row] = kLn2 * a.m + __logf(a.l); // log2 domain -> natural log
}

// <kPaged>: k and v are page pools read through a block table, Nmax is the
// capacity max_pages * page_size (see StridesPaged in attention.hip).
template <bool kPaged>
kDecodeFn __global__ void __launch_bounds__(kAttnThreads) attn_decode_d128_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const int* __restrict__ kv_len,
    __hip_bfloat16* __restrict__ o, float* __restrict__ lse, float* __restrict__ ws_o,
    float* __restrict__ ws_ml, int H, int G, int Nq, int Nmax, int S, int chunk, float scale,
    bool causal, Strides sq, StridesPaged<kPaged> sk, Strides sv) {
  static_assert(kKT * 64 == kImgElems && kDec128VPieces == 8);
  __shared__ Decode128WaveLds wave_lds[kWavesPerBlock];
  __shared__ __hip_bfloat16 p_lds_all[kWavesPerBlock][kQT][kPStride];

  // plain ints, not a structured binding: the tile lambdas capture them
  const Coords tc = thread_coords();
  const int lane = tc.lane, row16 = tc.row16, grp = tc.grp;
  const int wave = __builtin_amdgcn_readfirstlane(tc.wave);
  __hip_bfloat16(*p_lds)[kPStride] = p_lds_all[wave];
  // image (2 * buffer + D half) of the wave at + that * kImgElems
  const __hip_bfloat16* v_img = (const __hip_bfloat16*)wave_lds[wave].v[0][0];
  // V staging: the WAVE moves a 32x128 tile as 8 bf16x8 pieces per lane,
  // rows st_row + 4x, columns st_col..+7 (16 lanes per 256-byte row)
  const int st_row = grp; // 0..3
  const int st_col = row16 * 8; // 0..120
  // piece x: row & 3 = st_row, (row >> 2) & 1 = x & 1, row >> 3 = x >> 1
  const int st_half = st_col >> 6, st_vt = vt_idx(st_row, st_col & 63);

  // grid: (b, K/V head, tile group, split), split fastest
  const int Hkv = H / G;
  const int R = G * Nq;
  const int nt = (R + kDec128Cols - 1) / kDec128Cols;
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

  // Which keys are walked, per (column tile, phase). Split s owns keys
  // [s * chunk, (s + 1) * chunk), S * chunk >= Nmax >= len (launcher); a
  // split with k_begin >= len has none and returns before the barrier, all
  // threads alike (block-uniform), writing nothing; the merge kernel derives
  // the same live count from the same len and never reads its partial.
  // lim_max is the largest key any column of the wave's tile attends:
  // len - 1 when not causal or when the tile holds a column with i = Nq - 1
  // (a multiple of Nq in (c0, c1 + 1]: every tile that crosses a head
  // boundary, and the last tile, whose c1 + 1 = R = G * Nq), else the
  // position of its last column, the largest i of the tile. The wave walks
  // key0 = k_begin + 32 * (phase + P * t) < k_stop = min(k_begin + chunk,
  // lim_max + 1) <= len (wave-uniform).
  // Every stored column meets each of its keys exactly once: a key j <= lim
  // of a column of tile ct lies in the one split s = j / chunk (live:
  // k_begin <= j < len), there in the one 32-key tile key0 = j -
  // (j - k_begin) % 32, which belongs to the one phase ((key0 - k_begin) /
  // 32) % P of the one wave that owns (ct, phase); key0 <= j <= lim <=
  // lim_max and key0 < k_begin + chunk, so that wave walks it. Keys > lim
  // in a walked tile score -1e30 (the compare), rows >= len are never
  // loaded (the clamp). Key 0 is attended by every stored column (p >= 0,
  // because len >= Nq when causal) and sits in split 0, phase 0, t = 0 with
  // lim_max >= 0, so a stored column's merged maximum is a real score and
  // its l >= exp2(0).
  // The wipe: a column that meets only masked keys in a wave's walk keeps
  // m = -1e30 with alpha = exp2(0) = 1 and every p = exp2(0) = 1: finite
  // garbage in l and O (the V rows are real rows < len), which
  // exp2(-1e30 - M) = 0 removes wherever it meets a real maximum M: a later
  // tile of the same wave, another phase (block epilogue) or another split
  // (merge). The empty partial: a wave that walks nothing (skipped by
  // lim_max, no tile left for its phase, or the idle role) leaves m = -1e30,
  // l = 0, O = 0.
  const int k_begin = s * chunk;
  if (k_begin >= len) return;
  const int c0 = tile * kDec128Cols, c1 = min(c0 + kDec128Cols - 1, R - 1);
  int lim_max = len - 1;
  if (causal && (c1 + 1) / Nq == c0 / Nq) lim_max = len - Nq + (c1 - c0 / Nq * Nq);
  const int k_stop = tile < nt ? min(k_begin + chunk, lim_max + 1) : k_begin;

  // this lane's query column: Q B-fragments, and the last key it attends
  // (the idle role's tile >= nt reads column R - 1 and walks nothing)
  const int col_q = min(c0 + row16, R - 1);
  const int g_q = col_q / Nq;
  const int i_q = col_q - g_q * Nq;
  const int lim = causal ? len - Nq + i_q : len - 1;
  const __hip_bfloat16* qp =
      q + (int64_t)b * sq.b + (int64_t)(kvh * G + g_q) * sq.h + (int64_t)i_q * sq.r;
  bf16x8 qf[kKChunks128];
#pragma unroll
  for (int c = 0; c < kKChunks128; ++c) qf[c] = *(const bf16x8*)(qp + 32 * c + 8 * grp);

  const __hip_bfloat16* kp = k + (int64_t)b * sk.b + (int64_t)kvh * sk.h;
  const __hip_bfloat16* vp = v + (int64_t)b * sv.b + (int64_t)kvh * sv.h;
  // K fragments [16-key half h][k-chunk c] and V pieces of the tile at key0,
  // every row clamped to len - 1. kt / vt: the tile's page_bases() (paged);
  // the dense code keeps reading its (b, K/V head) slices kp / vp
  auto load_tile = [&](int key0, const __hip_bfloat16* kt, const __hip_bfloat16* vt,
                       bf16x8(&kf)[2][kKChunks128],
                       bf16x8(&vpc)[kDec128VPieces]) kDecodeFn __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t kr = min(key0 + 16 * h + row16, len - 1);
#pragma unroll
      for (int c = 0; c < kKChunks128; ++c) {
        kf[h][c] = *(const bf16x8*)((kPaged ? kt : kp) + kr * sk.r + 32 * c + 8 * grp);
      }
    }
    // K before V, pinned: loads return in order, so the wait in front of
    // the V image writes (after the math) also covers K, and the MFMAs at
    // the top of the next tile wait for nothing. With V first the compiler
    // puts a full wait for the NEXT tile's loads in front of this tile's math.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int x = 0; x < kDec128VPieces; ++x) {
      const int64_t vr = min(key0 + st_row + 4 * x, len - 1);
      vpc[x] = *(const bf16x8*)((kPaged ? vt : vp) + vr * sv.r + st_col);
    }
  };
  auto stage_v = [&](int buf, const bf16x8(&vpc)[kDec128VPieces]) kDecodeFn
      __attribute__((always_inline)) {
#pragma unroll
    for (int x = 0; x < kDec128VPieces; ++x) {
      *(bf16x8*)(&wave_lds[wave].v[buf][st_half][st_vt + (x & 1) * 256 + (x >> 1) * 64]) = vpc[x];
    }
  };

  const float scale2 = scale * kLog2e; // fold log2(e): exp -> v_exp_f32
  float m_run = -1e30f, l_run = 0.0f;
  f32x4 o_acc[kDChunks128];
#pragma unroll
  for (int db = 0; db < kDChunks128; ++db) o_acc[db] = f32x4{0, 0, 0, 0};

  const int key_step = P * kKT;
  int key0 = k_begin + phase * kKT;
  bool have = key0 < k_stop;
  bf16x8 kf[2][kKChunks128], vpc[kDec128VPieces];
  // Paged: a walked tile key0 < k_stop <= len lies in an allocated page, index
  // key0 / page_size <= (len - 1) / page_size < max_pages (len <= capacity),
  // so only table entries < ceil(len / page_size) are read. Its clamped rows
  // min(key0 + x, len - 1), x < 32, stay in [key0, key0 + 31]: the same
  // 32-aligned tile, hence the same page (page_size % 32 == 0), rows
  // 0..page_size-1 of a page id clamped into the pool. `walk` only ever
  // seeks to a tile that exists, so the entry it names is one of those.
  const __hip_bfloat16 *kt = kp, *vt = vp; // paged: the current tile's bases
  [[maybe_unused]] PageWalk walk = {0, 0};
  [[maybe_unused]] int ent_next = 0, lo_next = 0; // the NEXT tile's entry and page start
  [[maybe_unused]] PageTable tbl = nullptr; // block_table[b]
  if constexpr (kPaged) {
    if (have) {
      tbl = (PageTable)(sk.table + (int64_t)b * sk.max_pages);
      walk.pg = key0 / sk.page_size;
      walk.key_lo = walk.pg * sk.page_size;
      page_bases(tbl[walk.pg], walk.key_lo, kvh, k, v, sk, sv, kt, vt);
      if (key0 + key_step < k_stop) page_seek(walk, key0 + key_step, sk.page_size);
      ent_next = tbl[walk.pg];
      lo_next = walk.key_lo;
    }
  }
  if (have) {
    load_tile(key0, kt, vt, kf, vpc);
    stage_v(0, vpc);
  }
  int buf = 0;
  while (have) {
    // the next tile's loads stay in flight through this tile's math
    const int key_next = key0 + key_step;
    const bool has_next = key_next < k_stop;
    bf16x8 kf_next[2][kKChunks128];
    if constexpr (kPaged) page_bases(ent_next, lo_next, kvh, k, v, sk, sv, kt, vt);
    if (has_next) load_tile(key_next, kt, vt, kf_next, vpc);
    if constexpr (kPaged) {
      // the entry of the tile after next, behind the loads just issued; it
      // is first used at the top of the next round (the compiler sinks this
      // scalar load to the end of the round: still a round ahead of the
      // loads it feeds, which are themselves a round ahead of their math)
      if (key_next + key_step < k_stop) page_seek(walk, key_next + key_step, sk.page_size);
      ent_next = tbl[walk.pg];
      lo_next = walk.key_lo;
    }

    // ---- S^T = K Q^T: rows = key (16h + 4grp + r), col = row16 ----
    float sc[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < kKChunks128; ++c) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[h][c], qf[c], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = acc[r] * scale2; // log2-domain score
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
    // chunk db lies in the D half db / 4, there at db % 4 ----
#pragma unroll
    for (int db = 0; db < kDChunks128; ++db) {
      const bf16x8 vf = read_tr_frag(v_img + (2 * buf + (db >> 2)) * kImgElems, db & 3, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[db][r] *= a_o[r];
      o_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o_acc[db], 0, 0, 0);
    }

    if (has_next) {
      stage_v(buf ^ 1, vpc); // the pair of images this tile did not read
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < kKChunks128; ++c) kf[h][c] = kf_next[h][c];
    }
    key0 = key_next;
    buf ^= 1;
    have = has_next;
  }

  // ---- block epilogue: the waves' (m, l, O) through LDS, one barrier ----
  // (a wave overwrites its OWN images, after its own last read of them)
#pragma unroll
  for (int db = 0; db < kDChunks128; ++db) {
#pragma unroll
    for (int r = 0; r < 4; ++r) wave_lds[wave].part.o[4 * grp + r][16 * db + row16] = o_acc[db][r];
  }
  if (lane < kDec128Cols) {
    wave_lds[wave].part.ml[row16][0] = m_run;
    wave_lds[wave].part.ml[row16][1] = l_run;
  }
  decode_barrier();

  // tile t of the group: the partials of waves t, t + T, ... in ascending
  // phase; 16 x 32 (column, d4) slots, two (one per D half) per thread
  const int col = threadIdx.x >> 4, d4 = (threadIdx.x & 15) * 4;
  for (int t = 0; t < live; ++t) {
    const Decode128Acc a =
        decode128_combine(&wave_lds[t].part.o[0][0], &wave_lds[t].part.ml[0][0], P,
                          T * kDec128WaveLdsFloats, T * kDec128WaveLdsFloats, col, d4);
    const int gt = tg * kTileGroup + t; // < nt
    if (S == 1) {
      const int c = gt * kDec128Cols + col;
      if (c < R) decode128_store(a, o, lse, b, kvh, H, G, Nq, c, d4);
    } else {
      // all 16 columns: the duplicates of column R - 1 are finite and unread
      const int64_t part = (((int64_t)b * Hkv + kvh) * nt + gt) * S + s;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        *(f32x4*)(ws_o + part * kDec128PartO + col * kAttnD128 + 64 * half + d4) = a.o[half];
      }
      if (d4 == 0) {
        ws_ml[part * kDec128PartML + 2 * col] = a.m;
        ws_ml[part * kDec128PartML + 2 * col + 1] = a.l;
      }
    }
  }
}

// One block per (b, K/V head, tile group): for every live tile, combine the
// partials of the splits that ran, 0..n_live-1 (split s ran iff
// s * chunk < len, the split kernel's early return), and store the columns
// < R. Nothing else of the (uninitialised) workspace is read.
kDecodeFn __global__ void __launch_bounds__(kAttnThreads) attn_decode_d128_merge_kernel(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
    const int* __restrict__ kv_len, __hip_bfloat16* __restrict__ o, float* __restrict__ lse,
    int H, int G, int Nq, int Nmax, int S, int chunk, bool causal) {
  const int Hkv = H / G;
  const int R = G * Nq;
  const int nt = (R + kDec128Cols - 1) / kDec128Cols;
  const int groups = (nt + kTileGroup - 1) / kTileGroup;
  const int tg = blockIdx.x % groups;
  const int kvh = (blockIdx.x / groups) % Hkv;
  const int b = blockIdx.x / groups / Hkv;
  const int len = decode_len(kv_len, b, Nq, Nmax, causal);
  const int n_live = min(S, (len + chunk - 1) / chunk); // >= 1: len >= 1
  const int col = threadIdx.x >> 4, d4 = (threadIdx.x & 15) * 4;
  const int live = min(kTileGroup, nt - tg * kTileGroup);
  for (int t = 0; t < live; ++t) {
    const int gt = tg * kTileGroup + t;
    const int c = gt * kDec128Cols + col;
    if (c >= R) continue;
    const int64_t part = (((int64_t)b * Hkv + kvh) * nt + gt) * S;
    const Decode128Acc a =
        decode128_combine(ws_o + part * kDec128PartO, ws_ml + part * kDec128PartML, n_live,
                          kDec128PartO, kDec128PartML, col, d4);
    decode128_store(a, o, lse, b, kvh, H, G, Nq, c, d4);
  }
}

// Launches the pair for arguments attn_decode_tiled has checked; the
// workspace holds attn_decode_tiled_workspace_floats(B, Hkv, R, S, 128).
// Nmax is the capacity: k.size(2), or max_pages * page_size with a table.
static void attn_decode_tiled_d128(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                   const at::Tensor& kv_len, at::Tensor& o, at::Tensor& lse,
                                   at::Tensor& ws, double scale, bool causal, int64_t S,
                                   int64_t chunk, int64_t Nmax, const at::Tensor* table) {
  const int64_t B = q.size(0), H = q.size(1), Nq = q.size(2), Hkv = k.size(1);
  const int64_t G = H / Hkv, tiles = ceil_div(G * Nq, kDec128Cols);
  const int64_t groups = ceil_div(tiles, kTileGroup);
  auto stream = c10::hip::getCurrentHIPStream();
  float* ws_o = S > 1 ? ws.data_ptr<float>() : nullptr;
  float* ws_ml = S > 1 ? ws_o + B * Hkv * tiles * S * kDec128PartO : nullptr;
  auto launch = [&](auto kernel, auto sk) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * Hkv * groups * S)), dim3(kAttnThreads), 0,
                       stream, (const __hip_bfloat16*)q.data_ptr(),
                       (const __hip_bfloat16*)k.data_ptr(), (const __hip_bfloat16*)v.data_ptr(),
                       kv_len.data_ptr<int>(), (__hip_bfloat16*)o.data_ptr(),
                       lse.data_ptr<float>(), ws_o, ws_ml, (int)H, (int)G, (int)Nq, (int)Nmax,
                       (int)S, (int)chunk, (float)scale, causal, strides_of(q), sk, strides_of(v));
  };
  if (table) launch(attn_decode_d128_kernel<true>, paged_strides_of(k, *table));
  else launch(attn_decode_d128_kernel<false>, StridesPaged<false>{strides_of(k)});
  if (S > 1) {
    hipLaunchKernelGGL(attn_decode_d128_merge_kernel, dim3((unsigned)(B * Hkv * groups)),
                       dim3(kAttnThreads), 0, stream, (const float*)ws_o, (const float*)ws_ml,
                       kv_len.data_ptr<int>(), (__hip_bfloat16*)o.data_ptr(),
                       lse.data_ptr<float>(), (int)H, (int)G, (int)Nq, (int)Nmax, (int)S,
                       (int)chunk, causal);
  }
}

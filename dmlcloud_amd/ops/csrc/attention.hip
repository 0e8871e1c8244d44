// Flash attention for gfx950: forward and backward, MFMA bf16, head dim 64,
// self-attention geometry, any N >= 1, optional packed documents. Tiling
// mirrors ops/_attention_ref.py exactly. A block is 4 waves of one (b, h):
//   attn_fwd_kernel       wave owns 32 q rows (two 16-row sub-tiles), block
//                         128; 64-key K/V tiles stream past. Emits O, lse.
//   attn_bwd_delta_kernel delta = rowsum(dO * O), eight lanes per row.
//   attn_bwd_dkdv_kernel  wave owns 16 keys, block 64; 32-row Q/dO steps
//                         stream past. Emits dK, dV.
//   attn_bwd_dq_kernel    wave owns 16 q rows, block 64; 32-key K/V tiles
//                         stream past. Emits dQ.
// Fragment maps of v_mfma_f32_16x16x32_bf16, empirically confirmed
// (profiles/mfma_16x16x32_bf16_layout.txt):
//   A (bf16x8): lane l elem j <-> A[l%16][8*(l/16)+j]
//   B (bf16x8): lane l elem j <-> B[8*(l/16)+j][l%16]
//   C/D (f32x4): lane l reg r <-> D[4*(l/16)+r][l%16]
// S is computed TRANSPOSED (S^T = K Q^T) so each lane's scores share a
// single query (softmax row reductions = 2 xor-shuffles); P^T / dS^T go
// through small per-wave LDS slices to re-enter the next MFMA as the A
// operand. B operands that need a transpose (V, dO, Q, K) are staged as
// tiled 32x64 LDS images (vt_idx) and read back by read_tr_frag.
// Template flags: <kRagged> (crow) and <kDoc> (dstart, StridesDoc);
// <false, false> is the plain aligned dense code. The correctness arguments
// (ragged tails, causal diagonal, document skips, the wipe) stand next to
// their loops; tests/test_attention_*ref.py check the same tiles on the CPU.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_bf16.h>

#include <initializer_list>

#include "ops_common.h"

namespace dmlamd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.44269504f; // exp(x) = exp2(x * log2(e)): v_exp_f32
constexpr float kLn2 = 0.69314718f;

constexpr int kAttnD = 64; // head dim
constexpr int kQT = 16; // query rows per MFMA tile
constexpr int kKT = 32; // keys per kv tile (backward kernels)
constexpr int kPStride = 40; // P_lds row stride in bf16 (16B-aligned rows, backward)
constexpr int kWavesPerBlock = 4;
constexpr int kAttnThreads = kWavesPerBlock * kWave;
// K/V LDS row stride in bf16: multiple of 8 (16B-aligned vector rows) with
// (stride/2 dwords, 64 banks) gcd = 4 so 16 simultaneous row reads at one
// column offset span 16 distinct banks (rows at stride 88 bf16 = 44 dwords)
constexpr int kKVStride = 88;
// Why the forward uses 64-key tiles and two q sub-tiles per wave: with 64
// keys per softmax round the per-round fixed costs (max/sum cross-lane
// reductions, running-stat updates, O-accumulator rescale, P LDS
// round-trip waits, the block-wide staging barrier) halve per key while
// the MFMA count per key stays identical, and the shared K fragments and
// V fragment reads amortize over twice the MFMAs. 16 rows at stride 72
// bf16 = 36 dwords hit 16 distinct banks (gcd(36,64)=4).
constexpr int kKTF = 64; // fwd: keys per kv tile
constexpr int kPStrideF = 72; // fwd: P_lds row stride in bf16

// Block geometry, shared by the kernels and the launchers' grids.
constexpr int kFwdRowsPerBlock = kWavesPerBlock * 2 * kQT; // 128 (2 sub-tiles per wave)
constexpr int kBwdKeysPerBlock = kWavesPerBlock * 16; // 64 (dK/dV)
constexpr int kDqRowsPerBlock = kWavesPerBlock * kQT; // 64

// Tiled 32x64 LDS image index for ds_read_b64_tr_b16 consumption
// (tools/tr_probe.hip): elem[(col/16*2 + row/4%2)*256 + row/8*64 +
// row%4*16 + col%16] = T[row][col]. Row-major b128 reads also work on
// the image (any 8 contiguous cols within a 16-col sub-tile row).
constexpr int kImgElems = 32 * kAttnD; // one image
constexpr int kImgSub = 4 * kWave; // elements one transposed read covers
__device__ __forceinline__ int vt_idx(int row, int col) {
  return (((col >> 4) * 2 + ((row >> 2) & 1)) * 4 + (row >> 3)) * 64 + (row & 3) * 16 +
         (col & 15);
}

// B-operand fragment T[8*(l/16) + j][16*db + l%16] of the 32x64 image at
// `img` (empirically probed semantics, tools/tr_probe.hip: 16 contiguous
// per-lane 8-byte addresses cover a 64-element region transposed as
// 4x16): two hardware transpose reads, one per 4-row half.
__device__ __forceinline__ bf16x8 read_tr_frag(const __hip_bfloat16* img, int db, int lane) {
  bf16x8 f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const short4v t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) short4v*)&img[(db * 2 + half) * kImgSub + lane * 4]);
    __builtin_memcpy((char*)&f + 8 * half, &t, 8);
  }
  return f;
}

// Per-thread coordinates: row16 = q (or key) index inside a 16-row tile,
// grp = 16-lane group 0..3, (st_row, st_col) = the thread's bf16x8 piece of
// a staged 32x64 tile.
struct Coords {
  int lane, wave, row16, grp, st_row, st_col;
};
__device__ __forceinline__ Coords thread_coords() {
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  return {lane, tid / kWave, lane & 15, lane >> 4, tid >> 3, (tid & 7) * 8};
}

// per-tensor strides (elements): batch, head, row; the last dim must be
// contiguous. Lets the model pass transpose views without materializing.
struct Strides {
  int64_t b, h, r;
};

__device__ __forceinline__ const __hip_bfloat16* tslice(const __hip_bfloat16* t,
                                                        const Strides& st, int bh, int H) {
  return t + (int64_t)(bh / H) * st.b + (int64_t)(bh % H) * st.h;
}

// Ragged sequence lengths (N % 64 != 0): every kernel below takes a
// `kRagged` template flag. <false> is the aligned code, unchanged; <true>
// adds three things and nothing else:
//   * every global ROW index goes through crow(): min(row, N - 1). A tile
//     that hangs over the end of the sequence re-reads the last real row,
//     so no load can leave the tensor and the duplicates are finite data;
//   * the duplicates are masked out of the math (fwd: score = -1e30 for
//     key >= N; bwd: p = 0 for key >= N or q >= N, so dS = 0 * finite);
//   * every global store is predicated per row on row < N.
// Loop bounds need no change: they already round up to whole tiles.
template <bool kRagged>
__device__ __forceinline__ int crow(int row, int N) {
  if constexpr (kRagged) return min(row, N - 1);
  return row;
}

// Packed sequences (document mask): every kernel below also takes a
// `kDoc` template flag and an int32 `doc_start[B, N]` (shared by all
// heads). doc_start[b][i] is the index of the first token of the
// document token i belongs to; with causal attention query i attends
// keys doc_start[b][i] <= j <= i, so the mask is ONE integer per query
// row. <kDoc = false> is the code without it, unchanged. <true> adds:
//   * dstart(): the value read for row q is clamped to [0, q], so
//     whatever the tensor holds every row keeps its diagonal key and no
//     index derived from it can leave [0, N);
//   * the mask (fwd: score = -1e30 for key < start[q]; bwd: p = 0);
//   * tile SKIPS derived from it, all block- or wave-uniform (the
//     argument stands next to each loop).
// The launchers require causal = true with a doc_start.
// doc_start rides in the kernels' LAST stride argument, a
// StridesDoc<kDoc>: plain Strides for <false>, Strides plus the pointer
// for <true>. An argument of its own, even an empty struct, would move
// the implicit kernel arguments behind it and with them one load offset
// in the <false> kernels; this way their argument layout and instruction
// stream are exactly what they were.
template <bool kDoc>
struct StridesDoc : Strides {
  const int* doc_start;
};
template <>
struct StridesDoc<false> : Strides {};

// Grouped-query attention (GQA; MQA is Hkv = 1): every kernel below also
// takes a `kGqa` template flag. K and V (and dK, dV) then have Hkv = H / G
// heads, G an integer >= 1, and query head h reads K/V head h / G: the
// layout of repeat_interleave(G, dim=1), not h % Hkv. BH and H keep
// counting QUERY heads in every kernel. <kGqa = false> is the code without
// it, unchanged. <true>:
//   * forward and dQ keep their block per (b, query head, row block) and
//     every loop; only kp/vp come from kv_slice(): head (bh % H) / G;
//   * dK/dV runs one block per (b, K/V head, 64-key block) and walks the
//     q-steps of the group's G query heads one head after the other into
//     the same accumulators (the argument stands next to that loop).
// G rides in the K stride argument, a StridesGqa<kGqa>, for the reason
// doc_start rides in a StridesDoc: the <false> argument layout stays.
template <bool kGqa>
struct StridesGqa : Strides {
  int group; // G = H / Hkv
};
template <>
struct StridesGqa<false> : Strides {};

// The (b, K/V head) slice of k or v that query-head index bh reads.
template <bool kGqa>
__device__ __forceinline__ const __hip_bfloat16* kv_slice(const __hip_bfloat16* t,
                                                          const Strides& st, int bh, int H,
                                                          const StridesGqa<kGqa>& sk) {
  if constexpr (kGqa) return t + (int64_t)(bh / H) * st.b + (int64_t)((bh % H) / sk.group) * st.h;
  else return tslice(t, st, bh, H);
}

// The row is clamped to N - 1 in every instantiation: an aligned N still
// has 128-row forward blocks whose last waves lie wholly past N.
__device__ __forceinline__ int dstart(const int* __restrict__ ds, int row, int N) {
  const int r = min(row, N - 1);
  return min(max(ds[r], 0), r);
}

// Backward: the recomputed probability of the (key, q) pair with raw score
// `s`, exp(s * scale - lse[q]) with lse2 = lse[q] * log2(e), or 0 where the
// pair is masked. <kDoc>: row q reads keys q_lo <= key <= q_hi (the callers
// fold the causal and ragged ends into q_hi, so q_hi < N covers key < N
// too). Each test stands directly in its `if`, with the exp2 under it: a
// select, or a bool computed first and tested after, makes the compiler
// materialize the mask in registers inside the tile loops.
template <bool kRagged, bool kDoc>
__device__ __forceinline__ float bwd_prob(float s, float scale, float lse2, int key_g, int q_g,
                                          int q_lo, int q_hi, bool causal, int N) {
  float p = 0.0f;
  if constexpr (kDoc) {
    if (key_g >= q_lo && key_g <= q_hi) p = __builtin_amdgcn_exp2f(s * (scale * kLog2e) - lse2);
  } else {
    if ((!causal || key_g <= q_g) && (!kRagged || (key_g < N && q_g < N))) {
      p = __builtin_amdgcn_exp2f(s * (scale * kLog2e) - lse2);
    }
  }
  return p;
}

// ---------------------------------------------------------------- forward
// ONE WAVE owns two 16-row Q sub-tiles and iterates 64-key KV tiles that
// the block's 4 waves (consecutive q rows of ONE (b,h)) stage together, one
// coalesced bf16x8 global load per thread per piece. Online softmax keeps
// m/sumexp in registers; each sub-tile's 16x64 O accumulator is 4 C frags.
// Occupancy note: 204 VGPRs + 32 AGPRs -> 2 waves/SIMD. Forcing 3
// waves/SIMD via amdgpu_waves_per_eu(3) spills 164 B/lane and measured
// SLOWER (552 vs 508 us causal at the GPT-2 shape) — the spill traffic
// in the inner loop outweighs the extra latency hiding. Keep 2 waves.
template <bool kRagged, bool kDoc, bool kGqa>
__global__ void __launch_bounds__(kAttnThreads) attn_fwd_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, __hip_bfloat16* __restrict__ o,
    float* __restrict__ lse, int BH, int H, int N, float scale, bool causal_arg, Strides sq,
    StridesGqa<kGqa> sk, StridesDoc<kDoc> sv) {
  const bool causal = kDoc || causal_arg; // a document mask is causal by contract
  __shared__ __hip_bfloat16 p_lds_all[kWavesPerBlock][kQT][kPStrideF];
  __shared__ __hip_bfloat16 k_lds[2][kKTF][kKVStride];
  // V lives in TILED images for read_tr_frag. A 64-key tile is TWO
  // consecutive 32x64 images (key chunk c at offset c*kImgElems):
  //   elem[c*2048 + (db*2+half)*256 + g*64 + jj*16 + cc] = V[32c+8g+4half+jj][16db+cc]
  __shared__ __hip_bfloat16 v_tr[2][2 * kImgElems];

  // row16: q index inside the tile (and key row for K frags). Staging: a
  // 64x64 tile = 512 bf16x8 pieces, 2 per thread: (st_row, st_col) and
  // (st_row + 32, st_col)
  const auto [lane, wave, row16, grp, st_row, st_col] = thread_coords();
  __hip_bfloat16(*p_lds)[kPStrideF] = p_lds_all[wave];
  // tiled V image offset for the (st_row, st_col) piece; the second
  // piece lands at the same offset in the second 32x64 image
  const int st_vt = vt_idx(st_row, st_col);

  const int nqb = (N + kFwdRowsPerBlock - 1) / kFwdRowsPerBlock;
  const int64_t total_blocks = (int64_t)BH * nqb;

  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    const int bh = blk / nqb;
    const int qb0 = (blk - (int64_t)bh * nqb) * kFwdRowsPerBlock;
    const int i0 = qb0 + wave * 2 * kQT; // this wave's 32 q rows
    const bool valid = i0 < N;
    const __hip_bfloat16* qp = tslice(q, sq, bh, H);
    const __hip_bfloat16* kp = kv_slice(k, sk, bh, H, sk);
    const __hip_bfloat16* vp = kv_slice(v, sv, bh, H, sk);

    bf16x8 qf[2][2]; // [sub-tile][k-chunk]
    if (valid) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          qf[sub][c] =
              *(const bf16x8*)(qp + (int64_t)crow<kRagged>(i0 + 16 * sub + row16, N) * sq.r +
                               32 * c + 8 * grp);
        }
      }
    }

    const float scale2 = scale * kLog2e; // fold log2(e): exp -> v_exp_f32
    float m_run[2] = {-1e30f, -1e30f};
    float s_run[2] = {0.0f, 0.0f};
    f32x4 o_acc[2][4];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int db = 0; db < 4; ++db) o_acc[sub][db] = f32x4{0, 0, 0, 0};

    // Ragged N: kv_end_block <= N is the number of KEYS the block needs
    // and ntiles rounds it up to whole 64-key tiles, so the last tile may
    // cover keys >= N (clamped loads, masked scores). Causal diagonal: a
    // stored row q < N of this wave (i0 <= q < i0 + 32) needs keys 0..q.
    // Key q sits in the tile with j0 = 64 * (q / 64) <= q, and
    // q < min(qb0 + 128, N) = kv_end_block gives q / 64 < ntiles, while
    // j0 <= q < i0 + 32 = my_kv_end, so that tile is walked and not
    // skipped. Rows q >= N of a partly valid wave tile compute on clamped
    // data and are never stored. Key 0 < N is in tile 0, which every
    // sub-tile visits, so m_run is finite after the first tile.
    const int kv_end_block = causal ? min(qb0 + kFwdRowsPerBlock, N) : N;
    const int my_kv_end = causal ? (i0 + 2 * kQT) : N;

    // Documents (kDoc): row q attends keys start[q] <= key <= q, with
    // start[q] = dstart(q) in [0, q]. A lane owns one query per sub-tile,
    // so the mask is one register per sub-tile (q_start; q_span folds
    // the causal and ragged upper end into the same test). Two skips:
    //   * block: the walk begins at the tile holding start[qb0], tile
    //     jt_begin. It depends on (bh, qb0) only, so the prologue, the
    //     trip count and every __syncthreads() stay block-uniform. For a
    //     well-formed doc_start the block's first row has the smallest
    //     start, so no row loses a key. jt_begin <= qb0 / 64 < ntiles.
    //   * sub-tile: tiles with j0 + 64 <= start[qi0] (sub_start, the
    //     sub-tile's first row, wave-uniform) are skipped like the tiles
    //     past the diagonal; the barriers sit outside that branch.
    // Neither can skip a stored row's diagonal key q: its tile has
    // j0 <= q, and start[qb0] <= qb0 <= q, start[qi0] <= qi0 <= q put it
    // at or after both starting tiles. So whatever doc_start holds, every
    // stored row sees at least one unmasked score (its diagonal).
    // The wipe: a sub-tile that straddles a document boundary walks tiles
    // that are fully masked for its later rows before their first valid
    // key. On such a tile the row has m_run = -1e30 and every score
    // -1e30, so m_new = -1e30, alpha = exp2(0) = 1 and every p =
    // exp2(0) = 1: s_run grows by 64 and o_acc by a sum of 64 V rows per
    // tile — garbage, but finite. At the row's first tile with a valid
    // key m_new is a real score, alpha = exp2(-1e30 - m_new) = 0, and
    // s_run * alpha, o_acc * alpha wipe the garbage to exactly 0 before
    // the tile's own terms are added; the masked keys of that tile give
    // p = exp2(-1e30 - m_new) = 0. The diagonal key guarantees that tile
    // exists for every stored row.
    int jt_begin = 0;
    int q_start[2] = {0, 0};
    unsigned q_span[2] = {0, 0}; // min(q, N - 1) - start[q] >= 0
    int sub_start[2] = {0, 0};
    if constexpr (kDoc) {
      const int* dsp = sv.doc_start + (int64_t)(bh / H) * N;
      jt_begin = dstart(dsp, qb0, N) / kKTF;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        q_start[sub] = dstart(dsp, i0 + 16 * sub + row16, N);
        q_span[sub] = (unsigned)(min(i0 + 16 * sub + row16, N - 1) - q_start[sub]);
        sub_start[sub] = __builtin_amdgcn_readfirstlane(dstart(dsp, i0 + 16 * sub, N));
      }
    }
    const int j_begin = jt_begin * kKTF;
    const int buf0 = jt_begin & 1;

    // write-late double buffer (guide §6 G15): the NEXT tile's global
    // loads stay in flight through the current tile's compute; their
    // ds_write targets the other buffer just before the single barrier.
    *(bf16x8*)(&k_lds[buf0][st_row][st_col]) =
        *(const bf16x8*)(kp + (int64_t)crow<kRagged>(j_begin + st_row, N) * sk.r + st_col);
    *(bf16x8*)(&k_lds[buf0][st_row + 32][st_col]) =
        *(const bf16x8*)(kp + (int64_t)crow<kRagged>(j_begin + st_row + 32, N) * sk.r + st_col);
    *(bf16x8*)(&v_tr[buf0][st_vt]) =
        *(const bf16x8*)(vp + (int64_t)crow<kRagged>(j_begin + st_row, N) * sv.r + st_col);
    *(bf16x8*)(&v_tr[buf0][kImgElems + st_vt]) =
        *(const bf16x8*)(vp + (int64_t)crow<kRagged>(j_begin + st_row + 32, N) * sv.r + st_col);
    __syncthreads();

    const int ntiles = (kv_end_block + kKTF - 1) / kKTF;
    for (int jt = jt_begin; jt < ntiles; ++jt) {
      const int j0 = jt * kKTF;
      const int buf = jt & 1;
      bf16x8 knext0, knext1, vnext0, vnext1;
      const bool has_next = jt + 1 < ntiles;
      if (has_next) {
        knext0 = *(const bf16x8*)(kp + (int64_t)crow<kRagged>(j0 + kKTF + st_row, N) * sk.r +
                                  st_col);
        knext1 = *(const bf16x8*)(kp + (int64_t)crow<kRagged>(j0 + kKTF + 32 + st_row, N) * sk.r +
                                  st_col);
        vnext0 = *(const bf16x8*)(vp + (int64_t)crow<kRagged>(j0 + kKTF + st_row, N) * sv.r +
                                  st_col);
        vnext1 = *(const bf16x8*)(vp + (int64_t)crow<kRagged>(j0 + kKTF + 32 + st_row, N) * sv.r +
                                  st_col);
      }

      if (valid && j0 < my_kv_end) {
        // shared V fragments for both q sub-tiles: [key chunk][D chunk]
        bf16x8 vf[2][4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
          for (int db = 0; db < 4; ++db) {
            vf[c][db] = read_tr_frag(&v_tr[buf][c * kImgElems], db, lane);
          }
        }
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          const int qi0 = i0 + 16 * sub;
          if (causal && j0 >= qi0 + kQT) continue; // tile fully past diagonal
          if constexpr (kDoc) {
            if (j0 + kKTF <= sub_start[sub]) continue; // tile wholly in earlier documents
          }

          // ---- S^T = K Q^T for four 16-key quarters ----
          float sv[16]; // h*4 + r: key = j0 + 16h + 4grp + r, query = row16
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            f32x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const bf16x8 kf = *(const bf16x8*)(&k_lds[buf][16 * h + row16][32 * c + 8 * grp]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[sub][c], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float s = acc[r] * scale2; // log2-domain scores
              if constexpr (kDoc) {
                // start[q] <= key <= min(q, N - 1) as one unsigned range
                // test: the document, causal and ragged masks together
                const int key_g = j0 + 16 * h + 4 * grp + r;
                if ((unsigned)(key_g - q_start[sub]) > q_span[sub]) s = -1e30f;
              } else {
                if (causal) {
                  const int key_g = j0 + 16 * h + 4 * grp + r;
                  const int q_g = qi0 + row16;
                  if (key_g > q_g) s = -1e30f;
                }
                if constexpr (kRagged) {
                  if (j0 + 16 * h + 4 * grp + r >= N) s = -1e30f; // clamped duplicate key
                }
              }
              sv[h * 4 + r] = s;
            }
          }

          // ---- online softmax (per q = row16; reduce across grp groups) ----
          float mt = sv[0];
#pragma unroll
          for (int x = 1; x < 16; ++x) mt = fmaxf(mt, sv[x]);
          mt = fmaxf(mt, __shfl_xor(mt, 16, kWave));
          mt = fmaxf(mt, __shfl_xor(mt, 32, kWave));
          const float m_new = fmaxf(m_run[sub], mt);
          const float alpha = __builtin_amdgcn_exp2f(m_run[sub] - m_new); // -1e30 -> 0

          float ps = 0.0f;
#pragma unroll
          for (int x = 0; x < 16; ++x) {
            sv[x] = __builtin_amdgcn_exp2f(sv[x] - m_new); // raw v_exp_f32 rate
            ps += sv[x];
          }
          ps += __shfl_xor(ps, 16, kWave);
          ps += __shfl_xor(ps, 32, kWave);
          s_run[sub] = s_run[sub] * alpha + ps;
          m_run[sub] = m_new;

          // ---- P^T -> per-wave LDS slice (4 keys per 8-byte write) ----
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            bf16x4 pw;
#pragma unroll
            for (int r = 0; r < 4; ++r) pw[r] = (__bf16)sv[h * 4 + r];
            *(bf16x4*)(&p_lds[row16][16 * h + 4 * grp]) = pw;
          }

          float a_o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) a_o[r] = __shfl(alpha, 4 * grp + r, kWave);

          // ---- PV: A = P[q][key] from LDS, B = shared V fragments ----
          const bf16x8 pf0 = *(const bf16x8*)(&p_lds[row16][8 * grp]);
          const bf16x8 pf1 = *(const bf16x8*)(&p_lds[row16][32 + 8 * grp]);
#pragma unroll
          for (int db = 0; db < 4; ++db) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o_acc[sub][db][r] *= a_o[r];
            o_acc[sub][db] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf0, vf[0][db], o_acc[sub][db], 0, 0, 0);
            o_acc[sub][db] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf1, vf[1][db], o_acc[sub][db], 0, 0, 0);
          }
        }
      }
      if (has_next) {
        *(bf16x8*)(&k_lds[buf ^ 1][st_row][st_col]) = knext0;
        *(bf16x8*)(&k_lds[buf ^ 1][st_row + 32][st_col]) = knext1;
        *(bf16x8*)(&v_tr[buf ^ 1][st_vt]) = vnext0;
        *(bf16x8*)(&v_tr[buf ^ 1][kImgElems + st_vt]) = vnext1;
      }
      __syncthreads(); // readers of buf done AND buf^1 writes visible
    }

    if (valid) {
      // ---- epilogue: O /= sumexp, store; lse = m + log(sumexp) ----
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int db = 0; db < 4; ++db) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q_o = 4 * grp + r;
            const float denom = __shfl(s_run[sub], q_o, kWave);
            const float val = o_acc[sub][db][r] / denom;
            if (!kRagged || i0 + 16 * sub + q_o < N)
              o[(int64_t)bh * N * kAttnD + (int64_t)(i0 + 16 * sub + q_o) * kAttnD + 16 * db +
                row16] = __float2bfloat16(val);
          }
        }
        if (lane < 16 && (!kRagged || i0 + 16 * sub + row16 < N)) {
          // convert the log2-domain stats back to natural-log lse
          lse[(int64_t)bh * N + i0 + 16 * sub + row16] = kLn2 * m_run[sub] + __logf(s_run[sub]);
        }
      }
    }
  }
}

// ------------------------------------- launch plumbing (attn_fwd, attn_bwd)
static Strides strides_of(const at::Tensor& t) { return {t.stride(0), t.stride(1), t.stride(2)}; }

// The kernels' last stride argument (see StridesDoc).
template <bool kDoc>
static StridesDoc<kDoc> doc_strides_of(const at::Tensor& t, const int* doc_start) {
  if constexpr (kDoc) return {strides_of(t), doc_start};
  else return {strides_of(t)};
}

// The kernels' K stride argument (see StridesGqa).
template <bool kGqa>
static StridesGqa<kGqa> gqa_strides_of(const at::Tensor& t, int group) {
  if constexpr (kGqa) return {strides_of(t), group};
  else return {strides_of(t)};
}

// f(bool_constant<kRagged>, bool_constant<kDoc>, bool_constant<kGqa>): an
// aligned N keeps the unmasked code, any other the clamped/masked/predicated
// one; a doc_start kDoc; fewer K/V heads than query heads kGqa.
template <typename F>
static void with_variant(bool ragged, bool has_doc, bool gqa, F&& f) {
  auto pick_gqa = [&](auto ragged_c, auto doc_c) {
    gqa ? f(ragged_c, doc_c, std::true_type{}) : f(ragged_c, doc_c, std::false_type{});
  };
  if (ragged) {
    has_doc ? pick_gqa(std::true_type{}, std::true_type{})
            : pick_gqa(std::true_type{}, std::false_type{});
  } else {
    has_doc ? pick_gqa(std::false_type{}, std::true_type{})
            : pick_gqa(std::false_type{}, std::false_type{});
  }
}

static int attn_grid(int BH, int N, int rows_per_block) {
  const int64_t blocks = (int64_t)BH * ((N + rows_per_block - 1) / rows_per_block);
  return (int)std::min<int64_t>(blocks, kMaxGrid);
}

// Everything both launchers require of their tensors, before any launch.
// q is [B, H, N, 64]; k is [B, Hkv, N, 64] with 1 <= Hkv <= H and H % Hkv == 0
// (Hkv < H is grouped-query attention). `strided`: bf16 on q's device, last
// dim contiguous (reached through per-tensor strides), `like_q` shaped like q
// and `like_k` shaped like k. `dense`: the same, but indexed as contiguous
// [B*heads, N, 64]. `row_stats` (lse, delta): fp32 on q's device, >= B*H*N
// elements. Returns the group size G = H / Hkv.
using NamedTensor = std::pair<const char*, const at::Tensor&>;
using NamedTensors = std::initializer_list<NamedTensor>;
static int check_attn_args(const at::Tensor& q, const at::Tensor& k, NamedTensors strided_like_q,
                           NamedTensors strided_like_k, NamedTensors dense_like_q,
                           NamedTensors dense_like_k, NamedTensors row_stats) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.size(3) == kAttnD && q.size(2) >= 1,
              "q must be a device tensor [B,H,N,64] with N >= 1 (head dim 64 only)");
  TORCH_CHECK(k.dim() == 4 && k.size(0) == q.size(0) && k.size(2) == q.size(2) &&
                  k.size(3) == kAttnD && k.size(1) >= 1 && k.size(1) <= q.size(1) &&
                  q.size(1) % k.size(1) == 0,
              "k must be [B,Hkv,N,64] with q's B and N (self-attention geometry) and a head "
              "count Hkv that divides q's: got ", k.sizes(), " for q ", q.sizes());
  auto check = [&](const NamedTensor& a, at::ScalarType dtype, bool layout, const char* want) {
    TORCH_CHECK(a.second.scalar_type() == dtype && a.second.device() == q.device() && layout,
                a.first, " must be ", want, " on q's device");
  };
  for (const NamedTensor& a : strided_like_q) {
    check(a, at::kBFloat16, a.second.sizes() == q.sizes() && a.second.stride(3) == 1,
          "bf16, shaped like q, last dim contiguous,");
  }
  for (const NamedTensor& a : strided_like_k) {
    check(a, at::kBFloat16, a.second.sizes() == k.sizes() && a.second.stride(3) == 1,
          "bf16, shaped like k ([B,Hkv,N,64]), last dim contiguous,");
  }
  for (const NamedTensor& a : dense_like_q) {
    check(a, at::kBFloat16, a.second.sizes() == q.sizes() && a.second.is_contiguous(),
          "bf16, shaped like q, contiguous,");
  }
  for (const NamedTensor& a : dense_like_k) {
    check(a, at::kBFloat16, a.second.sizes() == k.sizes() && a.second.is_contiguous(),
          "bf16, shaped like k ([B,Hkv,N,64]), contiguous,");
  }
  for (const NamedTensor& a : row_stats) {
    check(a, at::kFloat, a.second.numel() >= q.size(0) * q.size(1) * q.size(2), "fp32[B*H*N]");
  }
  return (int)(q.size(1) / k.size(1));
}

// doc_start, when given: int32 [B, N], contiguous, on q's device, causal
// only. Returns its data pointer (nullptr when absent).
static const int* checked_doc_start(const c10::optional<at::Tensor>& doc_start,
                                    const at::Tensor& q, bool causal) {
  if (!doc_start.has_value() || !doc_start->defined()) return nullptr;
  const at::Tensor& ds = *doc_start;
  TORCH_CHECK(causal, "doc_start requires causal attention");
  TORCH_CHECK(ds.scalar_type() == at::kInt, "doc_start must be int32");
  TORCH_CHECK(ds.device() == q.device(), "doc_start must be on q's device");
  TORCH_CHECK(ds.dim() == 2 && ds.size(0) == q.size(0) && ds.size(1) == q.size(2),
              "doc_start must be [B, N]");
  TORCH_CHECK(ds.is_contiguous(), "doc_start must be contiguous");
  return ds.data_ptr<int>();
}

void attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse,
              double scale, bool causal, c10::optional<at::Tensor> doc_start) {
  const int G = check_attn_args(q, k, {{"q", q}}, {{"k", k}, {"v", v}}, {{"o", o}}, {},
                                {{"lse", lse}});
  const int* dsp = checked_doc_start(doc_start, q, causal);
  const int H = q.size(1), N = q.size(2), BH = q.size(0) * H;
  auto stream = c10::hip::getCurrentHIPStream();
  static_assert(kKTF % (2 * kQT) == 0); // a wave's 32 q rows also end at N then
  with_variant(N % kKTF != 0, dsp != nullptr, G > 1, [&](auto ragged, auto doc, auto gqa) {
    constexpr bool kDoc = decltype(doc)::value, kGqa = decltype(gqa)::value;
    hipLaunchKernelGGL((attn_fwd_kernel<decltype(ragged)::value, kDoc, kGqa>),
                       dim3(attn_grid(BH, N, kFwdRowsPerBlock)), dim3(kAttnThreads), 0, stream,
                       (const __hip_bfloat16*)q.data_ptr(), (const __hip_bfloat16*)k.data_ptr(),
                       (const __hip_bfloat16*)v.data_ptr(), (__hip_bfloat16*)o.data_ptr(),
                       lse.data_ptr<float>(), BH, H, N, (float)scale, causal, strides_of(q),
                       gqa_strides_of<kGqa>(k, G), doc_strides_of<kDoc>(v, dsp));
  });
}

// ===========================================================================
// Backward (flash recomputation, ops/_attention_ref.py::flash_attn_bwd_tiled)
// ===========================================================================
//
//   delta = rowsum(dO * O)                    (attn_bwd_delta_kernel)
//   P^T   = exp(K Q^T * scale - lse[q])       (recomputed per tile pair)
//   dP^T  = V dO^T
//   dS^T  = P^T * (dP^T - delta[q]) * scale
//   dV   += P^T  @ dO      dK += dS^T @ Q     (attn_bwd_dkdv_kernel,
//                                              wave owns a 16-key tile)
//   dQ   += dS @ K                            (attn_bwd_dq_kernel,
//                                              wave owns a 16-q tile)
//
// Every MFMA reuses the forward's fragment patterns; the only transposes
// (P^T/dS^T C-layout -> A operand) go through small per-wave LDS slices
// exactly like the forward's P.

// -------------------------------------------------- delta = rowsum(dO*O)
// Per-row kernel: r0 runs over the BH * N real rows only and every load
// and the store index with r0 (or its (bh, rr) split, rr < N), so it is
// correct for any N as it stands and needs no ragged variant.
__global__ void __launch_bounds__(kBlock) attn_bwd_delta_kernel(
    const __hip_bfloat16* __restrict__ dout, const __hip_bfloat16* __restrict__ o,
    float* __restrict__ delta, int64_t rows, int H, int N, Strides sdo) {
  // one wave per 8 rows: lane l -> row l/8, 8-elem chunk l%8
  const int64_t stride = ((int64_t)gridDim.x * kBlock) / 8;
  for (int64_t r0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / 8; r0 < rows; r0 += stride) {
    const int chunk = threadIdx.x & 7;
    const int bh = r0 / N;
    const int rr = r0 - (int64_t)bh * N;
    bf16x8 a = *(const bf16x8*)(tslice(dout, sdo, bh, H) + (int64_t)rr * sdo.r + 8 * chunk);
    bf16x8 b = *(const bf16x8*)(o + r0 * kAttnD + 8 * chunk);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += (float)a[j] * (float)b[j];
    // reduce the 8 chunks of this row (lanes l..l+7 within the wave)
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    if (chunk == 0) delta[r0] = s;
  }
}

// ------------------------------------------------------------- dK and dV
// Block = 4 waves, each owning a 16-key tile of one (b,h); q-tiles of 32
// rows (Q and dO staged in shared LDS) stream past. Per q-tile, per wave:
// 2 MFMAs S^T, 2 MFMAs dP^T, 4+4 MFMAs dV/dK accumulation (k = 32 q rows).
template <bool kRagged, bool kDoc, bool kGqa>
__global__ void __launch_bounds__(kAttnThreads) attn_bwd_dkdv_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    __hip_bfloat16* __restrict__ dk, __hip_bfloat16* __restrict__ dv, int BH, int H, int N,
    float scale, bool causal_arg, Strides sq, StridesGqa<kGqa> sk, Strides sv,
    StridesDoc<kDoc> sdo) {
  const bool causal = kDoc || causal_arg; // a document mask is causal by contract
  constexpr int kQStep = 32; // q rows per iteration (MFMA contraction width)
  static_assert(kQStep * kAttnD == kImgElems);
  __shared__ __hip_bfloat16 q_lds[kImgElems]; // tiled (vt_idx) image
  __shared__ __hip_bfloat16 do_lds[kImgElems]; // tiled (vt_idx) image
  // per-wave transpose slices, [key16][q32(+skew)] rows for A-operand reads
  __shared__ __hip_bfloat16 pt_lds_all[kWavesPerBlock][16][kPStride];
  __shared__ __hip_bfloat16 dst_lds_all[kWavesPerBlock][16][kPStride];

  const auto [lane, wave, row16, grp, st_row, st_col] = thread_coords(); // st_row 0..31
  __hip_bfloat16(*pt_lds)[kPStride] = pt_lds_all[wave];
  __hip_bfloat16(*dst_lds)[kPStride] = dst_lds_all[wave];

  const int nkb = (N + kBwdKeysPerBlock - 1) / kBwdKeysPerBlock;
  // kGqa: a block belongs to one (b, K/V head) and `bh` below counts those,
  // B * Hkv = BH / G of them; bh * group is then the (b, query head) index
  // of the first head of its group (kv_slice maps it back to the K/V
  // head), and the group's heads follow it.
  int group = 1;
  if constexpr (kGqa) group = sk.group;
  const int64_t total_blocks = (int64_t)(BH / group) * nkb;

  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    const int bh = blk / nkb;
    const int kb0 = (blk - (int64_t)bh * nkb) * kBwdKeysPerBlock;
    const int j0 = kb0 + wave * 16; // this wave's 16 keys
    const bool valid = j0 < N;
    // q-side pointers of the group's first head (of THE head without kGqa)
    const __hip_bfloat16* qp = tslice(q, sq, bh * group, H);
    const __hip_bfloat16* kp = kv_slice(k, sk, bh * group, H, sk);
    const __hip_bfloat16* vp = kv_slice(v, sv, bh * group, H, sk);
    const __hip_bfloat16* dop = tslice(dout, sdo, bh * group, H);
    const float* lsep = lse + (int64_t)bh * group * N;
    const float* delp = delta + (int64_t)bh * group * N;

    // wave-local K and V fragments for this key tile (row-major loads)
    bf16x8 kf[2], vf2[2];
    if (valid) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int kr = crow<kRagged>(j0 + row16, N);
        kf[c] = *(const bf16x8*)(kp + (int64_t)kr * sk.r + 32 * c + 8 * grp);
        vf2[c] = *(const bf16x8*)(vp + (int64_t)kr * sv.r + 32 * c + 8 * grp);
      }
    }

    f32x4 dv_acc[4], dk_acc[4]; // rows = key (4grp+r), cols = 16*db + row16
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      dv_acc[db] = f32x4{0, 0, 0, 0};
      dk_acc[db] = f32x4{0, 0, 0, 0};
    }

    // Ragged N: nkb rounds the key blocks up, so the last block's waves
    // may own keys >= N (clamped loads, p = 0, no store), and the q loop
    // walks 32-row steps while i0 < N, so the last step may cover q rows
    // >= N (clamped loads, p = 0: a padded query adds nothing to dK/dV).
    // Causal diagonal: a stored key j < N of this block needs q rows
    // j..N-1. kb0 is a multiple of 64, so i_start = kb0 <= j, and the
    // steps from kb0 to the one holding N - 1 cover every q in [j, N);
    // the per-wave skip only drops steps with i0 + 32 <= j0, i.e. whose
    // q rows are all below every key of the wave.
    // Documents (kDoc): p = 0 for key < start[q], start[q] = dstart(q)
    // loaded next to lse/delta for each 16-q half. i_start is unchanged
    // (the diagonal step is where a key's own document begins to read
    // it). A well-formed doc_start is non-decreasing, so once the first
    // row of a q-step starts behind this block's last key (kb0 + 63), no
    // row of this or any later step can reach a key of the block: leave
    // the loop. The test depends on (bh, kb0, i0) only, so the break is
    // block-uniform and sits before the step's barriers. A malformed
    // doc_start can only end the loop early (fewer terms, never a fault).
    // Groups (kGqa): dK[key] = sum over the group's G query heads of that
    // head's dS^T Q, and dV likewise, so the q-step walk above runs once
    // per head, in ascending head order, with that head's qp / dop / lsep /
    // delp, and every pass adds into the SAME dv_acc / dk_acc: the group
    // sum happens in the fp32 accumulators and each output element is
    // rounded and stored once. kf / vf2 are loaded once (all G heads read
    // this K/V head). Nothing above depends on the head: i_start, the
    // per-wave skip and valid are functions of (kb0, j0, i0), and doc_start
    // is shared by all heads, so under kDoc the break ends ONE head's walk
    // after the same number of steps for each head; the next head starts
    // again at i_start with step_start reloaded. The test still depends on
    // (b, kb0, i0) only, so it stays block-uniform for every head. Every
    // step ends with a barrier, so a head's first staging never overtakes
    // a reader of the previous head's last tiles. Query head g of the group
    // is (b, query head) index bh * group + g. <kGqa = false>: the do-while
    // is the code it wraps, run once.
    const int* dsp = nullptr;
    if constexpr (kDoc) dsp = sdo.doc_start + (int64_t)(bh * group / H) * N;
    const int i_start = causal ? (kb0 & ~(kQStep - 1)) : 0; // block-aligned diag
    int g = 0;
    do {
      // (the start of the NEXT step's first row is loaded a step ahead, so
      // the test does not wait on memory in front of the barrier)
      int step_start = 0;
      if constexpr (kDoc) step_start = dstart(dsp, i_start, N);
      for (int i0 = i_start; i0 < N; i0 += kQStep) {
        if constexpr (kDoc) {
          if (step_start > kb0 + kBwdKeysPerBlock - 1) break;
          step_start = dstart(dsp, i0 + kQStep, N);
        }
        // ---- stage Q and dO into tiled images (one bf16x8 per thread) ----
        const int st_t = vt_idx(st_row, st_col);
        const int st_g = crow<kRagged>(i0 + st_row, N);
        *(bf16x8*)(&q_lds[st_t]) = *(const bf16x8*)(qp + (int64_t)st_g * sq.r + st_col);
        *(bf16x8*)(&do_lds[st_t]) = *(const bf16x8*)(dop + (int64_t)st_g * sdo.r + st_col);
        __syncthreads();

        if (valid && (!causal || i0 + kQStep > j0)) {
          // two 16-q halves share this wave's key tile
#pragma unroll
          for (int hq = 0; hq < 2; ++hq) {
            const int q0 = i0 + 16 * hq; // this half's first q row
            const int qr = crow<kRagged>(q0 + row16, N);
            const float lse2_q = lsep[qr] * kLog2e; // log2 domain
            const float del_q = delp[qr];
            // kDoc: row q reads keys q_lo <= key <= q_hi = q (causal); a
            // padded row q >= N gets the empty range (q_hi = -1 < q_lo)
            int q_lo = 0, q_hi = 0;
            if constexpr (kDoc) {
              q_lo = dstart(dsp, q0 + row16, N);
              q_hi = (!kRagged || q0 + row16 < N) ? q0 + row16 : -1;
            }

            // ---- S^T = K Q^T (rows = key, cols = q) ----
            f32x4 acc = {0, 0, 0, 0};
            f32x4 dpt = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int rm = vt_idx(16 * hq + row16, 32 * c + 8 * grp);
              const bf16x8 qfr = *(const bf16x8*)(&q_lds[rm]);
              const bf16x8 dof = *(const bf16x8*)(&do_lds[rm]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[c], qfr, acc, 0, 0, 0);
              dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf2[c], dof, dpt, 0, 0, 0);
            }

            // ---- P^T and dS^T in C layout; write transposed slices ----
            // lane holds keys 4grp+r (rows), q = row16 (col)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float p = bwd_prob<kRagged, kDoc>(acc[r], scale, lse2_q, j0 + 4 * grp + r,
                                                      q0 + row16, q_lo, q_hi, causal, N);
              const float ds = p * (dpt[r] - del_q) * scale;
              // [key][q] slices: q column of this half = 16*hq + row16
              pt_lds[4 * grp + r][16 * hq + row16] = __float2bfloat16(p);
              dst_lds[4 * grp + r][16 * hq + row16] = __float2bfloat16(ds);
            }
          }
          // same-wave LDS visibility; A-operand reads below

          // ---- dV += P^T @ dO ; dK += dS^T @ Q  (contraction over 32 q) ----
          const bf16x8 ptf = *(const bf16x8*)(&pt_lds[row16][8 * grp]);
          const bf16x8 dstf = *(const bf16x8*)(&dst_lds[row16][8 * grp]);
#pragma unroll
          for (int db = 0; db < 4; ++db) {
            const bf16x8 dob = read_tr_frag(do_lds, db, lane);
            const bf16x8 qb = read_tr_frag(q_lds, db, lane);
            dv_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ptf, dob, dv_acc[db], 0, 0, 0);
            dk_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dstf, qb, dk_acc[db], 0, 0, 0);
          }
        }
        __syncthreads(); // staged tiles consumed before restage
      }
      if constexpr (kGqa) {
        // (after the last head these four are formed and never read; with
        // the exit test in front of them one SGPR spills in <false, true>)
        ++g;
        qp = tslice(q, sq, bh * group + g, H);
        dop = tslice(dout, sdo, bh * group + g, H);
        lsep = lse + (int64_t)(bh * group + g) * N;
        delp = delta + (int64_t)(bh * group + g) * N;
      }
    } while (kGqa && g < group);

    if (valid) {
#pragma unroll
      for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key_o = 4 * grp + r;
          if (kRagged && j0 + key_o >= N) continue;
          dv[(int64_t)bh * N * kAttnD + (int64_t)(j0 + key_o) * kAttnD + 16 * db + row16] =
              __float2bfloat16(dv_acc[db][r]);
          dk[(int64_t)bh * N * kAttnD + (int64_t)(j0 + key_o) * kAttnD + 16 * db + row16] =
              __float2bfloat16(dk_acc[db][r]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------- dQ
// Mirror of the forward: block = 4 waves x one 16-q tile; 32-key KV tiles
// (K and V staged shared). dq[q][d] += dS[q][key] @ K[key][d].
template <bool kRagged, bool kDoc, bool kGqa>
__global__ void __launch_bounds__(kAttnThreads) attn_bwd_dq_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    __hip_bfloat16* __restrict__ dq, int BH, int H, int N, float scale, bool causal_arg,
    Strides sq, StridesGqa<kGqa> sk, Strides sv, StridesDoc<kDoc> sdo) {
  const bool causal = kDoc || causal_arg; // a document mask is causal by contract
  static_assert(kKT * kAttnD == kImgElems);
  __shared__ __hip_bfloat16 k_lds[kImgElems]; // tiled (vt_idx) image
  __shared__ __hip_bfloat16 v_lds[kKT][kKVStride];
  __shared__ __hip_bfloat16 ds_lds_all[kWavesPerBlock][kQT][kPStride]; // [q][key32]

  const auto [lane, wave, row16, grp, st_row, st_col] = thread_coords();
  __hip_bfloat16(*ds_lds)[kPStride] = ds_lds_all[wave];

  const int nqb = (N + kDqRowsPerBlock - 1) / kDqRowsPerBlock;
  const int64_t total_blocks = (int64_t)BH * nqb;

  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    const int bh = blk / nqb;
    const int qb0 = (blk - (int64_t)bh * nqb) * kDqRowsPerBlock;
    const int i0 = qb0 + wave * kQT;
    const bool valid = i0 < N;
    const __hip_bfloat16* qp = tslice(q, sq, bh, H);
    const __hip_bfloat16* kp = kv_slice(k, sk, bh, H, sk);
    const __hip_bfloat16* vp = kv_slice(v, sv, bh, H, sk);
    const __hip_bfloat16* dop = tslice(dout, sdo, bh, H);
    const float* lsep = lse + (int64_t)bh * N;
    const float* delp = delta + (int64_t)bh * N;

    bf16x8 qf[2], dof[2];
    float lse_q = 0.0f, del_q = 0.0f;
    if (valid) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int qr = crow<kRagged>(i0 + row16, N);
        qf[c] = *(const bf16x8*)(qp + (int64_t)qr * sq.r + 32 * c + 8 * grp);
        dof[c] = *(const bf16x8*)(dop + (int64_t)qr * sdo.r + 32 * c + 8 * grp);
      }
      lse_q = lsep[crow<kRagged>(i0 + row16, N)] * kLog2e; // log2 domain
      del_q = delp[crow<kRagged>(i0 + row16, N)];
    }

    f32x4 dq_acc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) dq_acc[db] = f32x4{0, 0, 0, 0};

    // Ragged N: the key loop walks 32-key tiles while j0 < kv_end_block
    // <= N, so only the last tile can cover keys >= N (clamped loads,
    // p = 0). Causal diagonal: a stored row q < N of this wave
    // (i0 <= q < i0 + 16) needs keys 0..q; key q sits in the tile with
    // j0 = 32 * (q / 32) <= q < min(qb0 + 64, N) = kv_end_block, and
    // j0 <= q < i0 + 16 = my_kv_end, so it is walked and not skipped.
    const int kv_end_block = causal ? min(qb0 + kDqRowsPerBlock, N) : N;
    const int my_kv_end = causal ? (i0 + kQT) : N;

    // Documents (kDoc): p = 0 for key < start[q]; a lane owns one query,
    // so start[q] = dstart(q) is one register (q_lo). The key walk
    // begins at the 32-key tile holding start[qb0] (j_begin: depends on
    // (bh, qb0) only, so the barriers stay block-uniform), and a wave
    // also passes over tiles that end at or before start[i0] (wave_start,
    // wave-uniform; the barriers sit outside that branch). A stored row
    // q >= i0 >= qb0 keeps its diagonal: start[qb0] <= qb0 <= q and
    // start[i0] <= i0 <= q, so the tile holding key q is at or after
    // both. With a well-formed (non-decreasing) doc_start the first row
    // has the smallest start and no row loses a key.
    int j_begin = 0, q_lo = 0, q_hi = 0, wave_start = 0;
    if constexpr (kDoc) {
      const int* dsp = sdo.doc_start + (int64_t)(bh / H) * N;
      j_begin = dstart(dsp, qb0, N) & ~(kKT - 1);
      q_lo = dstart(dsp, i0 + row16, N);
      // causal upper end; a padded row q >= N gets the empty range
      q_hi = (!kRagged || i0 + row16 < N) ? i0 + row16 : -1;
      wave_start = __builtin_amdgcn_readfirstlane(dstart(dsp, i0, N));
    }

    for (int j0 = j_begin; j0 < kv_end_block; j0 += kKT) {
      const int st_g = crow<kRagged>(j0 + st_row, N);
      *(bf16x8*)(&k_lds[vt_idx(st_row, st_col)]) =
          *(const bf16x8*)(kp + (int64_t)st_g * sk.r + st_col);
      *(bf16x8*)(&v_lds[st_row][st_col]) = *(const bf16x8*)(vp + (int64_t)st_g * sv.r + st_col);
      __syncthreads();

      if (valid && j0 < my_kv_end && (!kDoc || j0 + kKT > wave_start)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) { // two 16-key halves
          // S^T rows = key (4grp+r), col = q (row16)
          f32x4 acc = {0, 0, 0, 0};
          f32x4 dpt = {0, 0, 0, 0};
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const bf16x8 kfr = *(const bf16x8*)(&k_lds[vt_idx(16 * h + row16, 32 * c + 8 * grp)]);
            const bf16x8 vfr = *(const bf16x8*)(&v_lds[16 * h + row16][32 * c + 8 * grp]);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[c], acc, 0, 0, 0);
            dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfr, dof[c], dpt, 0, 0, 0);
          }
          // dS^T -> [q][key] slice (4 consecutive keys pack per write)
          bf16x4 dsw;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = bwd_prob<kRagged, kDoc>(acc[r], scale, lse_q,
                                                    j0 + 16 * h + 4 * grp + r, i0 + row16, q_lo,
                                                    q_hi, causal, N);
            dsw[r] = (__bf16)(p * (dpt[r] - del_q) * scale);
          }
          *(bf16x4*)(&ds_lds[row16][16 * h + 4 * grp]) = dsw;
        }

        // ---- dq += dS @ K (contraction over the 32 keys) ----
        const bf16x8 dsf = *(const bf16x8*)(&ds_lds[row16][8 * grp]);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const bf16x8 kb = read_tr_frag(k_lds, db, lane);
          dq_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, kb, dq_acc[db], 0, 0, 0);
        }
      }
      __syncthreads();
    }

    if (valid) {
#pragma unroll
      for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q_o = 4 * grp + r;
          if (kRagged && i0 + q_o >= N) continue;
          dq[(int64_t)bh * N * kAttnD + (int64_t)(i0 + q_o) * kAttnD + 16 * db + row16] =
              __float2bfloat16(dq_acc[db][r]);
        }
      }
    }
  }
}

void attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor dout, at::Tensor o,
              at::Tensor lse, at::Tensor dq, at::Tensor dk, at::Tensor dv, at::Tensor delta,
              double scale, bool causal, c10::optional<at::Tensor> doc_start) {
  const int G = check_attn_args(q, k, {{"q", q}, {"dout", dout}}, {{"k", k}, {"v", v}},
                                {{"o", o}, {"dq", dq}}, {{"dk", dk}, {"dv", dv}},
                                {{"lse", lse}, {"delta", delta}});
  const int* dsp = checked_doc_start(doc_start, q, causal);
  const int H = q.size(1), N = q.size(2), BH = q.size(0) * H;
  auto stream = c10::hip::getCurrentHIPStream();

  const int64_t rows = (int64_t)BH * N;
  hipLaunchKernelGGL(attn_bwd_delta_kernel, dim3(grid_for(rows * 8, kBlock)), dim3(kBlock), 0,
                     stream, (const __hip_bfloat16*)dout.data_ptr(),
                     (const __hip_bfloat16*)o.data_ptr(), delta.data_ptr<float>(), rows, H, N,
                     strides_of(dout));

  // see crow(): <false> is the aligned code, for N that ends both kernels' blocks
  const bool ragged = N % kBwdKeysPerBlock != 0 || N % kDqRowsPerBlock != 0;
  with_variant(ragged, dsp != nullptr, G > 1, [&](auto ragged_c, auto doc, auto gqa) {
    constexpr bool kRagged = decltype(ragged_c)::value, kDoc = decltype(doc)::value,
                   kGqa = decltype(gqa)::value;
    // grid_bh: the (b, head) pairs the kernel's blocks split: B * Hkv for
    // dK/dV, B * H for dQ. The kernels themselves always take BH = B * H.
    auto launch = [&](auto kernel, int grid_bh, int rows_per_block, auto... outputs) {
      hipLaunchKernelGGL(kernel, dim3(attn_grid(grid_bh, N, rows_per_block)), dim3(kAttnThreads), 0,
                         stream, (const __hip_bfloat16*)q.data_ptr(),
                         (const __hip_bfloat16*)k.data_ptr(), (const __hip_bfloat16*)v.data_ptr(),
                         (const __hip_bfloat16*)dout.data_ptr(), lse.data_ptr<float>(),
                         delta.data_ptr<float>(), outputs..., BH, H, N, (float)scale, causal,
                         strides_of(q), gqa_strides_of<kGqa>(k, G), strides_of(v),
                         doc_strides_of<kDoc>(dout, dsp));
    };
    launch(attn_bwd_dkdv_kernel<kRagged, kDoc, kGqa>, BH / G, kBwdKeysPerBlock,
           (__hip_bfloat16*)dk.data_ptr(), (__hip_bfloat16*)dv.data_ptr());
    launch(attn_bwd_dq_kernel<kRagged, kDoc, kGqa>, BH, kDqRowsPerBlock,
           (__hip_bfloat16*)dq.data_ptr());
  });
}

} // namespace dmlamd
